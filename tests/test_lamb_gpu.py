"""volta_amd.optimization.LAMB at model level (a tiny two-stream model from the engine tests' fixtures) against the float64 restatement of
tests/lamb_restate.py fed the engine's own gradients, plus the optimizer's conventions: `.grad` untouched, per-tensor ratios inside a
fused query | key | value slot, checkpoint round trip, deferred clip_grad_norm_, skipped parameters, the zero1 refusal and tensors outside
the arena.  Where two runs of the same kernels on the same inputs are compared the gate is bit equality.  GPU only."""
import copy
import os
import sys
import types

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lamb_restate as R  # noqa: E402

NO_DECAY = ["bias", "LayerNorm.bias", "LayerNorm.weight"]
NOGRAD = "cls.bi_seq_relationship."            # another task's head: no gradient in the seeded runs
LR, WD, MAXN = (2e-3, 1e-3), (0.01, 0.0), (1.0, 1.0)


def _model(sd=None):
    from test_engine_gpu import build
    model, rcfg, _ = build("gated")
    if sd is not None:
        model.load_state_dict(sd)
    model.eval()                                # no dropout: the gradients are a function of the weights and the batch alone
    return model, rcfg


def _groups(named, **kw):
    """train_concap.py's two kinds of parameters as two groups (decay / no decay), each with its own lr."""
    dec = [p for n, p in named if not any(nd in n for nd in NO_DECAY)]
    nod = [p for n, p in named if any(nd in n for nd in NO_DECAY)]
    return [dict(params=dec, lr=LR[0], weight_decay=WD[0], max_grad_norm=MAXN[0], **kw), dict(params=nod, lr=LR[1], weight_decay=WD[1], max_grad_norm=MAXN[1], **kw)]


def _restated(named, moments=None):
    ts = []
    for n, p in named:
        z = torch.zeros_like(p)
        ts.append((n, p.detach(), z, z, 1 if any(nd in n for nd in NO_DECAY) else 0, n))
    ts.sort(key=lambda t: t[4])                 # param_groups order: the tensors of a group are consecutive
    return R.Lamb64(ts, [dict(lr=LR[i], wd=WD[i], max_norm=MAXN[i], step=0) for i in range(2)], R.hyper())


def _batch_args(rcfg):
    from oracle import volta_ref as V
    cb = {k: v.cuda() for k, v in V.synthetic_batch(rcfg, 4, 20, 36, seed=7).items()}
    return (cb["input_ids"], cb["image_feat"], cb["image_loc"], cb["segment_ids"], cb["input_mask"], cb["image_mask"],
            cb["lm_label_ids"], cb["image_label"], cb["image_cls"], None, None, None, None, None, cb["is_match"])


def _index(opt):
    return {id(p): i for i, p in enumerate(q for g in opt.param_groups for q in g["params"])}


def test_three_training_steps_against_the_restatement():
    from volta_amd.optimization import LAMB
    model, rcfg = _model()
    args = _batch_args(rcfg)
    named = list(model.named_parameters())
    opt = LAMB(_groups(named))
    W = _restated(named)
    idx = _index(opt)
    arena = model.materialize()
    for s in range(3):
        sum(model(*args)).sum().backward()
        grads = {n: p.grad.detach().clone() for n, p in named if p.grad is not None}
        assert len(grads) > 20
        gbits = arena.grad.clone()
        opt.step()
        W.step(grads)
        assert torch.equal(arena.grad.view(torch.int32), gbits.view(torch.int32))           # .grad keeps its bits (apex overwrites it)
        assert torch.equal(arena.shadow, arena.master.bfloat16()) and arena.shadow_version == arena.param_version()
        tr = opt.trust_ratios()
        assert set(tr) == set(grads)
        worst = 0.0
        for n, p in named:
            m, v = opt._moments(idx[id(p)])
            worst = max(worst, W.excess(n, p.detach(), m, v))
        for n in grads:
            w = W.last[n]
            worst = max(worst, R.ratio(tr[n][0], w["trust"], w["Etrust"]), R.ratio(tr[n][1], w["pn"], w["Epn"]), R.ratio(tr[n][2], w["un"], w["Eun"]))
        assert worst <= 1.0, (s, worst)
        qkv = [n for n in grads if ".attention_self." in n and n.endswith("weight") and n.rsplit(".", 2)[1] in ("query", "key", "value")]
        slots = {}
        for n in qkv:
            slots.setdefault(n.rsplit(".", 2)[0], []).append(tr[n][0])
        assert slots and all(len(r) == 3 and len(set(r)) == 3 for r in slots.values()), slots   # three tensors of one slot, three ratios
        opt.zero_grad()
        assert all(p.grad is None for _, p in named)                                          # set_grad_none is the default
    assert [g["step"] for g in opt.param_groups] == [3, 3]


def _seeded_run(steps, first=0, sd_model=None, sd_opt=None, clip=None, nograd=NOGRAD):
    """Seeded gradients written into the arena (the same for every run), an lr that changes every step.  Yields after each step."""
    from volta_amd.optimization import LAMB, clip_grad_norm_
    model, _ = _model(sd_model)
    arena = model.materialize()
    arena.refresh_shadow()
    named = list(model.named_parameters())
    opt = LAMB(_groups(named))
    if sd_opt is not None:
        opt.load_state_dict(sd_opt)
    for s in range(first, steps):
        g = torch.Generator(device="cuda").manual_seed(100 + s)
        arena.grad.copy_(torch.randn(arena.total, generator=g, device="cuda") * 0.01)
        for n, p in named:
            p.grad = None if n.startswith(nograd) else arena.view(n, "grad")
        if clip is not None:
            opt._fused is None and opt._setup()
            clip_grad_norm_(model.parameters(), 0.5, defer_to_optimizer=clip == "deferred")
            assert (arena.pending_clip is not None) == (clip == "deferred")
        for gi, grp in enumerate(opt.param_groups):
            grp["lr"] = LR[gi] * (s + 1) / 3
        opt.step()
        assert arena.pending_clip is None
        yield s, model, arena, opt, named
        opt.zero_grad()


def test_state_dict_round_trip_continues_bit_identically():
    """state_dict() after two steps loaded into a fresh model's fresh optimizer: the third step leaves the bits of the uninterrupted run.
    The layout is apex's: the step count in the param group, exp_avg / exp_avg_sq per parameter that has stepped."""
    for s, model, arena, opt, named in _seeded_run(3):
        if s == 1:
            sd_opt = copy.deepcopy(opt.state_dict())
            sd_model = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    idx = _index(opt)
    final = (arena.master.clone(), opt._fused["m"].clone(), opt._fused["v"].clone())
    assert [g["step"] for g in sd_opt["param_groups"]] == [2, 2]
    for n, p in named:
        i = idx[id(p)]
        assert (i in sd_opt["state"]) == (not n.startswith(NOGRAD)), n
        if i in sd_opt["state"]:
            assert sorted(sd_opt["state"][i]) == ["exp_avg", "exp_avg_sq"] and sd_opt["state"][i]["exp_avg"].shape == p.shape
    for s, model2, arena2, opt2, named2 in _seeded_run(3, first=2, sd_model=sd_model, sd_opt=sd_opt):
        pass
    assert [g["step"] for g in opt2.param_groups] == [3, 3]
    for a, b in zip(final, (arena2.master, opt2._fused["m"], opt2._fused["v"])):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_deferred_clip_equals_eager_scaling():
    """clip_grad_norm_ then step(): the coefficient folded into the step (deferred) and gradients scaled in place first (eager) leave the
    same bits.  The clip brings the norm to 0.5, under this optimizer's own max_grad_norm of 1: its divisor is 1 both times."""
    runs = {}
    for mode in ("deferred", "eager"):
        for s, model, arena, opt, named in _seeded_run(2, clip=mode):
            pass
        runs[mode] = (arena.master.clone(), opt._fused["m"].clone(), opt._fused["v"].clone(), arena.shadow.clone())
    for a, b in zip(runs["deferred"], runs["eager"]):
        assert torch.equal(a, b)
    for s, model, arena, opt, named in _seeded_run(2):
        pass
    assert not torch.equal(arena.master, runs["eager"][0])                                    # and the clip did something


def test_parameters_without_a_gradient_are_skipped():
    for s, model, arena, opt, named in _seeded_run(2):
        if s == 0:
            pass
    idx = _index(opt)
    ref, _ = _model()
    fresh = dict(ref.named_parameters())
    tr = opt.trust_ratios()
    skipped = [n for n, _ in named if n.startswith(NOGRAD)]
    assert skipped
    for n, p in named:
        m, v = opt._moments(idx[id(p)])
        if n in skipped:
            assert torch.equal(p.detach(), fresh[n].detach()) and not m.any() and not v.any() and n not in tr
            assert torch.equal(arena.view(n, "shadow"), p.detach().bfloat16())
        else:
            assert n in tr and not torch.equal(p.detach(), fresh[n].detach()), n
    assert sorted(opt.state_dict()["state"]) == sorted(idx[id(p)] for n, p in named if n not in skipped)


def test_zero1_is_refused_by_name():
    from volta_amd.optimization import LAMB
    model, _ = _model()
    model.materialize()
    named = list(model.named_parameters())
    opt = LAMB(_groups(named))
    model.__dict__["_ddp"] = types.SimpleNamespace(reducer=types.SimpleNamespace(mode="zero1", sharded=[], replicated=[]))
    try:
        for n, p in named:
            p.grad = model._arena.view(n, "grad")
        before = model._arena.master.clone()
        with pytest.raises(NotImplementedError, match="zero1.*'allreduce' or 'rs_ag'"):
            opt.step()
        with pytest.raises(NotImplementedError, match="zero1.*'allreduce' or 'rs_ag'"):
            LAMB(_groups(named))
        assert torch.equal(before, model._arena.master)
        model.__dict__["_ddp"] = types.SimpleNamespace(reducer=types.SimpleNamespace(mode="rs_ag", sharded=[], replicated=[]))
        opt.step()                                                                            # every rank holds the averaged gradient
        assert not torch.equal(before, model._arena.master)
    finally:
        model.__dict__["_ddp"] = None


def test_backbone_with_a_torch_head_steps_both():
    """A standalone BertModel with a torch head: one step() updates arena views and the head's tensors through the same table."""
    from test_backbone_gpu import _call, _setup
    from oracle import volta_ref as V
    from volta_amd.optimization import LAMB
    model, rcfg, _, _ = _setup("uniter")
    model.eval()
    cb = {k: v.cuda() for k, v in V.synthetic_batch(rcfg, 4, 20, 36, seed=9, pad=True).items()}
    head = nn.Sequential(nn.Linear(rcfg.pooler_size, 64), nn.GELU(), nn.Linear(64, 7))
    gen = torch.Generator().manual_seed(0)      # a generator of its own: the global seed is the engine's dropout seed, other tests' business
    with torch.no_grad():
        for q in head.parameters():
            q.copy_(torch.randn(q.shape, generator=gen) * 0.05)
    head = head.cuda()
    named = [("bert." + n, p) for n, p in model.named_parameters()] + [("head." + n, p) for n, p in head.named_parameters()]
    opt = LAMB(_groups(named))
    W = _restated(named)
    idx = _index(opt)
    for _ in range(2):
        opt.zero_grad()
        _, _, pt, pv, _ = _call(model, cb)
        nn.functional.cross_entropy(head(pt * pv), torch.arange(4, device="cuda") % 7).backward()
        grads = {n: p.grad.detach().clone() for n, p in named if p.grad is not None}
        hbits = {n: grads[n].clone() for n in grads if n.startswith("head.")}
        opt.step()
        W.step(grads)
        tr = opt.trust_ratios()
        worst = max(W.excess(n, p.detach(), *opt._moments(idx[id(p)])) for n, p in named)
        assert worst <= 1.0, worst
        for n, p in named:
            if n in grads:
                key = n if n.startswith("bert.") else idx[id(p)]                              # tensors outside the arena report by position
                key = n[len("bert."):] if key not in tr and isinstance(key, str) else key
                w = W.last[n]
                assert R.ratio(tr[key][0], w["trust"], w["Etrust"]) <= 1.0, n
        assert all(torch.equal(dict(named)[n].grad, hbits[n]) for n in hbits)
    assert len([k for k in tr if isinstance(k, int)]) == 4 and opt._fused["arena"] is not None
