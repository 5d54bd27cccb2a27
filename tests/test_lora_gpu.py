"""LoRA adapters end to end on the engine (volta_amd/lora.py), tiny configs and shape of tests/test_engine_gpu.py.

1  lora_B = 0 changes nothing, to the bit; lora_A.grad is exactly zero and lora_B.grad is s dqkv^T T within the fp32 bound of
   tests/lora_restate.py (checked where the engine's buffers still hold dqkv after the backward: the lowest attention sub-layer -- every
   attention sub-layer of these configs shares one set of backward temporaries).
2  Random lora_B with |s B A| between 0.1 and 0.5 of |W|: the engine against the oracle fed the merged fp32 weights W + s B A, autograd
   through the merge giving the adapter gradients.  Gates of tests/test_engine_gpu.py: states 2e-2, gradients 4e-2 / cosine 0.999,
   query and key (weights and adapters) 0.1 / 0.995.
3  mark_only_lora_trainable: adapter and head gradients keep the bits of the nothing-frozen run.
4  AdamW over the trainable parameters only.   5  merge_lora on the GPU.   6  RetrievalScorer on a model with adapters.
Also: a second backward without zero_grad doubles the adapter gradients, as it does every arena gradient."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lora_restate as LR  # noqa: E402

SEED = 0xABCDEF12345
SHAPE = (4, 20, 36)


def _pretrain(name, lora_kw=None, seed=2):
    from test_engine_gpu import build
    from oracle import volta_ref as R
    from volta_amd import lora
    model, rcfg, sd = build(name, seed=seed)
    if lora_kw is not None:
        lora.add_lora(model, **lora_kw)
    batch = R.synthetic_batch(rcfg, *SHAPE, seed=7, pad=True)
    cb = {k: v.cuda() for k, v in batch.items()}
    args = (cb["input_ids"], cb["image_feat"], cb["image_loc"], cb["segment_ids"], cb["input_mask"], cb["image_mask"],
            cb["lm_label_ids"], cb["image_label"], cb["image_cls"], None, None, None, None, None, cb["is_match"])
    return model, rcfg, sd, batch, args


def _randomise_B(model, ratio=0.3, seed=11):
    """lora_B ~ N(0, 1), scaled per adapter so that |s B A|_F = ratio |W|_F; returns the ratios."""
    from volta_amd import lora
    s = lora.lora_scale(model)
    gen = torch.Generator().manual_seed(seed)
    out = {}
    with torch.no_grad():
        for name, h in lora._adapted(model):
            Bm = torch.randn(h.lora_B.shape, generator=gen)
            A, W = h.lora_A.detach().cpu().double(), h.weight.detach().cpu().double()
            Bm = Bm * float(ratio * W.norm() / (s * (Bm.double() @ A)).norm())
            h.lora_B.copy_(Bm.to(h.lora_B.device))
            out[name] = float((s * (h.lora_B.detach().cpu().double() @ A)).norm() / W.norm())
    return out


def _grads(model):
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}


def _zero(model):
    for p in model.parameters():
        p.grad = None


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", ["vilbert", "uniter"])
def test_zero_lora_B_changes_nothing(name):
    kw = dict(r=8, alpha=16, targets=("query", "key", "value") if name == "uniter" else ("query", "value"))
    plain, _, _, _, args = _pretrain(name)
    model, _, _, _, _ = _pretrain(name, kw)
    outs = {}
    for train in (False, True):
        for tag, m in (("plain", plain), ("lora", model)):
            m.train(train)
            m.set_dropout_seed(SEED)
            _zero(m)
            losses = m(*args)
            sum(losses[:2]).sum().backward()                 # the MLM and region losses: their gradients do not read the atomically summed loss values
            torch.cuda.synchronize()
            eng = m._last[0]
            outs[tag] = ({k: t.clone() for k, t in eng.taps.items() if t is not None}, _grads(m), eng, [float(x.detach()) for x in losses])
        (taps_p, grads_p, _, loss_p), (taps_l, grads_l, eng, loss_l) = outs["plain"], outs["lora"]
        # the loss kernels sum their rows with float atomics: two runs of ONE model differ in the last bits of a loss, so "equal" is equality up
        # to that reordering, as in tests/test_frozen_backward_gpu.py (LOSS_RTOL, derived there); everything else is compared bit for bit
        assert all((a != a and b != b) or abs(a - b) <= 144 * 2.0 ** -24 * abs(b) for a, b in zip(loss_l, loss_p)), (train, loss_l, loss_p)
        for k, t in taps_p.items():
            assert torch.equal(t, taps_l[k]), (train, k)
        for k, g in grads_p.items():
            assert (g is None and grads_l[k] is None) or torch.equal(g, grads_l[k]), (train, k)
        adapters = [k for k in grads_l if ".lora_" in k]
        assert adapters and all(grads_l[k] is not None for k in adapters)
        for k in adapters:
            g = grads_l[k]
            assert torch.isfinite(g).all(), k
            if k.endswith("lora_A"):
                assert float(g.abs().max()) == 0.0, k
            else:
                assert float(g.abs().max()) > 0.0, k
        # lora_B.grad of the lowest attention sub-layer against s dqkv^T T from the buffers the backward left behind
        Ha = model.config.hidden_size
        dqkv = LR.bf16_value(eng.bufs["dqkv0_0"].view(torch.int16).cpu().numpy().view(np.uint16))
        checked = 0
        for c, t in enumerate(("query", "key", "value")):
            key = "bert.encoder.layer.0.attention_self.%s.lora_B" % t
            if key not in grads_l:
                continue
            srcs = [(dqkv[:, c * Ha:(c + 1) * Ha], LR.bf16_value(eng.bufs["L0_loraT0%d" % c].view(torch.int16).cpu().numpy().view(np.uint16)), 2.0)]
            if name == "uniter":                             # the shared adapter also sums the vision rows
                dq1 = LR.bf16_value(eng.bufs["dqkv1_0"].view(torch.int16).cpu().numpy().view(np.uint16))
                srcs.append((dq1[:, c * Ha:(c + 1) * Ha], LR.bf16_value(eng.bufs["L0_loraT1%d" % c].view(torch.int16).cpu().numpy().view(np.uint16)), 2.0))
            ref, e = LR.ref_dB(srcs)
            assert LR.worst_f32(grads_l[key].cpu().numpy(), ref, e) <= 1.0, key
            checked += 1
        assert checked >= 2


def test_adapter_gradients_accumulate_like_any_arena_gradient():
    """A second backward without zero_grad adds up (tests/test_engine_gpu.py::test_grad_accumulation_and_state_dict_roundtrip, with adapters)."""
    model, _, _, _, args = _pretrain("gated", dict(r=4, alpha=8, targets=("query", "key", "value")))
    _randomise_B(model)
    model.eval()
    step = lambda: sum(model(*args)).sum().backward()
    step()
    g1 = _grads(model)
    step()
    torch.cuda.synchronize()
    n = 0
    for k, p in model.named_parameters():
        assert torch.allclose(p.grad, 2 * g1[k], rtol=1e-4, atol=1e-6), k
        n += ".lora_" in k and float(g1[k].abs().max()) > 0
    assert n == 12                                             # q, k, v on both streams of the one attention sub-layer, A and B


# ---------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("name,targets", [("vilbert", ("query", "value")), ("uniter", ("query", "key", "value"))])
def test_engine_against_oracle_with_merged_weights(name, targets):
    from oracle import volta_ref as R
    from test_engine_gpu import rel_err
    from volta_amd import lora
    model, rcfg, sd, batch, args = _pretrain(name, dict(r=8, alpha=16, targets=targets))
    ratios = _randomise_B(model)
    assert ratios and all(0.1 <= v <= 0.5 for v in ratios.values()), ratios
    s = lora.lora_scale(model)
    model.train()
    model.set_dropout_seed(SEED)
    lm, img, nsp = model(*args)
    torch.cuda.synchronize()
    eng = model._last[0]
    aliases = R.param_aliases(rcfg)
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k not in aliases}
    ad = {n: p.detach().cpu().clone().requires_grad_(True) for n, p in model.named_parameters() if ".lora_" in n}
    full = dict(leaves)
    for n in ad:
        if n.endswith(".lora_A"):
            stem = n[:-len(".lora_A")]
            full[stem + ".weight"] = leaves[stem + ".weight"] + s * (ad[stem + ".lora_B"] @ ad[n])
    for a, t in aliases.items():
        full[a] = full[t]
    taps = {}
    olm, oimg, onsp = R.forward_from_batch(full, rcfg, batch, train=True, philox_seed=SEED, taps=taps)
    seen = 0
    for key, ref in taps.items():
        if key not in eng.taps or ref is None or ref.dim() < 2:
            continue
        e = rel_err(eng.taps[key].float().cpu().view(ref.shape), ref.detach())
        assert e < 2e-2, (name, key, e)
        seen += 1
    assert seen >= 8
    for got, ref, nm in ((lm, olm, "lm"), (img, oimg, "img")):
        g, r = float(got.detach()), float(ref.detach())
        assert abs(g - r) <= 1e-3 * max(abs(r), 1e-3) + 1e-4, (name, nm, g, r)
    (lm + img).sum().backward()
    (olm + oimg).sum().backward()
    torch.cuda.synchronize()
    named = dict(model.named_parameters())
    bad, n_ad = [], 0
    for k, leaf in list(leaves.items()) + list(ad.items()):
        g_ref = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
        assert named[k].grad is not None, k                  # no adapter (and no base parameter) is skipped
        g_got = named[k].grad.float().cpu()
        assert torch.isfinite(g_got).all(), k
        if float(g_ref.norm()) < 1e-6:
            assert ".lora_" not in k, (k, "an adapter with a zero reference gradient checks nothing")
            if float(g_got.norm()) > 5e-3:
                bad.append((k, "expected ~0", float(g_got.norm())))
            continue
        e = rel_err(g_got, g_ref)
        cos = float((g_got * g_ref).sum() / (g_got.norm() * g_ref.norm()))
        qk = "query." in k or "key." in k
        if e > (0.1 if qk else 4e-2) or cos < (0.995 if qk else 0.999):
            bad.append((k, e, cos, float(g_ref.norm())))
        n_ad += ".lora_" in k
    assert not bad, (name, bad[:12], len(bad))
    assert n_ad == len(ad) > 0


# ---------------------------------------------------------------------------------------------- 3, 4, 5
def _tasks_model(r=8):
    import test_frozen_backward_gpu as FB
    from volta_amd import lora
    model, loss_fn = FB._tasks("vilbert", "TASK1")
    lora.add_lora(model, r=r, alpha=16)
    _randomise_B(model)
    return model, loss_fn, FB


def test_only_lora_trainable_keeps_the_bits():
    from volta_amd import lora
    model, loss_fn, FB = _tasks_model()
    FB._step(model, loss_fn, 77)                             # nothing frozen
    ref = _grads(model)
    keep = [n for n in ref if ref[n] is not None and (".lora_" in n or n.startswith("clfs_dict."))]
    assert sum(".lora_" in n for n in keep) == 24 and len(keep) > 24
    _zero(model)
    lora.mark_only_lora_trainable(model, also=("clfs_dict.",))
    runs = []
    for _ in range(2):
        _zero(model)
        FB._step(model, loss_fn, 77)
        runs.append(_grads(model))
    eng = model._last[0]
    assert eng.pruned and eng.frozen
    named = dict(model.named_parameters())
    for n, g in runs[0].items():
        if n in keep:
            assert torch.equal(g, ref[n]), n                 # the bits of the nothing-frozen run
            assert torch.equal(g, runs[1][n]), n             # and of the same step once more
        elif not named[n].requires_grad:
            assert g is None, n
    arena = model._arena
    assert all(float(arena.view(n, "grad").abs().max()) == 0.0 for n in eng.pruned)
    assert not any(".lora_" in n for n in eng.pruned)


def test_adamw_moves_only_the_trainable_parameters():
    from volta_amd import lora
    from volta_amd.optimization import AdamW
    model, loss_fn, FB = _tasks_model()
    lora.mark_only_lora_trainable(model, also=("clfs_dict.",))
    model.materialize()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    opt = AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    losses = []
    for step in range(3):
        opt.zero_grad()
        losses.append(FB._step(model, loss_fn, 100 + step))
        opt.step()
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in losses), losses
    for n, p in model.named_parameters():
        if ".lora_" in n:
            assert not torch.equal(p.detach(), before[n]), n
        elif not p.requires_grad:
            assert torch.equal(p.detach(), before[n]), n


def test_merge_on_the_gpu():
    """The reference's keys again, eval predictions within rel_err 2e-2 of those before, and the next plan has no LoRA op."""
    from test_engine_gpu import rel_err, CONFIGS
    from test_tasks_gpu import TASK_CFG
    from oracle import volta_ref as R
    from volta_amd import _lib as L, lora
    model, _, FB = _tasks_model()
    model.eval()
    rcfg = R.RefConfig(dict(CONFIGS["vilbert"], clf_hidden_size=1536))
    cb = {k: v.cuda() for k, v in R.synthetic_batch(rcfg, *SHAPE, seed=9, pad=True).items()}
    call = lambda: model(cb["input_ids"], cb["image_feat"], cb["image_loc"], "TASK1", cb["segment_ids"], cb["input_mask"], cb["image_mask"])[0].detach().float().clone()
    has = lambda: any(o[0] == L.OP_GENERIC and o[4].fn == L.FN_LORA_FWD for o in model._last[0].fwd.ops)
    plain_keys = {k for k in model.state_dict() if ".lora_" not in k}
    with torch.no_grad():
        pre = call()
        assert has()
        lora.merge_lora(model)
        assert set(model.state_dict()) == plain_keys == set(R.make_task_weights(rcfg, TASK_CFG, list(TASK_CFG), seed=4, std=0.04))
        post = call()
        assert not has()
    assert rel_err(post, pre) < 2e-2 and TASK_CFG["TASK1"]["num_labels"] == pre.shape[-1]


# ---------------------------------------------------------------------------------------------- 6
def test_retrieval_scorer_with_adapters():
    import test_retrieval_gpu as RT
    from volta_amd import lora
    from volta_amd.retrieval import RetrievalScorer
    model = RT._tiny("vilbert", zero_shot=False)
    lora.add_lora(model, r=8, alpha=16)
    _randomise_B(model)
    caps, imgs = RT._inputs(model.config, 5, 7, 20, 37, seed=11)
    want = RT._loop(model, caps, imgs)
    for chunk in (4, 1000):
        _, S, Lg = RT._score(model, caps, imgs, chunk)
        RT._check(S, Lg, want, False, ("lora", chunk))
    uni = RT._tiny("uniter", zero_shot=False)                # the e4m3 path covers the single-width geometry: refused for the adapters, not the widths
    lora.add_lora(uni, r=8, alpha=16)
    with pytest.raises(NotImplementedError, match="LoRA"):
        sc = RetrievalScorer(uni, "TASK8", pair_chunk=16, projection_dtype="fp8")
        c, i = RT._inputs(uni.config, 2, 2, 20, 37, seed=3)
        sc.score_matrix(sc.encode_captions(*c), sc.encode_images(*i))
