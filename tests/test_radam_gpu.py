"""Fused RAdam / PlainRAdam (csrc/radam.hip, volta_amd.optimization) on the GPU against the reference's recorded run
(tests/golden/radam_reference.npz) and the float64 restatement (tests/radam_restate.py).

Gates: Restated.excess() <= 1 means every weight / moment lies within 2x the first-order fp32 error bound derived in
tests/radam_restate.py -- a bound for ANY fp32 evaluation of the element function, so the kernel, the reference and the restatement's
exact value must all agree to it.  Where two runs of the SAME kernel on the same inputs are compared the gate is bit equality."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from radam_restate import Restated  # noqa: E402

Z = np.load(os.path.join(HERE, "golden", "radam_reference.npz"))
N = len([k for k in Z.files if k.startswith("init_")])
NO_DECAY = ["bias", "LayerNorm.bias", "LayerNorm.weight"]


def _lrs(s):
    return [float(Z["base_lr"][i] * Z["lr_factor"][s]) for i in range(N)]


def _fixture_opt(cls, params):
    return cls([{"params": [p], "lr": float(Z["base_lr"][i]), "weight_decay": float(Z["wd"][i])} for i, p in enumerate(params)],
               lr=float(Z["base_lr"][0]))


def _fixture_steps(opt, params, first, last):
    for s in range(first, last):
        for i, g in enumerate(opt.param_groups):
            g["lr"] = _lrs(s)[i]
        for i, p in enumerate(params):
            p.grad = torch.from_numpy(Z["grad_%d" % i][s]).cuda() if Z["live"][s][i] else None
        opt.step()
        yield s


def _moments(opt, params):
    sd = opt.state_dict()["state"]
    return [(sd[i]["exp_avg"], sd[i]["exp_avg_sq"]) if i in sd else (torch.zeros_like(p), torch.zeros_like(p)) for i, p in enumerate(params)]


@pytest.mark.parametrize("tag", ["radam", "plain"])
def test_list_kernel_replays_the_reference(tag):
    """The fixture's six tensors as tensors outside any arena (vk_radam_step_list): weights and moments against the reference's values at
    every step, within the gate; the step counts and state_dict layout at the end equal the reference's."""
    from volta_amd.optimization import PlainRAdam, RAdam
    cls = RAdam if tag == "radam" else PlainRAdam
    params = [torch.from_numpy(Z["init_%d" % i]).cuda().requires_grad_(True) for i in range(N)]
    opt = _fixture_opt(cls, params)
    R = Restated([torch.from_numpy(Z["init_%d" % i]) for i in range(N)], plain=tag == "plain")
    wrong = Restated([torch.from_numpy(Z["init_%d" % i]) for i in range(N)], plain=tag == "plain", decay_after=True)
    worst, worst_wrong = 0.0, 0.0
    for s in _fixture_steps(opt, params, 0, int(Z["steps"])):
        grads = [torch.from_numpy(Z["grad_%d" % i][s]) if Z["live"][s][i] else None for i in range(N)]
        R.step(grads, _lrs(s), list(Z["wd"]))
        wrong.step(grads, _lrs(s), list(Z["wd"]))
        mv = _moments(opt, params)
        for i, p in enumerate(params):
            want = [torch.from_numpy(Z["%s_%s_%d" % (tag, k, i)][s]) for k in "pmv"]
            got = [p.detach().cpu(), mv[i][0].cpu(), mv[i][1].cpu()]
            worst = max(worst, R.excess(i, *got))
            worst_wrong = max(worst_wrong, wrong.excess(i, *got))
            assert float((got[0] - want[0]).abs().max()) <= 4 * float(R.Ep[i].max()) + 1e-30, (s, i)
    assert worst <= 1.0, worst
    assert worst_wrong > 10.0, worst_wrong             # decay after the update fails the gate
    sd = opt.state_dict()
    np.testing.assert_array_equal([sd["state"][i]["step"] for i in range(N)], Z["%s_sd_end_step" % tag])
    if tag == "radam":
        got = np.array([[np.nan if x is None else float(x) for x in b] for b in opt.buffer])
        np.testing.assert_array_equal(got, Z["radam_buffer"][-1])


@pytest.mark.parametrize("tag", ["radam", "plain"])
def test_loading_the_reference_state_dict_continues_to_its_values(tag):
    """The reference's mid-point state_dict (uneven step counts, one tensor without an entry) loaded into a fresh optimizer continues to
    the values the reference's own resumed run reaches (its buffer restarts empty, as after the reference's load)."""
    from volta_amd.optimization import PlainRAdam, RAdam
    cls = RAdam if tag == "radam" else PlainRAdam
    mid = int(Z["mid"])
    params = [torch.from_numpy(Z["%s_p_%d" % (tag, i)][mid - 1]).cuda().requires_grad_(True) for i in range(N)]
    opt = _fixture_opt(cls, params)
    steps = [int(x) for x in Z["%s_sd_mid_step" % tag]]
    ms = [torch.from_numpy(Z["%s_sd_mid_m_%d" % (tag, i)]) for i in range(N)]
    vs = [torch.from_numpy(Z["%s_sd_mid_v_%d" % (tag, i)]) for i in range(N)]
    opt.load_state_dict({"state": {i: {"step": steps[i], "exp_avg": ms[i], "exp_avg_sq": vs[i]} for i in range(N) if steps[i] > 0},
                         "param_groups": opt.state_dict()["param_groups"]})
    R = Restated([p.detach().cpu() for p in params], plain=tag == "plain")
    R.load([p.detach().cpu() for p in params], steps, ms, vs)
    worst = 0.0
    for k, s in enumerate(_fixture_steps(opt, params, mid, int(Z["steps"]))):
        R.step([torch.from_numpy(Z["grad_%d" % i][s]) if Z["live"][s][i] else None for i in range(N)], _lrs(s), list(Z["wd"]))
        for i, p in enumerate(params):
            worst = max(worst, R.excess(i, p.detach().cpu()))
            want = torch.from_numpy(Z["%s_resumed_p_%d" % (tag, i)][k])
            assert float((p.detach().cpu() - want).abs().max()) <= 4 * float(R.Ep[i].max()) + 1e-30, (s, i)
    assert worst <= 1.0, worst


def _task_model(seed=4):
    from test_engine_gpu import CONFIGS
    from oracle import volta_ref as R
    from volta_amd.config import BertConfig
    from volta_amd.modeling import BertForVLTasks
    cd = dict(CONFIGS["gated"], clf_hidden_size=256)
    task_cfg = {"TASK1": {"type": "VL-classifier", "num_labels": 5}}
    rcfg = R.RefConfig(cd)
    model = BertForVLTasks(BertConfig.from_dict(cd), task_cfg, ["TASK1"])
    model.load_state_dict(R.make_task_weights(rcfg, task_cfg, ["TASK1"], seed=seed, std=0.04), strict=True)
    return model, rcfg


def _train_task_groups(named):
    """train_task.py:208-219: one group per trainable parameter, 1e-4 for "vil_" keys (here also the task head, so that the small model has
    two lrs), no decay for biases and LayerNorms."""
    return [{"params": [p], "lr": 1e-4 if "vil_" in n or "clfs_dict" in n else 2e-5, "weight_decay": 0.0 if any(nd in n for nd in NO_DECAY) else 0.01}
            for n, p in named if p.requires_grad]


FROZEN = "bert.v_embeddings."          # a fixed_layers entry (volta/train_utils.py:250-255)
NOGRAD = "bert.t_pooler."              # a parameter the loss does not reach


def _arena_run(cls, steps, seed=0, clip=None):
    """The small gated task model with train_task-style groups and a hand-set lr schedule; seeded gradients written into the arena.  Yields
    (step, model, arena, optimizer, named parameters, gradients) once before the first step (step -1, gradients None) and after each."""
    from volta_amd.optimization import clip_grad_norm_
    model, _ = _task_model()
    model = model.cuda()
    for n, p in model.named_parameters():
        p.requires_grad_(not n.startswith(FROZEN))
    arena = model.materialize()
    named = list(model.named_parameters())
    groups = _train_task_groups(named)
    opt = cls(groups, lr=2e-5)
    bases = [grp["lr"] for grp in opt.param_groups]
    g = torch.Generator(device="cuda").manual_seed(seed)
    live = [(n, p) for n, p in named if p.requires_grad]
    yield -1, model, arena, opt, named, None
    for s in range(steps):
        grads = {}
        for n, p in live:
            if n.startswith(NOGRAD):
                p.grad = None
                continue
            gv = arena.view(n, "grad")
            gv.copy_(torch.randn(p.shape, generator=g, device="cuda") * (100.0 if s == 3 else 0.01))
            p.grad = gv
            grads[n] = gv.clone()
        if clip == "deferred":
            clip_grad_norm_(model.parameters(), 1.0, defer_to_optimizer=True)
        elif clip == "eager":
            clip_grad_norm_(model.parameters(), 1.0, defer_to_optimizer=False)
        elif clip == "torch":
            torch.nn.utils.clip_grad_norm_([p for _, p in live], 1.0)
        for grp, b in zip(opt.param_groups, bases):
            grp["lr"] = b * (s + 1) / steps
        opt.step()
        yield s, model, arena, opt, named, grads
        opt.zero_grad()


@pytest.mark.parametrize("name", ["RAdam", "PlainRAdam"])
def test_arena_kernel_against_the_restatement(name):
    """12 steps over the arena: results within the gate of the float64 restatement (per-parameter lrs, decay / no decay, a large-gradient
    step); frozen and gradient-less parameters keep bit-identical weights, moments and bf16 copies and have no state entry; after every
    step the bf16 copy equals bf16(master) and the shadow is marked fresh."""
    import volta_amd.optimization as O
    cls = getattr(O, name)
    for s, model, arena, opt, named, grads in _arena_run(cls, 12):
        tr = [(n, p) for n, p in named if p.requires_grad]
        if s < 0:
            arena.refresh_shadow()
            before = {n: p.detach().clone() for n, p in named if n.startswith(FROZEN) or n.startswith(NOGRAD)}
            sh_before = {n: arena.view(n, "shadow").clone() for n in before}
            R = Restated([p.detach() for _, p in tr], plain=name == "PlainRAdam")
            # the plausible mistake: RAdam with each group's own lr, PlainRAdam with RAdam's shared buffer (the first group's lr); decay
            # after the update is invisible at these lrs (2e-7 of a 2e-5 step is below fp32 resolution): the fixture tests gate that one
            wrong = Restated([p.detach() for _, p in tr], plain=False, own_lr=name == "RAdam")
            continue
        lrs = [grp["lr"] for grp in opt.param_groups]
        wds = [grp["weight_decay"] for grp in opt.param_groups]
        gl = [grads.get(n) for n, _ in tr]
        R.step(gl, lrs, wds)
        wrong.step(gl, lrs, wds)
        f = opt._fused
        worst = max(R.excess(i, p.detach(), f["m"][arena.offset[n]:arena.offset[n] + p.numel()].view(p.shape),
                             f["v"][arena.offset[n]:arena.offset[n] + p.numel()].view(p.shape)) for i, (n, p) in enumerate(tr))
        assert worst <= 1.0, (s, worst)
        assert torch.equal(arena.shadow, arena.master.bfloat16())
        assert arena.shadow_version == arena.param_version()
    assert max(wrong.excess(i, p.detach()) for i, (n, p) in enumerate(tr)) > 10.0
    for n, p in named:
        if n in before:
            o = arena.offset[n]
            assert torch.equal(p.detach(), before[n]) and torch.equal(arena.view(n, "shadow"), sh_before[n]), n
            assert not f["m"][o:o + p.numel()].any() and not f["v"][o:o + p.numel()].any(), n
    idx = {id(p): i for i, p in enumerate(q for grp in opt.param_groups for q in grp["params"])}
    sd = opt.state_dict()["state"]
    for n, p in tr:
        assert (idx[id(p)] in sd) == (not n.startswith(NOGRAD)), n
    assert all(sd[i]["step"] == 12 for i in sd)


def test_deferred_eager_and_torch_clip():
    """Deferred and eager clip_grad_norm_ give bit-identical weights and moments; torch.nn.utils.clip_grad_norm_ (train_task.py:283) then
    step() agrees with the restatement given the clipped gradients; two identical runs are bit-identical."""
    from volta_amd.optimization import RAdam
    runs = {}
    for mode in ("deferred", "eager", "deferred2"):
        for s, model, arena, opt, named, grads in _arena_run(RAdam, 4, clip=mode.rstrip("2")):
            pass
        runs[mode] = (arena.master.clone(), opt._fused["m"].clone(), opt._fused["v"].clone())
    for a, b, c in zip(runs["deferred"], runs["eager"], runs["deferred2"]):
        assert torch.equal(a, b) and torch.equal(a, c)
    for s, model, arena, opt, named, grads in _arena_run(RAdam, 4, clip="torch"):
        tr = [(n, p) for n, p in named if p.requires_grad]
        if s < 0:
            R = Restated([p.detach() for _, p in tr])
            continue
        # the arena gradients were clipped in place by torch: the restatement takes them as they are
        R.step([arena.view(n, "grad").clone() if n in grads else None for n, _ in tr], [g["lr"] for g in opt.param_groups],
               [g["weight_decay"] for g in opt.param_groups])
        assert max(R.excess(i, p.detach()) for i, (n, p) in enumerate(tr)) <= 1.0


def test_checkpoint_round_trip_is_bit_identical():
    """Saved at step 3 and restored into a fresh model and optimizer, the run continues bit-identically to step 6 (uniform step counts)."""
    from volta_amd.optimization import RAdam
    it = _arena_run(RAdam, 6)
    for s, model, arena, opt, named, grads in it:
        if s == 2:
            sd_opt = copy.deepcopy(opt.state_dict())
            sd_model = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
            buf = copy.deepcopy(opt.buffer)
    final = arena.master.clone()
    # replay: same seeded gradients for steps 3..5 into a restored model
    model2, _ = _task_model()
    model2.load_state_dict(sd_model)
    model2 = model2.cuda()
    for n, p in model2.named_parameters():
        p.requires_grad_(not n.startswith(FROZEN))
    arena2 = model2.materialize()
    named2 = list(model2.named_parameters())
    groups2 = _train_task_groups(named2)
    bases = [grp["lr"] for grp in groups2]
    opt2 = RAdam(groups2, lr=2e-5)
    opt2.load_state_dict(sd_opt)
    # the buffer restarts empty, as after the reference's load; with uniform step counts every slot a later step reads is refilled first
    assert opt2.buffer == [[None, None, None]] * 10 and buf != opt2.buffer
    g = torch.Generator(device="cuda").manual_seed(0)
    live = [(n, p) for n, p in named2 if p.requires_grad]
    for s in range(6):
        for n, p in live:
            if n.startswith(NOGRAD):
                p.grad = None
                continue
            gv = torch.randn(p.shape, generator=g, device="cuda") * (100.0 if s == 3 else 0.01)
            if s >= 3:
                arena2.view(n, "grad").copy_(gv)
                p.grad = arena2.view(n, "grad")
        if s >= 3:
            for grp, b in zip(opt2.param_groups, bases):
                grp["lr"] = b * (s + 1) / 6
            opt2.step()
            opt2.zero_grad()
    assert torch.equal(arena2.master, final)


def test_train_task_sequence_end_to_end():
    """train_task.py:204-290 in order: CPU model, RAdam over train_task groups, WarmupConstantSchedule, load_state_dict, model.to(cuda),
    the optimizer.state .cuda() loop, then forward / cross-entropy / backward / torch clip / step / scheduler / model.zero_grad."""
    from oracle import volta_ref as R
    from volta_amd.optimization import RAdam, WarmupConstantSchedule
    model, rcfg = _task_model()
    named = list(model.named_parameters())
    opt = RAdam(_train_task_groups(named), lr=2e-5)
    sched = WarmupConstantSchedule(opt, warmup_steps=2)
    g = torch.Generator().manual_seed(1)
    state = {i: {"step": 3, "exp_avg": torch.randn(p.shape, generator=g) * 1e-3, "exp_avg_sq": torch.rand(p.shape, generator=g) * 1e-6}
             for i, (_, p) in enumerate(named)}
    opt.load_state_dict({"state": state, "param_groups": opt.state_dict()["param_groups"]})
    model.to("cuda")
    for st in opt.state.values():
        for k, v in st.items():
            if torch.is_tensor(v):
                st[k] = v.cuda()
    model.train()
    batch = R.synthetic_batch(rcfg, 8, 20, 36, seed=9, pad=True)
    cb = {k: v.cuda() for k, v in batch.items()}
    target = torch.arange(8, device="cuda") % 5
    watch = {n: p.detach().clone() for n, p in named if n in ("bert.encoder.layer.0.attention_self.query.weight", "bert.t_pooler.dense.weight",
                                                              "clfs_dict.TASK1.logit_fc.3.weight")}
    assert len(watch) == 3, sorted(n for n, _ in named)[-8:]
    losses = []
    for _ in range(5):
        pred = model(cb["input_ids"], cb["image_feat"], cb["image_loc"], "TASK1", cb["segment_ids"], cb["input_mask"], cb["image_mask"])[0]
        loss = nn.functional.cross_entropy(pred, target)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
        sched.step()
        model.zero_grad()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0], losses
    steps = {s["step"] for s in opt.state_dict()["state"].values()}
    assert 8 in steps and steps <= {3, 8}, steps
    d = dict(named)
    for n, w in watch.items():
        assert not torch.equal(d[n].detach(), w), n


def test_backbone_with_a_torch_head_steps_arena_and_list_in_one_step():
    """A standalone BertModel with a torch head: one RAdam step updates the arena (vk_radam_step) and the head (vk_radam_step_list) as the
    restatement does."""
    from test_backbone_gpu import _call, _setup
    from oracle import volta_ref as R
    from volta_amd.optimization import RAdam
    model, rcfg, _, _ = _setup("uniter")
    model.eval()
    cb = {k: v.cuda() for k, v in R.synthetic_batch(rcfg, 4, 20, 36, seed=9, pad=True).items()}
    torch.manual_seed(0)
    vil_head = nn.Sequential(nn.Linear(rcfg.pooler_size, 64), nn.GELU(), nn.Linear(64, 7)).cuda()
    named = [("bert." + n, p) for n, p in model.named_parameters()] + [("vil_head." + n, p) for n, p in vil_head.named_parameters()]
    opt = RAdam(_train_task_groups(named), lr=2e-5)
    Rs = Restated([p.detach() for _, p in named])
    for _ in range(2):
        opt.zero_grad()
        _, _, pt, pv, _ = _call(model, cb)
        nn.functional.cross_entropy(vil_head(pt * pv), torch.arange(4, device="cuda") % 7).backward()
        grads = [p.grad.detach().clone() if p.grad is not None else None for _, p in named]
        opt.step()
        Rs.step(grads, [g["lr"] for g in opt.param_groups], [g["weight_decay"] for g in opt.param_groups])
        assert max(Rs.excess(i, p.detach()) for i, (_, p) in enumerate(named)) <= 1.0
    assert opt._fused["arena"] is not None and opt._fused.get("flist_key") and len(opt._fused["flist_key"]) == 4


def test_full_size_arena():
    """ctrl_vilbert_base (242 M arena elements), 7 steps crossing rectification at step 6: every parameter against the float64
    restatement run on the device -- catches chunk and class indexing over the whole arena."""
    from volta_amd.config import BertConfig
    from volta_amd.modeling import BertForVLPreTraining
    from volta_amd.optimization import RAdam
    cfg = BertConfig.from_json_file(os.path.join(os.path.dirname(HERE), "config", "ctrl_vilbert_base.json"))
    model = BertForVLPreTraining(cfg).cuda()
    arena = model.materialize()
    named = list(model.named_parameters())
    opt = RAdam(_train_task_groups(named), lr=2e-5)
    Rs = Restated([p.detach() for _, p in named])
    g = torch.Generator(device="cuda").manual_seed(5)
    for s in range(7):
        arena.grad.normal_(generator=g).mul_(0.01)
        for n, p in named:
            p.grad = arena.view(n, "grad")
        opt.step()
        Rs.step([arena.view(n, "grad") for n, _ in named], [x["lr"] for x in opt.param_groups], [x["weight_decay"] for x in opt.param_groups])
        assert [r for r in Rs.last if r is not None][0][1] == (s + 1 >= 6)
        worst = max(Rs.excess(i, p.detach()) for i, (_, p) in enumerate(named))
        assert worst <= 1.0, (s, worst)
    assert torch.equal(arena.shadow, arena.master.bfloat16())
