"""Frozen parameters end to end: a model whose backward list is pruned to what its trainable parameters need (requires_grad False ->
StepEngine(frozen=...)) against the same model with nothing frozen.  Two models from one state_dict, the same dropout seed and batch.

The property is equality of bits: what a trainable parameter's gradient sums, and in which order, does not depend on what else is
frozen, so every comparison is torch.equal.  Frozen sets a-g of tests/test_frozen_plan_cpu.py on ViLBERT, a and d on UNITER (one
embedding prefix for both modalities); the pre-training model, a BertForVLTasks and a standalone BertModel under a torch head.  Every
frozen model first runs one step with nothing frozen, so that the gradient ranges the pruned list leaves alone held non-zero values."""
import os
import sys

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SEED = 77
SHAPE = (4, 20, 36)
# The loss kernels add their rows' terms to one fp32 accumulator with atomics (csrc/heads.hip), in the order the rows happen to finish:
# two runs of one unfrozen model already differ in the last bits of a loss.  The forward list is the same list under every frozen set,
# so "equal losses" is equality up to that reordering: at most B * max(T, Rv) = 144 terms of one sign per accumulator, whose fp32 sum
# moves by less than (terms - 1) * 2^-24 relative under any order.  (The gradients do not read the loss values and are compared exactly.)
LOSS_RTOL = 144 * 2.0 ** -24


def _same_loss(a, b):
    return abs(a - b) <= LOSS_RTOL * abs(b)


def _plan_helpers():
    import test_frozen_plan_cpu as P
    return P


def _pretrain(name):
    from test_engine_gpu import build
    from oracle import volta_ref as R
    model, rcfg, _ = build(name)
    batch = R.synthetic_batch(rcfg, *SHAPE, seed=7, pad=True)
    cb = {k: v.cuda() for k, v in batch.items()}
    args = (cb["input_ids"], cb["image_feat"], cb["image_loc"], cb["segment_ids"], cb["input_mask"], cb["image_mask"],
            cb["lm_label_ids"], cb["image_label"], cb["image_cls"], None, None, None, None, None, cb["is_match"])
    model.train()
    return model, lambda: sum(model(*args)).sum()


def _tasks(name, task):
    from test_engine_gpu import CONFIGS
    from test_tasks_gpu import TASK_CFG
    from oracle import volta_ref as R
    from volta_amd.config import BertConfig
    from volta_amd.modeling import BertForVLTasks
    cd = dict(CONFIGS[name], clf_hidden_size=1536)
    rcfg = R.RefConfig(cd)
    ids = list(TASK_CFG)
    sd = R.make_task_weights(rcfg, TASK_CFG, ids, seed=4, std=0.04)
    model = BertForVLTasks(BertConfig.from_dict(cd), TASK_CFG, ids)
    model.load_state_dict(sd, strict=True)
    model = model.cuda().train()
    batch = R.synthetic_batch(rcfg, *SHAPE, seed=9, pad=True)
    cb = {k: v.cuda() for k, v in batch.items()}
    probe = {}

    def loss():
        pred = model(cb["input_ids"], cb["image_feat"], cb["image_loc"], task, cb["segment_ids"], cb["input_mask"], cb["image_mask"])[0]
        if "w" not in probe:
            probe["w"] = torch.randn(pred.shape, generator=torch.Generator().manual_seed(5)).cuda()
        return (pred * probe["w"]).sum()
    return model, loss


class _Backbone(nn.Module):
    """The torch head of a standalone BertModel, as tests/test_backbone_gpu.py trains one."""

    def __init__(self, bert):
        super().__init__()
        torch.manual_seed(3)
        self.head_t = nn.Linear(bert.config.pooler_size, 5).cuda()
        self.head_v = nn.Linear(bert.config.v_hidden_size, 1).cuda()


def _backbone(name):
    from test_backbone_gpu import _setup, _call
    from oracle import volta_ref as R
    bert, rcfg, _, _ = _setup(name)
    bert.train()
    wrap = _Backbone(bert)
    batch = R.synthetic_batch(rcfg, *SHAPE, seed=9, pad=True)
    cb = {k: v.cuda() for k, v in batch.items()}

    def loss():
        seq_t, seq_v, pooled_t, pooled_v, _ = _call(bert, cb)
        return wrap.head_t(pooled_t).square().sum() + wrap.head_v(seq_v).sum() + seq_t.mean()
    bert.__dict__["_head"] = wrap          # keeps the head alive with the model, outside its parameters
    return bert, loss


MAKERS = {"pretrain": _pretrain, "tasks": lambda name: _tasks(name, "TASK1"), "backbone": _backbone}


def _arena_names(model):
    """{arena name: Parameter}"""
    return dict(model.materialize().param_list())


def _freeze(model, case):
    """Applies frozen set `case`; returns (frozen arena names, names of the blocks frozen as a whole)."""
    P = _plan_helpers()
    arena = model.materialize()
    frozen = P.frozen_set(model.config, arena, case)
    for n, p in arena.param_list():
        p.requires_grad_(n not in frozen)
    return frozen, P.fully_frozen(arena, model._heads_mode, frozen)


def _unfreeze(model):
    for p in model.parameters():
        p.requires_grad_(True)


def _zero(model):
    for p in model.parameters():
        p.grad = None


def _step(model, loss_fn, seed=None):
    if seed is not None:
        model.set_dropout_seed(seed)
    loss = loss_fn()
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach())


def _grads(model):
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in _arena_names(model).items()}


_REF = {}


def _reference(kind, name):
    """The never-frozen model's losses and gradients of two consecutive steps (seeds SEED, SEED + 1) and of their accumulation: once per model."""
    key = (kind, name)
    if key not in _REF:
        model, loss_fn = MAKERS[kind](name)
        l1 = _step(model, loss_fn, SEED)
        g1 = _grads(model)
        _zero(model)
        l2 = _step(model, loss_fn)
        g2 = _grads(model)
        _zero(model)
        _step(model, loss_fn, SEED)
        _step(model, loss_fn)
        acc = _grads(model)
        _REF[key] = dict(l1=l1, g1=g1, l2=l2, g2=g2, acc=acc)
        del model, loss_fn
    return _REF[key]


def _compare(model, frozen, whole, want, tag):
    arena = model.materialize()
    unused = model._last[0].unused_params
    bad = []
    for n, p in arena.param_list():
        if n in frozen:
            assert p.grad is None, (tag, n)
        elif want[n] is None:
            assert p.grad is None or n in unused, (tag, n)
        elif not torch.equal(p.grad, want[n]):
            bad.append((n, float((p.grad - want[n]).abs().max())))
    assert not bad, (tag, bad[:6], len(bad))
    dirty = [n for n in sorted(whole) if n not in unused and bool(arena.view(n, "grad").any())]
    assert not dirty, (tag, "frozen blocks hold gradients", dirty[:6])


CASES = [("pretrain", "vilbert", c) for c in "abcdefg"] + [("pretrain", "uniter", c) for c in "ad"] + \
        [("tasks", "vilbert", c) for c in "acd"] + [("backbone", "vilbert", c) for c in "ac"]


@pytest.mark.parametrize("kind,name,case", CASES)
def test_frozen_step_equals_unfrozen(kind, name, case):
    """Loss, every trainable gradient and the zeroed frozen blocks of one step; the step before it ran unfrozen and left gradients everywhere."""
    ref = _reference(kind, name)
    model, loss_fn = MAKERS[kind](name)
    _step(model, loss_fn, SEED)
    assert bool(model.materialize().grad.any())
    _zero(model)
    frozen, whole = _freeze(model, case)
    got = _step(model, loss_fn, SEED)
    assert _same_loss(got, ref["l1"]), (got, ref["l1"])
    _compare(model, frozen, whole, ref["g1"], (kind, name, case))
    eng = model._last[0]
    assert (case == "g") == (not eng.frozen)
    if case != "g":
        assert whole and set(whole) - set(eng.unused_params) <= eng.pruned


@pytest.mark.parametrize("kind,name,case", [("pretrain", "vilbert", "c"), ("tasks", "vilbert", "b")])
def test_accumulation_under_a_frozen_set(kind, name, case):
    """Two micro-steps: the trainable gradients are the unfrozen model's accumulated ones, the frozen blocks stay zero."""
    ref = _reference(kind, name)
    model, loss_fn = MAKERS[kind](name)
    _step(model, loss_fn, SEED)
    _zero(model)
    frozen, whole = _freeze(model, case)
    _step(model, loss_fn, SEED)
    _step(model, loss_fn)
    _compare(model, frozen, whole, ref["acc"], (kind, name, case, "accumulated"))


def test_freeze_step_unfreeze_step():
    """Flipping requires_grad between steps selects the matching plan; back to nothing frozen, the step is the never-frozen model's second step."""
    ref = _reference("pretrain", "vilbert")
    model, loss_fn = _pretrain("vilbert")
    frozen, whole = _freeze(model, "c")
    assert _same_loss(_step(model, loss_fn, SEED), ref["l1"])
    pruned_plan = model._last[0]
    assert pruned_plan.frozen
    _compare(model, frozen, whole, ref["g1"], "frozen step")
    _zero(model)
    _unfreeze(model)
    assert _same_loss(_step(model, loss_fn), ref["l2"])
    assert not model._last[0].frozen and model._last[0] is not pruned_plan
    _compare(model, set(), set(), ref["g2"], "after the unfreeze")
    assert sum(1 for k in model._engines if k[3]) == 1          # one plan per mode, as before


def test_ddp_single_rank_and_zero1():
    """One step under DistributedDataParallel on a single-rank group leaves the gradients of the plain pruned backward: one mark per
    stage, so the buckets stand as they are.  mode="zero1" with a pruned plan is refused."""
    import torch.distributed as dist
    from volta_amd.parallel import DistributedDataParallel
    ref = _reference("pretrain", "vilbert")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29571")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        model, loss_fn = _pretrain("vilbert")
        frozen, whole = _freeze(model, "b")
        ddp = DistributedDataParallel(model, message_size=2000000)
        _step(model, loss_fn, SEED)
        assert len(ddp._plan(model._last[0])) >= 3, "expected several buckets"
        _compare(model, frozen, whole, ref["g1"], "ddp")
        _zero(model)
        DistributedDataParallel(model, message_size=2000000, mode="zero1")
        model.set_dropout_seed(SEED)
        with pytest.raises(NotImplementedError, match="frozen"):
            loss_fn().backward()
    finally:
        dist.destroy_process_group()


def test_adamw_and_clip_over_the_trainable_parameters():
    """Norm and updated weights are those of the unfrozen model's step restricted to the trainable parameters; frozen weights do not move."""
    from volta_amd.optimization import AdamW, clip_grad_norm_
    out = {}
    for which in ("unfrozen", "frozen"):
        model, loss_fn = _pretrain("vilbert")
        if which == "frozen":
            frozen, _ = _freeze(model, "c")
        _step(model, loss_fn, SEED)
        if which == "unfrozen":          # the same step, restricted afterwards: the frozen set's parameters lose their gradient and leave the optimizer
            frozen, _ = _freeze(model, "c")
            for n, p in model.materialize().param_list():
                if n in frozen:
                    p.grad = None
        before = {n: p.detach().clone() for n, p in model.materialize().param_list()}
        opt = AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3, weight_decay=0.01)
        norm = float(clip_grad_norm_(model.parameters(), 1e-2))
        opt.step()
        torch.cuda.synchronize()
        after = {n: p.detach().clone() for n, p in model.materialize().param_list()}
        assert all(torch.equal(after[n], before[n]) for n in frozen)
        assert any(not torch.equal(after[n], before[n]) for n in after if n not in frozen)
        out[which] = (norm, after)
    assert out["frozen"][0] == out["unfrozen"][0], (out["frozen"][0], out["unfrozen"][0])
    diff = [n for n in out["frozen"][1] if not torch.equal(out["frozen"][1][n], out["unfrozen"][1][n])]
    assert not diff, diff[:6]
