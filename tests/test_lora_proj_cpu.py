"""The LoRA targets attn_out, ffn_up and ffn_down on the CPU (volta_amd/lora.py): the public interface and the plans a
model with such adapters builds -- plans build without a GPU; helpers of tests/test_lora_cpu.py and tests/test_frozen_plan_cpu.py."""
import ctypes
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_frozen_plan_cpu as F  # noqa: E402
import test_lora_cpu as T0  # noqa: E402  (make, arena_of, engine)

S = F.S
SHAPE = T0.SHAPE
NEW = ("attn_out", "ffn_up", "ffn_down")
HOLDER = {"attn_out": "attention_output", "ffn_up": "intermediate", "ffn_down": "output"}


@pytest.fixture(scope="module")
def matrix():
    yield S.Matrix()


def proj_ops(plan, fn):
    from volta_amd import _lib as L
    return [i for i, o in enumerate(plan.ops) if o[0] == L.OP_GENERIC and o[4].fn == fn]


def problems(eng, g):
    from volta_amd import _lib as L
    arr = next(k for k in eng.keep if isinstance(k, ctypes.Array) and k._type_ in (L.LoraProjProblem, L.LoraProjBwdProblem) and ctypes.addressof(k) == g.p[0])
    assert len(arr) == g.n[0]
    return list(arr)


def widths(cfg, target, vision):
    H, I = (cfg.v_hidden_size, cfg.v_intermediate_size) if vision else (cfg.hidden_size, cfg.intermediate_size)
    return {"attn_out": (H, H), "ffn_up": (H, I), "ffn_down": (I, H)}[target]


# ---------------------------------------------------------------------------------------------- the public interface
def test_targets_and_defaults():
    import inspect
    from volta_amd import lora
    assert lora.TARGETS == ("query", "key", "value", "attn_out", "ffn_up", "ffn_down")
    assert inspect.signature(lora.add_lora).parameters["targets"].default == ("query", "value")


@pytest.mark.parametrize("target", NEW)
def test_names_shapes_dtypes_vilbert(matrix, target):
    from volta_amd import lora
    from volta_amd.modules import sublayer_schedule
    model = T0.make(matrix, "vilbert")
    cfg = model.config
    before = set(model.state_dict())
    names = lora.add_lora(model, r=8, alpha=16, targets=(target,), seed=3)
    kind = "attn" if target == "attn_out" else "ff"
    hosts = [n for n, typ in sublayer_schedule(cfg) if typ == kind]
    assert model.lora_config == dict(r=8, alpha=16.0, targets=[target], modalities=["text", "vision"], sublayers=hosts)
    want = []
    for n in hosts:
        node = model.bert.encoder.layer[n]._modules[HOLDER[target]]
        for v in ("", "v_"):
            if v + "dense" in node._modules:
                want += ["bert.encoder.layer.%d.%s.%sdense.lora_%s" % (n, HOLDER[target], v, ab) for ab in "AB"]
    assert names == want and any(".v_dense." in n for n in names) and any(".dense." in n for n in names)
    params = dict(model.named_parameters())
    assert set(names) == {n for n in params if n.endswith((".lora_A", ".lora_B"))}
    assert set(model.state_dict()) == before | set(names)
    for n in names:
        p = params[n]
        fin, fout = widths(cfg, target, ".v_dense." in n)
        assert p.dtype == torch.float32 and p.requires_grad and p._vk_owner is model
        assert tuple(p.shape) == ((8, fin) if n.endswith("lora_A") else (fout, 8)), n
        if n.endswith("lora_B"):
            assert float(p.detach().abs().max()) == 0.0
        else:
            bound = 1.0 / math.sqrt(fin)
            assert 0.9 * bound < float(p.detach().abs().max()) <= bound
    assert set(lora.lora_state_dict(model)) == set(names)


def test_shared_holders_get_one_adapter_uniter_and_standalone_bert(matrix):
    from volta_amd import lora
    model = T0.make(matrix, "uniter", "tasks")
    names = lora.add_lora(model, r=16, alpha=32, targets=NEW)
    assert names and not any(".v_" in n for n in names)
    n_sub = len(model.bert.encoder.layer)
    assert len(names) == 2 * (n_sub // 2) + 4 * (n_sub // 2)          # per attention sub-layer one adapter, per feed-forward sub-layer two; (A, B) each
    ff = next(l for l in model.bert.encoder.layer if "intermediate" in l._modules)
    assert ff.intermediate.v_dense is ff.intermediate.dense and ff.output.v_dense.lora_A is ff.output.dense.lora_A
    assert set(names) == {n for n, _ in model.named_parameters() if ".lora_" in n}
    sd = model.state_dict()
    assert all(n.replace(".dense.", ".v_dense.") in sd for n in names)          # the alias, as for the weights
    back = T0.make(matrix, "vilbert", "backbone")                               # a standalone BertModel is a root model too
    got = lora.add_lora(back, r=8, targets=NEW)
    assert got[0] == "encoder.layer.0.attention_output.dense.lora_A" and "encoder.layer.1.intermediate.dense.lora_A" in got
    arena = T0.arena_of(back)
    assert all("bert." + n in arena.params for n in got)


def test_seeded_draws_of_the_old_targets_do_not_move(matrix):
    """The rule in holder order: old targets alone draw what they drew before there were new ones (restated here from the rule); with new
    targets added, the holders of the first sub-layer -- Q, K, V of both streams come first -- still draw the same values."""
    from volta_amd import lora
    old = T0.make(matrix, "vilbert")
    names = lora.add_lora(old, r=8, targets=("query", "value"), seed=5)
    gen = torch.Generator().manual_seed(5)
    params = dict(old.named_parameters())
    for n in names:
        if n.endswith("lora_A"):
            fin = params[n].shape[1]
            want = (torch.rand(8, fin, generator=gen, dtype=torch.float32) * 2.0 - 1.0) * (1.0 / math.sqrt(fin))
            assert torch.equal(params[n].detach(), want), n
    assert names[0] == "bert.encoder.layer.0.attention_self.query.lora_A" and [n for n in names if ".layer.2." in n][:2] == [
        "bert.encoder.layer.2.attention_self.query.lora_A", "bert.encoder.layer.2.attention_self.query.lora_B"]
    both = T0.make(matrix, "vilbert")
    names2 = lora.add_lora(both, r=8, targets=("query", "value") + NEW, seed=5)
    p2 = dict(both.named_parameters())
    first = [n for n in names if ".layer.0." in n]
    assert names2[:len(first)] == first and all(torch.equal(p2[n].detach(), params[n].detach()) for n in first)
    # within a sub-layer the new holders come behind q, k, v of both streams; an attention sub-layer before the feed-forward one behind it
    order = [n for n in names2 if n.endswith("lora_A")]
    at = lambda frag: next(i for i, n in enumerate(order) if frag in n)
    assert at("layer.2.attention_self.v_value") < at("layer.2.attention_output.dense") < at("layer.2.attention_output.v_dense") < at("layer.3.intermediate.dense")
    assert at("layer.3.intermediate.dense") < at("layer.3.output.dense") < at("layer.3.intermediate.v_dense") < at("layer.3.output.v_dense") < at("layer.4.attention_self.query")


def test_sublayers_semantics_and_errors(matrix):
    from volta_amd import lora
    model = T0.make(matrix, "vilbert")
    with pytest.raises(ValueError):
        lora.add_lora(model, sublayers=[1])                                 # default targets: a feed-forward sub-layer hosts none of them
    with pytest.raises(ValueError):
        lora.add_lora(model, targets=("query",), sublayers=[1])
    with pytest.raises(ValueError):
        lora.add_lora(model, targets=("ffn_up",), sublayers=[0])
    with pytest.raises(ValueError):
        lora.add_lora(model, targets=("ffn_up", "ffn_down"), sublayers=[1, 2])      # any listed index that hosts none
    with pytest.raises(ValueError):
        lora.add_lora(model, targets=("query", "dense"))
    assert model.lora_config is None and not [n for n, _ in model.named_parameters() if "lora" in n]
    names = lora.add_lora(model, r=4, targets=("ffn_up",), sublayers=[1])
    assert names == ["bert.encoder.layer.1.intermediate.dense.lora_A", "bert.encoder.layer.1.intermediate.dense.lora_B"]
    assert model.lora_config["sublayers"] == [1]
    lora.remove_lora(model)
    names = lora.add_lora(model, r=4, targets=("value", "ffn_down"), sublayers=[2, 3])          # indices of either kind
    assert {n.split(".")[3] for n in names} == {"2", "3"} and model.lora_config["sublayers"] == [2, 3]
    lora.remove_lora(model)
    lora.add_lora(model)                                                     # the default dict is what it was
    assert model.lora_config == dict(r=8, alpha=16.0, targets=["query", "value"], modalities=["text", "vision"], sublayers=[0, 2, 4, 6])
    assert list(model.lora_config) == ["r", "alpha", "targets", "modalities", "sublayers"]


def test_merge_and_remove(matrix):
    from volta_amd import lora
    model = T0.make(matrix, "vilbert")
    before = {k: v.clone() for k, v in model.state_dict().items()}
    r, alpha = 8, 16
    names = lora.add_lora(model, r=r, alpha=alpha, targets=NEW)
    gen = torch.Generator().manual_seed(5)
    params = dict(model.named_parameters())
    with torch.no_grad():
        for n in names:
            if n.endswith("lora_B"):
                params[n].copy_(torch.randn(params[n].shape, generator=gen) * 0.05)
    s = alpha / r
    want = {}
    for n in names:
        if n.endswith("lora_A"):
            stem = n[:-len(".lora_A")]
            W, A, Bm = before[stem + ".weight"].double(), params[n].detach().double(), params[stem + ".lora_B"].detach().double()
            want[stem + ".weight"] = (W + s * (Bm @ A), 2.0 ** -23 * (W.abs() + (r + 2) * s * (Bm.abs() @ A.abs())))
    assert {k.split(".")[4] for k in want} == set(HOLDER.values())
    lora.merge_lora(model)
    after = model.state_dict()
    assert set(after) == set(before) and model.lora_config is None
    for k, v in after.items():
        if k in want:
            ref, bound = want[k]
            assert bool(((v.double() - ref).abs() <= bound).all()), k
            assert not torch.equal(v, before[k])
        else:
            assert torch.equal(v, before[k]), k
    lora.add_lora(model, r=4, targets=NEW)                   # a merged model takes adapters again
    mid = {k: v.clone() for k, v in model.state_dict().items() if ".lora_" not in k}
    lora.mark_only_lora_trainable(model)
    assert all(p.requires_grad == (".lora_" in n) for n, p in model.named_parameters())
    lora.load_lora_state_dict(model, {k: v + 1.0 for k, v in lora.lora_state_dict(model).items()})
    lora.remove_lora(model)
    assert set(model.state_dict()) == set(before) and all(torch.equal(model.state_dict()[k], v) for k, v in mid.items())
    with pytest.raises(RuntimeError):
        lora.remove_lora(model)


def test_fp8_refuses_feed_forward_adapters(matrix):
    from volta_amd import lora
    from volta_amd.engine import StepEngine
    from volta_amd.retrieval import split_plan
    model = T0.make(matrix, "uniter")
    lora.add_lora(model, targets=("ffn_down",))
    arena = T0.arena_of(model)
    B, T, Rv = SHAPE
    with pytest.raises(NotImplementedError, match="LoRA.*fp8"):
        StepEngine(model.config, arena, B, T, Rv, True, fp8=True)
    with pytest.raises(NotImplementedError, match="LoRA.*fp8"):
        StepEngine(model.config, arena, B, T, Rv, False, heads="score", part="pair", split=split_plan(model.config), projection_dtype="fp8")
    lora.remove_lora(model)
    lora.add_lora(model, targets=("attn_out",))
    with pytest.raises(NotImplementedError, match="LoRA.*fp8"):
        StepEngine(model.config, T0.arena_of(model), B, T, Rv, True, fp8=True)


# ---------------------------------------------------------------------------------------------- plans
def _kinds(ops):
    from volta_amd import _lib as L
    return [(o[0], o[4].fn if o[0] == L.OP_GENERIC else None, o[2] if o[0] == L.OP_GEMM else None) for o in ops]


def test_plans_without_the_new_adapters_keep_their_op_lists(matrix):
    """No adapters: the committed plan signatures (tests/test_lora_cpu.py runs the whole check).  Q / V adapters: no whole-projection op.
    attn_out + ffn_down: the adapter-less lists plus the new ops; ffn_up swaps that stream's GELU launch for a plain one plus its op."""
    from volta_amd import _lib as L, lora
    model = T0.make(matrix, "vilbert")
    plain = T0.engine(model, T0.arena_of(model))
    lora.add_lora(model, r=8)
    qv = T0.engine(model, T0.arena_of(model))
    assert not proj_ops(qv.fwd, L.FN_LORA_PROJ_FWD) and not proj_ops(qv.bwd, L.FN_LORA_PROJ_BWD)
    lora.remove_lora(model)
    lora.add_lora(model, r=8, targets=("attn_out", "ffn_down"))
    eng = T0.engine(model, T0.arena_of(model))
    text, unresolved = S.render(eng)
    assert unresolved == 0
    for a, b, fn in ((eng.fwd.ops, plain.fwd.ops, L.FN_LORA_PROJ_FWD), (eng.bwd.ops, plain.bwd.ops, L.FN_LORA_PROJ_BWD)):
        mine = [k for k in _kinds(a) if k[1] != fn]
        assert mine == _kinds(b) and len(a) - len(mine) == 8                  # one op per sub-layer and direction
    lora.remove_lora(model)
    lora.add_lora(model, r=8, targets=("ffn_up",), modalities=("text",), sublayers=[3])
    eng = T0.engine(model, T0.arena_of(model))
    at = proj_ops(eng.fwd, L.FN_LORA_PROJ_FWD)
    assert len(at) == 1
    gelu, bf16 = eng.fwd.ops[at[0] - 2], eng.fwd.ops[at[0] - 1]               # the vision stream keeps VK_EPI_GELU, in a launch of its own
    assert gelu[0] == bf16[0] == L.OP_GEMM and gelu[2] == L.EPI_GELU and bf16[2] == L.EPI_BF16 and gelu[3] == bf16[3] == 1
    p, = problems(eng, eng.fwd.ops[at[0]][4])
    q = bf16[4][0]
    assert p.act == 1 and p.G and not q.C2 and (p.X, p.Y, p.M, p.K, p.N, p.ldy) == (q.A, q.C, q.M, q.K, q.N, q.ldc) and p.ldg == p.N and p.scale == 2.0
    r = S.Renderer(eng)
    assert r.addr(p.G).startswith("buf:L3_gp0+0") and r.addr(p.Y).startswith("buf:L3_h0+0") and r.addr(p.T).startswith("buf:L3_loraTup0+0")
    assert len(eng.fwd.ops) == len(plain.fwd.ops) + 2
    # forward-only plans share one T per shape
    ev = T0.engine(model, T0.arena_of(model), train=False)
    assert len(proj_ops(ev.fwd, L.FN_LORA_PROJ_FWD)) == 1


def _stage(eng, k):
    """(first, last + 1) backward op index of sub-layer k (stage 0 = heads, then the sub-layers from the last one down)."""
    n_sub = len(eng.sublayer_ids)
    return eng.bwd_marks[n_sub - 1 - k], eng.bwd_marks[n_sub - k]


@pytest.mark.parametrize("family", ["vilbert", "uniter"])
def test_backward_positions_and_pruning(matrix, family):
    from volta_amd import _lib as L, lora
    from volta_amd.modules import sublayer_schedule
    model = T0.make(matrix, family)
    sched = list(sublayer_schedule(model.config))
    lora.add_lora(model, r=8, targets=NEW)
    arena = T0.arena_of(model)
    full = T0.engine(model, arena)
    lora.mark_only_lora_trainable(model)
    pre = model._arena_prefix
    frozen = {pre + n for n, p in model.named_parameters() if not p.requires_grad}
    eng = T0.engine(model, arena, frozen=frozen)
    for e in (full, eng):
        text, unresolved = S.render(e)
        assert unresolved == 0
        r = S.Renderer(e)
        ops = e.bwd.ops
        is_gemm = lambda o, layout, epi: o[0] == L.OP_GEMM and (o[1] & 0xFF) == layout and o[2] == epi
        for k, (n, typ) in enumerate(sched):
            lo, hi = _stage(e, k)
            at = [i for i in proj_ops(e.bwd, L.FN_LORA_PROJ_BWD) if lo <= i < hi]
            first = lambda pred: next((i for i in range(lo, hi) if pred(ops[i])), None)
            if typ == "attn":
                assert len(at) == 1
                attn_bwd = first(lambda o: o[0] == L.OP_ATTN_BWD)
                ps = problems(e, ops[at[0]][4])
                if attn_bwd is None:                         # the lowest sub-layer of the pruned plan: nothing reads dqkv, only dA and dB
                    assert e is eng and k == 0 and all(not p.dX and p.dA and p.dB for p in ps)
                else:                                        # directly behind the dd W_o dgrad, in front of the attention backward
                    assert at[0] < attn_bwd and is_gemm(ops[at[0] - 1], L.NN, L.EPI_BF16)
                    assert {q.C for q in ops[at[0] - 1][4]} == {p.dX for p in ps} and all(not p.R for p in ps)
                assert all(r.addr(p.X).startswith("buf:L%d_ctx" % n) and r.addr(p.dY).startswith("buf:dd") for p in ps)
            else:
                assert len(at) == 2                          # down, then up
                d1, d2 = first(lambda o: is_gemm(o, L.NN, L.EPI_MULR)), first(lambda o: is_gemm(o, L.NN, L.EPI_ADDR))
                side = first(lambda o: o[0] == L.OP_SIDE_BEGIN)
                assert d1 is not None and at[0] == d1 + 1                       # directly behind d1 ...
                assert (side is None or at[0] < side) and (d2 is None or at[0] < d2)          # ... in front of the weight gradients and d2: both read du
                if e is full:
                    assert side is not None and d2 is not None and at[0] < side < d2 < at[1]
                assert d2 is None or at[1] > d2                                 # behind the last dgrad
                down, up = problems(e, ops[at[0]][4]), problems(e, ops[at[1]][4])
                for p in down:
                    assert p.R and p.dX and p.ldr == p.K and r.addr(p.R).startswith("buf:L%d_gp" % n) and r.addr(p.X).startswith("buf:L%d_h" % n)
                    assert r.addr(p.dX).startswith("buf:du") and r.addr(p.dY).startswith("buf:dd")
                    assert p.dX in {q.C for q in ops[d1][4]}
                for p in up:
                    assert not p.R and r.addr(p.dY).startswith("buf:du") and p.N == down[0].K and p.K == down[0].N
                    assert bool(p.dX) == (e is full or k > 0)                  # dxn where the input gradient is live
                    assert not p.dX or r.addr(p.dX).startswith("buf:dx")
        # every adapter's gradient range is written
        writes = F.grad_writes(e)
        for name in arena.params:
            if ".lora_" in name:
                assert writes[4 * arena.offset[name]] >= 1, name
    # the pruned plan: no weight-gradient group at all (every base weight and LayerNorm is frozen), no write into a base parameter's range
    assert not [o for o in eng.bwd.ops if o[0] == L.OP_GEMM and (o[1] & 0xFF) == L.TN] and not F.wgrad_problems(eng)
    assert [o for o in full.bwd.ops if o[0] == L.OP_GEMM and (o[1] & 0xFF) == L.TN]
    off = F.ranges(arena, [n for n in arena.params if ".lora_" not in n and n in frozen and n not in eng.unused_params])
    assert not [o for o in F.grad_writes(eng) if F.inside(o, off)]
    assert len(eng.bwd.ops) < len(full.bwd.ops) and not any(".lora_" in n for n in eng.pruned)
    fwd = lambda t: t[t.index("# forward"):t.index("# backward")]
    assert fwd(S.render(eng)[0]) == fwd(S.render(full)[0])


def test_frozen_adapters_pass_the_gradient_through(matrix):
    """A frozen adapter above a trainable one keeps its share of dX and loses dA / dB; its range reads zero (pruned)."""
    from volta_amd import _lib as L, lora
    model = T0.make(matrix, "vilbert")
    lora.add_lora(model, r=8, targets=NEW, sublayers=[4, 5])
    arena = T0.arena_of(model)
    lora.mark_only_lora_trainable(model)
    frozen = {n for n, p in model.named_parameters() if not p.requires_grad}
    top = {n for n in arena.params if ".lora_" in n and ".layer.5." in n}
    eng = T0.engine(model, arena, frozen=frozen | top)
    per_op = [problems(eng, eng.bwd.ops[i][4]) for i in proj_ops(eng.bwd, L.FN_LORA_PROJ_BWD)]
    assert len(per_op) == 3                                  # sub-layer 5: down, up; sub-layer 4: out
    down, up, out = per_op
    assert all(p.dX and p.R and not p.dA and not p.dB for p in down) and all(p.dX and not p.R and not p.dA and not p.dB for p in up)
    assert all(not p.dX and p.dA and p.dB for p in out)      # nothing trainable below sub-layer 4
    assert top <= eng.pruned and not (eng.pruned & {n for n in arena.params if ".lora_" in n and ".layer.4." in n})
