"""volta_amd.lora on the CPU: the public interface (names, shapes, initialisation, state_dict, merge, errors), the arena's slots, and the
plans a model with adapters builds -- plans build without a GPU, as in tests/test_frozen_plan_cpu.py, whose helpers this module uses."""
import math
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_frozen_plan_cpu as F  # noqa: E402

ROOT = F.ROOT
S = F.S
SHAPE = (S.B, S.T, S.RV)


@pytest.fixture(scope="module")
def matrix():
    yield S.Matrix()


def make(matrix, family, kind="pretrain"):
    from volta_amd import modeling
    from volta_amd.config import BertConfig
    cfg = BertConfig.from_dict(dict(matrix.configs[family], clf_hidden_size=1536))
    if kind == "tasks":
        return modeling.BertForVLTasks(cfg, matrix.task_cfg, list(matrix.task_cfg))
    return (modeling.BertModel if kind == "backbone" else modeling.BertForVLPreTraining)(cfg)


def arena_of(model):
    from volta_amd.engine import ParamArena
    return ParamArena(model, torch.device("cpu"), prefix=model._arena_prefix)


def engine(model, arena, train=True, frozen=None, **kw):
    from volta_amd.engine import StepEngine
    B, T, Rv = SHAPE
    return StepEngine(model.config, arena, B, T, Rv, train, heads=model._heads_mode, frozen=frozen, **kw)


def lora_ops(plan, fn):
    from volta_amd import _lib as L
    return [i for i, o in enumerate(plan.ops) if o[0] == L.OP_GENERIC and o[4].fn == fn]


def problems(eng, g):
    """The problem array behind the generic arguments `g` of a LoRA op."""
    import ctypes
    from volta_amd import _lib as L
    arr = next(k for k in eng.keep if isinstance(k, ctypes.Array) and k._type_ in (L.LoraProblem, L.LoraBwdProblem) and ctypes.addressof(k) == g.p[0])
    assert len(arr) == g.n[0]
    return list(arr)


# ---------------------------------------------------------------------------------------------- the public interface
def test_names_shapes_init_and_state_dict_vilbert(matrix):
    from volta_amd import lora
    model = make(matrix, "vilbert")
    before = set(model.state_dict())
    names = lora.add_lora(model, r=8, alpha=16, seed=3)
    cfg = model.config
    sa = model.bert.encoder.layer[2].attention_self          # a cross-modal sub-layer: own v_* holders
    assert "bert.encoder.layer.2.attention_self.v_query.lora_A" in names and "bert.encoder.layer.2.attention_self.query.lora_B" in names
    assert not any(".key." in n or ".v_key." in n for n in names)
    assert tuple(sa.v_query.lora_A.shape) == (8, cfg.v_hidden_size) and tuple(sa.v_query.lora_B.shape) == (cfg.v_hidden_size, 8)
    assert tuple(sa.value.lora_A.shape) == (8, cfg.hidden_size) and sa.v_query.lora_A is not sa.query.lora_A
    params = dict(model.named_parameters())
    assert set(names) == {n for n in params if n.endswith((".lora_A", ".lora_B"))} and len(names) == len(set(names))
    assert set(model.state_dict()) == before | set(names)
    for n in names:
        p = params[n]
        assert p.dtype == torch.float32 and p.requires_grad and p._vk_owner is model
        p = p.detach()
        if n.endswith("lora_B"):
            assert float(p.abs().max()) == 0.0
        else:
            bound = 1.0 / math.sqrt(p.shape[1])
            assert 0.9 * bound < float(p.abs().max()) <= bound and abs(float(p.mean())) < 0.1 * bound
    assert model.lora_config == dict(r=8, alpha=16.0, targets=["query", "value"], modalities=["text", "vision"], sublayers=[0, 2, 4, 6])
    twin = make(matrix, "vilbert")
    lora.add_lora(twin, r=8, alpha=16, seed=3)
    other = make(matrix, "vilbert")
    lora.add_lora(other, r=8, alpha=16, seed=4)
    a = "bert.encoder.layer.2.attention_self.v_query.lora_A"
    assert torch.equal(dict(twin.named_parameters())[a], params[a]) and not torch.equal(dict(other.named_parameters())[a], params[a])
    # adapter state: strict on the adapter keys, touches nothing else
    sd = lora.lora_state_dict(model)
    assert set(sd) == set(names)
    base = {k: v.clone() for k, v in twin.state_dict().items() if k not in sd}
    lora.load_lora_state_dict(twin, {k: v + 1.0 for k, v in sd.items()})
    assert all(torch.equal(v, sd[k] + 1.0) for k, v in lora.lora_state_dict(twin).items())
    assert all(torch.equal(twin.state_dict()[k], v) for k, v in base.items())
    with pytest.raises(KeyError):
        lora.load_lora_state_dict(twin, {k: v for k, v in list(sd.items())[1:]})
    with pytest.raises(KeyError):
        lora.load_lora_state_dict(twin, dict(sd, **{"bert.encoder.layer.0.attention_self.key.lora_A": torch.zeros(8, 768)}))
    # restricted placement
    part = make(matrix, "vilbert")
    got = lora.add_lora(part, r=4, targets=("key",), modalities=("vision",), sublayers=[2, 6])
    assert got == ["bert.encoder.layer.%d.attention_self.v_key.lora_%s" % (n, ab) for n in (2, 6) for ab in "AB"]


def test_shared_sublayers_get_one_adapter_uniter(matrix):
    from volta_amd import lora
    model = make(matrix, "uniter", "tasks")
    names = lora.add_lora(model, r=16, alpha=32, targets=("query", "key", "value"))
    assert not any(".v_" in n for n in names) and len(names) == 2 * 3 * 2             # two attention sub-layers x q, k, v x (A, B)
    sa = model.bert.encoder.layer[0].attention_self
    assert sa.v_query is sa.query and sa.v_query.lora_A is sa.query.lora_A
    assert set(names) == {n for n, _ in model.named_parameters() if ".lora_" in n}
    assert "bert.encoder.layer.0.attention_self.v_query.lora_A" in model.state_dict()          # the alias, as for the weights
    back = make(matrix, "vilbert", "backbone")                                                # a standalone BertModel is a root model too
    assert lora.add_lora(back, r=8)[0] == "encoder.layer.0.attention_self.query.lora_A"
    assert "bert.encoder.layer.0.attention_self.query.lora_A" in arena_of(back).params


def test_argument_errors(matrix):
    from volta_amd import lora
    model = make(matrix, "vilbert")
    with pytest.raises(ValueError):
        lora.add_lora(model, r=12)
    with pytest.raises(ValueError):
        lora.add_lora(model, targets=("query", "dense"))
    with pytest.raises(ValueError):
        lora.add_lora(model, targets=())
    with pytest.raises(ValueError):
        lora.add_lora(model, sublayers=[1])                     # a feed-forward sub-layer
    assert not [n for n, _ in model.named_parameters() if "lora" in n] and model.lora_config is None
    with pytest.raises(RuntimeError):
        lora.mark_only_lora_trainable(model)
    lora.add_lora(model)
    with pytest.raises(RuntimeError):
        lora.add_lora(model, r=4)


def test_merge_and_remove(matrix):
    from volta_amd import lora
    model = make(matrix, "vilbert")
    before = {k: v.clone() for k, v in model.state_dict().items()}
    r, alpha = 8, 16
    names = lora.add_lora(model, r=r, alpha=alpha)
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
    lora.merge_lora(model)
    after = model.state_dict()
    assert set(after) == set(before) and model.lora_config is None
    for k, v in after.items():
        if k in want:
            ref, bound = want[k]
            assert bool(((v.double() - ref).abs() <= bound).all()), k
            assert not torch.equal(v, before[k])
        elif k.replace(".v_", ".") not in {w.replace(".v_", ".") for w in want}:
            assert torch.equal(v, before[k]), k
    lora.add_lora(model, r=4)                                # a merged model takes adapters again
    mid = {k: v.clone() for k, v in model.state_dict().items() if ".lora_" not in k}
    lora.remove_lora(model)
    assert set(model.state_dict()) == set(before) and all(torch.equal(model.state_dict()[k], v) for k, v in mid.items())
    with pytest.raises(RuntimeError):
        lora.remove_lora(model)


def test_bookkeeping_drops_arena_and_plans(matrix):
    """add / merge / remove drop the arena and every cached plan of the ROOT model, also when called on the nested BertModel."""
    from volta_amd import lora
    model = make(matrix, "vilbert")
    for call in (lambda: lora.add_lora(model.bert), lambda: lora.merge_lora(model.bert), lambda: lora.add_lora(model), lambda: lora.remove_lora(model)):
        model.__dict__["_arena"], model.__dict__["_engines"] = "stale", {"stale": 1}
        call()
        assert model._arena is None and model._engines == {}
    assert model.bert.__dict__.get("lora_config") is None


# ---------------------------------------------------------------------------------------------- arena and blocks
def test_arena_slots_and_frozen_blocks(matrix):
    from volta_amd import lora
    from volta_amd.engine import canonical_frozen, frozen_blocks
    model = make(matrix, "vilbert")
    names = lora.add_lora(model, r=8, targets=("query",))          # key and value without adapters: the Q|K|V grouping must not look for them
    arena = arena_of(model)
    assert arena.lora_scale == 2.0
    H = model.config.hidden_size
    for pre in ("bert.encoder.layer.2.attention_self.", "bert.encoder.layer.2.attention_self.v_"):
        w = arena.span([pre + k + ".weight" for k in ("query", "key", "value")], "master", (3 * H, H))
        b = arena.span([pre + k + ".bias" for k in ("query", "key", "value")], "master", (3 * H,))
        assert tuple(w.shape) == (3 * H, H) and tuple(b.shape) == (3 * H,)
    offs = [arena.offset[n] for n in names]
    assert len(set(offs)) == len(offs) and all(o % 1024 == 0 for o in offs)
    taken = sorted((arena.offset[n], arena.offset[n] + math.prod(arena.shape[n])) for n in arena.params)
    assert all(a[1] <= b[0] for a, b in zip(taken, taken[1:]))
    blocks = frozen_blocks(arena, "pretrain")
    stem = "bert.encoder.layer.2.attention_self.v_query"
    assert [stem + ".lora_A", stem + ".lora_B"] in blocks
    qkv = next(b for b in blocks if stem + ".weight" in b)
    assert len(qkv) == 6 and not any("lora" in n for n in qkv)
    assert canonical_frozen(arena, [stem + ".lora_A"], "pretrain") == frozenset()
    assert canonical_frozen(arena, [stem + ".lora_A", stem + ".lora_B"], "pretrain") == {stem + ".lora_A", stem + ".lora_B"}


# ---------------------------------------------------------------------------------------------- plans
def test_plans_without_adapters_are_unchanged():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "plan_signature.py"), "--check"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]


CASES = [("vilbert", "pretrain", ("query", "value")), ("vilbert", "tasks", ("query", "value")), ("vilbert", "backbone", ("query", "value")),
         ("uniter", "pretrain", ("query", "key", "value"))]


@pytest.mark.parametrize("family,kind,targets", CASES)
def test_adapters_add_one_op_per_sublayer_and_direction(matrix, family, kind, targets):
    from volta_amd import _lib as L, lora
    model = make(matrix, family, kind)
    kw = dict(task=("TASK1", matrix.task_cfg["TASK1"])) if kind == "tasks" else {}
    plain = engine(model, arena_of(model), **kw)
    names = lora.add_lora(model, r=8, targets=targets)
    arena = arena_of(model)
    eng = engine(model, arena, **kw)
    text, unresolved = S.render(eng)
    assert unresolved == 0
    kinds = lambda e: [(o[0], o[4].fn if o[0] == L.OP_GENERIC else None) for o in e.fwd.ops]
    fwd_at = lora_ops(eng.fwd, L.FN_LORA_FWD)
    n_attn = len(model.lora_config["sublayers"])
    assert len(fwd_at) == n_attn == len(lora_ops(eng.bwd, L.FN_LORA_BWD))
    assert [k for i, k in enumerate(kinds(eng)) if i not in fwd_at] == kinds(plain)          # the adapter-less list plus the LoRA ops
    for i in fwd_at:                                                                         # each right behind a Q|K|V launch: N = 3 Ha
        prev = eng.fwd.ops[i - 1]
        assert prev[0] == L.OP_GEMM and (prev[1] & 0xFF) == L.NT and all(q.N == 3 * q.K for q in prev[4])
        cs = {q.C: q for q in prev[4]}
        for p in problems(eng, eng.fwd.ops[i][4]):              # a column block of that launch's output, rows and widths of its stream
            q = next(q for c, q in cs.items() if 0 <= p.Y - c < 2 * q.N)
            assert (p.Y - q.C) % (2 * p.N) == 0 and (p.M, p.K, 3 * p.N, p.ldy, p.X) == (q.M, q.K, q.N, q.ldc, q.A) and p.r == 8 and p.scale == 2.0
    # every adapter's gradient range is written, by exactly one backward op
    writes = F.grad_writes(eng)
    for n in arena.params:
        if ".lora_" in n:
            assert writes[4 * arena.offset[n]] >= 1, n
    base_writes = F.grad_writes(plain)
    assert sum(writes.values()) - sum(base_writes.values()) == sum(writes[4 * arena.offset[n]] for n in arena.params if ".lora_" in n)
    # eval and attention-map plans carry the forward op too
    assert len(lora_ops(engine(model, arena, train=False, **kw).fwd, L.FN_LORA_FWD)) == n_attn
    if kind == "pretrain" and family == "vilbert":
        assert len(lora_ops(engine(model, arena, train=False, attn_maps=True).fwd, L.FN_LORA_FWD)) == n_attn


@pytest.mark.parametrize("family,kind,targets", CASES)
def test_only_lora_trainable_prunes_below_the_lowest_adapter(matrix, family, kind, targets):
    from volta_amd import _lib as L, lora
    from volta_amd.modules import sublayer_schedule
    model = make(matrix, family, kind)
    sched = list(sublayer_schedule(model.config))
    attn = [n for n, typ in sched if typ == "attn"]
    low = attn[1]                                            # adapters from the second attention sub-layer up
    lora.add_lora(model, r=8, targets=targets, sublayers=[n for n in attn if n >= low])
    kw = dict(task=("TASK1", matrix.task_cfg["TASK1"])) if kind == "tasks" else {}
    arena = arena_of(model)
    full = engine(model, arena, **kw)
    lora.mark_only_lora_trainable(model, also=("clfs_dict.",))
    pre = model._arena_prefix
    frozen = {pre + n for n, p in model.named_parameters() if not p.requires_grad}
    assert frozen and all(".lora_" not in n for n in frozen)
    eng = engine(model, arena, frozen=frozen, **kw)
    text, unresolved = S.render(eng)
    assert unresolved == 0
    # no op points into the gradient range of a frozen base parameter
    off = F.ranges(arena, F.fully_frozen(arena, eng.heads, frozen) - set(eng.unused_params))
    writes = F.grad_writes(eng)
    assert not [o for o in writes if F.inside(o, off)]
    for n in arena.params:
        if ".lora_" in n:
            assert writes[4 * arena.offset[n]] >= 1, n
    # nothing of a sub-layer or embedding below the lowest adapted sub-layer remains: the stages behind it are empty
    marks = eng.bwd_marks                                      # stage 0 = heads, then the sub-layers from the last one down, then the embeddings
    k_low = [n for n, _ in sched].index(low)
    stage_of_low = len(sched) - k_low                          # backward stage index of sub-layer `low`
    assert len(set(marks[stage_of_low:])) == 1, marks
    assert marks[stage_of_low] > marks[stage_of_low - 1]
    # every attention backward launch at or above it remains
    count = lambda e, kind_: sum(1 for o in e.bwd.ops if o[0] == kind_)
    below = sum(1 for n in attn if n < low)
    per_sub = count(full, L.OP_ATTN_BWD) // len(attn)
    assert count(eng, L.OP_ATTN_BWD) == count(full, L.OP_ATTN_BWD) - below * per_sub > 0
    assert len(lora_ops(eng.bwd, L.FN_LORA_BWD)) == len(attn) - below == len(lora_ops(full.bwd, L.FN_LORA_BWD))
    # the lowest adapted sub-layer computes no input gradient: its LoRA problems carry no dX
    assert all(not p.dX for p in problems(eng, eng.bwd.ops[lora_ops(eng.bwd, L.FN_LORA_BWD)[-1]][4]))
    # events: pruning orphans no wait (the exemption of test_frozen_plan_cpu: waits that dangle in the unpruned list already)
    base_dangling = {e for _, e in F.events(full)}
    assert all(e in base_dangling for _, e in F.events(eng)), F.events(eng)
    assert eng.bwd.ops[-1][0] == L.OP_JOIN and len(eng.bwd_marks) == len(full.bwd_marks)
    fwd = lambda t: t[t.index("# forward"):t.index("# backward")]
    assert fwd(text) == fwd(S.render(full)[0])


def test_lora_problems_of_a_pruned_plan(matrix):
    """dX only where the input gradient is live; a frozen adapter above a trainable one keeps its share of dX and loses dA / dB."""
    from volta_amd import _lib as L, lora
    model = make(matrix, "vilbert")
    lora.add_lora(model, r=8, sublayers=[4, 6])
    arena = arena_of(model)
    lora.mark_only_lora_trainable(model)
    frozen = {n for n, p in model.named_parameters() if not p.requires_grad}
    top = {n for n in arena.params if ".lora_" in n and ".layer.6." in n}

    per_op = lambda e: [problems(e, e.bwd.ops[i][4]) for i in lora_ops(e.bwd, L.FN_LORA_BWD)]
    eng = engine(model, arena, frozen=frozen)
    low, high = per_op(eng)[::-1]                             # backward order: sub-layer 6 first
    assert all(not p.dX and p.dA and p.dB for p in low)      # sub-layer 4: nothing trainable below it
    assert all(p.dX and p.dA and p.dB for p in high if p.M == S.B * S.T) and len(high) == 4
    eng2 = engine(model, arena, frozen=frozen | top)          # the adapters of sub-layer 6 frozen too
    low2, high2 = per_op(eng2)[::-1]
    assert all(p.dX and not p.dA and not p.dB for p in high2 if p.M == S.B * S.T)
    assert [p.M for p in high2] == [S.B * S.T] * 2          # the vision stream has no trainable parameter upstream: its frozen adapters drop out
    assert top <= eng2.pruned and not (eng2.pruned & {n for n in arena.params if ".lora_" in n and ".layer.4." in n})
    assert [(p.dA, p.dB) for p in low2] == [(p.dA, p.dB) for p in low]


def test_fp8_refuses_adapters(matrix):
    from volta_amd import lora
    from volta_amd.engine import StepEngine
    from volta_amd.retrieval import split_plan
    model = make(matrix, "uniter")
    lora.add_lora(model)
    arena = arena_of(model)
    B, T, Rv = SHAPE
    with pytest.raises(NotImplementedError, match="LoRA.*fp8"):
        StepEngine(model.config, arena, B, T, Rv, True, fp8=True)
    with pytest.raises(NotImplementedError, match="LoRA.*fp8"):
        StepEngine(model.config, arena, B, T, Rv, False, heads="score", part="pair", split=split_plan(model.config), projection_dtype="fp8")
    eng = StepEngine(model.config, arena, B, T, Rv, False, heads="score", part="pair", split=split_plan(model.config), projection_dtype="bf16")
    from volta_amd import _lib as L
    assert len(lora_ops(eng.fwd, L.FN_LORA_FWD)) == 2 and not eng.bwd.ops


# ---------------------------------------------------------------------------------------------- the C ABI
def test_qkv_host_refusals_without_gpu():
    """vk_lora_fwd / vk_lora_bwd refuse on the host before any launch, under their own names and with their own cap (K, N <= 1024: the
    row product stages a whole panel in LDS).  Host addresses, no device: every call here must come back refused."""
    import ctypes
    from volta_amd import _lib as L
    err = lambda: L.lib.vk_last_error().decode()
    buf = (ctypes.c_char * 8192)()
    a = (ctypes.addressof(buf) + 15) & ~15
    T, Y, dT, dX, dA, dB = a + 512, a + 1024, a + 1536, a + 2048, a + 3072, a + 4096

    def fwd_p(**kw):
        f = dict(X=a, A=a, B=a, T=T, Y=Y, dyn=None, M=4, K=64, N=64, r=4, ldx=64, ldy=64, scale=1.0, reserved_=0)
        f.update(kw)
        return L.LoraProblem(**f)

    def bwd_p(**kw):
        f = dict(X=a, A=a, B=a, T=T, dY=Y, dT=dT, dX=dX, dA=dA, dB=dB, dyn=None, M=4, K=64, N=64, r=4, ldx=64, ldy=64, lddx=64, accumulate=0,
                 scale=1.0, reserved_=0)
        f.update(kw)
        return L.LoraBwdProblem(**f)

    def fwd(*ps, n=None):
        assert L.lib.vk_lora_fwd((L.LoraProblem * max(len(ps), 1))(*ps), len(ps) if n is None else n, None) != 0
        assert err().startswith("vk_lora_fwd: "), err()
        return err()

    def bwd(*ps, n=None, work=a):
        assert L.lib.vk_lora_bwd((L.LoraBwdProblem * max(len(ps), 1))(*ps), len(ps) if n is None else n, work, None) != 0
        assert err().startswith("vk_lora_bwd: "), err()
        return err()

    for call, prob, y in ((fwd, fwd_p, "Y"), (bwd, bwd_p, "dY")):
        # the cap of these entry points, whatever the whole-projection ones take
        assert "K = 1088, N = 64 (multiples of 64, at most 1024)" in call(prob(K=1088, ldx=1088))
        assert "K = 64, N = 1088 (multiples of 64, at most 1024)" in call(prob(N=1088, ldy=1088))
        assert "K = 96, N = 64 (multiples of 64, at most 1024)" in call(prob(K=96, ldx=96))
        assert "problem 0: r = 12 (4, 8, 16 or 32)" in call(prob(r=12))
        assert "problem 0: NULL operand 2" in call(prob(B=None))
        assert "problem 0: operand 4 is not 16-byte aligned" in call(prob(**{y: Y + 2}))
        assert "problem 0: leading dimensions 56 / 64" in call(prob(ldx=56))
        assert "problem 1: r = 8, problem 0 has 4 (one rank per call)" in call(prob(), prob(r=8, T=T + 64, Y=Y + 256) if call is fwd else prob(r=8, dT=dT + 64))
        assert "0 problems (1 .. 6)" in call(prob(), n=0)
        assert "7 problems (1 .. 6)" in call(prob(), n=7)
    assert "problems 0 and 1 write the same T or Y" in fwd(fwd_p(), fwd_p(Y=Y + 256))
    assert "problems 0 and 1 write the same T or Y" in fwd(fwd_p(), fwd_p(T=T + 64))
    assert "problems 0 and 1 write the same dT" in bwd(bwd_p(), bwd_p(dA=dA + 512, dB=dB + 512))
    assert "problem 0: dA and dB are both set" in bwd(bwd_p(dB=None))
    assert "problem 0: dA and dB are both set" in bwd(bwd_p(dA=dA + 4))
    assert "problem 0 has no output" in bwd(bwd_p(dA=None, dB=None, dX=None))
    assert "problem 0: dX alignment / lddx 56" in bwd(bwd_p(lddx=56))
    assert "problem 1 writes the gradients of an earlier problem without `accumulate`" in bwd(bwd_p(), bwd_p(dT=dT + 64))
    assert "problem 1: a shared adapter has one dA, one dB" in bwd(bwd_p(), bwd_p(dT=dT + 64, dA=dA + 512, accumulate=1))
    assert "problem 1: the (at most 3) adapters that add into one dX share its shape" in bwd(bwd_p(), bwd_p(dT=dT + 64, dA=dA + 512, dB=dB + 512, M=3))
    assert "dA of problem 1 is dB of problem 0" in bwd(bwd_p(), bwd_p(dT=dT + 64, dA=dB, dB=dA + 512, dX=None))
    assert "workspace must be a 16-byte aligned buffer of vk_lora_bwd_work_bytes()" in bwd(bwd_p(), work=None)
    assert "workspace must be a 16-byte aligned buffer of vk_lora_bwd_work_bytes()" in bwd(bwd_p(), work=a + 8)
    one = (L.LoraBwdProblem * 1)(bwd_p())
    assert L.lib.vk_lora_bwd_work_bytes(one, 0) < 0 and L.lib.vk_lora_bwd_work_bytes(one, 7) < 0 and L.lib.vk_lora_bwd_work_bytes(None, 1) < 0
    assert L.lib.vk_lora_bwd_work_bytes((L.LoraBwdProblem * 1)(bwd_p(K=0)), 1) < 0
    assert L.lib.vk_lora_bwd_work_bytes(one, 1) == 256 * ((4 * (64 + 64) * 4 + 255) // 256)          # one row block: r (K + N) floats
