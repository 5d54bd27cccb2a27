"""LoRA dropout on the CPU: the `dropout` argument of volta_amd.lora, the plans a model with a rate builds (plans build without a GPU, as
in tests/test_lora_cpu.py, whose helpers this module uses), the host-side refusals of the vk_lora_*_drop entry points, and the ctypes
mirrors of what the header gained."""
import ctypes
import os
import subprocess
import sys
import tempfile

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_lora_cpu as T0  # noqa: E402

ROOT, S, SHAPE = T0.ROOT, T0.S, T0.SHAPE
make, arena_of, engine, lora_ops = T0.make, T0.arena_of, T0.engine, T0.lora_ops
ALL = ("query", "key", "value", "attn_out", "ffn_up", "ffn_down")


@pytest.fixture(scope="module")
def matrix():
    yield S.Matrix()


# ---------------------------------------------------------------------------------------------- the public interface
def test_argument_errors(matrix):
    from volta_amd import lora
    model = make(matrix, "vilbert")
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            lora.add_lora(model, dropout=bad)
    assert model.lora_config is None and not [n for n, _ in model.named_parameters() if "lora" in n]
    with pytest.raises(RuntimeError):
        lora.set_lora_dropout(model, 0.1)                    # no adapters yet
    lora.add_lora(model, dropout=0.25)
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            lora.set_lora_dropout(model, bad)
    assert model.lora_config["dropout"] == 0.25


def test_lora_config_keys(matrix):
    from volta_amd import lora
    five = ["r", "alpha", "targets", "modalities", "sublayers"]
    model = make(matrix, "vilbert")
    lora.add_lora(model, r=8, alpha=16)
    assert list(model.lora_config) == five and lora.lora_dropout(model) == 0.0
    assert model.lora_config == dict(r=8, alpha=16.0, targets=["query", "value"], modalities=["text", "vision"], sublayers=[0, 2, 4, 6])
    other = make(matrix, "vilbert")
    lora.add_lora(other, r=8, alpha=16, dropout=0.0)
    assert list(other.lora_config) == five and other.lora_config == model.lora_config
    lora.set_lora_dropout(model, 0.1)
    assert list(model.lora_config) == five + ["dropout"] and model.lora_config["dropout"] == 0.1 and lora.lora_dropout(model) == 0.1
    lora.set_lora_dropout(model, 0.0)
    assert list(model.lora_config) == five                   # a stored config without the key means 0
    third = make(matrix, "vilbert")
    lora.add_lora(third, dropout=0.05)
    assert list(third.lora_config) == five + ["dropout"] and third.lora_config["dropout"] == 0.05 and lora.lora_scale(third) == 2.0
    assert arena_of(third).lora_scale == 2.0


def test_set_lora_dropout_drops_plans_and_keeps_parameters(matrix):
    from volta_amd import lora
    model = make(matrix, "vilbert")
    names = lora.add_lora(model.bert, dropout=0.1)           # through the nested BertModel: the root's state
    before = {n: p for n, p in model.named_parameters()}
    values = {n: p.detach().clone() for n, p in before.items()}
    model.__dict__["_arena"], model.__dict__["_engines"] = "the arena", {"a cached plan": 1}
    lora.set_lora_dropout(model.bert, 0.3)
    assert model._engines == {} and model._arena == "the arena"          # the plans go, the arena stays
    assert model.lora_config["dropout"] == 0.3 and model.bert.__dict__.get("lora_config") is None
    after = dict(model.named_parameters())
    assert set(after) == set(before) and all(after[n] is before[n] and torch.equal(after[n], values[n]) for n in before)
    assert set(names) == {n for n in after if ".lora_" in n}
    model.__dict__["_arena"] = None
    sd = lora.lora_state_dict(model)
    lora.load_lora_state_dict(model, sd)                      # unaffected by the rate
    lora.merge_lora(model)
    assert model.lora_config is None


# ---------------------------------------------------------------------------------------------- plans
DROP_FNS = lambda L: {L.FN_LORA_FWD: L.FN_LORA_FWD_DROP, L.FN_LORA_BWD: L.FN_LORA_BWD_DROP, L.FN_LORA_PROJ_FWD: L.FN_LORA_PROJ_FWD_DROP,
                      L.FN_LORA_PROJ_BWD: L.FN_LORA_PROJ_BWD_DROP}


def kept_array(eng, addr, n):
    arr = next(k for k in eng.keep if isinstance(k, ctypes.Array) and ctypes.addressof(k) == addr)
    assert len(arr) == n
    return list(arr)


def lora_problems(eng, plan, fns):
    """[(op index, fn, problem, its vk_dropout or None)] of the LoRA ops of a plan, in list order"""
    from volta_amd import _lib as L
    out = []
    for i, o in enumerate(plan.ops):
        if o[0] == L.OP_GENERIC and o[4].fn in fns:
            g = o[4]
            probs = kept_array(eng, g.p[0], g.n[0])
            drops = kept_array(eng, g.p[2], g.n[0]) if g.p[2] else [None] * len(probs)
            out += [(i, g.fn, p, d) for p, d in zip(probs, drops)]
    return out


def model_sites(eng):
    """(site, threshold) of every active dropout entry below the LoRA base that the plan's argument structures hold, in order"""
    from volta_amd import _lib as L
    out = []

    def walk(o):
        if isinstance(o, L.Dropout):
            if o.threshold and o.site < eng.LORA_SITE_BASE:
                out.append((o.site, o.threshold))
        elif isinstance(o, ctypes.Array):
            if isinstance(o._type_, type) and issubclass(o._type_, (ctypes.Structure, ctypes.Array)):
                for x in o:
                    walk(x)
        elif isinstance(o, ctypes.Structure):
            for f in o._fields_:
                walk(getattr(o, f[0]))
    for k in eng.keep:
        walk(k)
    return out


@pytest.mark.parametrize("family,kind,targets", [("vilbert", "pretrain", ("query", "value")), ("uniter", "tasks", ("query", "key", "value")),
                                                 ("vilbert", "backbone", ALL), ("uniter", "pretrain", ALL)])
def test_training_plan_with_a_rate(matrix, family, kind, targets):
    from volta_amd import _lib as L, lora
    p = 0.1
    model = make(matrix, family, kind)
    kw = dict(task=("TASK1", matrix.task_cfg["TASK1"])) if kind == "tasks" else {}
    plain = engine(model, arena_of(model), **kw)
    lora.add_lora(model, r=8, targets=targets, dropout=p)
    arena = arena_of(model)
    eng = engine(model, arena, lora_dropout=lora.lora_dropout(model), **kw)
    nodrop = engine(model, arena, **kw)
    text, unresolved = S.render(eng)
    assert unresolved == 0
    old, new = list(DROP_FNS(L)), list(DROP_FNS(L).values())
    kinds = lambda plan: [(o[0], o[4].fn if o[0] == L.OP_GENERIC else None) for o in plan.ops]
    swap = lambda ks: [(k, DROP_FNS(L).get(fn, fn)) for k, fn in ks]
    # the lists of the plan without a rate, every LoRA op replaced by its _drop form
    for a, b in ((eng.fwd, nodrop.fwd), (eng.bwd, nodrop.bwd)):
        assert kinds(a) == swap(kinds(b)) and not lora_ops(a, old[0]) and not any(fn in old for _, fn in kinds(a))
    fwd, bwd = lora_problems(eng, eng.fwd, new), lora_problems(eng, eng.bwd, new)
    assert fwd and len(bwd) == len(fwd) == len(lora_problems(nodrop, nodrop.fwd, old))
    thr = int(p * 2 ** 32)
    assert thr == 429496729
    seed = eng.seed.data_ptr()
    for _, _, q, d in fwd + bwd:
        assert d.threshold == thr and d.seed == seed and d.site >= eng.LORA_SITE_BASE and abs(d.scale - 1.0 / (1.0 - p)) < 1e-6
    # a site per problem: distinct, counted up from the base in list order (sub-layer, stream, target)
    sites = [d.site for _, _, _, d in fwd]
    assert len(set(sites)) == len(sites) and sorted(sites) == list(range(eng.LORA_SITE_BASE, eng.LORA_SITE_BASE + len(sites))) and eng.LORA_SITE_BASE >= 1 << 20
    if targets != ALL:
        assert sites == sorted(sites)                        # one op per sub-layer: the counter's order is the list's
    # each backward problem replays its forward problem's stream: same T, same site
    by_T = {q.T: d.site for _, _, q, d in fwd}
    assert len(by_T) == len(fwd) and all(by_T[q.T] == d.site for _, _, q, d in bwd)
    # a shared adapter (uniter) has a site per stream
    if family == "uniter":
        by_A = {}
        for _, _, q, d in fwd:
            by_A.setdefault(q.A, []).append(d.site)
        assert all(len(v) == 2 and v[0] != v[1] for v in by_A.values())
    # the model's own sites did not move: those of the plan without adapters
    assert eng.site == plain.site == nodrop.site
    own = model_sites(plain)
    assert own and model_sites(eng) == own == model_sites(nodrop)
    # a rebuilt plan hands out the same sites
    again = engine(model, arena, lora_dropout=p, **kw)
    assert [d.site for _, _, _, d in lora_problems(again, again.fwd, new)] == sites
    assert S.render(again)[0] == text


def test_frozen_plan_keeps_the_sites(matrix):
    """Pruning drops backward problems, not sites: what remains replays its forward problem's site."""
    from volta_amd import _lib as L, lora
    model = make(matrix, "vilbert")
    lora.add_lora(model, r=8, sublayers=[4, 6], dropout=0.2)
    arena = arena_of(model)
    lora.mark_only_lora_trainable(model)
    frozen = {n for n, p in model.named_parameters() if not p.requires_grad}
    top = {n for n in arena.params if ".lora_" in n and ".layer.6." in n}
    full = engine(model, arena, lora_dropout=0.2)
    eng = engine(model, arena, frozen=frozen | top, lora_dropout=0.2)
    new = list(DROP_FNS(L).values())
    site_of = lambda e: {q.T - e.bufs["L4_loraT00"].data_ptr(): d.site for _, _, q, d in lora_problems(e, e.fwd, new)}
    assert sorted(site_of(full).values()) == sorted(site_of(eng).values())
    fwd = {q.T: d.site for _, _, q, d in lora_problems(eng, eng.fwd, new)}
    bwd = lora_problems(eng, eng.bwd, new)
    assert bwd and len(bwd) < len(fwd) and all(fwd[q.T] == d.site for _, _, q, d in bwd)
    assert any(not q.dA and q.dX for _, _, q, d in bwd)      # a frozen adapter with a live dX keeps its dropout entry


def test_plans_that_take_no_mask(matrix):
    """An eval plan, a score plan and a p = 0 plan are the plans built without the argument."""
    from volta_amd import lora
    from volta_amd.engine import StepEngine
    from volta_amd.retrieval import split_plan
    model = make(matrix, "uniter")
    lora.add_lora(model, r=8, targets=ALL, dropout=0.1)
    arena = arena_of(model)
    B, T, Rv = SHAPE
    text = lambda e: S.render(e)[0]
    assert text(engine(model, arena, train=False, lora_dropout=0.1)) == text(engine(model, arena, train=False))
    assert text(engine(model, arena, lora_dropout=0.0)) == text(engine(model, arena))
    assert text(engine(model, arena, lora_dropout=0.1)) != text(engine(model, arena))
    score = lambda **kw: StepEngine(model.config, arena, B, T, Rv, False, heads="score", part="pair", split=split_plan(model.config), projection_dtype="bf16", **kw)
    assert text(score(lora_dropout=0.1)) == text(score())
    with pytest.raises(ValueError):
        engine(model, arena, lora_dropout=1.0)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_ctypes_mirrors_match_the_header():
    """The new VK_FN_* values and the structures the _drop entry points take, against a C translation unit compiled from the header."""
    from volta_amd import _lib as L
    enums = {"VK_FN_LORA_FWD": L.FN_LORA_FWD, "VK_FN_LORA_BWD": L.FN_LORA_BWD, "VK_FN_LORA_PROJ_FWD": L.FN_LORA_PROJ_FWD, "VK_FN_LORA_PROJ_BWD": L.FN_LORA_PROJ_BWD,
             "VK_FN_LORA_FWD_DROP": L.FN_LORA_FWD_DROP, "VK_FN_LORA_BWD_DROP": L.FN_LORA_BWD_DROP, "VK_FN_LORA_PROJ_FWD_DROP": L.FN_LORA_PROJ_FWD_DROP,
             "VK_FN_LORA_PROJ_BWD_DROP": L.FN_LORA_PROJ_BWD_DROP, "VK_LORA_MAX_PROBLEMS": L.LORA_MAX_PROBLEMS}
    structs = {"vk_dropout": L.Dropout, "vk_lora_problem": L.LoraProblem, "vk_lora_bwd_problem": L.LoraBwdProblem, "vk_lora_proj_problem": L.LoraProjProblem,
               "vk_lora_proj_bwd_problem": L.LoraProjBwdProblem, "vk_generic_args": L.GenericArgs}
    fields = [("vk_dropout", f[0]) for f in L.Dropout._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "volta_hip.h"\nint main(void){'
    src += "".join('printf("%s %%d\\n", (int)%s);' % (n, n) for n in enums)
    src += "".join('printf("%s %%zu\\n", sizeof(%s));' % (n, n) for n in structs)
    src += "".join('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f) for s, f in fields)
    # the declarations themselves: a prototype that disagrees with the header's does not compile
    src += ("int (*f1)(const vk_lora_problem*, const vk_dropout*, int, vk_stream_t) = vk_lora_fwd_drop;"
            "int (*f2)(const vk_lora_bwd_problem*, const vk_dropout*, int, void*, vk_stream_t) = vk_lora_bwd_drop;"
            "int (*f3)(const vk_lora_proj_problem*, const vk_dropout*, int, vk_stream_t) = vk_lora_proj_fwd_drop;"
            "int (*f4)(const vk_lora_proj_bwd_problem*, const vk_dropout*, int, void*, vk_stream_t) = vk_lora_proj_bwd_drop;"
            "(void)f1; (void)f2; (void)f3; (void)f4; return 0;}")
    with tempfile.TemporaryDirectory() as d:
        c, obj = os.path.join(d, "s.c"), os.path.join(d, "s.o")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-c", c, "-o", obj])          # the prototypes
        exe = os.path.join(d, "s")
        open(c, "w").write(src.replace("= vk_lora_fwd_drop", "= 0").replace("= vk_lora_bwd_drop", "= 0").replace("= vk_lora_proj_fwd_drop", "= 0")
                           .replace("= vk_lora_proj_bwd_drop", "= 0"))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = subprocess.check_output([exe]).decode().split()
    got = dict(zip(out[0::2], map(int, out[1::2])))
    for n, v in enums.items():
        assert got[n] == v, (n, got[n], v)
    for n, cls in structs.items():
        assert ctypes.sizeof(cls) == got[n], (n, ctypes.sizeof(cls), got[n])
    for s, f in fields:
        assert getattr(L.Dropout, f).offset == got["%s.%s" % (s, f)], f
    assert L.FN_LORA_FWD_DROP == L.FN_LORA_PROJ_BWD + 1          # appended behind the existing values
    for name, n_args in (("vk_lora_fwd_drop", 4), ("vk_lora_bwd_drop", 5), ("vk_lora_proj_fwd_drop", 4), ("vk_lora_proj_bwd_drop", 5)):
        fn = getattr(L.lib, name)
        assert name in L.EXPORTS and len(fn.argtypes) == n_args and fn.argtypes[1] == ctypes.POINTER(L.Dropout) and fn.restype == ctypes.c_int


def test_host_refusals_without_gpu():
    """The refusals are made on the host before any launch: they need no device."""
    from volta_amd import _lib as L
    err = lambda: L.lib.vk_last_error().decode()
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 15) & ~15
    on, off = L.Dropout(None, 1 << 20, 1 << 31, 2.0), L.Dropout(None, 0, 0, 1.0)
    p = (L.LoraProblem * 1)(L.LoraProblem(a, a, a, a, a + 1024, None, 4, 64, 64, 4, 64, 64, 1.0, 0))
    assert L.lib.vk_lora_fwd_drop(p, (L.Dropout * 1)(on), 1, None) != 0 and "vk_lora_fwd_drop: problem 0" in err() and "NULL seed" in err()
    assert L.lib.vk_lora_fwd_drop(p, None, 1, None) != 0 and "NULL dropout" in err()
    assert L.lib.vk_lora_fwd_drop(p, (L.Dropout * 1)(off), 0, None) != 0 and "0 problems" in err()
    pp = (L.LoraProjProblem * 1)(L.LoraProjProblem(a, a, a, a, a + 1024, None, None, 4, 64, 64, 4, 64, 64, 0, 1.0, 0))
    assert L.lib.vk_lora_proj_fwd_drop(pp, (L.Dropout * 1)(on), 1, None) != 0 and "vk_lora_proj_fwd_drop: problem 0" in err() and "NULL seed" in err()
    b = (L.LoraBwdProblem * 1)(L.LoraBwdProblem(a, a, a, a, a, a + 512, a + 1024, a + 2048, a + 3072, None, 4, 64, 64, 4, 64, 64, 64, 0, 1.0, 0))
    assert L.lib.vk_lora_bwd_drop(b, (L.Dropout * 1)(on), 1, a, None) != 0 and "vk_lora_bwd_drop: problem 0" in err() and "NULL seed" in err()
    assert L.lib.vk_lora_bwd_drop(b, (L.Dropout * 1)(off), 1, None, None) != 0 and "workspace" in err()
    pb = (L.LoraProjBwdProblem * 1)(L.LoraProjBwdProblem(a, a, a, a, a, a + 512, a + 1024, a + 2048, a + 3072, None, None, 4, 64, 64, 4, 64, 64, 64, 0, 0, 1.0))
    assert L.lib.vk_lora_proj_bwd_drop(pb, (L.Dropout * 1)(on), 1, a, None) != 0 and "vk_lora_proj_bwd_drop: problem 0" in err() and "NULL seed" in err()
    assert L.lib.vk_lora_proj_bwd_drop(pb, (L.Dropout * 1)(on), 7, a, None) != 0 and "7 problems" in err()
