"""The LAMB contract without a GPU: a plain fp32 torch implementation lies inside the gates of tests/lamb_restate.py on every case of its
table, every deliberately wrong contract lies outside on at least one (so the GPU tests' gates can tell them apart), the piece-table
builder tiles every tensor exactly once, the library's host-side table checks refuse what the header says they refuse (they run before
any launch, so they need no GPU), and the Python class's refusals and checkpoint layout on CPU tensors."""
import ctypes as C
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lamb_restate as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lamb32(case, inp):
    """The contract in plain fp32 torch on the CPU, NSTEPS steps.  Yields (step index, {name: (p, m, v)}, {name: table row}) after each."""
    h = case.h
    st = {s.name: [inp[s.name][k].clone() for k in "pmv"] for s in R.LAYOUT}
    steps = [case.step0, case.step0]
    f = torch.float32
    for k in range(R.NSTEPS):
        steps = [t + 1 for t in steps]
        grads = R.step_grads(inp, k)
        live = [s for s in R.LAYOUT if grads[s.name] is not None]
        gs = torch.tensor(case.grad_scale, dtype=f) * (torch.tensor(case.clip, dtype=f) if case.clip is not None else 1.0)
        S = [0.0, 0.0]
        for s in live:
            g = grads[s.name]
            S[s.group] += float((g * g).sum())
        cdiv = []
        for gi in range(2):
            norm = torch.tensor(math.sqrt(sum(S) if h.global_norm else S[gi]), dtype=f) * gs.abs()
            mx = case.max_norm[gi]
            cdiv.append(norm / torch.tensor(mx, dtype=f) if mx is not None and mx > 0 and float(norm) > R.f32(mx) else torch.tensor(1.0))
        rows = {}
        for s in live:
            p, m, v = st[s.name]
            wd, lr = torch.tensor(case.wd[s.group], dtype=f), torch.tensor(case.lr[s.group], dtype=f)
            bc1, bc2 = (torch.tensor(x, dtype=f) for x in R.bias_corrections(h, steps[s.group]))
            b1, b2, eps = (torch.tensor(x, dtype=f) for x in (h.b1, h.b2, h.eps))
            g = (grads[s.name] * gs) / cdiv[s.group]
            if not h.adam_w and float(wd) != 0:
                g = g + wd * p
            m = b1 * m + ((1 - b1) if h.grad_averaging else 1.0) * g
            v = b2 * v + ((1 - b2) * g) * g
            u = (m / bc1) / ((v / bc2).sqrt() + eps)
            if h.adam_w and float(wd) != 0:
                u = u + wd * p
            pn, un = (p * p).sum().sqrt(), (u * u).sum().sqrt()
            trust = pn / un if float(pn) != 0 and float(un) != 0 else torch.tensor(1.0)
            rat = lr * trust
            rows[s.name] = (float(rat), float(trust), float(pn), float(un))
            st[s.name] = [p - rat * u, m, v]
            assert all(x.dtype == f for x in st[s.name])
        yield k, st, rows


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_fp32_implementation_lies_inside_the_gates(case):
    inp = R.lamb_inputs(case)
    W = R.restated(case, inp)
    worst = 0.0
    for k, st, rows in lamb32(case, inp):
        W.step(R.step_grads(inp, k), case.grad_scale, case.clip)
        assert set(rows) == set(W.last)
        for s in R.LAYOUT:
            worst = max(worst, W.excess(s.name, *st[s.name]))
            if s.name in rows:
                worst = max(worst, W.excess_table(s.name, rows[s.name]))
        assert worst <= 1.0, (k, worst)
    for n in case.skip:                      # a skipped tensor: nothing of it moves, and it has no row
        assert all(torch.equal(a, inp[n][key]) for a, key in zip(st[n], "pmv"))
    # the special tensors did what they are there for
    if "zero_u" in W.last:
        assert W.last["zero_u"]["un"] == 0.0 and W.last["zero_u"]["trust"] == 1.0


def test_every_wrong_contract_lies_outside_on_some_case():
    """The fp32 implementation of the RIGHT contract against each wrong restatement: the largest excess over the table."""
    runs = []
    for case in R.CASES:
        inp = R.lamb_inputs(case)
        runs.append((case, inp, list((k, {n: [x.clone() for x in t] for n, t in st.items()}, rows) for k, st, rows in lamb32(case, inp))))
    for var in R.Lamb64.VARIANTS:
        worst = 0.0
        for case, inp, steps in runs:
            W = R.restated(case, inp, var)
            for k, st, rows in steps:
                W.step(R.step_grads(inp, k), case.grad_scale, case.clip)
                worst = max([worst] + [W.excess(s.name, *st[s.name]) for s in R.LAYOUT])
        assert worst > 10.0, (var, worst)


def test_query_key_value_of_one_slot_have_three_ratios():
    case = R.CASES[0]
    inp = R.lamb_inputs(case)
    W = R.restated(case, inp)
    W.step(R.step_grads(inp, 0), case.grad_scale, case.clip)
    for a, b, c in (("w_q", "w_k", "w_v"), ("b_q", "b_k", "b_v")):
        assert len({W.last[a]["trust"], W.last[b]["trust"], W.last[c]["trust"]}) == 3


# ------------------------------------------------------------------------------------------------ tables
def _rows(numels, groups=None, base=1 << 20):
    """Table rows over made-up, 16-byte aligned addresses."""
    rows, at = [], base
    for i, n in enumerate(numels):
        span = (4 * n + 15) // 16 * 16 + 16
        rows.append((at, at + span, at + 2 * span, at + 3 * span, 0, n, i % 3, groups[i] if groups else 0))
        at += 4 * span
    return rows


def _work_bytes(T, P, G):
    from volta_amd import _lib as L
    return L.lib.vk_lamb_work_bytes(T.ctypes.data, len(T), P.ctypes.data, len(P), G.ctypes.data, len(G))


def test_piece_tables_tile_every_tensor_once():
    from volta_amd.optimization import lamb_tables
    gen = np.random.default_rng(3)
    numels = [1, 3, 1023, 1024, 1025, 2 * 1024 + 5, 0, 64, 64, 64, (1 << 31) + 5] + [int(x) for x in gen.integers(1, 5000, size=40)]
    groups = sorted(int(x) for x in gen.integers(0, 4, size=len(numels)))
    T, P, G = lamb_tables(_rows(numels, groups), [1.0, None, 0.0, 2.5])
    assert len(T) == len(numels) and P.dtype.itemsize == 16 and T.dtype.itemsize == 64
    assert P["offset"].dtype == np.int64 and int(P["offset"].max()) >= 1 << 31           # 64-bit offsets
    assert P["count"].min() >= 1 and P["count"].max() <= 1024
    at = 0
    for t, n in enumerate(numels):
        mine = P[int(T["piece0"][t]):int(T["piece0"][t]) + int(T["npieces"][t])]
        assert int(T["piece0"][t]) == at and (mine["tensor"] == t).all()                  # consecutive, never another tensor's
        assert len(mine) == (n + 1023) // 1024
        assert (mine["offset"] == np.arange(len(mine), dtype=np.int64) * 1024).all()      # in order, no gap, no overlap ...
        assert int(mine["count"].sum()) == n                                              # ... exactly once
        assert ((mine["offset"] + mine["count"]) <= n).all()                              # never past its tensor
        at += len(mine)
    assert at == len(P)
    for gi in range(4):
        mine = [t for t in range(len(numels)) if groups[t] == gi]
        want = sum((numels[t] + 1023) // 1024 for t in mine)
        assert int(G["piece1"][gi]) - int(G["piece0"][gi]) == want
    assert list(G["max_grad_norm"]) == [1.0, 0.0, 0.0, 2.5]
    assert int(G["piece0"][0]) == 0 and int(G["piece1"][-1]) == len(P) and (G["piece0"][1:] == G["piece1"][:-1]).all()
    assert _work_bytes(T, P, G) >= 4 * 3 * len(P) and _work_bytes(T, P, G) % 4 == 0
    with pytest.raises(ValueError):
        lamb_tables(_rows([5, 5], [1, 0]), [1.0, 1.0])                                    # groups must ascend


def test_library_refuses_bad_tables_on_the_host():
    """vk_lamb_work_bytes and vk_lamb_step run the same host-side checks before anything else: each refusal of the header's list."""
    from volta_amd import _lib as L
    from volta_amd.optimization import lamb_tables
    numels = [5, 2053, 64]

    def fresh():
        return lamb_tables(_rows(numels, [0, 0, 1]), [1.0, 0.0])

    def refused(T, P, G, word):
        assert _work_bytes(T, P, G) <= 0
        assert word in L.lib.vk_last_error().decode(), L.lib.vk_last_error()
        a = L.LambArgs()
        a.tensors, a.pieces, a.groups, a.ntensors, a.npieces, a.ngroups = T.ctypes.data, P.ctypes.data, G.ctypes.data, len(T), len(P), len(G)
        a.beta1, a.beta2, a.eps = 0.9, 0.999, 1e-6
        assert L.lib.vk_lamb_step(C.byref(a), None) != 0                                  # refused before the device tables are looked at
        assert word in L.lib.vk_last_error().decode()

    T, P, G = fresh()
    assert _work_bytes(T, P, G) > 0
    for field in "pgmv":
        T, P, G = fresh(); T[field][1] += 2; refused(T, P, G, "alignment")
    T, P, G = fresh(); T["shadow"][0] = (1 << 20) + 1; refused(T, P, G, "alignment")
    T, P, G = fresh(); T["p"][2] = 0; refused(T, P, G, "required")
    T, P, G = fresh(); T["numel"][0] = -5; refused(T, P, G, "numel")
    T, P, G = fresh(); P["count"][1] = 1025; refused(T, P, G, "count")
    T, P, G = fresh(); P["count"][0] = 0; refused(T, P, G, "count")
    T, P, G = fresh(); P["count"][3] = 6; refused(T, P, G, "past its tensor")           # the last piece of tensor 1 holds 5
    T, P, G = fresh(); P["count"][0] = 6; refused(T, P, G, "past its tensor")
    T, P, G = fresh(); P["offset"][2] = 0; refused(T, P, G, "in order")               # tensor 1's second piece laid over its first
    T, P, G = fresh(); P["count"][3] = 4; refused(T, P, G, "cover")                      # an element nobody steps
    T, P, G = fresh(); P["tensor"][1] = 0; refused(T, P, G, "belongs to")
    T, P, G = fresh(); T["cls"][0] = 64; refused(T, P, G, "class")
    T, P, G = fresh(); T["group"][2] = 2; refused(T, P, G, "group")
    T, P, G = fresh(); T["group"][0] = 1; refused(T, P, G, "group")                      # groups do not ascend
    T, P, G = fresh(); G["piece1"][0] -= 1; refused(T, P, G, "group")
    T, P, G = fresh(); T["piece0"][1] = 0; refused(T, P, G, "pieces")
    T, P, G = fresh()
    assert L.lib.vk_lamb_work_bytes(T.ctypes.data, len(T), P.ctypes.data, len(P) - 1, G.ctypes.data, len(G)) <= 0
    assert L.lib.vk_lamb_work_bytes(T.ctypes.data, len(T), P.ctypes.data, len(P), G.ctypes.data, 0) <= 0
    a = L.LambArgs()                                                                      # good tables, no scratch: refused as well
    a.tensors, a.pieces, a.groups, a.ntensors, a.npieces, a.ngroups = T.ctypes.data, P.ctypes.data, G.ctypes.data, len(T), len(P), len(G)
    a.d_tensors = a.d_pieces = a.d_groups = a.table = 16
    a.beta1, a.beta2, a.eps = 0.9, 0.999, 1e-6
    assert L.lib.vk_lamb_step(C.byref(a), None) != 0 and b"work" in L.lib.vk_last_error()
    a.beta1 = 1.0
    assert L.lib.vk_lamb_step(C.byref(a), None) != 0 and b"betas" in L.lib.vk_last_error()


def test_struct_mirrors_match_the_header():
    from volta_amd import _lib as L
    src = '#include <stdio.h>\n#include "volta_hip.h"\nint main(void){' + "".join(
        'printf("%s %%zu\\n", sizeof(%s));' % (n, n) for n in L.LAMB_STRUCTS) + \
        'printf("c %d %d %d %d %d\\n", VK_LAMB_CLASSES, VK_LAMB_PIECE, VK_LAMB_ADAM_W_MODE, VK_LAMB_GRAD_AVERAGING, VK_LAMB_GLOBAL_NORM);return 0;}'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    sizes = dict((ln.split()[0], int(ln.split()[1])) for ln in out if ln.startswith("vk_"))
    for name, cls in L.LAMB_STRUCTS.items():
        assert C.sizeof(cls) == sizes[name], (name, C.sizeof(cls), sizes[name])
    consts = [int(x) for x in [ln for ln in out if ln.startswith("c ")][0].split()[1:]]
    assert consts == [L.LAMB_CLASSES, L.LAMB_PIECE, L.LAMB_ADAM_W_MODE, L.LAMB_GRAD_AVERAGING, L.LAMB_GLOBAL_NORM]
    assert R.PIECE == L.LAMB_PIECE


# ------------------------------------------------------------------------------------------------ the Python class on CPU tensors
def _cpu_params():
    g = torch.Generator().manual_seed(0)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((3, 5), (7,), (2, 2, 2))]


def test_constructor_refusals():
    from volta_amd.optimization import LAMB
    ps = _cpu_params()
    with pytest.raises(RuntimeError, match="AMSGrad"):
        LAMB(ps, amsgrad=True)
    with pytest.raises(RuntimeError, match="common to all groups"):
        LAMB([{"params": ps[:1]}, {"params": ps[1:], "betas": (0.8, 0.999)}])
    with pytest.raises(RuntimeError, match="common to all groups"):
        LAMB([{"params": ps[:1]}, {"params": ps[1:], "grad_averaging": False}])
    with pytest.raises(ValueError):
        LAMB(ps, lr=-1.0)
    opt = LAMB([{"params": ps[:1], "lr": 1e-2, "max_grad_norm": None}, {"params": ps[1:], "weight_decay": 0.0}])     # what may differ
    d = opt.defaults
    assert (d["lr"], d["bias_correction"], d["betas"], d["eps"], d["weight_decay"], d["grad_averaging"], d["max_grad_norm"]) == \
        (1e-3, True, (0.9, 0.999), 1e-6, 0.01, True, 1.0)
    assert opt.adam_w_mode == 1 and opt.set_grad_none is True and opt.global_grad_norm is False
    with pytest.raises(RuntimeError, match="not a contiguous CUDA float32 tensor"):
        opt.step()                                                                        # no CPU path


def test_state_dict_round_trip_in_pending_form():
    """apex's layout, loaded before the parameters are on the GPU: param_groups[i]["step"] and {"exp_avg", "exp_avg_sq"} per parameter that
    has stepped, indexed in param_groups order, kept until the first setup and returned unchanged by state_dict()."""
    from volta_amd.optimization import LAMB
    ps = _cpu_params()
    opt = LAMB([{"params": ps[:2]}, {"params": ps[2:], "weight_decay": 0.0, "lr": 5e-4}])
    sd0 = opt.state_dict()
    assert sd0["state"] == {} and all("step" not in g for g in sd0["param_groups"])
    g = torch.Generator().manual_seed(1)
    state = {0: {"exp_avg": torch.randn(3, 5, generator=g), "exp_avg_sq": torch.rand(3, 5, generator=g)},
             2: {"exp_avg": torch.randn(2, 2, 2, generator=g), "exp_avg_sq": torch.rand(2, 2, 2, generator=g)}}      # parameter 1 never stepped
    groups = [dict(gr, step=7 + i) for i, gr in enumerate(sd0["param_groups"])]
    opt.load_state_dict({"state": state, "param_groups": groups})
    assert opt._fused is None and sorted(opt._pending) == [0, 2]
    assert [gr["step"] for gr in opt.param_groups] == [7, 8]
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 2] and [gr["step"] for gr in sd["param_groups"]] == [7, 8]
    for i in (0, 2):
        assert sorted(sd["state"][i]) == ["exp_avg", "exp_avg_sq"]
        assert torch.equal(sd["state"][i]["exp_avg"].view_as(state[i]["exp_avg"]), state[i]["exp_avg"])
        assert torch.equal(sd["state"][i]["exp_avg_sq"].view_as(state[i]["exp_avg_sq"]), state[i]["exp_avg_sq"])
    opt2 = LAMB([{"params": ps[:2]}, {"params": ps[2:], "weight_decay": 0.0, "lr": 5e-4}])
    opt2.load_state_dict(sd)                                                              # and round again
    assert sorted(opt2._pending) == [0, 2] and [gr["step"] for gr in opt2.param_groups] == [7, 8]
    with pytest.raises(ValueError):
        opt2.load_state_dict({"state": {5: state[0]}, "param_groups": groups})
    with pytest.raises(ValueError):
        opt2.load_state_dict({"state": {1: state[0]}, "param_groups": groups})
    opt2.zero_grad()                                                                      # set_grad_none is the default
    ps[0].grad = torch.zeros_like(ps[0])
    opt2.zero_grad(set_to_none=False)
    assert ps[0].grad is not None
    opt2.zero_grad()
    assert ps[0].grad is None
