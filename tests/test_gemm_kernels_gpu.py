"""The grouped GEMM kernels (csrc/gemm.hip, gemm256.hip, gemm4w.hip, gemm_common.h) against the float64 restatement of
tests/gemm_restate.py, at the smallest shapes at which each mechanism can go wrong.  GPU only.

Inputs (gemm_restate.Case).  Gaussian family: A ~ N(0, 1), B ~ N(0, 1 / K), bias, R and the previous C ~ N(0, 1), all rounded to bf16
(bias fp32), so u = acc + bias is of order 1.  Integer family: operands in [-4, 4], bias / R / previous C in [-8, 8]: every partial sum
is exact in fp32 in any order and the output must be BITWISE the float64 result rounded once.  Every launch names its geometry.

Bounds (derived in gemm_restate's docstring, none tuned): e_acc = (Kc + 4) 2^-24 (|A|.|B| + |bias| (+ |C_prev|)) for the fp32
accumulator in any summation order; fp32 outputs and bias_grad within e_acc; bf16 outputs within e_f + 2^-8 (|f(ref)| + e_f) with e_f
the epilogue's propagation of e_acc (MULR |R| e_acc + |R ref| 2^-24, ADDR e_acc + |R| 2^-24, GELU 1.13 e_acc + e_formula, gelu'
0.80 e_acc + e_formula'), e_formula = 4 x the measured fp32 error of the kernel's own erf polynomial against float64.

Every output (C, C2, bias_grad) lies 8 columns into a wider buffer with 256 sentinel elements in front and behind, 3 sentinel rows
below and sentinel columns up to ldc -- position-dependent NaN patterns -- and is compared as raw bits: everything outside the output
must come back unchanged, columns [N, n_store) of an F32 output must be exact zeros.  Every case is launched twice into fresh buffers
and must give the same bits.

1. epilogue x layout x geometry: M in {300, 129}, N in {197 .. 200} (one full wave block plus each ragged class N % 4), K = 96 with lda
   padded to 128 (TN: K = 133); all seven epilogues in NT and NN, F32 / F32_ACC with bias_grad in TN; ldr = ldc + 8 in half of the R
   cases; ldc = 8 k + 4 for M = 300 (plain fast-path stores) and 8 k for M = 129 (LDS-staged stores); F32_ACC twice in a row.
   The odd-N MULR / ADDR cases are the regression test of the residual operand's buffer extent: before it was rounded up to an even
   element count the last element of the last row lost its residual in every geometry (raw buffer loads are range-checked per dword).
2. K-loop depth: 256 x 256 and 300 x 200 with 1 .. 11 K-steps of 32 (rings of 5, 3 and 6 K-steps, 2-deep double buffer of 64), plus
   ragged K in {1, 8, 37, 72, 100} for NT, whose B rows are not padded; F32 epilogue.
3. the persistent walk: 32 NT / NN problems of N = 2304 with M from {1, 8, 100, 255, 256, 257, 300} and K from {32, 64, 96, 160, 224,
   352}, one with M = 0: consecutive tiles of a workgroup belong to problems of different K, with fewer K-steps than the prologue
   stages; 2 tiles per workgroup (asserted from the launcher's grid rule before the launch), 3 or more under vk_gemm_reserve_cus(128);
   the one-tile-per-workgroup launch must give the same bits.
4. `dyn` = 0, 1, 255, 256, 257, 300, 1000 on a 300-row (NT / NN) or 300-deep (TN) problem.  A count of 0 writes nothing in NT / NN and
   an all-zero dW and db (or the previous C unchanged) in TN: every kernel's K loop runs zero times, all its stages are out of range
   and zero-fill, and the epilogue runs on zero accumulators.
5. split accumulation: 2 parts of K = 128 on a ragged 300 x 200 and 30 parts (the maximum) of K = 1920, geometries 258 / 259, NT and TN.

Measured on an MI355X over the 213 tests below (worst |err| / bound, Gaussian family; share of bf16 elements that are not the exactly
rounded float64 value; the last test prints the table): fp32 outputs and bias_grad at most 0.20 of e_acc (0.02 in the epilogue matrix,
0.20 where Kc is 1 .. 32); bf16 outputs 0.981 .. 0.995 of their bound in every group, layout and epilogue -- the bound is one half ulp
plus e_f, and some element always lies next to a rounding boundary --; BF16 / ADDR / MULR / RELU 0.001 .. 0.007 % of the elements not the
exactly rounded value, GELU and gelu' 0.073 .. 0.096 %; the integer family bitwise exact throughout.  Both families, every geometry.
Before the two fixes that came with this file: the odd-N MULR / ADDR cases failed in all nine geometries at exactly [M-1, N-1], and the
ragged F32_ACC path added C[m][4 k] to all four columns of a 4-group (a bit cast of a vector element that compiled to element 0).
Wall time of the file on the MI355X: 13 s (slowest test 1.2 s)."""
import os
import sys
from collections import defaultdict

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_restate as G  # noqa: E402
from gemm_restate import NT, NN, TN, BF16, GELU, MULR, ADDR, F32, RELU, F32_ACC  # noqa: E402

pytestmark = pytest.mark.gpu

PERSISTENT, ONE_TILE = 0x1000, 0x2000
GEOMETRIES = {"auto": 0, "tile128x128": 128, "tile256x256": 258, "tile256x192": 259, "tile256x128": 260, "tile256x128_4wave": 261, "tile128x128_4wave_ring": 262,
              "tile256x256_persistent": 258 | PERSISTENT, "tile256x192_persistent": 259 | PERSISTENT}
geometry_param = pytest.mark.parametrize("geometry", list(GEOMETRIES.values()), ids=list(GEOMETRIES))
LAYOUTS = {"NT": NT, "NN": NN, "TN": TN}
WORST = defaultdict(G.Worst)          # (group, layout, epilogue) -> worst ratio / inexact share, printed by the last test
_CASES = {}                           # cases (inputs + float64 reference) are built once and shared by every geometry


def _mods():
    from volta_amd import _lib as L, ops
    return L, ops


def cached(key, make):
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


def device_inputs(case):
    if not hasattr(case, "dev"):
        def up(t):          # an operand without rows (M = 0) still gets a pointer: the dispatcher rejects a NULL R
            return None if t is None else (torch.zeros(1, t.shape[1], dtype=t.dtype) if t.numel() == 0 else t).cuda()
        case.dev = {k: up(getattr(case, k)) for k in ("A", "B", "bias", "R")}
        case.dev["dyn"] = torch.tensor([case.dyn], dtype=torch.int32, device="cuda") if case.dyn is not None else None
    return case.dev


def fresh_outputs(case):
    return {k: g.flat.cuda() for k, g in case.out.items()}


def problem(ops, case, outs):
    d = device_inputs(case)
    view = {k: g.view(outs[k]) for k, g in case.out.items()}
    return ops.gemm_problem(d["A"], d["B"], view["C"], case.layout, case.M, case.N, case.K, bias=d["bias"], R=d["R"],
                            C2=view.get("C2"), bias_grad=view["bias_grad"][0] if case.bias_grad else None, dyn=d["dyn"],
                            n_store=case.n_store, lda=case.lda, ldb=case.ldb, ldc=case.ldc, ldr=case.ldr or None)


def same_bits(a, b):
    return all(torch.equal(a[k].view(torch.int16 if a[k].dtype == torch.bfloat16 else torch.int32),
                           b[k].view(torch.int16 if b[k].dtype == torch.bfloat16 else torch.int32)) for k in a)


def launch(cases, geometry, passes=1):
    """one launch (or `passes` in a row) of the problems of `cases` into fresh sentinel buffers; the buffers, on the host"""
    L, ops = _mods()
    outs = [fresh_outputs(c) for c in cases]
    probs = [problem(ops, c, o) for c, o in zip(cases, outs)]
    for _ in range(passes):
        ops.gemm_grouped(cases[0].layout, cases[0].epi, probs, geometry=geometry)
    torch.cuda.synchronize()
    return [{k: v.cpu() for k, v in o.items()} for o in outs]


def run_and_check(case, geometry, group, passes=1):
    got = launch([case], geometry, passes)[0]
    msgs = case.check(got, passes=passes, worst=WORST[(group, G.LAYOUT_NAMES[case.layout], G.EPI_NAMES[case.epi])])
    again = launch([case], geometry, passes)[0]
    if not same_bits(got, again):
        msgs.append("%s: two launches gave different bits" % case.ident())
    return msgs


# ---- 1. epilogue x layout x geometry ------------------------------------------------------------------------------------------------
def matrix_case(layout, epi, M, N, family):
    def make():
        K = 96 + 37 if layout == TN else 96
        wide = (N in (197, 200)) == (M == 300)
        return G.Case(layout, epi, M, N, K, family, seed=M * 1000 + N, ldc=None if M == 300 else G._up(N, 8) + 16,
                      ldr_extra=8 if wide else 0, n_store=G._up(N, 4) + 4 if (epi == F32 and M == 300) else 0, bias_grad=layout == TN)
    return cached(("matrix", layout, epi, M, N, family), make)


MATRIX = [(ln, en) for ln in ("NT", "NN") for en in ("BF16", "GELU", "MULR", "ADDR", "F32", "RELU", "F32_ACC")] + [("TN", "F32"), ("TN", "F32_ACC")]


@geometry_param
@pytest.mark.parametrize("layout_name,epi_name", MATRIX)
def test_epilogue_matrix(layout_name, epi_name, geometry):
    layout, epi = LAYOUTS[layout_name], getattr(G, epi_name)
    msgs = []
    for family in (["gauss"] if epi == GELU else ["gauss", "int"]):
        for M in (300, 129):
            for N in (197, 198, 199, 200):
                case = matrix_case(layout, epi, M, N, family)
                msgs += run_and_check(case, geometry, "matrix")
                if epi == F32_ACC:
                    msgs += run_and_check(case, geometry, "matrix", passes=2)
    assert not msgs, "\n".join(msgs[:20])


# ---- 2. K-loop depth ----------------------------------------------------------------------------------------------------------------
@geometry_param
@pytest.mark.parametrize("layout_name", ["NT", "NN", "TN"])
def test_k_loop_depth(layout_name, geometry):
    layout = LAYOUTS[layout_name]
    msgs = []
    for family in ("gauss", "int"):
        for M, N in ((256, 256), (300, 200)):
            for K in [32 * s for s in range(1, 12)] + ([1, 8, 37, 72, 100] if layout == NT else []):
                case = cached(("depth", layout, M, N, K, family), lambda: G.Case(layout, F32, M, N, K, family, seed=K))
                msgs += run_and_check(case, geometry, "depth")
    assert not msgs, "\n".join(msgs[:20])


# ---- 3. the persistent walk over mixed problems ---------------------------------------------------------------------------------------
WALK_M = [1, 8, 100, 255, 256, 257, 300]
WALK_K = [32, 64, 96, 160, 224, 352]
NUM_CU = 256


def persistent_grid(total, reserved):
    """persistent_grid of csrc/gemm256.hip: as few workgroups as walk the tile list in the same number of rounds, in whole multiples of 8"""
    ncu = NUM_CU - reserved
    if total <= ncu:
        return total
    rounds = -(-total // ncu)
    even = (-(-total // rounds) + 7) & ~7
    return min(even, ncu)


def tiles_of(cases, bn):
    return sum(-(-c.M // 256) * -(-c.N // bn) for c in cases)


def walk_cases(layout, epi):
    def make():
        out = []
        for i in range(32):
            M = 0 if (layout == NT and i == 15) else WALK_M[i % 7]
            out.append(G.Case(layout, epi, M, 2304, WALK_K[i % 6], "gauss", seed=100 + i, ldc=2304 + 16, ldr_extra=8 * (i % 2)))
        return out
    return cached(("walk", layout, epi), make)


@pytest.mark.parametrize("epi_name", ["BF16", "GELU", "ADDR"])
@pytest.mark.parametrize("layout_name", ["NT", "NN"])
def test_persistent_walk_over_mixed_problems(layout_name, epi_name):
    L, ops = _mods()
    layout, epi = LAYOUTS[layout_name], getattr(G, epi_name)
    cases = walk_cases(layout, epi)
    t256, t192 = tiles_of(cases, 256), tiles_of(cases, 192)
    assert t256 >= 288
    # the heuristic of gemm_dispatch (geometry 0): 256-row tiles from 160 tiles on, the narrower ones when their rounds x width is smaller;
    # the walk when there are more tiles than CUs
    assert t256 >= 160 and -(-t192 // 256) * 192 < 0.97 * -(-t256 // 256) * 256 and t192 > NUM_CU, "geometry 0 must resolve to the 256 x 192 walk"
    for total in (t256, t192):
        assert -(-total // persistent_grid(total, 0)) >= 2 and -(-total // persistent_grid(total, 128)) >= 3
    worst = WORST[("walk", layout_name, epi_name)]
    base, msgs = {}, []
    for edge in (258, 259):
        got = launch(cases, edge | PERSISTENT)
        for c, g in zip(cases, got):
            msgs += c.check(g, worst=worst)
        base[edge] = got
    assert not msgs, "\n".join(msgs[:20])

    def must_equal(got, want, what):
        bad = [i for i, (g, w) in enumerate(zip(got, want)) if not same_bits(g, w)]
        assert not bad, "%s: problems %s differ bitwise from the checked persistent launch" % (what, bad)

    for edge in (258, 259):
        must_equal(launch(cases, edge | PERSISTENT), base[edge], "second launch of %d" % edge)
        must_equal(launch(cases, edge | ONE_TILE), base[edge], "one tile per workgroup, %d" % edge)
    must_equal(launch(cases, 0), base[259], "the heuristic's launch")
    must_equal(launch(cases, 0), base[259], "the heuristic's second launch")
    try:
        assert L.lib.vk_gemm_reserve_cus(128) == 0
        must_equal(launch(cases, 258 | PERSISTENT), base[258], "3 tiles per workgroup, 258")
        must_equal(launch(cases, 259 | PERSISTENT), base[259], "4 tiles per workgroup, 259")
        must_equal(launch(cases, 0), base[259], "the heuristic's launch with reserved CUs")
    finally:
        L.lib.vk_gemm_reserve_cus(0)


# ---- 4. device-side counts ----------------------------------------------------------------------------------------------------------
COUNTS = [0, 1, 255, 256, 257, 300, 1000]


@geometry_param
@pytest.mark.parametrize("layout_name", ["NT", "NN", "TN"])
def test_device_side_counts(layout_name, geometry):
    layout = LAYOUTS[layout_name]
    msgs = []
    for family in ("gauss", "int"):
        for count in COUNTS:
            for epi in ((F32, F32_ACC) if layout == TN else (BF16, GELU, ADDR)):
                if family == "int" and epi == GELU:
                    continue
                if layout == TN:
                    make = lambda: G.Case(TN, epi, 129, 198, 300, family, seed=count, dyn=count, bias_grad=True)      # noqa: E731
                else:
                    make = lambda: G.Case(layout, epi, 300, 200, 96, family, seed=count, dyn=count)                  # noqa: E731
                case = cached(("dyn", layout, epi, count, family), make)
                msgs += run_and_check(case, geometry, "dyn")
    assert not msgs, "\n".join(msgs[:20])


# ---- 5. split accumulation at the edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,nparts", [(300, 200, 128, 2), (256, 256, 1920, 30)])
@pytest.mark.parametrize("geometry", [258, 259])
@pytest.mark.parametrize("layout_name", ["NT", "TN"])
def test_split_accumulation_edges(layout_name, geometry, M, N, K, nparts):
    L, ops = _mods()
    layout = LAYOUTS[layout_name]
    epi = F32 if layout == TN else ADDR
    case = cached(("split", layout, M, N, K), lambda: G.Case(layout, epi, M, N, K, "gauss", seed=K + M, bias_grad=layout == TN, ldr_extra=8))
    d = device_inputs(case)
    ws, cnt = ops.split_workspace(layout, M, N, nparts, geometry, "cuda")
    ws.fill_(0xFF)                     # NaN patterns: every word the reducer reads must have been written
    slices = ops.k_slices(d["A"], d["B"], layout, K, nparts)
    assert len(slices) == nparts
    first = None
    for rep in range(3):
        outs = fresh_outputs(case)
        parts = ops.split_parts(problem(ops, case, outs), layout, slices, ws, cnt)
        ops.gemm_grouped(layout, epi, parts, geometry=geometry)
        torch.cuda.synchronize()
        got = {k: v.cpu() for k, v in outs.items()}
        assert int(cnt.abs().sum()) == 0, "every tile's counter must be back at zero"
        if first is None:
            first = got
            msgs = case.check(got, worst=WORST[("split", layout_name, G.EPI_NAMES[epi])])
            assert not msgs, "\n".join(msgs[:20])
        else:
            assert same_bits(got, first), "launch %d gave other bits" % rep


# ---- what the cases above measured --------------------------------------------------------------------------------------------------
def test_zz_report_worst_ratios():
    """prints the worst |err| / bound per group, layout and epilogue of this session's cases (run the file with -s to see it)"""
    for (group, layout, epi), w in sorted(WORST.items()):
        share = "%.4f %%" % (100.0 * w.inexact / w.bf16_elems) if w.bf16_elems else "-"
        print("gemm kernels: %-6s %s %-7s worst |err| / bound %.3f   bf16 elements not exactly rounded: %s" % (group, layout, epi, w.ratio, share))
        assert w.ratio <= 1.0
