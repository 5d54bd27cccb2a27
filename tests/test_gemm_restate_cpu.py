"""The checker of the GEMM kernel tests checked (tests/gemm_restate.py): it must accept a correct fp32 evaluation and reject planted
faults.  No GPU.

(a) A correct fp32 evaluation -- torch's CPU fp32 matmul of the same bf16 operands and a straightforward fp32 epilogue (GELU through
    torch.erf), written into the guarded buffers as a kernel would -- passes at the shapes of tests/test_gemm_kernels_gpu.py, every
    layout, epilogue and input family, with no element excluded.
(b) Each planted fault in that evaluation is rejected, by BOTH input families wherever both apply (GELU has the Gaussian family only):
    last K element of the last A row dropped; one K-step of 32 skipped; one K-step of 32 counted twice; bias omitted on the columns of
    the ragged last 4-group; R[M-1, N-1] read as 0; one output row taken from the neighbouring row tile; `dyn` off by one; F32_ACC
    overwriting instead of adding.  A fault whose planted element happens to be zero (one integer draw in nine) would be no fault: the test
    takes the first seed at which it is not.  No fault was found that only the integer family catches at these shapes; what the integer family adds is
    magnitude independence -- the Gaussian bounds are relative to |A|.|B|, and a fault that changes an output by less than 2^-8 of it
    (one dropped product among thousands under a bf16 epilogue) passes them and cannot pass a bitwise comparison.
(c) The error of the kernel's erf polynomial, restated in numpy float32, against float64 erf: the constants the GELU bounds are built
    from are the measurement."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_restate as G  # noqa: E402
from gemm_restate import NT, NN, TN, BF16, GELU, MULR, ADDR, F32, RELU, F32_ACC  # noqa: E402

BIAS_EPIS = (BF16, GELU, ADDR, F32, RELU)


class Vacuous(Exception):
    """the element a fault would remove is zero in this draw: planting it would change nothing"""


def evaluate_fp32(case, fault=None, passes=1):
    """The buffers a correct fp32 GEMM leaves behind (or one with `fault` planted)."""
    c = case
    M, N, K, layout, epi = c.M, c.N, c.K, c.layout, c.epi
    a, b = c.A.float(), c.B.float()
    dyn = c.dyn
    if fault == "dyn_off_by_one":
        assert dyn is not None and 0 < dyn < (K if layout == TN else M)
        dyn = dyn + 1
    rows, Kc = M, K
    if dyn is not None:
        if layout == TN:
            Kc = min(dyn, K)
        else:
            rows = min(dyn, M)
    if layout == TN:
        a = a[:Kc, :M].t().contiguous()          # [M, Kc]
        bt = b[:Kc, :N].contiguous()             # [Kc, N]
    else:
        a = a[:M, :K].contiguous()
        bt = b[:N, :K].t().contiguous() if layout == NT else b[:K, :N].contiguous()
    if fault == "drop_last_k":
        if float(a[M - 1, Kc - 1]) == 0 or not bool((bt[Kc - 1] != 0).any()):
            raise Vacuous
        a[M - 1, Kc - 1] = 0
    if fault == "skip_kstep":
        assert Kc >= 64
        a[:, 32:64] = 0
    acc = a @ bt
    if fault == "double_kstep":
        assert Kc >= 64
        acc = acc + a[:, 32:64] @ bt[32:64]
    bias = c.bias.clone() if (c.bias is not None and epi != MULR) else None
    if fault == "no_bias_ragged":
        first = (N - 1) // 4 * 4
        if not bool((bias[first:N] != 0).all()):
            raise Vacuous
        bias[first:N] = 0
    R = c.R.float()[:M, :N].clone() if c.R is not None else None
    if fault == "r_last_zero":
        if float(R[M - 1, N - 1]) == 0:
            raise Vacuous
        R[M - 1, N - 1] = 0
    got = {k: g.flat.clone() for k, g in c.out.items()}
    cview = c.out["C"].view(got["C"])
    for _ in range(passes):
        u = acc if bias is None else acc + bias
        if epi == F32_ACC and fault != "acc_overwrite":
            u = u + cview[:M, :N]
        out2 = None
        if epi in (BF16, F32, F32_ACC):
            out = u
        elif epi == RELU:
            out = torch.relu(u)
        elif epi == ADDR:
            out = u + R
        elif epi == MULR:
            out = u * R
        else:
            cdf = 0.5 * (1.0 + torch.erf(u * 0.7071067811865476))
            out, out2 = u * cdf, cdf + u * torch.exp(-0.5 * u * u) * 0.3989422804014327
        if fault == "row_from_neighbour_tile":
            assert M > 128 and rows > 128
            out = out.clone()
            out[0] = out[128]
        cview[:rows, :N] = out[:rows].to(cview.dtype)
        if epi == F32 and c.n_store > N:
            cview[:rows, N:c.n_store] = 0
        if out2 is not None:
            c.out["C2"].view(got["C2"])[:rows, :N] = out2[:rows].to(torch.bfloat16)
        if c.bias_grad:
            bg = c.out["bias_grad"].view(got["bias_grad"])
            s = a.sum(dim=1)
            bg[0, :M] = s + bg[0, :M] if epi == F32_ACC else s
    return got


def epilogues_of(layout):
    return [F32, F32_ACC] if layout == TN else [BF16, GELU, MULR, ADDR, F32, RELU, F32_ACC]


def families_of(epi):
    return ["gauss"] if epi == GELU else ["gauss", "int"]


def matrix_case(layout, epi, M, N, family, seed=0):
    """a case of the epilogue x layout matrix of the GPU tests (same constructor arguments as there)"""
    K = 96 + 37 if layout == TN else 96
    wide = (N in (197, 200)) == (M == 300)
    return G.Case(layout, epi, M, N, K, family, seed=seed + M * 1000 + N, ldc=None if M == 300 else G._up(N, 8) + 16,
                  ldr_extra=8 if wide else 0, n_store=G._up(N, 4) + 4 if (epi == F32 and M == 300) else 0,
                  bias_grad=layout == TN)


@pytest.mark.parametrize("layout", [NT, NN, TN], ids=["NT", "NN", "TN"])
def test_a_correct_fp32_evaluation_is_accepted(layout):
    worst = G.Worst()
    n = 0
    for epi in epilogues_of(layout):
        for family in families_of(epi):
            for M in (300, 129):
                for N in (197, 198, 199, 200):
                    case = matrix_case(layout, epi, M, N, family)
                    passes = 2 if epi == F32_ACC else 1
                    msgs = case.check(evaluate_fp32(case, passes=passes), passes=passes, worst=worst)
                    assert not msgs, msgs
                    n += 1
    assert n == len(epilogues_of(layout)) * 16 - (8 if layout != TN else 0)
    assert worst.ratio <= 1.0


@pytest.mark.parametrize("layout", [NT, NN, TN], ids=["NT", "NN", "TN"])
def test_k_depths_and_device_counts_are_accepted(layout):
    for family in ("gauss", "int"):
        for M, N in ((256, 256), (300, 200)):
            ks = [32 * s for s in range(1, 12)] + ([1, 8, 37, 72, 100] if layout == NT else [])
            for K in ks:
                case = G.Case(layout, F32, M, N, K, family, seed=K)
                msgs = case.check(evaluate_fp32(case))
                assert not msgs, msgs
        for count in (0, 1, 255, 256, 257, 300, 1000):
            if layout == TN:
                cases = [G.Case(TN, e, 129, 198, 300, family, seed=count, dyn=count, bias_grad=True) for e in (F32, F32_ACC)]
            else:
                cases = [G.Case(layout, e, 300, 200, 96, family, seed=count, dyn=count) for e in (BF16, GELU, ADDR) if not (family == "int" and e == GELU)]
            for case in cases:
                msgs = case.check(evaluate_fp32(case))
                assert not msgs, msgs


def test_walk_and_split_shapes_are_accepted():
    for layout in (NT, NN):
        for epi in (BF16, GELU, ADDR):
            for M, K in ((0, 64), (1, 32), (257, 352), (300, 160)):
                case = G.Case(layout, epi, M, 2304, K, "gauss", seed=M + K, ldc=2304 + 16, ldr_extra=8)
                msgs = case.check(evaluate_fp32(case))
                assert not msgs, msgs
    for layout, epi in ((NT, ADDR), (TN, F32)):
        for M, N, K in ((300, 200, 128), (256, 256, 1920)):
            case = G.Case(layout, epi, M, N, K, "gauss", seed=K + M, bias_grad=layout == TN, ldr_extra=8)
            msgs = case.check(evaluate_fp32(case))
            assert not msgs, msgs


FAULTS = ["drop_last_k", "skip_kstep", "double_kstep", "no_bias_ragged", "r_last_zero", "row_from_neighbour_tile", "dyn_off_by_one", "acc_overwrite"]


def applies(fault, layout, epi):
    if fault == "no_bias_ragged":
        return epi in BIAS_EPIS
    if fault == "r_last_zero":
        return epi in (MULR, ADDR)
    if fault == "acc_overwrite":
        return epi == F32_ACC
    return True


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_faults_are_rejected(fault):
    n = 0
    for layout in (NT, NN, TN):
        for epi in epilogues_of(layout):
            if not applies(fault, layout, epi):
                continue
            for family in families_of(epi):
                for M, N in ((300, 199), (129, 198)):
                    for seed in range(3, 40):          # the first draw in which the fault removes something
                        if fault == "dyn_off_by_one":
                            K = 300 if layout == TN else 96
                            case = G.Case(layout, epi, M, N, K, family, seed=seed + N, dyn=100, bias_grad=layout == TN)
                        else:
                            case = matrix_case(layout, epi, M, N, family, seed=seed)
                        try:
                            faulty = evaluate_fp32(case, fault=fault)
                            break
                        except Vacuous:
                            continue
                    else:
                        raise AssertionError("no draw in which %s removes something" % fault)
                    assert not case.check(evaluate_fp32(case)), "the unmodified evaluation must pass"
                    msgs = case.check(faulty)
                    assert msgs, "%s was not caught: %s" % (fault, case.ident())
                    n += 1
    assert n >= 4


def test_guard_band_and_pad_columns_are_checked():
    case = matrix_case(NT, F32, 300, 199, "gauss")
    good = evaluate_fp32(case)
    assert not case.check(good)
    g = case.out["C"]
    for flat_index in (0, G.GUARD - 1, G.GUARD + g.col0 - 1, G.GUARD + g.col0 + case.n_store, G.GUARD + g.col0 + 300 * g.ld, good["C"].numel() - 1):
        bad = {k: v.clone() for k, v in good.items()}
        bad["C"][flat_index] = 1.0
        assert case.check(bad), flat_index
    bad = {k: v.clone() for k, v in good.items()}
    bad["C"][G.GUARD + g.col0 + 5 * g.ld + case.N] = 1e-30          # a pad column of [N, n_store) that is not an exact zero
    assert case.check(bad)
    case = matrix_case(NT, GELU, 129, 197, "gauss")
    good = evaluate_fp32(case)
    bad = {k: v.clone() for k, v in good.items()}
    bad["C2"][G.GUARD + case.out["C2"].col0 + case.N] = 0.0           # the element right of the last column of row 0
    assert not case.check(good) and case.check(bad)


def test_the_gelu_formula_error_is_the_measured_one():
    rel, absolute, deriv = G.measure_formula_error()
    print("gelu_both in fp32 against float64 over [-12, 12]: value %.3g relative to max(|x|, 1) (%.3g absolute), derivative %.3g absolute" % (rel, absolute, deriv))
    assert 0.5 * G.FORMULA_VALUE_REL_MEASURED <= rel <= G.FORMULA_VALUE_REL_MEASURED
    assert 0.5 * G.FORMULA_DERIV_ABS_MEASURED <= deriv <= G.FORMULA_DERIV_ABS_MEASURED
    assert G.FORMULA_FACTOR == 4.0


def test_bf16_rounding_is_nearest_even():
    x = torch.randn(4096, generator=torch.Generator().manual_seed(0)) * 3
    x[:4] = torch.tensor([1.00390625, 1.01171875, -1.00390625, 0.0])      # ties: to even
    want = x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert (G.bf16_bits(x.numpy()) == want).all()
    assert (G.bf16_value(want) == x.to(torch.bfloat16).double().numpy()).all()


def test_the_dispatcher_rejects_a_residual_it_cannot_bound():
    """MULR / ADDR read R four bytes at a time under a per-dword bounds check whose extent ends on an even element count inside ldr: an odd
    ldr (or one below N) is rejected on the host, before any launch."""
    from volta_amd import _lib as L
    fake = 0x10000          # never dereferenced: the argument checks come first
    for ldr, ok_text in ((199, b"ldr must be even"), (196, b"ldr must be even and >= N")):
        p = L.GemmProblem(fake, fake, fake, None, None, fake, None, None, 300, 197, 128, 128, 128, 200, ldr, 0)
        arr = (L.GemmProblem * 1)(p)
        for epi in (L.EPI_MULR, L.EPI_ADDR):
            assert L.lib.vk_gemm_grouped_ex(L.NT, epi, arr, 1, 128, None) != 0
            assert ok_text in L.lib.vk_last_error(), L.lib.vk_last_error()
