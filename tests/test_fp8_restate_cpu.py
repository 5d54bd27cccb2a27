"""tests/fp8_restate.py against itself and against torch.float8_e4m3fn: the bit-arithmetic encode / decode, the fp32 emulations inside
their own float64 gates on every case of the tables (zero exemptions), every planted bug caught on the cases named for it, and the
exactness condition of the integer family.  CPU only."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_restate as R  # noqa: E402
import gemm_restate as G  # noqa: E402


def torch_bytes(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def test_decode_agrees_with_torch_on_all_256_bytes():
    b = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(b).view(torch.float8_e4m3fn).double().numpy()
    got = R.e4m3_decode(b)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and int(np.isnan(got).sum()) == 2
    fin = ~np.isnan(got)
    assert np.array_equal(got[fin], want[fin]) and np.array_equal(np.signbit(got[fin]), np.signbit(want[fin]))
    assert np.array_equal(R.e4m3_encode(got[fin].astype(np.float32)), b[fin])          # every finite byte survives the round trip


def dense_sample():
    vals = R.e4m3_decode(np.arange(0x7F, dtype=np.uint8))[:0x7F]                # the non-negative finite values, ascending
    ties = 0.5 * (vals[1:] + vals[:-1])
    pts = np.concatenate([vals, ties, [464.0, 448.0, 2.0 ** -6, 2.0 ** -9, 2.0 ** -10, 0.0]]).astype(np.float32)
    near = np.concatenate([pts, np.nextafter(pts, np.float32(np.inf)), np.nextafter(pts, np.float32(-np.inf))])
    g = np.random.default_rng(5)
    dense = np.concatenate([near, g.uniform(0, 470, 200000).astype(np.float32), (g.uniform(0, 1, 200000) ** 8 * 0.05).astype(np.float32),
                            np.array([1e-30, 1e-45, 500.0, 1e30, np.inf], dtype=np.float32)])
    return np.concatenate([dense, -dense])


def test_encode_agrees_with_torch_on_a_dense_sample_with_every_tie():
    x = dense_sample()
    got = R.e4m3_encode(x)
    assert np.array_equal(got, torch_bytes(np.clip(x, -448, 448)))             # the clamp of pack4_fp8, then torch's conversion
    assert np.array_equal(R.e4m3_encode(x, "no_saturate"), torch_bytes(x))      # without it: NaN beyond 464, as torch gives
    assert R.e4m3_encode(np.float32([464.0]))[0] == 0x7E and R.e4m3_encode(np.float32([464.0]), "no_saturate")[0] == 0x7E
    assert R.e4m3_encode(np.float32([np.nextafter(np.float32(464), np.float32(500))]), "no_saturate")[0] == 0x7F
    t = R.e4m3_encode(x, "truncate")
    fin = np.isfinite(x)
    assert (np.abs(R.e4m3_decode(t[fin])) <= np.minimum(np.abs(x[fin]), 448)).all()
    assert R.e4m3_encode(np.float32([-0.0, -1e-9]))[0] == 0x80 and R.e4m3_encode(np.float32([-0.0, -1e-9]))[1] == 0x80


def test_half_ulp_is_the_one_of_ln_restate():
    x = np.array([0.0, 2.0 ** -9, 2.0 ** -6, 1.0, 1.9, 2.0, 447.0, 448.0])
    assert np.array_equal(R.half_ulp_e4m3(x), [2.0 ** -10, 2.0 ** -10, 2.0 ** -10, 2.0 ** -4, 2.0 ** -4, 2.0 ** -3, 16.0, 16.0])


QUANT = R.quant_cases()


def test_quantiser_emulation_inside_its_gates_on_every_case():
    assert len(QUANT) == 2 * (21 + 10)
    msgs = []
    for c in QUANT:
        msgs += c.check(*c.emulate())
    assert not msgs, "\n".join(msgs[:20])


@pytest.mark.parametrize("bug", list(R.PLANTED_QUANT))
def test_planted_quantiser_bug_is_caught(bug):
    named = R.PLANTED_QUANT[bug](QUANT)
    assert len(named) >= 4
    missed = [c.ident() for c in named if not c.check(*c.emulate(bug))]
    assert not missed, "%s passes on %s" % (bug, missed)


def test_cast_emulation_inside_its_gate():
    bits = R.cast_source_bits()
    assert bits.size % 8 == 0 and bits.size >= 65282
    for mul in R.CAST_MULS:
        q = R.emulate_cast(bits, mul)
        assert not R.cast_gate(bits, mul, q)
        with np.errstate(over="ignore"):
            assert np.array_equal(q, torch_bytes(np.clip(R.bf16_to_f32(bits) * np.float32(mul), -448, 448)))


@pytest.mark.parametrize("bug", ["truncate", "no_saturate"])
def test_planted_cast_bug_is_caught(bug):
    bits = R.cast_source_bits()
    for mul in R.CAST_MULS:
        assert R.cast_gate(bits, mul, R.emulate_cast(bits, mul, bug)), (bug, mul)


def test_gemm_emulation_inside_its_bounds_on_every_case():
    """the fp32 emulation of every GEMM case, buffers and all, passes the very check the kernel's outputs go through"""
    cases = R.all_gemm_cases()
    assert len(cases) > 300
    msgs = []
    for c in cases:
        msgs += c.check(R.emulate_gemm(c))
    for N in (40960, 40704):
        for c in R.auto_cases(N):
            msgs += c.check(R.emulate_gemm(c))
    assert not msgs, "\n".join(msgs[:20])


@pytest.mark.parametrize("bug", list(R.PLANTED_GEMM))
def test_planted_gemm_bug_is_caught(bug):
    named = R.PLANTED_GEMM[bug]()
    assert len(named) >= 4
    missed = [c.ident() for c in named if not c.check(R.emulate_gemm(c, bug))]
    assert not missed, "%s passes on %s" % (bug, missed)


def test_integer_family_stays_exact_in_fp32():
    seen = 0
    for c in R.all_gemm_cases() + R.auto_cases(40960) + R.auto_cases(40704):
        if c.family == "int":
            mag = c.ops.mag + (np.abs(c.ops.bias[:c.N]) if c.ops.bias is not None else 0.0)
            assert (mag.max() if mag.size else 0.0) * 8 + 64 < 2 ** 24, c.ident()
            assert c.ops.acc.size == 0 or np.array_equal(c.ops.acc, np.rint(c.ops.acc))
            seen += 1
    assert seen > 100


def test_pad_contract_is_asserted():
    o = R.operands(300, 200, 200, "gauss", 300200)
    a = o.A8.copy()
    a[7, 201] = 0x38
    with pytest.raises(AssertionError):
        R.assert_pad_contract(a, o.B8, 300, 200, 200)
    b = o.B8.copy()
    b[0, 255] = 0x7F
    with pytest.raises(AssertionError):
        R.assert_pad_contract(o.A8, b, 300, 200, 200)
    b[0, 255] = 0x7E
    R.assert_pad_contract(o.A8, b, 300, 200, 200)


def test_guards_see_a_stray_write():
    c = R.c8_cases()[0]
    got = R.emulate_gemm(c)
    got["c8"][R.GUARD + 8 + c.N] ^= 1                       # the byte right behind row 0
    got["C"].view(torch.int16)[G.GUARD - 1] ^= 1
    msgs = c.check(got)
    assert any("c8:" in m and "outside" in m for m in msgs) and any("C:" in m and "outside" in m for m in msgs)
