"""The row grouping of the LayerNorm kernels (csrc/layernorm.hip): a forward wave takes one row of a 4-row workgroup, a backward wave
walks 4 rows of a 16-row workgroup with gamma and the rows' statistics fetched once and the Philox keys and uniform counter words on the
scalar unit.  Through the C ABI, on the NaN-padded, canary-filled buffers of tests/test_ln_kernels_gpu.py, against the float64 restatement
of tests/ln_restate.py under its gates -- never against the kernels themselves:
  * H in {768, 1024, 260} x M in {1, 3, 4, 5, 15, 16, 17, 33}: a row first, in the middle and last in a wave's group and in a workgroup,
    waves without a row; dropout off / before / after the normalisation, with and without the residual and addvec;
  * paired launches, `dyn` below M;
  * position independence, without any reference: row r of a launch over M rows has the bits of row r of a launch over r + 1 rows;
  * the generator: the Philox words behind the keep decisions, pinned from both sides by two thresholds per word;
  * every launch twice on fresh buffers, same bits."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ln_restate as A  # noqa: E402
import test_ln_kernels_gpu as K  # noqa: E402

pytestmark = pytest.mark.gpu

HS = (768, 1024, 260)
MS = (1, 3, 4, 5, 15, 16, 17, 33)
VARIANTS = [(mode, x, addvec) for mode in ("none", "pre", "post") for x in (True, False) for addvec in (False, True)]


def _run_case(case):
    """Forward and backward of one case, each twice on fresh buffers: gates, write sets, NaN-freedom, repeatability."""
    inp = A.make_inputs(case)
    fwd, (zb, mean, rstd), bwd = K._refs(case, inp)
    f1 = K.Fwd(inp, case.z, case.dyn, case.y8).run().host()
    job = K.Fwd(inp, case.z, case.dyn, case.y8).run()
    K._compare_fwd(case.id, job, job.host(), fwd)
    K._same_bits(case.id, f1, job.host())
    b1 = K.Bwd(inp, zb, mean, rstd, case.dd, case.dyn, case.acc).run().host()
    job = K.Bwd(inp, zb, mean, rstd, case.dd, case.dyn, case.acc).run()
    K._compare_bwd(case.id, job, job.host(), bwd)
    K._same_bits(case.id, b1, job.host())


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("M", MS)
def test_rows_and_widths(M, H):
    for k, (mode, x, addvec) in enumerate(VARIANTS):
        _run_case(A._c(M, H, mode, "randn", split=bool(k & 1) and M > 1, addvec=addvec, x=x, z=("own", "alias", "null")[k % 3], y8=(k % 4 == 3),
                       name="rows-M%d-H%d-%s-x%d-a%d" % (M, H, mode, x, addvec)))


PAIRS = [(5, 18, 768), (16, 1, 768), (0, 7, 768)]


@pytest.mark.parametrize("Ma,Mb,H", PAIRS, ids=["Ma%d-Mb%d-H%d" % p for p in PAIRS])
def test_pairs(Ma, Mb, H):
    """vk_ln_fwd_pair / vk_ln_bwd_pair: each job inside its own gates and write sets, twice with the same bits."""
    L = K._lib()
    cases = K._pair_cases(Ma, Mb, H)
    inps = [A.make_inputs(c) for c in cases]
    frefs = [A.restate_fwd(i) for i in inps]
    bins = [A.backward_inputs(f) for f in frefs]
    brefs = [A.restate_bwd(i, *b) for i, b in zip(inps, bins)]
    fouts, bouts = [], []
    for _ in range(2):
        jobs = [K.Fwd(i) for i in inps]
        L.check(L.lib.vk_ln_fwd_pair(C.byref(jobs[0].args), C.byref(jobs[1].args), L.stream_ptr()))
        torch.cuda.synchronize()
        fouts.append([j.host() for j in jobs])
        for c, j, o, r in zip(cases, jobs, fouts[-1], frefs):
            K._compare_fwd(c.id, j, o, r)
        jobs = [K.Bwd(i, *b) for i, b in zip(inps, bins)]          # separate dgamma / dbeta: each job assigns its own
        L.check(L.lib.vk_ln_bwd_pair(C.byref(jobs[0].args), C.byref(jobs[1].args), L.stream_ptr()))
        torch.cuda.synchronize()
        bouts.append([j.host() for j in jobs])
        for c, j, o, r in zip(cases, jobs, bouts[-1], brefs):
            if j.M > 0:
                K._compare_bwd(c.id, j, o, r)
            else:           # a job without rows: the empty column sums, nothing else written
                assert bool((o["dgamma"][:H] == 0).all()) and bool((o["dbeta"][:H] == 0).all())
                assert bool((K._bits(o["partial"]) == K.CAN32).all())
    for c, o1, o2 in zip(cases, fouts[0] + bouts[0], fouts[1] + bouts[1]):
        K._same_bits(c.id, o1, o2)


def test_dyn_below_m():
    """The single-job path with a device row count inside a wave's group and inside a workgroup."""
    for M, dyn in ((17, 6), (33, 18)):
        _run_case(A._c(M, 768, "pre", "randn", split=True, addvec=True, dyn=dyn, name="rows-dyn-M%d-dyn%d" % (M, dyn)))


def test_position_independence():
    """Row r of a launch over M rows equals, bit for bit, row r of a launch over r + 1 rows of the same buffers: forward y, z, mean, rstd;
    backward dz, dd."""
    M, H, rows = 17, 768, (0, 3, 4, 15, 16)
    case = A._c(M, H, "pre", "randn", split=True, addvec=True, name="position-M%d" % M)
    inp = A.make_inputs(case)
    zb, mean, rstd = A.backward_inputs(A.restate_fwd(inp))
    full_f = K.Fwd(inp).run().host()
    full_b = K.Bwd(inp, zb, mean, rstd).run().host()
    for r in rows:
        f = K.Fwd(inp)
        f.args.M = r + 1
        short = f.run().host()
        for key in ("y", "z", "mean", "rstd"):
            assert torch.equal(K._bits(short[key][r]), K._bits(full_f[key][r])), "forward %s: row %d depends on its place in the group" % (key, r)
            assert bool((K._bits(short[key][r + 1:]) == (K.CAN16 if key in ("y", "z") else K.CAN32)).all()), "forward %s: written past row %d" % (key, r)
        b = K.Bwd(inp, zb, mean, rstd)
        b.args.M = r + 1
        short = b.run().host()
        for key in ("dz", "dd"):
            assert torch.equal(K._bits(short[key][r]), K._bits(full_b[key][r])), "backward %s: row %d depends on its place in the group" % (key, r)
            assert bool((K._bits(short[key][r + 1:]) == K.CAN16).all()), "backward %s: written past row %d" % (key, r)


def _tuples():
    """64 (seed, row, site, c4): c4 = 0, row = 2^32 - 1, seed_hi != 0 and == 0 among them."""
    rng = np.random.RandomState(7)
    seeds = (A.SEED, 0x0123456789ABCDEF, 0x00000000DEADBEEF, 0xFFFFFFFF00000001)
    fixed = [(A.SEED, 0xFFFFFFFF, 11, 0), (0x00000000DEADBEEF, 0, 0, 0), (0xFFFFFFFF00000001, 0xFFFFFFFF, 0x7FFFFFFF, 191), (A.SEED, 1, 1, 511)]
    out = list(fixed)
    while len(out) < 64:
        k = len(out)
        row = int(rng.randint(0, 2 ** 31)) * 2 + int(rng.randint(0, 2)) if k % 3 else int(rng.randint(0, 40))
        out.append((seeds[k % 4], row, int(rng.randint(0, 2 ** 31)), int(rng.randint(0, 512)) if k % 5 else 0))
    return out


def test_generator_words():
    """The words behind the keep decisions are those of oracle.volta_ref.philox_u32.  A dropout-only launch (one row of ones, no residual,
    gamma = 1, beta = 0, scale 1) stores z = keep, and the backward (which draws the words again, on the 64-bit multiply) dd = keep dz:
    element c is kept at threshold w and dropped at threshold w + 1 exactly when its word is w.  The Philox row is set through seg[0] = (site, div, 0, row): launch row 0 maps to 0 / div * 0 + 0 % div + row."""
    from oracle import volta_ref as R
    from volta_amd import ops
    L = K._lib()
    Hmax = 2048
    ones = torch.ones(1, Hmax, dtype=torch.bfloat16, device=K.DEV)
    gamma, beta = torch.ones(Hmax, device=K.DEV), torch.zeros(Hmax, device=K.DEV)
    seed_t = torch.zeros(1, dtype=torch.int64, device=K.DEV)
    # backward inputs: dy alternates +-1 and z = dy, mean 0, rstd 1, gamma 1: s1 = 0, s2 = 1, dz = dy - z = ... would vanish, so z = 0.5 dy:
    # xh = 0.5 dy, s2 = mean(0.5 dy^2) = 0.5, dz = dy - 0.5 dy 0.5 = 0.75 dy: non-zero everywhere and exact in bf16
    dy = torch.ones(1, Hmax, dtype=torch.bfloat16, device=K.DEV)
    dy[:, 1::2] = -1.0
    zin = (0.5 * dy.float()).bfloat16()
    zero1, one1 = torch.zeros(1, device=K.DEV), torch.ones(1, device=K.DEV)
    checked = 0
    for seed, row, site, c4 in _tuples():
        H = 768 if c4 < 192 else 2048
        ops.set_seed(seed_t, seed)
        want = R.philox_raw(np.array([c4], np.uint32), np.array([row], np.uint32), np.array([site], np.uint32), np.zeros(1, np.uint32),
                            seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, rounds=R.DROPOUT_PHILOX_ROUNDS).reshape(4)
        if row < 64:                     # the same words through the entry the issue names
            assert np.array_equal(want, R.philox_u32(seed, site, row + 1, 4 * (c4 + 1))[row, 4 * c4:])
        segs = (L.DropRows * 2)()
        segs[0] = L.DropRows(site, 1 << 30, 0, row if row < 2 ** 31 else row - 2 ** 32)
        segs[1] = L.DropRows(site + 1, 0, 0, 0)
        for e in range(4):
            w = int(want[e])
            for thr, kept in ((w, 1.0), (w + 1, 0.0)):
                if thr == 0 or thr > 0xFFFFFFFF:           # threshold 0 is "dropout off"; no threshold drops the largest word
                    continue
                both = []
                for _ in range(2):
                    y = K._canary16((1, H))
                    z = K._canary16((1, H))
                    mean, rstd = K._canary32(1), K._canary32(1)
                    a = L.LnArgs(ones.data_ptr(), None, None, gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), z.data_ptr(), mean.data_ptr(),
                                 rstd.data_ptr(), None, 1, H, 1, 0, 1.0, L.Dropout(seed_t.data_ptr(), 999, thr, 1.0), segs)
                    L.check(L.lib.vk_ln_fwd(C.byref(a), L.stream_ptr()))
                    # the backward draws the same words (its own call of the generator): dd = keep dz, with dz != 0 by construction
                    dz, dd = K._canary16((1, H)), K._canary16((1, H))
                    partial = K._canary32(2 * H)
                    dg, db = K._canary32(H), K._canary32(H)
                    ab = L.LnBwdArgs(dy.data_ptr(), zin.data_ptr(), zero1.data_ptr(), one1.data_ptr(), gamma.data_ptr(), dz.data_ptr(), dd.data_ptr(),
                                     partial.data_ptr(), dg.data_ptr(), db.data_ptr(), None, 1, H, 1, 0, 1.0, 0, L.Dropout(seed_t.data_ptr(), 999, thr, 1.0), segs)
                    L.check(L.lib.vk_ln_bwd(C.byref(ab), L.stream_ptr()))
                    torch.cuda.synchronize()
                    both.append((z.cpu(), dz.cpu(), dd.cpu()))
                for t0, t1 in zip(*both):
                    assert torch.equal(K._bits(t0), K._bits(t1))
                zf, dzf, ddf = both[0]
                c = 4 * c4 + e
                msg = "seed %#x row %d site %d c4 %d word %d: threshold %#x, the oracle's word is %#x" % (seed, row, site, c4, e, thr, w)
                assert float(zf[0, c]) == kept, "forward keep = %r, %s" % (float(zf[0, c]), msg)
                assert float(dzf[0, c]) != 0.0
                assert float(ddf[0, c]) == kept * float(dzf[0, c]), "backward dd = %r, dz = %r, %s" % (float(ddf[0, c]), float(dzf[0, c]), msg)
                checked += 1
    assert checked >= 2 * 4 * 64 - 8
