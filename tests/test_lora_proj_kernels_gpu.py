"""vk_lora_proj_fwd / vk_lora_proj_bwd on their own (csrc/lora.hip), against the float64 restatement and bounds of tests/lora_restate.py.

The buffers, sentinels and stage-by-stage comparison are those of tests/test_lora_kernels_gpu.py: every output lies inside a wider buffer of
position-dependent NaN sentinels compared as raw bits (rows below M, guards in front and behind, the pad columns of ld = width + 8), every
case runs twice into fresh buffers and must give the same bits, and no element is left out of a comparison.  The bounds, none tuned:
    T, Y (act = 0), dT, dA, dB, dX    lora_restate's own
    act = 1                           v, e_acc = ref_Y(...);  Y: e_f = 1.13 e_acc + e_formula_value(v),  G: e_f = 0.80 e_acc + e_formula_deriv(v)
                                      (gemm_restate's GELU bounds: the kernel runs the GEMM epilogue's gelu_both)
    R != NULL                         delta, e_acc = the adapter term sum_c dT_c A_c and its accumulation bound;  ref = dXprev + R delta,
                                      e_f = |R| e_acc + |R delta| 2^-24  (gemm_restate's VK_EPI_MULR bound; the kernel adds dXprev inside the
                                      same fused multiply-add, so the add has no rounding of its own)
each then through |out - ref| <= e_f + 2^-8 (|ref| + e_f).

Shapes: M = 1, 17 (a ragged 4-row lane group), 65 (one row past a 64-row workgroup of the row products), 300 (two 256-row blocks of the
partial sums); the long dimension at one 64-column tile, at the old cap 1024 (exactly one LDS chunk), at 1088 (one tile past it: a second,
short chunk), at the feed-forward width 3072 and at the new cap 4096 -- on the K side (T, dA, dX) and on the N side (dT, dB, Y).  r = 4 and
32 at the extremes (32 rows x one chunk fills the 64 KB stage; 4 takes the most row groups per wave), 8 and 16 once each."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_restate as GR  # noqa: E402
import lora_restate as R  # noqa: E402
import test_lora_kernels_gpu as K0  # noqa: E402  (Grid, Flat and the bit-level transfers)

pytestmark = pytest.mark.gpu
Grid, Flat, dev16 = K0.Grid, K0.Flat, K0.dev16


def P(st=0, ad=0, act=0, frozen=False):
    return dict(st=st, ad=ad, act=act, frozen=frozen)


def one(M, K, N, r, act=0, dx=True, rho=False, frozen=False, acc_first=False):
    return dict(r=r, streams=[(M, K, N)], probs=[P(act=act, frozen=frozen)], dx=[dx], rho=[rho], acc_first=acc_first)


# streams: [(M, K, N)], each with one X, one dX (dx) and one R (rho); a problem names its stream and its adapter, has its own Y / dY (/ G)
CASES = {
    "m1_k64_n64_r4": one(1, 64, 64, 4),
    "m17_k4096_n64_r4": one(17, 4096, 64, 4),
    "m17_k64_n4096_r4_gelu": one(17, 64, 4096, 4, act=1),
    "m65_k4096_n64_r32_rho": one(65, 4096, 64, 32, rho=True),
    "m65_k64_n4096_r32": one(65, 64, 4096, 32),
    "m300_k1088_n64_r32": one(300, 1088, 64, 32),
    "m300_k64_n1088_r4": one(300, 64, 1088, 4),
    "m17_k1024_n1024_r32": one(17, 1024, 1024, 32),
    "m65_k3072_n768_r8_rho": one(65, 3072, 768, 8, rho=True),                 # the FFN-down adapter's shape
    "m65_k768_n3072_r16_gelu": one(65, 768, 3072, 16, act=1),                 # the FFN-up adapter's shape
    "m300_k3072_n768_r32_rho": one(300, 3072, 768, 32, rho=True),
    "m300_k768_n3072_r4_gelu": one(300, 768, 3072, 4, act=1),
    "m1_k4096_n4096_r32_gelu_rho": one(1, 4096, 4096, 32, act=1, rho=True),
    "m300_k4096_n1088_r4": one(300, 4096, 1088, 4),
    "m65_k1088_n1024_r4_no_dx": one(65, 1088, 1024, 4, dx=False),             # dX = NULL: only dA and dB
    "m17_k1088_n64_r32_frozen": one(17, 1088, 64, 32, frozen=True),           # dA = dB = NULL: only the share of dX
    "m17_k3072_n1088_r32_frozen_rho": one(17, 3072, 1088, 32, frozen=True, rho=True),
    "m65_k64_n1088_r4_accumulate_first": one(65, 64, 1088, 4, acc_first=True),
    # one adapter shared by two streams of different M: the second source accumulates, gradients summed in list order
    "shared_two_sources": dict(r=32, streams=[(17, 1088, 192), (300, 1088, 192)], probs=[P(0, 0), P(1, 0)], dx=[True, False], rho=[False, False]),
    # two adapters add into one dX, through one R, in one read-modify-write; the second one is frozen
    "two_into_one_dx_rho": dict(r=4, streams=[(65, 3072, 128)], probs=[P(0, 0), P(0, 1, frozen=True)], dx=[True], rho=[True]),
    # the GELU and the plain forward in one call (a feed-forward sub-layer with an adapter on one stream's up projection only)
    "mixed_act_two_streams": dict(r=32, streams=[(17, 192, 3072), (65, 192, 1088)], probs=[P(0, 0, act=1), P(1, 1)], dx=[True, True], rho=[False, False]),
}
assert 16 <= len(CASES) + 1 <= 24          # + the refusal test


def run_case(case, check):
    """One forward and one backward call on fresh buffers.  -> every output's bits.  check: compare with the restatement."""
    from volta_amd import ops
    rng = np.random.default_rng(4321)
    r, probs, acc_first = case["r"], case["probs"], case.get("acc_first", False)
    q16 = lambda a: R.bf16_value(R.bf16_bits(a))
    fam, ad = {}, {}
    for i, p in enumerate(probs):
        M, K, N = case["streams"][p["st"]]
        fam[i] = R.family("gauss", rng, M, K, N, r)
        if p["ad"] in ad:                      # a shared adapter: the later problem takes the first one's A and B
            fam[i]["A"], fam[i]["B"] = ad[p["ad"]]["A"], ad[p["ad"]]["B"]
        else:
            ad[p["ad"]] = dict(A=fam[i]["A"], B=fam[i]["B"], K=K, N=N, frozen=p["frozen"])
    s = fam[0]["s"]
    # ---- buffers: per stream X, dX, R; per problem Y, dY, G, T, dT; per adapter dA, dB
    xg, dxg, rg, dxprev, rho = {}, {}, {}, {}, {}
    for st, (M, K, N) in enumerate(case["streams"]):
        first = next(i for i, p in enumerate(probs) if p["st"] == st)
        xg[st], dxg[st] = Grid(M, K + 8, 11 * st), Grid(M, K + 8, 5 + st)
        xg[st].put(0, fam[first]["X"])
        dxprev[st] = fam[first]["dXprev"]
        dxg[st].put(0, dxprev[st])
        if case["dx"][st]:
            dxg[st].mark(0, K)
        for i, p in enumerate(probs):
            if p["st"] == st:
                fam[i]["X"] = fam[first]["X"]
        grids = [xg[st], dxg[st]]
        if case["rho"][st]:
            rho[st] = q16(GR.gelu64(rng.standard_normal((M, K)) * 1.5)[1])          # what a GELU epilogue leaves: gelu' of pre-activations
            rg[st] = Grid(M, K + 16, 17 + st)
            rg[st].put(0, rho[st])
            grids.append(rg[st])
        for g in grids:
            g.upload()
    yg, dyg, gg = {}, {}, {}
    for i, p in enumerate(probs):
        M, K, N = case["streams"][p["st"]]
        yg[i], dyg[i] = Grid(M, N + 8, 7 + i), Grid(M, N + 8, 3 + i)
        yg[i].put(0, fam[i]["Yprev"])
        yg[i].mark(0, N)
        dyg[i].put(0, fam[i]["dY"])
        yg[i].upload(), dyg[i].upload()
        if p["act"]:
            gg[i] = Grid(M, N + 16, 23 + i)
            gg[i].mark(0, N)
            gg[i].upload()
    Tb = {i: Flat(case["streams"][p["st"]][0] * r, 100 + i) for i, p in enumerate(probs)}
    dTb = {i: Flat(case["streams"][p["st"]][0] * r, 200 + i) for i, p in enumerate(probs)}
    Ad = {a: dev16(R.bf16_bits(v["A"])) for a, v in ad.items()}
    Bd = {a: dev16(R.bf16_bits(v["B"])) for a, v in ad.items()}
    prevA = {a: (rng.integers(-8, 9, (r, v["K"])).astype(np.float64) if acc_first else None) for a, v in ad.items()}
    prevB = {a: (rng.integers(-8, 9, (v["N"], r)).astype(np.float64) if acc_first else None) for a, v in ad.items()}
    dAb = {a: Flat(r * v["K"], 300 + a, f32=True, prev=prevA[a]) for a, v in ad.items()}
    dBb = {a: Flat(v["N"] * r, 400 + a, f32=True, prev=prevB[a]) for a, v in ad.items()}
    # ---- problems
    fwd, bwd, seen = [], [], set()
    for i, p in enumerate(probs):
        st, a = p["st"], p["ad"]
        M, K, N = case["streams"][st]
        T = Tb[i].view((M, r))
        fwd.append(ops.lora_proj_problem(xg[st].view(0, K), Ad[a], Bd[a], T, yg[i].view(0, N), s, G=gg[i].view(0, N) if p["act"] else None))
        frozen = ad[a]["frozen"]
        bwd.append(ops.lora_proj_bwd_problem(xg[st].view(0, K), Ad[a], Bd[a], T, dyg[i].view(0, N), dTb[i].view((M, r)),
                                             dxg[st].view(0, K) if case["dx"][st] else None,
                                             None if frozen else dAb[a].view((r, K)), None if frozen else dBb[a].view((N, r)), s,
                                             R=rg[st].view(0, K) if case["rho"][st] else None, accumulate=(a in seen) or (acc_first and i == 0)))
        seen.add(a)
    ops.lora_proj_fwd(fwd)
    torch.cuda.synchronize()
    T = {i: Tb[i].after() for i in Tb}
    Y = {i: yg[i].after() for i in yg}
    G = {i: gg[i].after() for i in gg}
    for st in xg:
        xg[st].after()
    # ---- backward
    ops.lora_proj_bwd(bwd)
    torch.cuda.synchronize()
    dT = {i: dTb[i].after() for i in dTb}
    dA = {a: dAb[a].after(written=not ad[a]["frozen"]) for a in dAb}
    dB = {a: dBb[a].after(written=not ad[a]["frozen"]) for a in dBb}
    dX = {st: dxg[st].after() for st in dxg}
    for st in xg:
        xg[st].after()
        if st in rg:
            rg[st].after()
    for i in Tb:
        dyg[i].after()
        assert np.array_equal(yg[i].after(), Y[i]), "the backward changed Y"
        assert np.array_equal(Tb[i].after(), T[i]), "the backward changed T"
        if i in gg:
            assert np.array_equal(gg[i].after(), G[i]), "the backward changed G"
    out = dict(T=T, Y=Y, G=G, dT=dT, dA=dA, dB=dB, dX=dX)
    if not check:
        return out
    # ---- the restatement, stage by stage
    worst = {}

    def cmp16(name, bits, ref, e):
        worst[name] = max(worst.get(name, 0.0), R.worst_bf16(bits, ref, e))

    def cmp32(name, bits, ref, e):
        worst[name] = max(worst.get(name, 0.0), R.worst_f32(bits.view(np.float32), ref, e))

    Tv, dTv = {}, {}
    for i, p in enumerate(probs):
        M, K, N = case["streams"][p["st"]]
        f = fam[i]
        cmp16("T", T[i].reshape(M, r), *R.ref_T(f["X"], f["A"]))
        Tv[i] = R.bf16_value(T[i]).reshape(M, r)
        v, e = R.ref_Y(f["Yprev"], Tv[i], f["B"], s)
        if p["act"]:
            y, d = GR.gelu64(v)
            cmp16("Y_gelu", Y[i][:M, :N], y, 1.13 * e + GR.e_formula_value(v))
            cmp16("G", G[i][:M, :N], d, 0.80 * e + GR.e_formula_deriv(v))
        else:
            cmp16("Y", Y[i][:M, :N], v, e)
        cmp16("dT", dT[i].reshape(M, r), *R.ref_dT(f["dY"], f["B"], s))
        dTv[i] = R.bf16_value(dT[i]).reshape(M, r)
    for a, v in ad.items():
        if v["frozen"]:
            continue
        src = [i for i, p in enumerate(probs) if p["ad"] == a]
        cmp32("dB", dB[a].reshape(v["N"], r), *R.ref_dB([(fam[i]["dY"], Tv[i], s) for i in src], prevB[a]))
        cmp32("dA", dA[a].reshape(r, v["K"]), *R.ref_dA([(dTv[i], fam[i]["X"]) for i in src], prevA[a]))
    for st, (M, K, N) in enumerate(case["streams"]):
        if not case["dx"][st]:
            continue
        mem = [(dTv[i], fam[i]["A"]) for i, p in enumerate(probs) if p["st"] == st]
        if case["rho"][st]:
            delta, e = R.ref_dX(np.zeros((M, K)), mem)
            cmp16("dX_rho", dX[st][:M, :K], dxprev[st] + rho[st] * delta, np.abs(rho[st]) * e + np.abs(rho[st] * delta) * R.U24)
        else:
            cmp16("dX", dX[st][:M, :K], *R.ref_dX(dxprev[st], mem))
    print({k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_lora_proj_kernels(name):
    case = CASES[name]
    first = run_case(case, check=True)
    again = run_case(case, check=False)
    for key in first:
        for k in first[key]:
            assert np.array_equal(first[key][k], again[key][k]), "%s[%s] differs between two launches" % (key, k)


def test_refusals():
    """Bad arguments are refused on the host, before any launch: every buffer keeps its sentinels."""
    from volta_amd import _lib as L
    M, W = 4, 4224
    names = ("X", "A", "B", "T", "Y", "G", "dY", "dT", "dX", "R", "R2")
    bits = {n: R.sentinels16(M * W, 31 * i) for i, n in enumerate(names)}
    t = {n: dev16(b) for n, b in bits.items()}
    g32 = {n: R.sentinels32(32 * W, 7 * i) for i, n in enumerate(("dA", "dB", "work"))}
    t32 = {n: K0.dev32(b) for n, b in g32.items()}
    a = lambda n, off=0: t[n].data_ptr() + off
    err = lambda: L.lib.vk_last_error().decode()

    def fwd(n=1, **kw):
        d = dict(X=a("X"), A=a("A"), B=a("B"), T=a("T"), Y=a("Y"), G=None, dyn=None, M=M, K=64, N=64, r=4, ldx=64, ldy=64, ldg=0, scale=1.0, act=0)
        d.update(kw)
        arr = (L.LoraProjProblem * 2)(L.LoraProjProblem(**d), L.LoraProjProblem(**d))
        return L.lib.vk_lora_proj_fwd(arr, n, None)

    def bwd_problem(**kw):
        d = dict(X=a("X"), A=a("A"), B=a("B"), T=a("T"), dY=a("dY"), dT=a("dT"), dX=a("dX"), dA=t32["dA"].data_ptr(), dB=t32["dB"].data_ptr(), R=None, dyn=None,
                 M=M, K=64, N=64, r=4, ldx=64, ldy=64, lddx=64, ldr=0, accumulate=0, scale=1.0)
        d.update(kw)
        return L.LoraProjBwdProblem(**d)

    def bwd(*ps, n=None):
        arr = (L.LoraProjBwdProblem * max(1, len(ps)))(*ps)
        return L.lib.vk_lora_proj_bwd(arr, len(ps) if n is None else n, t32["work"].data_ptr(), None)

    assert fwd(K=4160, ldx=4160) != 0 and "K = 4160" in err() and "problem 0" in err()
    assert fwd(N=4160, ldy=4160) != 0 and "N = 4160" in err()
    assert fwd(K=96, ldx=96) != 0 and "K = 96" in err()
    assert fwd(r=12) != 0 and "r = 12" in err()
    assert fwd(act=1) != 0 and "act = 1" in err() and "G" in err()
    assert fwd(act=1, G=a("G"), ldg=60) != 0 and "ldg" in err()
    assert fwd(act=0, G=a("G"), ldg=64) != 0 and "act = 0" in err()
    assert fwd(act=2) != 0
    assert fwd(X=None) != 0 and "NULL operand 0" in err()
    assert fwd(Y=a("Y", 2)) != 0 and "operand 4 is not 16-byte aligned" in err()
    assert fwd(ldx=60) != 0 and "leading" in err()
    assert fwd(n=0) != 0 and "0 problems" in err()
    assert fwd(n=7) != 0
    assert fwd(n=2) != 0 and "problems 0 and 1" in err()                         # both write the same T and Y
    assert bwd(bwd_problem(K=4160, ldx=4160, lddx=4160)) != 0 and "K = 4160" in err()
    assert bwd(bwd_problem(K=96, ldx=96, lddx=96)) != 0 and "K = 96" in err()
    assert bwd(bwd_problem(r=12)) != 0 and "r = 12" in err()
    assert bwd(bwd_problem(dT=None)) != 0 and "NULL operand 5" in err()
    assert bwd(bwd_problem(dX=a("dX", 4))) != 0 and "dX" in err()
    assert bwd(bwd_problem(R=a("R", 6), ldr=64)) != 0 and "R alignment" in err()
    assert bwd(bwd_problem(dA=None)) != 0 and "frozen" in err()
    assert bwd(bwd_problem(dA=None, dB=None, dX=None)) != 0 and "no output" in err()
    two = (bwd_problem(R=a("R"), ldr=64), bwd_problem(R=a("R2"), ldr=64, dT=a("dT", 1024), dA=None, dB=None))
    assert bwd(*two) != 0 and "problem 1" in err() and "one R" in err()          # two problems on one dX with different R
    assert bwd(bwd_problem(R=a("R"), ldr=64), bwd_problem(dT=a("dT", 1024), dA=None, dB=None)) != 0 and "one R" in err()
    assert bwd(bwd_problem(), n=0) != 0 and "0 problems" in err()
    assert L.lib.vk_lora_proj_bwd((L.LoraProjBwdProblem * 1)(bwd_problem()), 1, None, None) != 0 and "workspace" in err()
    assert L.lib.vk_lora_proj_bwd_work_bytes((L.LoraProjBwdProblem * 1)(bwd_problem()), 0) < 0
    torch.cuda.synchronize()
    for n in t:
        assert np.array_equal(K0.host16(t[n]), bits[n]), "%s changed" % n
    for n in t32:
        assert np.array_equal(K0.host32(t32[n]), g32[n]), "%s changed" % n
