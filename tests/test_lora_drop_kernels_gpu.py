"""vk_lora_fwd_drop / vk_lora_bwd_drop / vk_lora_proj_fwd_drop / vk_lora_proj_bwd_drop on their own (csrc/lora.hip), against the float64
restatement of tests/lora_drop_restate.py (the keep masks of oracle.volta_ref.philox_keep_mask) with the bounds of tests/lora_restate.py.

Buffers, sentinels and the stage-by-stage comparison are those of tests/test_lora_kernels_gpu.py / test_lora_proj_kernels_gpu.py: every
output lies inside a wider buffer of position-dependent NaN sentinels compared as raw bits (rows below M -- below *dyn where a case has
one --, guards in front and behind, the other column blocks of qkv, the pad columns of ld = width + 8), and no element is left out of a
comparison.  Every case runs
    p = 0.5, integer family     c = 2 is exact: every output BITWISE the float64 result (cases with a GELU or a saved gelu' take the
                                gauss family here too: neither is exact arithmetic)
    p = 0.1, gauss family       inside the bounds; the same seed once more: the same bits, dA / dB included; another seed: other bits
Shapes, the smallest that reach every path: Q|K|V entries at K = N = 64 (the least), 576 (the 512-element lane stride takes a partial
second trip) and 1024 (the limit); whole-projection entries at (K, N) = (64, 192), (1088, 64) (one 1024-column LDS chunk plus a 64 tail)
and, at M = 65 only, (3072, 768) and (768, 3072); M = 1, 63 (a partial wave group), 65 (one row past a 64-row workgroup), 257 (one row
past a VK_LORA_ROW_BLOCK record), one case with *dyn below M; r = 4, 8, 16, 32 at one shape, 8 elsewhere."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_restate as GR  # noqa: E402
import lora_drop_restate as D  # noqa: E402
import lora_restate as R  # noqa: E402
import test_lora_kernels_gpu as K0  # noqa: E402  (Grid, Flat and the bit-level transfers)

pytestmark = pytest.mark.gpu
Grid, Flat, dev16 = K0.Grid, K0.Flat, K0.dev16
SEED_A, SEED_B = 0x1234_5678_9ABC_DEF1, 0x0FED_CBA9_8765_4321
SITE0 = 1 << 20


def P(st=0, ad=0, col=0, act=0, frozen=False):
    return dict(st=st, ad=ad, col=col, act=act, frozen=frozen)


def qkv(M, KN, r=8, **kw):
    return dict(api="qkv", r=r, streams=[(M, KN, KN)], probs=[P(col=1)], dx=[True], rho=[False], **kw)


def proj(M, K, N, r=8, act=0, rho=False, **kw):
    return dict(api="proj", r=r, streams=[(M, K, N)], probs=[P(act=act)], dx=[True], rho=[rho], **kw)


# streams: [(M, K, N)], each with one X, one dX (dx) and, whole projections only, one R (rho); a problem names its stream, its adapter and
# (Q|K|V entries) its column block; dyn: {stream: rows}
CASES = {
    "qkv_m1_64": qkv(1, 64),
    "qkv_m63_576_r4": qkv(63, 576, 4),
    "qkv_m63_576_r8": qkv(63, 576, 8),
    "qkv_m63_576_r16": qkv(63, 576, 16),
    "qkv_m63_576_r32": qkv(63, 576, 32),
    "qkv_m65_1024": qkv(65, 1024),
    "qkv_m257_64": qkv(257, 64),
    "qkv_m257_576_dyn130": qkv(257, 576, dyn={0: 130}),
    # q and v of one stream: two problems with sites of their own add into one dX in one read-modify-write
    "qkv_two_into_one_dx": dict(api="qkv", r=8, streams=[(65, 576, 576)], probs=[P(0, 0, 0), P(0, 1, 2)], dx=[True], rho=[False]),
    # one adapter shared by two streams: the second problem accumulates; each stream has a site (and a mask) of its own
    "qkv_shared_two_sources": dict(api="qkv", r=8, streams=[(63, 64, 64), (257, 64, 64)], probs=[P(0, 0, 0), P(1, 0, 0)], dx=[True, True], rho=[False, False]),
    # a frozen adapter (dA = dB = NULL) beside a trainable one: its share of dX is masked all the same
    "qkv_frozen_live_dx": dict(api="qkv", r=8, streams=[(65, 64, 64)], probs=[P(0, 0, 0), P(0, 1, 1, frozen=True)], dx=[True], rho=[False]),
    "proj_m1_64_192": proj(1, 64, 192),
    "proj_m63_1088_64": proj(63, 1088, 64),
    "proj_m257_64_192": proj(257, 64, 192),
    "proj_m257_1088_64_r32": proj(257, 1088, 64, 32),
    "proj_m65_3072_768_rho": proj(65, 3072, 768, rho=True),              # the FFN-down adapter: R != NULL
    "proj_m65_768_3072_gelu": proj(65, 768, 3072, act=1),                # the FFN-up adapter: act = 1 with G
    "proj_shared_two_sources": dict(api="proj", r=8, streams=[(63, 1088, 64), (65, 1088, 64)], probs=[P(0, 0), P(1, 0)], dx=[True, False], rho=[False, False]),
    "proj_frozen_two_into_one_dx": dict(api="proj", r=8, streams=[(65, 64, 192)], probs=[P(0, 0), P(0, 1, frozen=True)], dx=[True], rho=[False]),
}


def inexact(case):
    return any(p["act"] for p in case["probs"]) or any(case["rho"])


def run_case(case, kind, p, seed, drop_entry=True, check=False):
    """One forward and one backward call on fresh buffers -> every output's bits.  drop_entry False: the unmasked entry points (p must be
    0).  check: compare with the restatement (bitwise for the integer family)."""
    from volta_amd import ops
    rng = np.random.default_rng(977)
    api, r, probs = case["api"], case["r"], case["probs"]
    rows = lambda st: case.get("dyn", {}).get(st, case["streams"][st][0])
    sites = [SITE0 + 11 * i + 5 for i in range(len(probs))]
    c = D.scale(p)
    fam, ad = {}, {}
    for i, pr in enumerate(probs):
        M, K, N = case["streams"][pr["st"]]
        fam[i] = R.family(kind, rng, M, K, N, r)
        if pr["ad"] in ad:                      # a shared adapter: the later problem takes the first one's A and B
            fam[i]["A"], fam[i]["B"] = ad[pr["ad"]]["A"], ad[pr["ad"]]["B"]
        else:
            ad[pr["ad"]] = dict(A=fam[i]["A"], B=fam[i]["B"], K=K, N=N, frozen=pr["frozen"])
    s = fam[0]["s"]
    q16 = lambda a: R.bf16_value(R.bf16_bits(a))
    # ---- buffers: per stream X, dX, R (and the 3N-wide qkv / dqkv of the Q|K|V entries); per problem T, dT (Y, dY, G of a whole projection)
    xg, dxg, rg, yq, dyq, dxprev, rho, dyn_t = {}, {}, {}, {}, {}, {}, {}, {}
    for st, (M, K, N) in enumerate(case["streams"]):
        first = next(i for i, pr in enumerate(probs) if pr["st"] == st)
        xg[st], dxg[st] = Grid(M, K + 8, 11 * st), Grid(M, K + 8, 5 + st)
        xg[st].put(0, fam[first]["X"])
        dxprev[st] = fam[first]["dXprev"]
        dxg[st].put(0, dxprev[st])
        if case["dx"][st]:
            dxg[st].body(dxg[st].written)[:rows(st), :K] = True
        for i, pr in enumerate(probs):
            if pr["st"] == st:
                fam[i]["X"] = fam[first]["X"]
        grids = [xg[st], dxg[st]]
        if case["rho"][st]:
            rho[st] = q16(GR.gelu64(rng.standard_normal((M, K)) * 1.5)[1])
            rg[st] = Grid(M, K + 16, 17 + st)
            rg[st].put(0, rho[st])
            grids.append(rg[st])
        if api == "qkv":
            yq[st], dyq[st] = Grid(M, 3 * N, 7 + st), Grid(M, 3 * N, 3 + st)
            for i, pr in enumerate(probs):
                if pr["st"] == st:
                    yq[st].put(pr["col"] * N, fam[i]["Yprev"])
                    yq[st].body(yq[st].written)[:rows(st), pr["col"] * N:(pr["col"] + 1) * N] = True
                    dyq[st].put(pr["col"] * N, fam[i]["dY"])
            grids += [yq[st], dyq[st]]
        for g in grids:
            g.upload()
        if st in case.get("dyn", {}):
            dyn_t[st] = torch.tensor([rows(st)], dtype=torch.int32, device="cuda")
    yg, dyg, gg = {}, {}, {}
    if api == "proj":
        for i, pr in enumerate(probs):
            M, K, N = case["streams"][pr["st"]]
            yg[i], dyg[i] = Grid(M, N + 8, 7 + i), Grid(M, N + 8, 3 + i)
            yg[i].put(0, fam[i]["Yprev"])
            yg[i].body(yg[i].written)[:rows(pr["st"]), :N] = True
            dyg[i].put(0, fam[i]["dY"])
            yg[i].upload(), dyg[i].upload()
            if pr["act"]:
                gg[i] = Grid(M, N + 16, 23 + i)
                gg[i].body(gg[i].written)[:rows(pr["st"]), :N] = True
                gg[i].upload()
    Tb = {i: Flat(case["streams"][pr["st"]][0] * r, 100 + i) for i, pr in enumerate(probs)}
    dTb = {i: Flat(case["streams"][pr["st"]][0] * r, 200 + i) for i, pr in enumerate(probs)}
    Ad = {a: dev16(R.bf16_bits(v["A"])) for a, v in ad.items()}
    Bd = {a: dev16(R.bf16_bits(v["B"])) for a, v in ad.items()}
    dAb = {a: Flat(r * v["K"], 300 + a, f32=True) for a, v in ad.items()}
    dBb = {a: Flat(v["N"] * r, 400 + a, f32=True) for a, v in ad.items()}
    seed_t = torch.tensor([seed], dtype=torch.int64, device="cuda")
    # ---- problems
    fwd, bwd, drops, seen = [], [], [], set()
    for i, pr in enumerate(probs):
        st, a = pr["st"], pr["ad"]
        M, K, N = case["streams"][st]
        T, dT, frozen = Tb[i].view((M, r)), dTb[i].view((M, r)), ad[a]["frozen"]
        dX = dxg[st].view(0, K) if case["dx"][st] else None
        acc = a in seen
        if api == "qkv":
            fwd.append(ops.lora_problem(xg[st].view(0, K), Ad[a], Bd[a], T, yq[st].view(pr["col"] * N, N), s, dyn=dyn_t.get(st)))
            b = ops.lora_bwd_problem(xg[st].view(0, K), Ad[a], Bd[a], T, dyq[st].view(pr["col"] * N, N), dT, dX, dAb[a].view((r, K)), dBb[a].view((N, r)), s,
                                     accumulate=acc, dyn=dyn_t.get(st))
            if frozen:
                b.dA = b.dB = None
            bwd.append(b)
        else:
            fwd.append(ops.lora_proj_problem(xg[st].view(0, K), Ad[a], Bd[a], T, yg[i].view(0, N), s, G=gg[i].view(0, N) if pr["act"] else None, dyn=dyn_t.get(st)))
            bwd.append(ops.lora_proj_bwd_problem(xg[st].view(0, K), Ad[a], Bd[a], T, dyg[i].view(0, N), dT, dX,
                                                 None if frozen else dAb[a].view((r, K)), None if frozen else dBb[a].view((N, r)), s,
                                                 R=rg[st].view(0, K) if case["rho"][st] else None, accumulate=acc, dyn=dyn_t.get(st)))
        drops.append(ops.lora_drop(seed_t, sites[i], p))
        if not frozen:
            seen.add(a)
    if drop_entry:
        (ops.lora_fwd_drop if api == "qkv" else ops.lora_proj_fwd_drop)(fwd, drops)
    else:
        assert p == 0.0
        (ops.lora_fwd if api == "qkv" else ops.lora_proj_fwd)(fwd)
    torch.cuda.synchronize()
    T = {i: Tb[i].after() for i in Tb}
    Y = {i: (yq[pr["st"]] if api == "qkv" else yg[i]).after() for i, pr in enumerate(probs)}
    G = {i: gg[i].after() for i in gg}
    for st in xg:
        xg[st].after()
    if drop_entry:
        (ops.lora_bwd_drop if api == "qkv" else ops.lora_proj_bwd_drop)(bwd, drops)
    else:
        (ops.lora_bwd if api == "qkv" else ops.lora_proj_bwd)(bwd)
    torch.cuda.synchronize()
    dT = {i: dTb[i].after() for i in dTb}
    dA = {a: dAb[a].after(written=not ad[a]["frozen"]) for a in dAb}
    dB = {a: dBb[a].after(written=not ad[a]["frozen"]) for a in dBb}
    dX = {st: dxg[st].after() for st in dxg}
    for st in xg:
        xg[st].after()
        if st in rg:
            rg[st].after()
    for i, pr in enumerate(probs):
        (dyq[pr["st"]] if api == "qkv" else dyg[i]).after()
        assert np.array_equal((yq[pr["st"]] if api == "qkv" else yg[i]).after(), Y[i]), "the backward changed Y"
        assert np.array_equal(Tb[i].after(), T[i]), "the backward changed T"
        if i in gg:
            assert np.array_equal(gg[i].after(), G[i]), "the backward changed G"
        Me, M = rows(pr["st"]), case["streams"][pr["st"]][0]               # rows past *dyn: T and dT keep their sentinels
        for flat, bits in ((Tb[i], T[i]), (dTb[i], dT[i])):
            assert np.array_equal(bits[Me * r:], flat.bits[R.GUARD + Me * r:R.GUARD + M * r]), "a row past *dyn was written"
    out = dict(T=T, Y=Y, G=G, dT=dT, dA=dA, dB=dB, dX=dX)
    if not check:
        return out
    # ---- the restatement, stage by stage
    exact = kind == "int"
    worst = {}

    def cmp16(name, bits, ref, e):
        if exact:
            assert R.exact_bf16(bits, ref), "%s: not bitwise the float64 result" % name
        else:
            worst[name] = max(worst.get(name, 0.0), R.worst_bf16(bits, ref, e))

    def cmp32(name, bits, ref, e):
        vals = bits.view(np.float32)
        if exact:
            assert R.exact_f32(vals, ref), "%s: not exactly the float64 result" % name
        else:
            worst[name] = max(worst.get(name, 0.0), R.worst_f32(vals, ref, e))

    keep, Tv, dTv, Xe = {}, {}, {}, {}
    for i, pr in enumerate(probs):
        M, K, N = case["streams"][pr["st"]]
        Me, f = rows(pr["st"]), fam[i]
        keep[i] = D.keep_mask(seed, sites[i], M, K, p)[:Me]                  # the mask of the rows of X as passed
        if p > 0:
            assert 0 < keep[i].sum() < keep[i].size or keep[i].size < 64
        Xe[i] = f["X"][:Me]
        cmp16("T", T[i][:Me * r].reshape(Me, r), *D.ref_T(Xe[i], f["A"], keep[i], c))
        Tv[i] = R.bf16_value(T[i][:Me * r]).reshape(Me, r)
        col = pr["col"] if api == "qkv" else 0
        v, e = R.ref_Y(f["Yprev"][:Me], Tv[i], f["B"], s)
        if pr["act"]:
            y, d = GR.gelu64(v)
            cmp16("Y_gelu", Y[i][:Me, :N], y, 1.13 * e + GR.e_formula_value(v))
            cmp16("G", G[i][:Me, :N], d, 0.80 * e + GR.e_formula_deriv(v))
        else:
            cmp16("Y", Y[i][:Me, col * N:(col + 1) * N], v, e)
        cmp16("dT", dT[i][:Me * r].reshape(Me, r), *R.ref_dT(f["dY"][:Me], f["B"], s))
        dTv[i] = R.bf16_value(dT[i][:Me * r]).reshape(Me, r)
    for a, v in ad.items():
        if v["frozen"]:
            continue
        src = [i for i, pr in enumerate(probs) if pr["ad"] == a]
        cmp32("dB", dB[a].reshape(v["N"], r), *R.ref_dB([(fam[i]["dY"][:Tv[i].shape[0]], Tv[i], s) for i in src]))
        cmp32("dA", dA[a].reshape(r, v["K"]), *D.ref_dA([(dTv[i], Xe[i], keep[i], c) for i in src]))
    for st, (M, K, N) in enumerate(case["streams"]):
        if not case["dx"][st]:
            continue
        Me = rows(st)
        mem = [(dTv[i], fam[i]["A"], keep[i], c) for i, pr in enumerate(probs) if pr["st"] == st]
        if case["rho"][st]:
            delta, e = D.ref_dX_term(mem)
            rh = rho[st][:Me]
            cmp16("dX_rho", dX[st][:Me, :K], dxprev[st][:Me] + rh * delta, np.abs(rh) * e + np.abs(rh * delta) * R.U24)
        else:
            cmp16("dX", dX[st][:Me, :K], *D.ref_dX(dxprev[st][:Me], mem))
    print(kind, p, {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst
    return out


def same(a, b):
    return all(np.array_equal(a[key][k], b[key][k]) for key in a for k in a[key])


@pytest.mark.parametrize("name", list(CASES))
def test_lora_drop_kernels(name):
    case = CASES[name]
    run_case(case, "gauss" if inexact(case) else "int", 0.5, SEED_A, check=True)
    first = run_case(case, "gauss", 0.1, SEED_A, check=True)
    again = run_case(case, "gauss", 0.1, SEED_A)
    for key in first:
        for k in first[key]:
            assert np.array_equal(first[key][k], again[key][k]), "%s[%s] differs between two launches with one seed" % (key, k)
    other = run_case(case, "gauss", 0.1, SEED_B)
    M, K, _ = case["streams"][0]
    if M * K >= 4096:                       # 64 elements at p = 0.1: two seeds may well keep the same ones
        for key in ("T", "dA", "dX"):
            assert any(not np.array_equal(first[key][k], other[key][k]) for k in first[key]), "%s does not depend on the seed" % key
    assert same({k: first[k] for k in ("dT",)}, {k: other[k] for k in ("dT",)})          # dT reads no mask


@pytest.mark.parametrize("name", ["qkv_m63_576_r4", "qkv_m257_576_dyn130", "qkv_shared_two_sources", "qkv_frozen_live_dx", "proj_m63_1088_64",
                                  "proj_m65_3072_768_rho", "proj_m65_768_3072_gelu", "proj_frozen_two_into_one_dx"])
def test_zero_thresholds_are_the_unmasked_entry_points(name):
    """Every _drop entry with all thresholds 0 (and no seed) gives the bits of the old entry point on the same inputs."""
    case = CASES[name]
    old = run_case(case, "gauss", 0.0, SEED_A, drop_entry=False)
    new = run_case(case, "gauss", 0.0, SEED_A, drop_entry=True, check=True)
    for key in old:
        for k in old[key]:
            assert np.array_equal(old[key][k], new[key][k]), "%s[%s]" % (key, k)


def test_one_zero_threshold_among_masked_problems():
    """A problem with threshold 0 beside a masked one: the masked kernels run, the unmasked problem keeps the old entry point's bits."""
    from volta_amd import ops
    case = CASES["qkv_two_into_one_dx"]
    orig = ops.lora_drop
    calls = []

    def mixed(seed_t, site, p):
        calls.append(site)
        return orig(seed_t, site, p if len(calls) % 2 else 0.0)       # problem 0 masked, problem 1 not

    old = run_case(case, "gauss", 0.0, SEED_A, drop_entry=False)
    ops.lora_drop = mixed
    try:
        new = run_case(case, "gauss", 0.1, SEED_A)
    finally:
        ops.lora_drop = orig
    assert np.array_equal(old["T"][1], new["T"][1]) and np.array_equal(old["dT"][1], new["dT"][1])
    assert np.array_equal(old["dA"][1], new["dA"][1]) and np.array_equal(old["dB"][1], new["dB"][1])
    assert not np.array_equal(old["T"][0], new["T"][0]) and not np.array_equal(old["dA"][0], new["dA"][0])


def test_refusals():
    """Bad arguments are refused on the host, before any launch: every buffer keeps its sentinels."""
    from volta_amd import _lib as L
    M, W = 4, 256
    names = ("X", "A", "B", "T", "Y", "dY", "dT", "dX")
    bits = {n: R.sentinels16(M * W, 31 * i) for i, n in enumerate(names)}
    t = {n: dev16(b) for n, b in bits.items()}
    g32 = {n: R.sentinels32(32 * W, 7 * i) for i, n in enumerate(("dA", "dB", "work"))}
    t32 = {n: K0.dev32(b) for n, b in g32.items()}
    seed_t = torch.tensor([5, 6], dtype=torch.int64, device="cuda")
    a = lambda n, off=0: t[n].data_ptr() + off
    err = lambda: L.lib.vk_last_error().decode()
    on = lambda seed=seed_t.data_ptr(), thr=1 << 31, scale=2.0: L.Dropout(seed, SITE0, thr, scale)
    two = lambda d: (L.Dropout * 2)(d, d)

    def fwd(kind, drop, n=1, **kw):
        d = dict(X=a("X"), A=a("A"), B=a("B"), T=a("T"), Y=a("Y"), dyn=None, M=M, K=64, N=64, r=4, ldx=64, ldy=64, scale=1.0)
        if kind == "proj":
            d.update(G=None, ldg=0, act=0)
            d.update(kw)
            return L.lib.vk_lora_proj_fwd_drop((L.LoraProjProblem * 2)(L.LoraProjProblem(**d), L.LoraProjProblem(**d)), drop, n, None)
        d.update(reserved_=0)
        d.update(kw)
        return L.lib.vk_lora_fwd_drop((L.LoraProblem * 2)(L.LoraProblem(**d), L.LoraProblem(**d)), drop, n, None)

    def bwd(kind, drop, n=1, work=True, **kw):
        d = dict(X=a("X"), A=a("A"), B=a("B"), T=a("T"), dY=a("dY"), dT=a("dT"), dX=a("dX"), dA=t32["dA"].data_ptr(), dB=t32["dB"].data_ptr(), dyn=None,
                 M=M, K=64, N=64, r=4, ldx=64, ldy=64, lddx=64, accumulate=0, scale=1.0)
        wk = t32["work"].data_ptr() if work else None
        if kind == "proj":
            d.update(R=None, ldr=0)
            d.update(kw)
            return L.lib.vk_lora_proj_bwd_drop((L.LoraProjBwdProblem * 2)(L.LoraProjBwdProblem(**d), L.LoraProjBwdProblem(**d)), drop, n, wk, None)
        d.update(reserved_=0)
        d.update(kw)
        return L.lib.vk_lora_bwd_drop((L.LoraBwdProblem * 2)(L.LoraBwdProblem(**d), L.LoraBwdProblem(**d)), drop, n, wk, None)

    for kind, stem in (("qkv", "vk_lora_"), ("proj", "vk_lora_proj_")):
        for call, nm in ((fwd, stem + "fwd_drop"), (bwd, stem + "bwd_drop")):
            assert call(kind, two(on(seed=None))) != 0 and nm in err() and "problem 0" in err() and "NULL seed" in err()          # a threshold without a seed
            assert call(kind, (L.Dropout * 2)(on(), on(seed=None)), n=2) != 0 and "problem 1" in err() and "NULL seed" in err()
            assert call(kind, two(on(seed=seed_t.data_ptr() + 4))) != 0 and "seed" in err()
            assert call(kind, None) != 0 and "NULL dropout" in err()
            assert call(kind, two(on()), n=0) != 0 and "0 problems" in err()                                                    # n out of range
            assert call(kind, two(on()), n=7) != 0 and "7 problems" in err()
            assert call(kind, two(on()), X=a("X", 2)) != 0 and "operand 0 is not 16-byte aligned" in err() and nm in err()        # a misaligned pointer
            assert call(kind, two(on()), r=12) != 0 and "r = 12" in err()
            assert call(kind, two(on()), K=96, ldx=96) != 0 and "K = 96" in err()
        assert bwd(kind, two(on()), work=False) != 0 and "workspace" in err()
        assert bwd(kind, two(on()), dX=a("dX", 4)) != 0 and "dX" in err()
        assert fwd(kind, two(on()), n=2) != 0 and "problems 0 and 1" in err()                                                    # both write the same T and Y
    torch.cuda.synchronize()
    for n in t:
        assert np.array_equal(K0.host16(t[n]), bits[n]), "%s changed" % n
    for n in t32:
        assert np.array_equal(K0.host32(t32[n]), g32[n]), "%s changed" % n
