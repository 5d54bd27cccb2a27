"""vk_lora_fwd / vk_lora_bwd on their own (csrc/lora.hip), against the float64 restatement and bounds of tests/lora_restate.py.

Every output lies inside a wider buffer of position-dependent NaN sentinels compared as raw bits: the columns of the other projections in
the 3N-wide qkv / dqkv buffers, the rows below M, the elements in front and behind, the pad columns of X and dX (ld = K + 8).  Every case
runs twice into fresh buffers and must give the same bits.  Shapes: the smallest at which the mechanisms can go wrong -- M around the
4-row lanes of the expand kernel (1, 15, 16, 17), around the 64-row workgroups of the row products (64, 65) and past one 256-row block of
the partial sums (300); K and N at one 64-column tile, a ragged count of 512-element wave passes (192, 768) and the LDS limit (1024)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lora_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

# name -> r, streams [(M, K, N)], problems [(stream, column block, adapter)], dx: per stream, acc_first: the first problem accumulates
single = lambda M, K, N, r, dx=True: dict(r=r, streams=[(M, K, N)], probs=[(0, 1, 0)], dx=[dx])
CASES = {
    "m1_k64_n64_r4": single(1, 64, 64, 4),
    "m15_k192_n64_r8": single(15, 192, 64, 8),
    "m16_k64_n192_r16": single(16, 64, 192, 16, dx=False),
    "m17_k768_n768_r32": single(17, 768, 768, 32),
    "m64_k1024_n1024_r32": single(64, 1024, 1024, 32),
    "m65_k1024_n64_r4": single(65, 1024, 64, 4, dx=False),
    "m300_k768_n768_r8": single(300, 768, 768, 8),
    "m300_k192_n1024_r16": single(300, 192, 1024, 16),
    "m64_k64_n1024_r8": single(64, 64, 1024, 8, dx=False),
    "m17_k1024_n192_r4": single(17, 1024, 192, 4),
    "m65_k768_n1024_r16": single(65, 768, 1024, 16),
    "m300_k1024_n1024_r32": single(300, 1024, 1024, 32, dx=False),
    # q, k and v of one stream: three adapters, one read-modify-write of dX
    "list3_one_stream": dict(r=8, streams=[(65, 768, 768)], probs=[(0, 0, 0), (0, 1, 1), (0, 2, 2)], dx=[True]),
    # two streams of different M x three projections; the second stream's input gradient is not live
    "list6_two_streams": dict(r=16, streams=[(17, 192, 192), (300, 192, 192)],
                              probs=[(0, 0, 0), (0, 1, 1), (0, 2, 2), (1, 0, 3), (1, 1, 4), (1, 2, 5)], dx=[True, False]),
    # one adapter shared by two streams: the second source accumulates; gradients summed in list order
    "shared_two_sources": dict(r=8, streams=[(64, 192, 192), (300, 192, 192)], probs=[(0, 0, 0), (1, 0, 0)], dx=[True, True]),
    # `accumulate` on the first problem adds to what dA / dB hold
    "accumulate_first": dict(r=4, streams=[(65, 64, 192)], probs=[(0, 2, 0)], dx=[True], acc_first=True),
}


def dev16(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda().view(torch.bfloat16)


def dev32(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int32)).cuda().view(torch.float32)


def host16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16).copy()


def host32(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32).copy()


class Grid:
    """A [rows + EXTRA_ROWS, ld] bf16 buffer between two guards, all sentinels until `put` writes a block."""

    def __init__(self, rows, ld, start):
        self.rows, self.ld = rows, ld
        self.bits = R.sentinels16(2 * R.GUARD + (rows + R.EXTRA_ROWS) * ld, start)
        self.written = np.zeros(self.bits.shape, dtype=bool)

    def body(self, a):
        return a[R.GUARD:R.GUARD + (self.rows + R.EXTRA_ROWS) * self.ld].reshape(self.rows + R.EXTRA_ROWS, self.ld)

    def put(self, c0, values):
        self.body(self.bits)[:values.shape[0], c0:c0 + values.shape[1]] = R.bf16_bits(values)

    def upload(self):
        self.dev = dev16(self.bits)
        return self

    def view(self, c0, ncols):
        return self.body(self.dev)[:self.rows, c0:c0 + ncols]

    def mark(self, c0, ncols):
        """these columns of rows < M are outputs"""
        self.body(self.written)[:self.rows, c0:c0 + ncols] = True

    def after(self):
        out = host16(self.dev)
        assert np.array_equal(out[~self.written], self.bits[~self.written]), "a sentinel or an input changed"
        return self.body(out)


class Flat:
    """n elements between two guards (bf16: T, dT; fp32: dA, dB)"""

    def __init__(self, n, start, f32=False, prev=None):
        self.n, self.f32 = n, f32
        self.bits = (R.sentinels32 if f32 else R.sentinels16)(2 * R.GUARD + n, start)
        if prev is not None:
            self.bits[R.GUARD:R.GUARD + n] = np.ascontiguousarray(prev, dtype=np.float32).reshape(-1).view(np.uint32)
        self.dev = (dev32 if f32 else dev16)(self.bits)

    def view(self, shape):
        return self.dev[R.GUARD:R.GUARD + self.n].view(shape)

    def after(self, written=True):
        out = (host32 if self.f32 else host16)(self.dev)
        keep = np.ones(out.shape, dtype=bool)
        if written:
            keep[R.GUARD:R.GUARD + self.n] = False
        assert np.array_equal(out[keep], self.bits[keep]), "a sentinel changed"
        return out[R.GUARD:R.GUARD + self.n]


def run_case(case, kind, check):
    """One forward and one backward call on fresh buffers.  -> every output's bits.  check: compare with the restatement."""
    from volta_amd import ops
    rng = np.random.default_rng(1234)
    r = case["r"]
    nad = 1 + max(a for _, _, a in case["probs"])
    fam, ad = {}, {}
    for i, (st, col, a) in enumerate(case["probs"]):
        M, K, N = case["streams"][st]
        fam[i] = R.family(kind, rng, M, K, N, r)
        if a in ad:                      # a shared adapter: the later problem takes the first one's A and B
            fam[i]["A"], fam[i]["B"] = ad[a]["A"], ad[a]["B"]
        else:
            ad[a] = dict(A=fam[i]["A"], B=fam[i]["B"], K=K, N=N)
    s = fam[0]["s"]
    # ---- buffers
    xg, qg, dqg, dxg, dxprev = {}, {}, {}, {}, {}
    for st, (M, K, N) in enumerate(case["streams"]):
        first = next(i for i, p in enumerate(case["probs"]) if p[0] == st)
        xg[st], qg[st], dqg[st], dxg[st] = Grid(M, K + 8, 11 * st), Grid(M, 3 * N, 7 + st), Grid(M, 3 * N, 3 + st), Grid(M, K + 8, 5 + st)
        xg[st].put(0, fam[first]["X"])
        dxprev[st] = fam[first]["dXprev"]
        dxg[st].put(0, dxprev[st])
        for i, (st2, col, a) in enumerate(case["probs"]):
            if st2 == st:
                fam[i]["X"] = fam[first]["X"]
                qg[st].put(col * N, fam[i]["Yprev"])
                qg[st].mark(col * N, N)
                dqg[st].put(col * N, fam[i]["dY"])
        if case["dx"][st]:
            dxg[st].mark(0, K)
        for g in (xg[st], qg[st], dqg[st], dxg[st]):
            g.upload()
    Tb = {i: Flat(case["streams"][st][0] * r, 100 + i) for i, (st, _, _) in enumerate(case["probs"])}
    dTb = {i: Flat(case["streams"][st][0] * r, 200 + i) for i, (st, _, _) in enumerate(case["probs"])}
    Ad = {a: dev16(R.bf16_bits(v["A"])) for a, v in ad.items()}
    Bd = {a: dev16(R.bf16_bits(v["B"])) for a, v in ad.items()}
    acc_first = case.get("acc_first", False)
    prevA = {a: (rng.integers(-8, 9, (r, v["K"])).astype(np.float64) if acc_first else None) for a, v in ad.items()}
    prevB = {a: (rng.integers(-8, 9, (v["N"], r)).astype(np.float64) if acc_first else None) for a, v in ad.items()}
    dAb = {a: Flat(r * v["K"], 300 + a, f32=True, prev=prevA[a]) for a, v in ad.items()}
    dBb = {a: Flat(v["N"] * r, 400 + a, f32=True, prev=prevB[a]) for a, v in ad.items()}
    assert len(ad) == nad
    # ---- forward
    fwd, bwd, seen = [], [], set()
    for i, (st, col, a) in enumerate(case["probs"]):
        M, K, N = case["streams"][st]
        fwd.append(ops.lora_problem(xg[st].view(0, K), Ad[a], Bd[a], Tb[i].view((M, r)), qg[st].view(col * N, N), s))
        bwd.append(ops.lora_bwd_problem(xg[st].view(0, K), Ad[a], Bd[a], Tb[i].view((M, r)), dqg[st].view(col * N, N), dTb[i].view((M, r)),
                                        dxg[st].view(0, K) if case["dx"][st] else None, dAb[a].view((r, K)), dBb[a].view((N, r)), s,
                                        accumulate=(a in seen) or (acc_first and i == 0)))
        seen.add(a)
    ops.lora_fwd(fwd)
    torch.cuda.synchronize()
    T = {i: Tb[i].after() for i in Tb}
    Y = {st: qg[st].after() for st in qg}
    for st in xg:
        xg[st].after()
    # ---- backward
    ops.lora_bwd(bwd)
    torch.cuda.synchronize()
    dT = {i: dTb[i].after() for i in dTb}
    dA = {a: dAb[a].after() for a in dAb}
    dB = {a: dBb[a].after() for a in dBb}
    dX = {st: dxg[st].after() for st in dxg}
    for st in xg:
        xg[st].after()
        dqg[st].after()
        assert np.array_equal(qg[st].after(), Y[st]), "the backward changed qkv"
    for i in Tb:
        assert np.array_equal(Tb[i].after(), T[i]), "the backward changed T"
    out = dict(T=T, Y=Y, dT=dT, dA=dA, dB=dB, dX=dX)
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

    Tv, dTv = {}, {}
    for i, (st, col, a) in enumerate(case["probs"]):
        M, K, N = case["streams"][st]
        f = fam[i]
        cmp16("T", T[i].reshape(M, r), *R.ref_T(f["X"], f["A"]))
        Tv[i] = R.bf16_value(T[i]).reshape(M, r)
        cmp16("Y", Y[st][:M, col * N:(col + 1) * N], *R.ref_Y(f["Yprev"], Tv[i], f["B"], s))
        cmp16("dT", dT[i].reshape(M, r), *R.ref_dT(f["dY"], f["B"], s))
        dTv[i] = R.bf16_value(dT[i]).reshape(M, r)
    for a, v in ad.items():
        src = [i for i, p in enumerate(case["probs"]) if p[2] == a]
        cmp32("dB", dB[a].reshape(v["N"], r), *R.ref_dB([(fam[i]["dY"], Tv[i], s) for i in src], prevB[a]))
        cmp32("dA", dA[a].reshape(r, v["K"]), *R.ref_dA([(dTv[i], fam[i]["X"]) for i in src], prevA[a]))
    for st, (M, K, N) in enumerate(case["streams"]):
        if case["dx"][st]:
            mem = [(dTv[i], fam[i]["A"]) for i, p in enumerate(case["probs"]) if p[0] == st]
            cmp16("dX", dX[st][:M, :K], *R.ref_dX(dxprev[st], mem))
    print(kind, {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst
    return out


@pytest.mark.parametrize("kind", ["gauss", "int"])
@pytest.mark.parametrize("name", list(CASES))
def test_lora_kernels(name, kind):
    case = CASES[name]
    first = run_case(case, kind, check=True)
    again = run_case(case, kind, check=False)
    for key in first:
        for k in first[key]:
            assert np.array_equal(first[key][k], again[key][k]), "%s[%s] differs between two launches" % (key, k)


def test_refusals():
    """Bad arguments are refused on the host, before any launch."""
    from volta_amd import _lib as L
    bad = (L.LoraProblem * 1)(L.LoraProblem(None, None, None, None, None, None, 16, 64, 64, 12, 64, 192, 1.0, 0))
    assert L.lib.vk_lora_fwd(bad, 1, None) != 0 and b"r = 12" in L.lib.vk_last_error()
    assert L.lib.vk_lora_fwd(bad, 7, None) != 0
    badb = (L.LoraBwdProblem * 1)(L.LoraBwdProblem())
    assert L.lib.vk_lora_bwd(badb, 1, None, None) != 0
