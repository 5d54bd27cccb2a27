"""The gated attention kernels (csrc/attention.hip, csrc/attention_generic.hip) through the C ABI against the float64 restatement of
tests/attn_restate.py, elementwise, under the gates derived there: ctx, the saved log-sum-exp (lse), dQ, dK, dV and, where requested, the
attention maps (probs).  Every case runs on a layout the engine's defaults never produce:
  * Q, K, V are column views into one wider buffer per modality (ld > 3H, different per modality); its pad columns and the rows past
    B*L hold NaN, and so does the mask buffer past its B*L values.  Every output then matching its gate shows that nothing outside
    the contract's inputs was read (the NaN read check);
  * ctx (ldo > H), lse, dQ / dK / dV (ldg > 3H) and probs are prefilled with a NaN canary.  Every element the contract assigns must
    be written, every other element must keep its canary bits: pad columns and rows, ctx / lse / dQ of a modality that is not a query,
    dK / dV of a modality that is not a key, the maps of blocks that are gated off (the canary write-set check).
The case table (shapes, paths, gate patterns, dropout) is tests/attn_restate.py's; tests/test_attention_cpu.py checks its dispatch and
the gates.  GPU only."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_restate as A  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
CAN16 = -91                         # bf16 canary bits 0xFFA5: a negative NaN no bf16 conversion produces
CAN32 = 0xFFA5A5A5 - (1 << 32)      # fp32 canary bits
XR = 3                              # rows past B*L in every buffer


def _lib():
    from volta_amd import _lib as L
    return L


def _canary16(shape):
    return torch.full(shape, CAN16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def _canary32(n):
    return torch.full((n,), CAN32, dtype=torch.int32, device=DEV).view(torch.float32)


def _layout(H):
    """Per modality: (ld, column offsets of Q, K, V), (ldo, column of ctx / dO), (ldg, columns of dQ, dK, dV); all multiples of 8."""
    return ([(3 * H + 24, (0, H + 8, 2 * H + 16)), (3 * H + 56, (8, H + 24, 2 * H + 48))],
            [(H + 16, 8), (H + 24, 16)],
            [(3 * H + 32, (0, H + 8, 2 * H + 24)), (3 * H + 48, (16, H + 24, 2 * H + 40))])


class Launch:
    """Device buffers of one case, the launches, and the host copies of every output buffer."""

    def __init__(self, inp, gate, p, probs=False):
        L = _lib()
        B, nh, dh, Ls = inp["B"], inp["nh"], inp["dh"], inp["L"]
        H = nh * dh
        self.B, self.nh, self.H, self.Ls, self.gate, self.probs_on = B, nh, H, Ls, gate, probs
        self.lay = _layout(H)
        nan = float("nan")
        self.seed_t = torch.zeros(1, dtype=torch.int64, device=DEV)
        from volta_amd import ops
        ops.set_seed(self.seed_t, A.SEED)
        self.src, self.maskb, self.dob, self.ctxb, self.lseb, self.dqkvb = [], [], [], [], [], []
        for m in range(2):
            n = B * Ls[m]
            (ld, offs), (ldo, co), (ldg, _) = self.lay[0][m], self.lay[1][m], self.lay[2][m]
            s = torch.full((n + XR, ld), nan, dtype=torch.bfloat16)
            for t, c in zip((inp["q"][m], inp["k"][m], inp["v"][m]), offs):
                s[:n, c:c + H] = t
            self.src.append(s.to(DEV))
            mb = torch.full((n + 40,), nan)
            mb[:n] = inp["mask"][m].reshape(-1)
            self.maskb.append(mb.to(DEV))
            d = torch.full((n + XR, ldo), nan, dtype=torch.bfloat16)
            d[:n, co:co + H] = inp["do"][m]
            self.dob.append(d.to(DEV))
            self.ctxb.append(_canary16((n + XR, ldo)))
            self.lseb.append(_canary32(B * nh * Ls[m] + 8))
            self.dqkvb.append(_canary16((n + XR, ldg)))
        self.probsb = [[_canary32(B * nh * Ls[i] * Ls[j] + 8) if probs else None for j in range(2)] for i in range(2)]
        aa = L.AttnArgs()
        for m in range(2):
            (ld, offs), (ldo, co) = self.lay[0][m], self.lay[1][m]
            base = self.src[m].data_ptr()
            aa.q[m], aa.k[m], aa.v[m] = base + 2 * offs[0], base + 2 * offs[1], base + 2 * offs[2]
            aa.ld[m], aa.L[m] = ld, Ls[m]
            aa.mask[m] = self.maskb[m].data_ptr()
            aa.ctx[m], aa.ldo[m], aa.lse[m] = self.ctxb[m].data_ptr() + 2 * co, ldo, self.lseb[m].data_ptr()
        aa.B, aa.nh, aa.scale, aa.dh = B, nh, 1.0 / math.sqrt(dh), dh
        for i in range(2):
            for j in range(2):
                aa.gate[i][j] = gate[i][j]
                aa.drop[i][j] = L.dropout_cfg(self.seed_t.data_ptr(), A.SITES[i][j], p) if (gate[i][j] and p > 0) else L.dropout_cfg(None, 0, 0.0)
                aa.probs[i][j] = self.probsb[i][j].data_ptr() if probs else None
        bw = L.AttnBwdArgs()
        for m in range(2):
            (ldo, co), (ldg, goffs) = self.lay[1][m], self.lay[2][m]
            bw.dctx[m] = self.dob[m].data_ptr() + 2 * co
            base = self.dqkvb[m].data_ptr()
            bw.dq[m], bw.dk[m], bw.dv[m] = base + 2 * goffs[0], base + 2 * goffs[1], base + 2 * goffs[2]
            bw.ldg[m] = ldg
        self.aa, self.bw = aa, bw

    def run(self, backward=True):
        L = _lib()
        L.check(L.lib.vk_gated_attn_fwd(C.byref(self.aa), L.stream_ptr()))
        if backward:
            L.check(L.lib.vk_gated_attn_bwd(C.byref(self.aa), C.byref(self.bw), L.stream_ptr()))
        torch.cuda.synchronize()
        return self

    def host(self):
        """Every output buffer, as a host tensor (bf16 / fp32 values)."""
        out = dict(ctx=[t.cpu() for t in self.ctxb], lse=[t.cpu() for t in self.lseb], dqkv=[t.cpu() for t in self.dqkvb])
        if self.probs_on:
            out["probs"] = [[self.probsb[i][j].cpu() for j in range(2)] for i in range(2)]
        return out


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _check_gate(name, got, ref, gate):
    r, i, g, w, e = A.worst(got, ref, gate)
    assert r <= 1.0, "%s: |got - ref| / gate = %.3g at flat %d: got %r ref %r gate %.3g" % (name, r, i, g, w, e)


def _check_canary(name, buf, assigned):
    """Elements outside `assigned` (a bool tensor of buf's shape) keep the canary bits; inside, none does."""
    can = CAN16 if buf.dtype == torch.bfloat16 else CAN32
    b = _bits(buf)
    kept = b == can
    assert bool(kept[~assigned].all()), "%s: %d element(s) outside the write set were written" % (name, int((~kept[~assigned]).sum()))
    assert not bool(kept[assigned].any()), "%s: %d element(s) of the write set were not written" % (name, int(kept[assigned].sum()))


def _compare(lc, out, ref, backward=True):
    B, nh, H, Ls, gate = lc.B, lc.nh, lc.H, lc.Ls, lc.gate
    for m in range(2):
        n = B * Ls[m]
        qa, ka = bool(gate[m][0] or gate[m][1]), bool(gate[0][m] or gate[1][m])
        ldo, co = lc.lay[1][m]
        ldg, goffs = lc.lay[2][m]
        ctx, lse = out["ctx"][m], out["lse"][m]
        asg = torch.zeros(ctx.shape, dtype=torch.bool)
        if qa:
            asg[:n, co:co + H] = True
            _check_gate("ctx[%d]" % m, ctx[:n, co:co + H].float(), ref["ctx"][m], ref["g_ctx"][m])
            _check_gate("lse[%d]" % m, lse[:B * nh * Ls[m]], ref["lse"][m], ref["g_lse"][m])
        _check_canary("ctx[%d]" % m, ctx, asg)
        asg = torch.zeros(lse.shape, dtype=torch.bool)
        asg[:B * nh * Ls[m]] = qa
        _check_canary("lse[%d]" % m, lse, asg)
        if not backward:
            continue
        g = out["dqkv"][m]
        asg = torch.zeros(g.shape, dtype=torch.bool)
        for key, c, on in (("dq", goffs[0], qa), ("dk", goffs[1], ka), ("dv", goffs[2], ka)):
            if on:
                asg[:n, c:c + H] = True
                _check_gate("%s[%d]" % (key, m), g[:n, c:c + H].float(), ref[key][m], ref["g_" + key][m])
        _check_canary("dqkv[%d]" % m, g, asg)
    if lc.probs_on:
        for i in range(2):
            for j in range(2):
                pb = out["probs"][i][j]
                nel = B * nh * Ls[i] * Ls[j]
                asg = torch.zeros(pb.shape, dtype=torch.bool)
                if gate[i][j]:
                    asg[:nel] = True
                    _check_gate("probs[%d][%d]" % (i, j), pb[:nel], ref["probs"][i][j].reshape(-1), ref["g_probs"][i][j].reshape(-1))
                _check_canary("probs[%d][%d]" % (i, j), pb, asg)


def _case(case):
    sh = case.shape
    inp = A.make_inputs(sh.B, sh.nh, sh.dh, sh.T, sh.R, case.dist, seed=A.case_seed(case))
    gate = A.GATES[case.gname]
    lc = Launch(inp, gate, case.p, case.probs).run(backward=not case.fwd_only)
    ref = A.restate(inp, gate, case.p)
    _compare(lc, lc.host(), ref, backward=not case.fwd_only)


_TABLE = A.table_cases()


@pytest.mark.parametrize("case", _TABLE, ids=[c.id for c in _TABLE])
def test_kernels_match_restatement(case):
    _case(case)


def test_largest_backward_shapes():
    """At head size 64 and 128: the largest vision length the generic backward's LDS admits (vk_gated_attn_lds_bytes, searched here)."""
    for case in A.largest_cases(_lib().lib):
        _case(case)


def test_more_than_512_keys_is_refused():
    """513 keys per query row: the generic forward returns an error instead of launching (512 run in the table)."""
    L = _lib()
    inp = A.make_inputs(1, 1, 64, 80, 433, "mid")
    lc = Launch(inp, A.GATES["all"], 0.0)
    assert L.lib.vk_gated_attn_fwd(C.byref(lc.aa), L.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert bool((_bits(lc.ctxb[0]) == CAN16).all()) and bool((_bits(lc.lseb[1]) == CAN32).all())


@pytest.mark.parametrize("shape,gname,probs", [(A.Shape("bench", 256, 12, 64, 20, 37, ""), "all", False),
                                               (A.Shape("mfma64", 3, 8, 128, 38, 64, ""), "tt+tv", False),
                                               (A.Shape("gen", 3, 12, 64, 65, 129, ""), "all", True)], ids=["bench", "mfma128", "generic"])
def test_deterministic(shape, gname, probs):
    """Two identical forward + backward launches write the same bits into every output buffer."""
    inp = A.make_inputs(shape.B, shape.nh, shape.dh, shape.T, shape.R, "mid", seed=9)
    a = Launch(inp, A.GATES[gname], 0.1, probs).run().host()
    b = Launch(inp, A.GATES[gname], 0.1, probs).run().host()
    for key in ("ctx", "lse", "dqkv"):
        for m in range(2):
            assert torch.equal(_bits(a[key][m]), _bits(b[key][m])), (key, m)
    if probs:
        for i in range(2):
            for j in range(2):
                assert torch.equal(_bits(a["probs"][i][j]), _bits(b["probs"][i][j])), (i, j)
