"""The fused dropout + residual + LayerNorm kernels (csrc/layernorm.hip) through the C ABI against the float64 restatement of
tests/ln_restate.py, elementwise, under the gates derived there: y, the saved z, mean, rstd, the row-quantised y8 / y8_scale, dz, dd,
dgamma and dbeta.  Every case runs on buffers the engine never produces:
  * every input has XR rows of NaN past M, gamma / beta / addvec a NaN tail past H: every output matching its gate, with no NaN in it,
    shows that nothing outside the contract's inputs was read (the NaN read check);
  * every output (and the tail of `partial`) is prefilled with a NaN canary: every element the contract assigns must be written, every
    other element -- rows at or past min(*dyn, M), tails past H or M -- must keep its canary bits (the canary write-set check);
  * every launch runs a second time on fresh buffers and must write the same bits (LayerNorm uses no atomics).
The backward is fed the restatement's own z / mean / rstd, so it does not depend on the forward kernel; one chained case feeds it the
forward kernel's outputs.  The case table is tests/ln_restate.py's; tests/test_ln_cpu.py checks its dispatch and the gates.  No buffer is
smaller than its contract and no launch is refused on purpose except the ln_check rejections, which return before launching.  GPU only."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ln_restate as A  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
CAN16 = -91                         # bf16 canary bits 0xFFA5: a negative NaN no bf16 conversion produces
CAN32 = 0xFFA5A5A5 - (1 << 32)      # fp32 canary bits
CAN8 = 0xFF                         # e4m3 NaN: the saturating conversion never produces it
XR = 3                              # rows past M in every buffer
XC = 8                              # elements past H in every vector
NAN = float("nan")


def _lib():
    from volta_amd import _lib as L
    return L


def _canary16(shape):
    return torch.full(shape, CAN16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def _canary32(n):
    return torch.full((n,), CAN32, dtype=torch.int32, device=DEV).view(torch.float32)


def _rows16(t, M, H):
    """bf16 [M + XR, H] on the device: t in rows [0, M), NaN below."""
    out = torch.full((M + XR, H), NAN, dtype=torch.bfloat16)
    out[:M] = t
    return out.to(DEV)


def _vec32(t, n, extra):
    """fp32 [n + extra] on the device: t, then a NaN tail."""
    out = torch.full((n + extra,), NAN, dtype=torch.float32)
    out[:n] = t
    return out.to(DEV)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def _seed_tensor():
    from volta_amd import ops
    t = torch.zeros(1, dtype=torch.int64, device=DEV)
    ops.set_seed(t, A.SEED)
    return t


def _segs(inp):
    L = _lib()
    arr = (L.DropRows * 2)()
    for i, sg in enumerate(inp["segs"]):
        arr[i] = L.DropRows(*sg)
    return arr


def _drop(inp, seed_t):
    L = _lib()
    return L.dropout_cfg(seed_t.data_ptr(), 999, inp["p"]) if inp["p"] > 0 else L.dropout_cfg(None, 0, 0.0)     # drop.site is ignored: seg[].site


def _ptr(t):
    return t.data_ptr() if t is not None else None


class Fwd:
    """Device buffers and vk_ln_args of one forward job; host() returns every output buffer."""

    def __init__(self, inp, z="own", dyn=None, y8=False, H=None):
        L = _lib()
        M, Hd = inp["M"], inp["H"]
        self.inp, self.M, self.H, self.zmode, self.y8_on = inp, M, Hd, z, y8
        self.seed_t = _seed_tensor()
        self.d = _rows16(inp["d"], M, Hd)
        self.d0 = self.d.clone()
        self.x = _rows16(inp["x"], M, Hd) if inp["x"] is not None else None
        self.addvec = _vec32(inp["addvec"], Hd, XC) if inp["addvec"] is not None else None
        self.gamma, self.beta = _vec32(inp["gamma"], Hd, XC), _vec32(inp["beta"], Hd, XC)
        self.y = _canary16((M + XR, Hd))
        self.z = _canary16((M + XR, Hd)) if z == "own" else self.d if z == "alias" else None
        self.mean, self.rstd = _canary32(M + XR), _canary32(M + XR)
        self.dyn = torch.tensor([dyn], dtype=torch.int32, device=DEV) if dyn is not None else None
        a = L.LnArgs(_ptr(self.d), _ptr(self.x), _ptr(self.addvec), _ptr(self.gamma), _ptr(self.beta), _ptr(self.y), _ptr(self.z),
                     _ptr(self.mean), _ptr(self.rstd), _ptr(self.dyn), M, Hd if H is None else H, inp["split"], inp["post"], inp["out_scale"],
                     _drop(inp, self.seed_t), _segs(inp))
        if y8:
            self.ld8 = (Hd + 7) // 8 * 8 + 8
            self.y8 = torch.full((M + XR, self.ld8), CAN8, dtype=torch.uint8, device=DEV)
            self.sc = _canary32(M + XR)
            a.y8, a.y8_scale, a.ld8 = self.y8.data_ptr(), self.sc.data_ptr(), self.ld8
        self.args = a

    def run(self):
        L = _lib()
        L.check(L.lib.vk_ln_fwd(C.byref(self.args), L.stream_ptr()))
        torch.cuda.synchronize()
        return self

    def host(self):
        out = dict(y=self.y.cpu(), mean=self.mean.cpu(), rstd=self.rstd.cpu(), z=self.z.cpu() if self.z is not None else None)
        if self.y8_on:
            out.update(y8=self.y8.cpu(), sc=self.sc.cpu())
        return out


class Bwd:
    """Device buffers and vk_ln_bwd_args of one backward job fed (zb, mean, rstd)."""

    def __init__(self, inp, zb, mean, rstd, dd=True, dyn=None, acc=0, shared=None, H=None):
        L = _lib()
        M, Hd = inp["M"], inp["H"]
        self.inp, self.M, self.H, self.dd_on = inp, M, Hd, dd
        self.seed_t = _seed_tensor()
        self.dy, self.zb = _rows16(inp["dy"], M, Hd), _rows16(zb, M, Hd)
        self.mean_in, self.rstd_in = _vec32(mean, M, XR), _vec32(rstd, M, XR)
        self.gamma = _vec32(inp["gamma"], Hd, XC)
        self.dz = _canary16((M + XR, Hd))
        self.dd = _canary16((M + XR, Hd)) if dd else None
        self.nrec = A.partial_rows(M)
        self.partial = _canary32(self.nrec * 2 * Hd + 64)
        if shared is not None:
            self.dgamma, self.dbeta = shared
        else:
            self.dgamma, self.dbeta = _canary32(Hd + XC), _canary32(Hd + XC)
            if acc & 1:
                self.dgamma[:Hd], self.dbeta[:Hd] = inp["dgamma0"].to(DEV), inp["dbeta0"].to(DEV)
        self.dyn = torch.tensor([dyn], dtype=torch.int32, device=DEV) if dyn is not None else None
        self.args = L.LnBwdArgs(_ptr(self.dy), _ptr(self.zb), _ptr(self.mean_in), _ptr(self.rstd_in), _ptr(self.gamma), _ptr(self.dz),
                                _ptr(self.dd), _ptr(self.partial), _ptr(self.dgamma), _ptr(self.dbeta), _ptr(self.dyn), M,
                                Hd if H is None else H, inp["split"], inp["post"], inp["out_scale"], acc, _drop(inp, self.seed_t), _segs(inp))

    def run(self):
        L = _lib()
        L.check(L.lib.vk_ln_bwd(C.byref(self.args), L.stream_ptr()))
        torch.cuda.synchronize()
        return self

    def host(self):
        return dict(dz=self.dz.cpu(), dd=self.dd.cpu() if self.dd is not None else None, dgamma=self.dgamma.cpu(), dbeta=self.dbeta.cpu(),
                    partial=self.partial.cpu())


RATIOS = {}


def _check_gate(cid, name, got, ref, gate):
    r, i, g, w, e = A.worst(got, ref, gate)
    if r > RATIOS.get(name, (-1.0, ""))[0]:
        RATIOS[name] = (r, cid)
    print("LNRATIO %s %s %.4g" % (cid, name, r))
    assert r <= 1.0, "%s %s: |got - ref| / gate = %.3g at flat %d: got %r ref %r gate %.3g" % (cid, name, r, i, g, w, e)


def _check_canary(name, buf, assigned, can=None):
    """Elements outside `assigned` (a bool tensor of buf's shape) keep the canary bits; inside, none does."""
    can = can if can is not None else (CAN16 if buf.dtype == torch.bfloat16 else CAN32)
    kept = _bits(buf) == can
    assert bool(kept[~assigned].all()), "%s: %d element(s) outside the write set were written" % (name, int((~kept[~assigned]).sum()))
    assert not bool(kept[assigned].any()), "%s: %d element(s) of the write set were not written" % (name, int(kept[assigned].sum()))


def _rows_mask(shape, n):
    m = torch.zeros(shape, dtype=torch.bool)
    m[:n] = True
    return m


def _compare_fwd(cid, job, out, ref, only=None):
    """Gates, write sets and NaN-freedom of one forward job's host buffers; only = the outputs whose gates are asserted (None: all)."""
    n, M, H = ref["rows"], job.M, job.H
    on = (lambda k: only is None or k in only)
    for key in ("y", "z"):
        buf = out[key]
        if buf is None:
            continue
        if key == "z" and job.zmode == "alias":          # z is d: rows past the launch keep the input's bits (its NaN rows included)
            assert torch.equal(_bits(buf[n:]), _bits(job.d0.cpu()[n:])), cid + " z (aliasing d): a row past the launch was written"
        else:
            _check_canary(cid + " " + key, buf, _rows_mask(buf.shape, n))
        assert bool(torch.isfinite(buf[:n].float()).all()), "%s %s: not finite" % (cid, key)
        if on(key):
            _check_gate(cid, key, buf[:n].float(), ref[key], ref["g_" + key])
    for key in ("mean", "rstd") + (("sc",) if job.y8_on else ()):
        buf = out[key]
        _check_canary(cid + " " + key, buf, _rows_mask(buf.shape, n))
        assert bool(torch.isfinite(buf[:n]).all()), "%s %s: not finite" % (cid, key)
        if on(key):
            _check_gate(cid, "y8_scale" if key == "sc" else key, buf[:n], ref[key], ref["g_" + key])
    if job.y8_on:
        q = out["y8"]
        asg = torch.zeros(q.shape, dtype=torch.bool)
        asg[:n, :H] = True
        _check_canary(cid + " y8", q, asg, CAN8)
        deq = q[:n, :H].contiguous().view(torch.float8_e4m3fn).float() * out["sc"][:n, None]
        if on("y8"):
            _check_gate(cid, "y8", deq, ref["y8"], ref["g_y8"])


def _compare_bwd(cid, job, out, ref, only=None, deferred=False):
    n, M, H = ref["rows"], job.M, job.H
    on = (lambda k: only is None or k in only)
    for key in ("dz", "dd"):
        buf = out[key]
        if buf is None:
            continue
        _check_canary(cid + " " + key, buf, _rows_mask(buf.shape, n))
        assert bool(torch.isfinite(buf[:n].float()).all()), "%s %s: not finite" % (cid, key)
        if on(key):
            _check_gate(cid, key, buf[:n].float(), ref[key], ref["g_" + key])
    for key in ("dgamma", "dbeta"):
        buf = out[key]
        _check_canary(cid + " " + key, buf, _rows_mask(buf.shape, 0 if deferred else H))
        if not deferred:
            assert bool(torch.isfinite(buf[:H]).all()), "%s %s: not finite" % (cid, key)
            if on(key):
                _check_gate(cid, key, buf[:H], ref[key], ref["g_" + key])
    tail = out["partial"][job.nrec * 2 * H:]
    assert bool((_bits(tail) == CAN32).all()), cid + " partial: written past its vk_ln_bwd_partial_rows(M) records"


def _same_bits(cid, a, b):
    for key in a:
        if a[key] is not None:
            assert torch.equal(_bits(a[key]), _bits(b[key])), "%s %s: two identical launches differ" % (cid, key)


def _refs(case, inp):
    n = A.case_rows(case)
    fwd = A.restate_fwd(inp, n, case.y8)
    zb, mean, rstd = A.backward_inputs(A.restate_fwd(inp) if n < case.M else fwd)
    return fwd, (zb, mean, rstd), A.restate_bwd(inp, zb, mean, rstd, n, case.dd, case.acc)


@pytest.mark.parametrize("case", A.CASES, ids=[c.id for c in A.CASES])
def test_kernels_match_restatement(case):
    inp = A.make_inputs(case)
    fwd, (zb, mean, rstd), bwd = _refs(case, inp)
    const = case.profile == "const"          # ill-conditioned on purpose (ln_restate.CASES): finiteness, write sets and the gate of mean
    f1 = Fwd(inp, case.z, case.dyn, case.y8).run().host()
    job = Fwd(inp, case.z, case.dyn, case.y8).run()
    _compare_fwd(case.id, job, job.host(), fwd, only=("mean",) if const else None)
    _same_bits(case.id, f1, job.host())
    b1 = Bwd(inp, zb, mean, rstd, case.dd, case.dyn, case.acc).run().host()
    job = Bwd(inp, zb, mean, rstd, case.dd, case.dyn, case.acc).run()
    _compare_bwd(case.id, job, job.host(), bwd, only=() if const else None)
    _same_bits(case.id, b1, job.host())


def test_chained_forward_backward():
    """The backward fed the forward KERNEL's z, mean and rstd (what the engine does): restated on exactly those inputs."""
    case = A.CASE["M1000-H768-pre-randn-split"]
    inp = A.make_inputs(case)
    f = Fwd(inp).run()
    out = f.host()
    _compare_fwd("chained", f, out, A.restate_fwd(inp))
    zb, mean, rstd = out["z"][:case.M], out["mean"][:case.M], out["rstd"][:case.M]
    b = Bwd(inp, zb, mean, rstd).run()
    _compare_bwd("chained", b, b.host(), A.restate_bwd(inp, zb, mean, rstd))


# ------------------------------------------------------------------------------------------------ two jobs in one launch
def _pair_cases(Ma, Mb, H):
    """Two different jobs of equal H: row count, dropout mode, row mapping and out_scale all differ."""
    return (A._c(Ma, H, "pre", split=True, addvec=True, name="pair-a-M%d-H%d" % (Ma, H)),
            A._c(Mb, H, "post05", "wide", split=True, seg="single", name="pair-b-M%d-H%d" % (Mb, H)))


PAIRS = [(33, 50, 768), (5, 1000, 1284), (0, 50, 768), (33, 0, 768), (17, 16, 2048)]


@pytest.mark.parametrize("Ma,Mb,H", PAIRS, ids=["Ma%d-Mb%d-H%d" % p for p in PAIRS])
def test_forward_pair(Ma, Mb, H):
    """vk_ln_fwd_pair: bitwise the two single launches, inside the gates; a job without rows writes nothing."""
    L = _lib()
    cases = _pair_cases(Ma, Mb, H)
    inps = [A.make_inputs(c) for c in cases]
    single = [Fwd(i).run().host() if i["M"] > 0 else Fwd(i).host() for i in inps]
    jobs = [Fwd(i) for i in inps]
    L.check(L.lib.vk_ln_fwd_pair(C.byref(jobs[0].args), C.byref(jobs[1].args), L.stream_ptr()))
    torch.cuda.synchronize()
    for c, i, j, s in zip(cases, inps, jobs, single):
        out = j.host()
        _compare_fwd(c.id, j, out, A.restate_fwd(i))
        _same_bits(c.id, s, out)


@pytest.mark.parametrize("Ma,Mb,H", PAIRS, ids=["Ma%d-Mb%d-H%d" % p for p in PAIRS])
def test_backward_pair_shared_layernorm(Ma, Mb, H):
    """vk_ln_bwd_pair in the engine's shared-LayerNorm form: job a assigns dgamma / dbeta (accumulate 0), job b adds to the same
    vectors (accumulate 1).  dz / dd are bitwise those of the single launches, dgamma / dbeta bitwise those of a then b alone, and the
    sum of both jobs within the sum of their gates.  A job without rows contributes a zero sum."""
    L = _lib()
    cases = _pair_cases(Ma, Mb, H)
    inps = [A.make_inputs(c) for c in cases]
    bins = [A.backward_inputs(A.restate_fwd(i)) for i in inps]
    refs = [A.restate_bwd(i, *b) for i, b in zip(inps, bins)]

    def jobs():
        shared = (_canary32(H + XC), _canary32(H + XC))
        return [Bwd(i, *b, acc=k, shared=shared) for k, (i, b) in enumerate(zip(inps, bins))]
    single = jobs()
    for j in single:
        j.run()
    pair = jobs()
    L.check(L.lib.vk_ln_bwd_pair(C.byref(pair[0].args), C.byref(pair[1].args), L.stream_ptr()))
    torch.cuda.synchronize()
    total = {}
    for key in ("dgamma", "dbeta"):
        total[key] = refs[0][key] + refs[1][key]
        total["g_" + key] = A.G * (refs[0]["E_" + key] + refs[1]["E_" + key] + A.U * total[key].abs()) + A.TINY
    for c, j, s, r in zip(cases, pair, single, refs):
        out = j.host()
        _compare_bwd(c.id, j, out, dict(r, **total))
        _same_bits(c.id, s.host(), out)


# ------------------------------------------------------------------------------------------------ accumulate bits
def test_deferred_finalize():
    """accumulate bit 1: the launch leaves dgamma / dbeta at their canary (dz / dd are written); vk_ln_bwd_finalize with the same
    arguments then produces the bits of the undeferred launch.  With bit 0 as well, onto a known prior value."""
    L = _lib()
    for cid, acc in (("M1000-H768-pre-randn-split", 0), ("M33-H768-pre-randn-split-acc", 1), ("M17-H1536-none-randn-dyn9-acc", 1)):
        case = A.CASE[cid]
        inp = A.make_inputs(case)
        _, (zb, mean, rstd), ref = _refs(case._replace(acc=acc), inp)
        plain = Bwd(inp, zb, mean, rstd, dyn=case.dyn, acc=acc).run().host()
        job = Bwd(inp, zb, mean, rstd, dyn=case.dyn, acc=acc | 2).run()
        out = job.host()
        if acc:                  # the prior value is still there, untouched
            assert torch.equal(out["dgamma"][:case.H], inp["dgamma0"]) and torch.equal(out["dbeta"][:case.H], inp["dbeta0"])
            assert bool((_bits(out["dgamma"][case.H:]) == CAN32).all()) and bool((_bits(out["dbeta"][case.H:]) == CAN32).all())
            _compare_bwd(cid, job, dict(out, dgamma=_canary32(case.H + XC).cpu(), dbeta=_canary32(case.H + XC).cpu()), ref, deferred=True)
        else:
            _compare_bwd(cid, job, out, ref, deferred=True)
        L.check(L.lib.vk_ln_bwd_finalize(C.byref(job.args), L.stream_ptr()))
        torch.cuda.synchronize()
        out = job.host()
        _compare_bwd(cid + "-finalized", job, out, ref)
        _same_bits(cid, plain, out)


# ------------------------------------------------------------------------------------------------ rejections
def _untouched(job):
    for key, buf in job.host().items():
        if buf is not None and not (key == "z" and getattr(job, "zmode", "") == "alias"):
            can = CAN8 if buf.dtype == torch.uint8 else CAN16 if buf.dtype == torch.bfloat16 else CAN32
            assert bool((_bits(buf) == can).all()), key + ": written by a rejected launch"


def _rejected(rc):
    L = _lib()
    torch.cuda.synchronize()
    assert rc != 0
    msg = L.lib.vk_last_error().decode()
    assert "H" in msg and len(msg) > 8, msg


@pytest.mark.parametrize("H", [6, 0, 2052])
def test_bad_width_is_refused(H):
    """ln_check: H must be a positive multiple of 4 and at most 2048.  The buffers are sized for a valid H; nothing is launched."""
    L = _lib()
    inp = A.make_inputs(A._c(5, 2048, "pre", split=True, name="reject"))
    f = Fwd(inp, y8=True, H=H)
    _rejected(L.lib.vk_ln_fwd(C.byref(f.args), L.stream_ptr()))
    _untouched(f)
    zb, mean, rstd = A.backward_inputs(A.restate_fwd(inp))
    b = Bwd(inp, zb, mean, rstd, H=H)
    _rejected(L.lib.vk_ln_bwd(C.byref(b.args), L.stream_ptr()))
    _untouched(b)
    _rejected(L.lib.vk_ln_fwd_pair(C.byref(f.args), C.byref(f.args), L.stream_ptr()))
    _rejected(L.lib.vk_ln_bwd_pair(C.byref(b.args), C.byref(b.args), L.stream_ptr()))
    _untouched(f)
    _untouched(b)


@pytest.mark.parametrize("why", ["unequal_H", "dyn_a", "dyn_b"])
def test_bad_pair_is_refused(why):
    """A pair needs one H and static row counts in both jobs."""
    L = _lib()
    Hb = 1024 if why == "unequal_H" else 768
    ca, cb = A._c(9, 768, "pre", split=True, name="reject-a"), A._c(7, Hb, "post", name="reject-b")
    ia, ib = A.make_inputs(ca), A.make_inputs(cb)
    fa, fb = Fwd(ia, dyn=9 if why == "dyn_a" else None), Fwd(ib, dyn=7 if why == "dyn_b" else None)
    _rejected(L.lib.vk_ln_fwd_pair(C.byref(fa.args), C.byref(fb.args), L.stream_ptr()))
    ba = Bwd(ia, *A.backward_inputs(A.restate_fwd(ia)), dyn=9 if why == "dyn_a" else None)
    bb = Bwd(ib, *A.backward_inputs(A.restate_fwd(ib)), dyn=7 if why == "dyn_b" else None)
    _rejected(L.lib.vk_ln_bwd_pair(C.byref(ba.args), C.byref(bb.args), L.stream_ptr()))
    for job in (fa, fb, ba, bb):
        _untouched(job)


def test_zz_report_worst_ratios():
    """Prints the worst |got - ref| / gate seen per output in this run, and the case it occurred in (recorded, not asserted beyond <= 1)."""
    for name in sorted(RATIOS):
        print("LNWORST %-9s %.4f  %s" % (name, RATIOS[name][0], RATIOS[name][1]))
    assert all(r <= 1.0 for r, _ in RATIOS.values())
