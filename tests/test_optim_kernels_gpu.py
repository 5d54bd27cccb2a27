"""The optimizer and reduction kernels (csrc/optim.hip, the cast and product of csrc/misc.hip) through the C ABI against the float64
restatements of tests/optim_restate.py, elementwise, under the gates derived there, on buffers the engine never produces:
  * every input is followed by a NaN pad; p / g / m / v of skipped chunks and tensors, g of masked chunks, the gaps between slabs and the
    rows past a device-side count hold NaN: every result finite and inside its gate shows nothing outside the contract's inputs was used;
  * every output is prefilled with a NaN canary (0xFFA5 / 0xFFA5A5A5): what the contract assigns must be written, everything else --
    skipped chunks, untouched tensors, pads, sums outside the range, the floats behind the scratch, rows past the count -- keeps its bits;
  * the forms the header calls bit-identical are compared bit for bit, and every launch repeated gives the same bits.
The case table is tests/optim_restate.py's; tests/test_optim_cpu.py checks the gates themselves.  Refusals return before launching.  GPU only."""
import ctypes as C
import math
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_restate as A  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
CAN16 = -91                         # bf16 canary bits 0xFFA5: a negative NaN no bf16 conversion produces
CAN32 = 0xFFA5A5A5 - (1 << 32)      # fp32 canary bits
PAD = 64
NAN = float("nan")


def _lib():
    from volta_amd import _lib as L
    return L


def _can16(n):
    return torch.full((n,), CAN16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def _can32(n):
    return torch.full((n,), CAN32, dtype=torch.int32, device=DEV).view(torch.float32)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _is_can(t):
    return bool((_bits(t) == (CAN16 if t.dtype == torch.bfloat16 else CAN32)).all())


def _no_can(t):
    return not bool((_bits(t) == (CAN16 if t.dtype == torch.bfloat16 else CAN32)).any())


def _padded(t, fill=NAN, pad=PAD):
    """t on the device followed by `pad` elements of NaN (fp32) -- or of canary bits when fill is None."""
    out = _can32(t.numel() + pad) if fill is None else torch.full((t.numel() + pad,), fill, dtype=torch.float32, device=DEV)
    out[:t.numel()] = t.to(DEV)
    return out


def _ok(rc):
    L = _lib()
    L.check(rc)


def _refused(rc):
    assert rc != 0 and _lib().lib.vk_last_error()
    torch.cuda.synchronize()


def _args(h, n=0, p=None, g=None, m=None, v=None, shadow=None, cls=None, clip=None):
    L = _lib()
    a = L.AdamwArgs()
    a.p, a.g, a.m, a.v, a.shadow, a.chunk_class, a.clip, a.n = p, g, m, v, shadow, cls, clip, n
    for i in range(8):
        a.cls_lr_mult[i], a.cls_wd[i] = h.mult[i], h.wd[i]
    a.lr, a.beta1, a.beta2, a.eps, a.step_mult, a.grad_scale = h.lr, h.b1, h.b2, h.eps, h.step_mult, h.grad_scale
    return a


def _clip_dev(h):
    return None if h.clip is None else torch.tensor([NAN, h.clip, NAN, NAN], dtype=torch.float32, device=DEV)


def _descs(rows):
    """Device copy of a vk_adamw_tensor array from (p, g, m, v, numel, cls) rows."""
    L = _lib()
    arr = (L.AdamwTensor * len(rows))()
    for i, (p, g, m, v, numel, cls) in enumerate(rows):
        arr[i] = L.AdamwTensor(p, g, m, v, numel, cls, 0)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)


# ================================================================================================ AdamW over the arena
class Arena:
    """Device buffers of one arena case: NaN / canary in skipped chunks and pads, chunk_class as an offset view with `fill` around it."""

    def __init__(self, case, inp, fill=255):
        n = case.nch * A.CHUNK
        self.case, self.n = case, n
        ce = A.cls_elem(inp["cls"], case.nch)
        self.skip = (ce == A.SKIP).to(DEV)
        self.p, self.m, self.v = (_padded(inp[k], None) for k in "pmv")
        for t in (self.p, self.m, self.v):
            _bits(t)[:n][self.skip] = CAN32
        self.gs = []
        for g in inp["gs"]:
            g = _padded(g)
            g[:n][self.skip] = NAN
            self.gs.append(g)
        self.shadow = _can16(n + PAD) if case.shadow else None
        self.clsbuf = None
        if inp["cls"] is not None:
            size = (case.cls_off + case.nch + 4 + 3) // 4 * 4
            self.clsbuf = torch.full((size,), fill, dtype=torch.uint8, device=DEV)
            self.clsbuf[case.cls_off:case.cls_off + case.nch] = inp["cls"].to(DEV)
        self.clip = _clip_dev(case.h)

    def cls_ptr(self):
        return None if self.clsbuf is None else self.clsbuf.data_ptr() + self.case.cls_off

    def step(self, s, form, ncus=None):
        L = _lib()
        a = _args(self.case.h, self.n, self.p.data_ptr(), self.gs[s].data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                  None if self.shadow is None else self.shadow.data_ptr(), self.cls_ptr(), None if self.clip is None else self.clip.data_ptr())
        if form == "wide":
            _ok(L.lib.vk_adamw_step(C.byref(a), L.stream_ptr()))
        elif form == "narrow":
            _ok(L.lib.vk_adamw_step_on(C.byref(a), ncus, L.stream_ptr()))
        else:                                              # the list form over the same data: whole chunks, or every chunk cut at 301 floats
            cuts = ((0, A.CHUNK),) if form == "list-chunks" else ((0, 301), (301, A.CHUNK))
            cls = [0] * self.case.nch if self.clsbuf is None else self.clsbuf[self.case.cls_off:self.case.cls_off + self.case.nch].tolist()
            rows = []
            for c in range(self.case.nch):
                for lo, hi in cuts:
                    rows.append(tuple(t.data_ptr() + 4 * (c * A.CHUNK + lo) for t in (self.p, self.gs[s], self.m, self.v)) + (hi - lo, cls[c]))
            self.d = _descs(rows)
            _ok(L.lib.vk_adamw_step_list(C.byref(a), self.d.data_ptr(), len(rows), A.CHUNK, L.stream_ptr()))
        torch.cuda.synchronize()
        return [t.clone() for t in (self.p, self.m, self.v)] + ([self.shadow.clone()] if self.shadow is not None and not form.startswith("list") else [])


@pytest.mark.parametrize("case", A.ADAM_CASES, ids=[c.id for c in A.ADAM_CASES])
def test_adamw_arena_forms_against_the_restatement_and_each_other(case):
    inp = A.adam_inputs(case)
    n = case.nch * A.CHUNK
    ce = A.cls_elem(inp["cls"], case.nch).to(DEV)
    live = ce != A.SKIP
    clean = {k: torch.where(live, inp[k].to(DEV), torch.zeros((), device=DEV)) for k in "pmv"}
    ref = A.AdamW64(clean["p"], clean["m"], clean["v"], ce, case.h)
    runs = [("wide", None, 255), ("wide", None, 0)] + [("narrow", k, 255) for k in A.NCUS] + [("narrow", 24, 0), ("list-chunks", None, 255), ("list-cut", None, 255)]
    arenas = [Arena(case, inp, fill) for _, _, fill in runs]
    for s in range(A.ADAM_STEPS):
        ref.step(torch.where(live, inp["gs"][s].to(DEV), torch.zeros((), device=DEV)))
        outs = [ar.step(s, form, ncus) for ar, (form, ncus, _) in zip(arenas, runs)]
        p, m, v = outs[0][:3]
        for t in (p, m, v):                                # the write set: live chunks written and finite, skipped chunks and the pad keep their bits
            assert _is_can(t[n:]) and _is_can(t[:n][~live]) and bool(torch.isfinite(t[:n][live]).all())
        ex = max(A.ratio(got[:n][live], want[live], err[live]) for got, want, err in ((p, ref.p, ref.Ep), (m, ref.m, ref.Em), (v, ref.v, ref.Ev)))
        assert ex <= 1.0, (case.id, s, ex)
        if case.shadow:
            sh = outs[0][3]
            assert _is_can(sh[n:]) and _is_can(sh[:n][~live]) and _same(sh[:n][live], p[:n][live].cpu().bfloat16().to(DEV))
        for (form, ncus, fill), o in zip(runs[1:], outs[1:]):
            assert len(o) >= 3 and all(_same(x, y) for x, y in zip(outs[0], o)), (case.id, s, form, ncus, fill)


# ================================================================================================ AdamW over a tensor list
def _carve(table, which_arr, data, filler):
    """One buffer holding every tensor of the table for array `which_arr`, 16-byte-aligned starts (+ the table's offset for the one array it
    names), gaps and pad of `filler` bits / NaN; returns (buffer, element offsets)."""
    offs, at = [], 8
    for numel, _, which, off in table:
        o = at + (off if which == which_arr else 0)
        offs.append(o)
        at = (o + numel + 8 + 3) // 4 * 4
    buf = _can32(at + PAD) if filler is None else torch.full((at + PAD,), NAN, dtype=torch.float32, device=DEV)
    for o, t in zip(offs, data):
        buf[o:o + t.numel()] = t.to(DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, offs


def _list_data(table, seed):
    gen = torch.Generator().manual_seed(seed)
    return [A.adam_data(numel, gen) for numel, _, _, _ in table]


def test_adamw_list_against_the_restatement():
    L = _lib()
    table = A.list_table()
    data = _list_data(table, 11)
    h = A.hyper(clip=0.71, grad_scale=0.5)
    livet = [0 <= cls <= 7 for _, cls, _, _ in table]
    ce = torch.cat([torch.full((numel,), cls, dtype=torch.int64) for numel, cls, _, _ in table]).to(DEV)
    cat = lambda k: torch.cat([d[k] for d in data]).to(DEV)
    ref = A.AdamW64(cat(0), cat(1), cat(2), ce, h)
    results = []
    for rep in range(2):
        bufs = {}
        for k, name in enumerate("pmv"):
            src = [d[k] if lv else torch.full_like(d[k], NAN) for d, lv in zip(data, livet)]
            bufs[name] = _carve(table, name, src, None)
            for o, (numel, _, _, _), lv in zip(bufs[name][1], table, livet):
                if not lv:
                    _bits(bufs[name][0])[o:o + numel] = CAN32
        clip = _clip_dev(h)
        a = _args(h, clip=clip.data_ptr())
        snaps = []
        for s in range(A.ADAM_STEPS):
            gb, go = _carve(table, "g", [d[3][s] if lv else torch.full_like(d[3][s], NAN) for d, lv in zip(data, livet)], NAN)
            rows = [tuple(bufs[x][0].data_ptr() + 4 * bufs[x][1][i] for x in "p") + (gb.data_ptr() + 4 * go[i],) +
                    tuple(bufs[x][0].data_ptr() + 4 * bufs[x][1][i] for x in "mv") + (numel, cls) for i, (numel, cls, _, _) in enumerate(table)]
            d = _descs(rows)
            _ok(L.lib.vk_adamw_step_list(C.byref(a), d.data_ptr(), len(rows), max(t[0] for t in table), L.stream_ptr()))
            torch.cuda.synchronize()
            snaps.append({x: bufs[x][0].clone() for x in "pmv"})
            if rep == 0:
                ref.step(torch.cat([d_[3][s] for d_ in data]))
                for x, want, err in (("p", ref.p, ref.Ep), ("m", ref.m, ref.Em), ("v", ref.v, ref.Ev)):
                    buf, offs = bufs[x]
                    inside = torch.zeros(buf.numel(), dtype=torch.bool, device=DEV)
                    at = 0
                    for o, (numel, cls, _, _), lv in zip(offs, table, livet):
                        if lv:
                            inside[o:o + numel] = True
                            assert bool(torch.isfinite(buf[o:o + numel]).all())
                            ex = A.ratio(buf[o:o + numel], want[at:at + numel], err[at:at + numel])
                            assert ex <= 1.0, (s, x, numel, cls, ex)
                        at += numel
                    assert _is_can(buf[~inside])             # gaps, pad, and the tensors of class VK_CHUNK_SKIP, 8 and -1
        results.append(snaps)
    assert all(_same(results[0][s][x], results[1][s][x]) for s in range(A.ADAM_STEPS) for x in "pmv")


def test_sqnorm_list_slots_are_functions_of_their_own_tensor():
    L = _lib()
    table = A.list_table()
    gen = torch.Generator().manual_seed(12)
    gs = [torch.randn(numel, generator=gen) if cls != A.SKIP else torch.full((numel,), NAN) for numel, cls, _, _ in table]
    gb, go = _carve(table, "g", gs, NAN)
    wf = L.lib.vk_grad_sqnorm_list_work_floats()
    assert wf == 2 * 64                                       # 64 double partials per tensor

    def run(order, max_numel):
        rows = [(None, gb.data_ptr() + 4 * go[i], None, None, table[i][0], table[i][1]) for i in order]
        d = _descs(rows)
        work, sums = _can32(len(order) * wf + PAD), _can32(len(order) + PAD)
        _ok(L.lib.vk_grad_sqnorm_list(d.data_ptr(), len(order), max_numel, work.data_ptr(), sums.data_ptr(), L.stream_ptr()))
        torch.cuda.synchronize()
        assert _is_can(sums[len(order):]) and _is_can(work[len(order) * wf:]) and _no_can(sums[:len(order)])
        return sums[:len(order)].clone()
    full = list(range(len(table)))
    mx = max(t[0] for t in table)
    s0 = run(full, mx)
    for i, (numel, cls, _, _) in enumerate(table):
        want = float((gs[i].double() ** 2).sum()) if cls != A.SKIP else 0.0           # VK_CHUNK_SKIP alone is left out (exactly 0, its NaN g not read); 8 and -1 are summed
        assert A.ratio(s0[i], want, A.E_LIST * want) <= 1.0, (i, numel, cls, float(s0[i]), want)
    assert all(_same(s0, run(full, x)) for x in A.list_max_numels(mx))
    rev = full[::-1][::2]
    assert _same(s0[rev], run(rev, mx))
    assert _same(s0[5:6], run([5], table[5][0]))
    d = _descs([(None, gb.data_ptr(), None, None, 4, 0)])
    sums = _can32(8)
    _refused(L.lib.vk_grad_sqnorm_list(d.data_ptr(), 65536, 4, sums.data_ptr(), sums.data_ptr(), L.stream_ptr()))
    assert _is_can(sums)


# ================================================================================================ norms
def _plan_on_device(total, mode):
    exp, mask, heavy, hskip = A.norm_plan(total, mode)
    g = torch.full((total * A.CHUNK + PAD,), NAN, dtype=torch.float32, device=DEV)
    want = torch.empty(total, dtype=torch.float64, device=DEV)
    for lo in range(0, total, 32768):
        hi = min(lo + 32768, total)
        g[lo * A.CHUNK:hi * A.CHUNK] = A.norm_grad(exp, DEV, lo, hi)
        want[lo:hi] = A.chunk_sums64(g[lo * A.CHUNK:hi * A.CHUNK])
    maskd = None
    if mask is not None:
        maskd = torch.full((total + PAD,), 0, dtype=torch.uint8, device=DEV)      # live classes behind the mask: a read past it would add NaN chunks
        maskd[:total] = mask.to(DEV)
        g[:total * A.CHUNK].view(-1, A.CHUNK)[maskd[:total] == A.SKIP] = NAN
        want = torch.where(maskd[:total] == A.SKIP, torch.zeros_like(want), want)
    return g, maskd, want


def _check_out(out, S, N, pre, mx, tag):
    norm, En, coef, Ec = A.norm_clip64(S, (N + 1) * A.U, pre, mx)
    o = out.cpu()
    assert _is_can(out[2:]) and A.ratio(o[0], norm, En) <= 1.0 and A.ratio(o[1], coef, Ec) <= 1.0, (tag, o[:2].tolist(), norm, coef, En, Ec)
    if mx <= 0:
        assert float(o[1]) == 1.0


def _norm_forms(total, mode, pre, max_mode, tag):
    L = _lib()
    st = L.stream_ptr()
    g, mask, want = _plan_on_device(total, mode)
    n = total * A.CHUNK
    S = float(want.sum())
    mx = A.max_norm_for(max_mode, math.sqrt(S) * pre)
    mp = None if mask is None else mask.data_ptr()
    nb = L.lib.vk_grad_norm_workspace_floats()
    assert nb == A.NORM_BLOCKS
    outs = []
    for rep in range(2):                                       # the one-call form
        partial, out = _can32(nb + PAD), _can32(8)
        if mask is None:
            _ok(L.lib.vk_grad_norm_clip(g.data_ptr(), n, pre, mx, partial.data_ptr(), out.data_ptr(), st))
        else:
            _ok(L.lib.vk_grad_norm_clip_masked(g.data_ptr(), n, mp, pre, mx, partial.data_ptr(), out.data_ptr(), st))
        torch.cuda.synchronize()
        assert _is_can(partial[nb:]) and _no_can(partial[:nb])
        _check_out(out, S, A.n_partial(n), pre, mx, tag + " one-call")
        outs.append((partial, out))
    assert _same(outs[0][0], outs[1][0]) and _same(outs[0][1], outs[1][1])

    def chunks(ranges, zero):                                  # the shard-decomposable form
        sums = _can32(total + 2 * A.SQ_GROUPS + PAD)
        if zero:
            sums[:total] = 0
        for c0, k in ranges:
            _ok(L.lib.vk_grad_sqnorm_chunks(g.data_ptr(), c0, k, mp, sums.data_ptr(), st))
        torch.cuda.synchronize()
        return sums
    sums = chunks([(0, total)], False)
    assert _is_can(sums[total:]) and A.ratio(sums[:total], want, (A.N_CHUNK + 1) * A.U * want) <= 1.0, tag
    assert _same(sums, chunks([(0, total)], False))
    for c0, k in A.chunk_ranges(total):
        part = chunks([(c0, k)], False)
        assert _same(part[c0:c0 + k], sums[c0:c0 + k]) and _is_can(part[:c0]) and _is_can(part[c0 + k:]), (tag, c0, k)

    def finish(sums):
        out = _can32(8)
        _ok(L.lib.vk_grad_norm_from_chunks(sums.data_ptr(), total, pre, mx, out.data_ptr(), st))
        torch.cuda.synchronize()
        assert _is_can(sums[total + 2 * A.SQ_GROUPS:])        # nothing behind the 256 floats of scratch
        _check_out(out, S, A.N_CHUNK, pre, mx, tag + " chunks")
        return out
    keep = sums[:total].clone()
    out = finish(sums)
    assert _same(keep, sums[:total]) and _same(out, finish(sums))
    for ranges in A.shard_plans(total):
        parts = len(ranges)
        sh = chunks(ranges, True)
        assert _same(sh[:total], keep), (tag, parts)
        assert _same(finish(sh), out), (tag, parts)


@pytest.mark.parametrize("case", A.NORM_CASES, ids=[c.id for c in A.NORM_CASES])
def test_norm_forms_against_the_restatement_and_shard_decomposition(case):
    total = A.full_chunks() if case.total == A.FULL else case.total
    _norm_forms(total, case.mask, A.f32(case.pre_scale), case.max_mode, case.id)


# ================================================================================================ slab sums, tail, axpy
def _slabs(nslabs, n, stride, gen, dtype=torch.float32):
    src = torch.full((nslabs * stride + PAD,), NAN, dtype=torch.float32, device=DEV)
    data = torch.randn(nslabs, n, generator=gen).to(DEV)
    for s in range(nslabs):
        src[s * stride:s * stride + n] = data[s]
    return src, data


def _seq(data):
    a = data[0].clone()
    for s in range(1, data.shape[0]):
        a += data[s]
    return a


@pytest.mark.parametrize("nslabs", A.SLAB_COUNTS)
def test_sum_slabs_f32_gives_the_bits_of_the_sequential_sum(nslabs):
    L = _lib()
    gen = torch.Generator().manual_seed(20 + nslabs)
    for n in A.SLAB_NS:
        for stride in A.slab_strides(n):
            src, data = _slabs(nslabs, n, stride, gen)
            want, bound = A.slabs64(data)
            got = []
            for rep in range(2):
                dst = _can32(n + PAD)
                _ok(L.lib.vk_sum_slabs_f32(dst.data_ptr(), src.data_ptr(), stride, nslabs, n, L.stream_ptr()))
                torch.cuda.synchronize()
                assert _is_can(dst[n:]) and _same(dst[:n], _seq(data)) and A.ratio(dst[:n], want, bound) <= 1.0, (nslabs, n, stride)
                got.append(dst)
            assert _same(*got)


@pytest.mark.parametrize("case", A.SLAB_BF, ids=[c.id for c in A.SLAB_BF])
def test_sum_slabs_bf16_rounds_the_sequential_sum_and_stops_at_the_device_count(case):
    L = _lib()
    gen = torch.Generator().manual_seed(31)
    n = case.rows * case.row_len
    rows = case.rows if case.dyn is None else min(case.dyn, case.rows)
    stride = A.slab_strides(n)[1]
    src, data = _slabs(case.nslabs, n, stride, gen)
    for s in range(case.nslabs):
        src[s * stride + rows * case.row_len:s * stride + n] = NAN
    dyn = None if case.dyn is None else torch.tensor([case.dyn, -1, -1, -1], dtype=torch.int32, device=DEV)
    got = []
    for rep in range(2):
        dst = _can16(n + PAD)
        _ok(L.lib.vk_sum_slabs_bf16(dst.data_ptr(), src.data_ptr(), stride, case.nslabs, n, None if dyn is None else dyn.data_ptr(), case.row_len, L.stream_ptr()))
        torch.cuda.synchronize()
        k = rows * case.row_len
        assert _is_can(dst[k:]) and _same(dst[:k], _seq(data)[:k].cpu().bfloat16().to(DEV)), case.id
        got.append(dst)
    assert _same(*got)


def test_side_tail_sixteen_mixed_jobs_in_one_launch():
    L = _lib()
    gen = torch.Generator().manual_seed(41)
    results = []
    for rep in range(2):
        gen.manual_seed(41)
        jobs, checks = (L.TailJob * 16)(), []
        keep = []
        for i, (kind, n, count, count2, acc) in enumerate(A.TAIL_JOBS):
            if kind == 0:
                stride = (n + 3) // 4 * 4 + 4 * (i % 3)
                src, data = _slabs(count, n, stride, gen)
                dst = _can32(n + PAD)
                jobs[i] = L.TailJob(dst.data_ptr(), None, src.data_ptr(), None, stride, n, 0, count, 0, 0)
                checks.append((0, dst, n, data, None))
                keep.append(src)
            else:
                H = n
                rec = torch.randn(count, 2, H, generator=gen)
                rec2 = torch.randn(count2, 2, H, generator=gen) if count2 else None
                old = torch.randn(2, H, generator=gen) if acc else None
                r1, r2 = _padded(rec.reshape(-1)), None if rec2 is None else _padded(rec2.reshape(-1))
                dg, db = _can32(H + PAD), _can32(H + PAD)
                if acc:
                    dg[:H], db[:H] = old[0].to(DEV), old[1].to(DEV)
                jobs[i] = L.TailJob(dg.data_ptr(), db.data_ptr(), r1.data_ptr(), None if r2 is None else r2.data_ptr(), count2 or 0, H, 1, count, acc, 0)
                checks.append((1, (dg, db), H, A.tail_cols64(rec, rec2, old), None))
                keep += [r1, r2]
        _ok(L.lib.vk_side_tail(jobs, 16, L.stream_ptr()))
        torch.cuda.synchronize()
        outs = []
        for i, (kind, dst, n, ref, _) in enumerate(checks):
            if kind == 0:
                want, bound = A.slabs64(ref)
                assert _is_can(dst[n:]) and _same(dst[:n], _seq(ref)) and A.ratio(dst[:n], want, bound) <= 1.0, i
                outs.append(dst)
            else:
                (want, bound) = ref
                for k in range(2):
                    assert _is_can(dst[k][n:]) and A.ratio(dst[k][:n], want[k], bound[k]) <= 1.0, (i, k, A.TAIL_JOBS[i])
                    outs.append(dst[k])
        results.append(outs)
    assert all(_same(x, y) for x, y in zip(*results))


def test_axpy_against_the_restatement():
    L = _lib()
    gen = torch.Generator().manual_seed(51)
    for n, alpha in ((4, 1.0), (1028, -0.37), (A.GRID_SLABS + 4, 3.0)):
        x, y0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        want, bound = A.axpy64(y0.to(DEV), x.to(DEV), A.f32(alpha))
        got = []
        for rep in range(2):
            xd, y = _padded(x), _padded(y0, None)
            _ok(L.lib.vk_axpy_f32(y.data_ptr(), xd.data_ptr(), alpha, n, L.stream_ptr()))
            torch.cuda.synchronize()
            assert _is_can(y[n:]) and A.ratio(y[:n], want, bound) <= 1.0, (n, alpha)
            got.append(y)
        assert _same(*got)


# ================================================================================================ cast, mul
def _cast(src, n):
    L = _lib()
    dst = _can16(n + PAD)
    _ok(L.lib.vk_cast_f32_bf16(src.data_ptr(), dst.data_ptr(), n, L.stream_ptr()))
    torch.cuda.synchronize()
    assert _is_can(dst[n:])
    return dst


def test_cast_rounds_to_nearest_even():
    gen = torch.Generator().manual_seed(61)
    for n in A.CAST_NS:
        x = torch.randn(n, generator=gen) * torch.pow(10.0, torch.randint(-20, 20, (n,), generator=gen).float())
        src = _padded(x)
        dst = _cast(src, n)
        assert _same(dst[:n], x.bfloat16().to(DEV)), n
        assert _same(dst, _cast(src, n))
    s = A.cast_specials()
    for lead in (0, 8):                                      # through the 8-wide body and through the scalar tail
        x = torch.cat([torch.ones(lead), s, torch.ones(-(lead + len(s)) % 8 + (0 if lead else 3))])
        n = len(x) if lead else len(s)
        got = _cast(_padded(x), n)[lead:lead + len(s)].cpu()
        want = s.bfloat16()
        nan = torch.isnan(s)
        print("cast specials (lead %d): got %s want %s" % (lead, [hex(b & 0xFFFF) for b in _bits(got).tolist()], [hex(b & 0xFFFF) for b in _bits(want).tolist()]))
        assert bool(torch.isnan(got[nan].float()).all()) and _same(got[~nan], want[~nan]), lead


@pytest.mark.parametrize("case", A.MUL_CASES, ids=[c.id for c in A.MUL_CASES])
def test_mul_bf16_rounds_the_exact_product(case):
    L = _lib()
    gen = torch.Generator().manual_seed(71)
    n = case.rows * case.row_len
    rows = case.rows if case.dyn is None else min(case.dyn, case.rows)
    k = rows * case.row_len
    a, b = (torch.randn(n, generator=gen) * 8).bfloat16(), (torch.rand(n, generator=gen) + 0.01).bfloat16()
    want = (a.float() * b.float()).bfloat16()[:k].to(DEV)

    def dev(t):
        out = torch.full((n + PAD,), NAN, dtype=torch.bfloat16, device=DEV)
        out[:k] = t[:k].to(DEV)
        return out
    ad, bd = dev(a), dev(b)
    dyn = None if case.dyn is None else torch.tensor([case.dyn, -1, -1, -1], dtype=torch.int32, device=DEV)
    got = []
    for rep in range(2):
        out = _can16(n + PAD)
        _ok(L.lib.vk_mul_bf16(ad.data_ptr(), bd.data_ptr(), out.data_ptr(), n, None if dyn is None else dyn.data_ptr(), case.row_len, L.stream_ptr()))
        torch.cuda.synchronize()
        assert _is_can(out[k:]) and _same(out[:k], want), case.id
        got.append(out)
    assert _same(*got)


# ================================================================================================ refusals
def test_refusals_launch_nothing():
    L = _lib()
    st = L.stream_ptr()
    h = A.hyper()
    p, m, v, g = _can32(4096), _can32(4096), _can32(4096), _can32(4096)
    sh, out, partial, sums = _can16(4096), _can32(8), _can32(A.NORM_BLOCKS + 8), _can32(1024)
    cls = torch.zeros(8, dtype=torch.uint8, device=DEV)
    a = _args(h, 1000, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), sh.data_ptr())
    _refused(L.lib.vk_adamw_step(C.byref(a), st))
    _refused(L.lib.vk_adamw_step_on(C.byref(a), 24, st))
    a.n = 2048
    _refused(L.lib.vk_adamw_step_on(C.byref(a), 0, st))
    _refused(L.lib.vk_adamw_step_on(C.byref(a), 257, st))
    d = _descs([(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 4, 0)])
    _refused(L.lib.vk_adamw_step_list(C.byref(a), d.data_ptr(), 65536, 4, st))
    _refused(L.lib.vk_grad_norm_clip_masked(g.data_ptr(), 1028, cls.data_ptr(), 1.0, 1.0, partial.data_ptr(), out.data_ptr(), st))   # a mask, ragged arena
    _refused(L.lib.vk_grad_norm_clip(g.data_ptr(), 1026, 1.0, 1.0, partial.data_ptr(), out.data_ptr(), st))
    _refused(L.lib.vk_grad_norm_clip(g.data_ptr() + 4, 1024, 1.0, 1.0, partial.data_ptr(), out.data_ptr(), st))
    _refused(L.lib.vk_grad_sqnorm_chunks(g.data_ptr() + 4, 0, 1, None, sums.data_ptr(), st))
    _refused(L.lib.vk_grad_norm_from_chunks(sums.data_ptr(), 3, 1.0, 1.0, out.data_ptr(), st))
    _refused(L.lib.vk_grad_norm_from_chunks(sums.data_ptr(), 0, 1.0, 1.0, out.data_ptr(), st))
    _refused(L.lib.vk_grad_norm_from_chunks(sums.data_ptr(), -2, 1.0, 1.0, out.data_ptr(), st))
    _refused(L.lib.vk_axpy_f32(p.data_ptr(), g.data_ptr(), 1.0, 1026, st))
    _refused(L.lib.vk_axpy_f32(p.data_ptr() + 4, g.data_ptr(), 1.0, 1024, st))
    _refused(L.lib.vk_axpy_f32(p.data_ptr(), g.data_ptr() + 8, 1.0, 1024, st))
    _refused(L.lib.vk_sum_slabs_f32(p.data_ptr() + 4, g.data_ptr(), 1024, 2, 1024, st))
    _refused(L.lib.vk_sum_slabs_f32(p.data_ptr(), g.data_ptr(), 1026, 2, 1024, st))
    _refused(L.lib.vk_sum_slabs_bf16(sh.data_ptr(), g.data_ptr() + 4, 1024, 2, 1024, None, 8, st))
    _refused(L.lib.vk_sum_slabs_bf16(sh.data_ptr() + 4, g.data_ptr(), 1024, 2, 1024, None, 8, st))
    _refused(L.lib.vk_sum_slabs_bf16(sh.data_ptr(), g.data_ptr(), 1024, 2, 1022, None, 8, st))
    sh2, sh3 = _can16(4096), _can16(4096)
    _refused(L.lib.vk_mul_bf16(sh2.data_ptr(), sh3.data_ptr(), sh.data_ptr(), 1028, None, 8, st))
    _refused(L.lib.vk_mul_bf16(sh2.data_ptr(), sh3.data_ptr(), sh.data_ptr(), 1024, None, 12, st))
    for k in range(3):
        ptrs = [sh2.data_ptr(), sh3.data_ptr(), sh.data_ptr()]
        ptrs[k] += 8
        _refused(L.lib.vk_mul_bf16(ptrs[0], ptrs[1], ptrs[2], 1024, None, 8, st))
    _refused(L.lib.vk_cast_f32_bf16(g.data_ptr() + 4, sh.data_ptr(), 1024, st))
    _refused(L.lib.vk_cast_f32_bf16(g.data_ptr(), sh.data_ptr() + 2, 1024, st))
    jobs = (L.TailJob * 17)()
    for i in range(17):
        jobs[i] = L.TailJob(p.data_ptr(), None, g.data_ptr(), None, 1024, 1024, 0, 2, 0, 0)
    _refused(L.lib.vk_side_tail(jobs, 17, st))
    jobs[1].kind = 2
    _refused(L.lib.vk_side_tail(jobs, 2, st))
    jobs[1].kind, jobs[1].dst = 0, p.data_ptr() + 4
    _refused(L.lib.vk_side_tail(jobs, 2, st))
    torch.cuda.synchronize()
    assert all(_is_can(t) for t in (p, m, v, g, sh, sh2, sh3, out, partial, sums))
    # the same three calls with aligned pointers are accepted and compute
    x, y = torch.ones(1024, device=DEV), torch.ones(1024, device=DEV)
    _ok(L.lib.vk_axpy_f32(y.data_ptr(), x.data_ptr(), 2.0, 1024, st))
    a16, o16, s32 = torch.full((1024,), 2.0, dtype=torch.bfloat16, device=DEV), _can16(1024), torch.ones(2048, device=DEV)
    _ok(L.lib.vk_mul_bf16(a16.data_ptr(), a16.data_ptr(), o16.data_ptr(), 1024, None, 8, st))
    torch.cuda.synchronize()
    assert bool((y == 3).all()) and bool((o16.float() == 4).all())
    _ok(L.lib.vk_sum_slabs_bf16(o16.data_ptr(), s32.data_ptr(), 1024, 2, 1024, None, 8, st))
    torch.cuda.synchronize()
    assert bool((o16.float() == 2).all())


# ================================================================================================ byte offsets past 2^32
def test_large_arena_index_arithmetic():
    free, _ = torch.cuda.mem_get_info()
    if free < 16 << 30:
        pytest.skip("needs 16 GiB of free device memory, %.1f GiB free" % (free / 2 ** 30))
    L = _lib()
    t0 = time.time()
    total = (1 << 20) + 3                                    # 2^30 + 3 * 1024 fp32 elements
    exp, mask, _, _ = A.norm_plan(total, "none")
    exp[-3:] = torch.tensor([A.HEAVY, A.HEAVY + 1, A.HEAVY + 2])
    mask = torch.zeros(total, dtype=torch.uint8)
    mask[-2] = A.SKIP
    n = total * A.CHUNK
    g = torch.full((n + PAD,), NAN, dtype=torch.float32, device=DEV)
    want = torch.empty(total, dtype=torch.float64, device=DEV)
    for lo in range(0, total, 65536):
        hi = min(lo + 65536, total)
        g[lo * A.CHUNK:hi * A.CHUNK] = A.norm_grad(exp, DEV, lo, hi)
        want[lo:hi] = A.chunk_sums64(g[lo * A.CHUNK:hi * A.CHUNK])
    dst = _can16(n + PAD)
    _ok(L.lib.vk_cast_f32_bf16(g.data_ptr(), dst.data_ptr(), n, L.stream_ptr()))
    torch.cuda.synchronize()
    assert _is_can(dst[n:])
    for lo in range(0, total, 65536):
        hi = min(lo + 65536, total)
        assert _same(dst[lo * A.CHUNK:hi * A.CHUNK], g[lo * A.CHUNK:hi * A.CHUNK].bfloat16()), lo
    del dst
    maskd = torch.zeros(total + PAD, dtype=torch.uint8, device=DEV)
    maskd[:total] = mask.to(DEV)
    g[(total - 2) * A.CHUNK:(total - 1) * A.CHUNK] = NAN
    want[-2] = 0.0
    S = float(want.sum())
    pre = A.f32(1.0 / 1024)
    mx = A.max_norm_for("below", math.sqrt(S) * pre)
    partial, out = _can32(A.NORM_BLOCKS + PAD), _can32(8)
    _ok(L.lib.vk_grad_norm_clip_masked(g.data_ptr(), n, maskd.data_ptr(), pre, mx, partial.data_ptr(), out.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    assert _is_can(partial[A.NORM_BLOCKS:])
    _check_out(out, S, A.n_partial(n), pre, mx, "large one-call")
    sums = _can32(total + 1 + 2 * A.SQ_GROUPS + PAD)         # total is odd: one zero slot makes the count even
    sums[total] = 0
    _ok(L.lib.vk_grad_sqnorm_chunks(g.data_ptr(), 0, total, maskd.data_ptr(), sums.data_ptr(), L.stream_ptr()))
    out2 = _can32(8)
    _ok(L.lib.vk_grad_norm_from_chunks(sums.data_ptr(), total + 1, pre, mx, out2.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    assert A.ratio(sums[:total], want, (A.N_CHUNK + 1) * A.U * want) <= 1.0 and _is_can(sums[total + 1 + 2 * A.SQ_GROUPS:])
    _check_out(out2, S, A.N_CHUNK, pre, mx, "large chunks")
    print("large case: %.1f s" % (time.time() - t0))
