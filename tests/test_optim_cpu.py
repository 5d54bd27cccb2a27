"""The gates of tests/optim_restate.py are worth something: fp32 torch emulations of each contract, written here independently of the
restatement, stay inside every gate on every table case (no element exempted); every deliberately wrong variant leaves its gate by at least
10x on a named case; the norm gates reject a dropped chunk and an included skipped chunk at the full-size chunk count; and the host-side index
arithmetic the kernels rely on covers every chunk exactly once.  Runs without a GPU."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_restate as A  # noqa: E402

F = torch.float32


def _t(x):
    return torch.tensor(x, dtype=F)


# ------------------------------------------------------------------------------------------------ fp32 emulations of the AdamW contract
def _emu_plain(p, m, v, g, ce, h):
    """One fp32 operation per line of the header's formula."""
    live = ce <= 7
    c = ce.long().clamp(0, 7)
    gs = _t(h.grad_scale) * (_t(h.clip) if h.clip is not None else _t(1.0))
    gr = g * gs
    m2 = _t(h.b1) * m + (_t(1.0) - _t(h.b1)) * gr
    v2 = _t(h.b2) * v + (_t(1.0) - _t(h.b2)) * gr * gr
    lrc = _t(h.lr) * torch.tensor(h.mult, dtype=F)[c]
    step = lrc * _t(h.step_mult)
    q = p - step * (m2 / (v2.sqrt() + _t(h.eps)))
    d = lrc * torch.tensor(h.wd, dtype=F)[c]
    q = torch.where(d > 0, q - d * q, q)
    return torch.where(live, q, p), torch.where(live, m2, m), torch.where(live, v2, v)


def _emu_addc(p, m, v, g, ce, h):
    """pytorch-transformers' own call sequence (mul_ / add_ / addcmul_ / addcdiv_ with Python-double scalars), class by class."""
    p, m, v = p.clone(), m.clone(), v.clone()
    gr = g * (h.grad_scale * (h.clip if h.clip is not None else 1.0))
    for c in range(8):
        idx = (ce == c).nonzero().flatten()
        if not len(idx):
            continue
        pc, mc, vc, gc = p[idx], m[idx], v[idx], gr[idx]
        mc.mul_(h.b1).add_(gc, alpha=1.0 - h.b1)
        vc.mul_(h.b2).addcmul_(gc, gc, value=1.0 - h.b2)
        denom = vc.sqrt().add_(h.eps)
        pc.addcdiv_(mc, denom, value=-(h.lr * h.mult[c] * h.step_mult))
        if h.wd[c] > 0:
            pc.add_(pc, alpha=-(h.lr * h.mult[c] * h.wd[c]))
        p[idx], m[idx], v[idx] = pc, mc, vc
    return p, m, v


@pytest.mark.parametrize("case", A.ADAM_CASES, ids=[c.id for c in A.ADAM_CASES])
def test_fp32_emulations_of_adamw_stay_inside_the_gates(case):
    inp = A.adam_inputs(case)
    ce = A.cls_elem(inp["cls"], case.nch)
    ref = A.AdamW64(inp["p"], inp["m"], inp["v"], ce, case.h)
    states = {"plain": (_emu_plain, [inp["p"], inp["m"], inp["v"]]), "addc": (_emu_addc, [inp["p"], inp["m"], inp["v"]])}
    for s in range(A.ADAM_STEPS):
        ref.step(inp["gs"][s])
        for name, (fn, st) in states.items():
            st[:] = fn(st[0], st[1], st[2], inp["gs"][s], ce, case.h)
            assert all(bool(torch.isfinite(x).all()) for x in st)
            ex = ref.excess(*st)
            assert ex <= 1.0, (case.id, name, s, ex)
    skipped = ce > 7
    assert torch.equal(ref.p[skipped], inp["p"].double()[skipped])


def test_every_wrong_adamw_variant_leaves_its_gate_by_10x():
    small = [c for c in A.ADAM_CASES if c.nch <= 400]
    report = {}
    for var in A.AdamW64.VARIANTS:
        best = (0.0, None)
        for case in small:
            inp = A.adam_inputs(case)
            ce = A.cls_elem(inp["cls"], case.nch)
            ref, bad = A.AdamW64(inp["p"], inp["m"], inp["v"], ce, case.h), A.AdamW64(inp["p"], inp["m"], inp["v"], ce, case.h, variant=var)
            ref.step(inp["gs"][0])
            bad.step(inp["gs"][0])
            ex = ref.excess(bad.p, bad.m, bad.v)
            if ex > best[0]:
                best = (ex, case.id)
        report[var] = best
        print("variant %-13s rejected by case %-28s at %.3g x its gate" % (var, best[1], best[0]))
    assert all(ex >= 10.0 for ex, _ in report.values()), report


# ------------------------------------------------------------------------------------------------ sums of squares, norm, clip
def _seq_rows(x):
    """fp32 row sums of [rows, k], strictly left to right."""
    s = torch.zeros(x.shape[0], dtype=F)
    for j in range(x.shape[1]):
        s += x[:, j]
    return s


def _pair_rows(x):
    """fp32 row sums of [rows, 2^k] by halving."""
    while x.shape[1] > 1:
        x = x[:, 0::2] + x[:, 1::2]
    return x[:, 0]


def _resolve(case):
    return A.full_chunks() if case.total == A.FULL else case.total


def _emu_chunk_sums(exp, mask, order):
    out = torch.empty(len(exp), dtype=F)
    for lo in range(0, len(exp), 8192):
        hi = min(lo + 8192, len(exp))
        g = A.norm_grad(exp, lo=lo, hi=hi).view(-1, A.CHUNK)
        out[lo:hi] = order(g * g)
    return out if mask is None else torch.where(mask == A.SKIP, torch.zeros_like(out), out)


def _emu_norm(S64, pre_scale, max_norm):
    norm = torch.tensor(math.sqrt(S64), dtype=F) * _t(pre_scale)
    coef = _t(1.0)
    if max_norm > 0:
        coef = torch.minimum(_t(max_norm) / (norm + _t(1e-6)), _t(1.0))
    return float(norm), float(coef)


@pytest.mark.parametrize("case", A.NORM_CASES, ids=[c.id for c in A.NORM_CASES])
def test_fp32_emulations_of_the_norms_stay_inside_the_gates_and_the_gates_reject_dropped_work(case):
    total = _resolve(case)
    exp, mask, heavy, hskip = A.norm_plan(total, case.mask)
    want = A.plan_sums64(exp, mask)
    if total <= 258:                                        # the closed form of the plan is the sum of the generated data
        assert torch.equal(want, A.chunk_sums64(A.norm_grad(exp), mask))
    S = float(want.sum())
    pre = A.f32(case.pre_scale)
    n = total * A.CHUNK
    mx = A.max_norm_for(case.max_mode, math.sqrt(S) * pre)
    for order in (_seq_rows, _pair_rows):
        sums = _emu_chunk_sums(exp, mask, order)
        assert A.ratio(sums, want, (A.N_CHUNK + 1) * A.U * want) <= 1.0
        # chunk form: the chunk sums in double; masked form: runs of chunks added on in fp32 up to n_partial(n) elements, then double
        per = A.n_partial(n) // A.CHUNK
        runs = torch.stack([_seq_rows(sums[i:i + per][None, :])[0] for i in range(0, total, per)])
        for S_emu, N in ((float(sums.double().sum()), A.N_CHUNK), (float(runs.double().sum()), A.n_partial(n))):
            norm, En, coef, Ec = A.norm_clip64(S, (N + 1) * A.U, pre, mx)
            got = _emu_norm(S_emu, pre, mx)
            assert A.ratio(got[0], norm, En) <= 1.0 and A.ratio(got[1], coef, Ec) <= 1.0, (case.id, order.__name__, N, got, norm, coef)
    if case.max_mode == "zero":
        assert A.norm_clip64(S, A.U, pre, mx)[2:] == (1.0, 0.0)
    # dropped / extra work, against the gate of each form (the one-call form's, with N = n_partial(n), is the widest)
    for N in (A.N_CHUNK, A.n_partial(n)):
        norm, En, coef, Ec = A.norm_clip64(S, (N + 1) * A.U, pre, mx)
        for c in heavy:
            r = A.ratio(math.sqrt(S - float(want[c])) * pre, norm, En)
            print("%s N=%d: dropping heavy chunk %d leaves the norm gate at %.3g x" % (case.id, N, c, r))
            assert r > 1.0, (case.id, "dropping chunk %d passes" % c, r)
        if hskip is not None:
            extra = float(A.BASESQ[hskip % 8] * 4.0 ** int(exp[hskip]))
            r = A.ratio(math.sqrt(S + extra) * pre, norm, En)
            print("%s N=%d: including skipped chunk %d leaves the norm gate at %.3g x" % (case.id, N, hskip, r))
            assert r > 1.0, (case.id, "including skipped chunk %d passes" % hskip, r)
    # the sub-ranges and shard plans of the table: inside the arena, chunk0 > 0, and every plan covers each chunk exactly once
    assert all(c0 > 0 and k in (1, 2, 3, 5) and c0 + k <= total for c0, k in A.chunk_ranges(total)) and (total < 8 or len(A.chunk_ranges(total)) >= 4)
    for plan in A.shard_plans(total):
        seen = torch.zeros(total, dtype=torch.int64)
        for c0, k in plan:
            assert k > 0
            seen[c0:c0 + k] += 1
        assert bool((seen == 1).all()) and len(plan) in (2, 3, 7)
    assert total < 7 or [len(p) for p in A.shard_plans(total)] == [2, 3, 7]


def test_list_sums_emulation_stays_inside_its_gate():
    gen = torch.Generator().manual_seed(3)
    for numel, _, _, _ in A.list_table():
        g = torch.randn(numel, generator=gen)
        want = float((g.double() ** 2).sum())
        pad = torch.cat([g, torch.zeros(-numel % 4)]).view(-1, 4)
        for order in (_seq_rows, _pair_rows):
            got = float(order(pad * pad).double().sum().float())
            assert A.ratio(got, want, A.E_LIST * want) <= 1.0
    assert A.ratio(0.9999 * want, want, A.E_LIST * want) > 10.0
    mx = max(A.LIST_NUMELS)
    assert A.list_max_numels(mx)[0] == mx and all(x > mx for x in A.list_max_numels(mx)[1:])


# ------------------------------------------------------------------------------------------------ slabs, tail, axpy, bit statements
def test_slab_tail_and_axpy_emulations_stay_inside_their_gates():
    gen = torch.Generator().manual_seed(4)
    for nslabs in A.SLAB_COUNTS:
        for n in A.SLAB_NS[:-1]:
            assert all(st % 4 == 0 and st >= n for st in A.slab_strides(n)) and max(A.slab_strides(n)) > n + 3
            src = torch.randn(nslabs, n, generator=gen)
            want, bound = A.slabs64(src)
            seq = A.slabs_seq32(src)
            assert A.ratio(seq, want, bound) <= 1.0 and A.ratio(src.sum(0), want, bound) <= 1.0
            assert torch.equal(seq, _seq_rows(src.t().contiguous()))
            if nslabs > 1:
                assert A.ratio(src[1:].double().sum(0), want, bound) > 10.0          # a dropped slab
            else:
                assert float(bound.max()) == 0.0 and torch.equal(seq, src[0])
    for kind, H, count, count2, acc in A.TAIL_JOBS:
        if kind != 1:
            continue
        rec = torch.randn(count, 2, H, generator=gen)
        rec2 = torch.randn(count2, 2, H, generator=gen) if count2 else None
        old = torch.randn(2, H, generator=gen) if acc else None
        want, bound = A.tail_cols64(rec, rec2, old)
        allrec = torch.cat([x for x in (rec, rec2, old[None] if acc else None) if x is not None])
        for got in (allrec.sum(0), _seq_rows(allrec.permute(1, 2, 0).reshape(2 * H, -1)).view(2, H)):
            assert A.ratio(got, want, bound) <= 1.0
        if acc:
            assert A.ratio(got - old, want, bound) > 10.0                            # accumulate ignored
    x, y = torch.randn(4096, generator=gen), torch.randn(4096, generator=gen)
    for alpha in (1.0, -0.37, 3.0):
        want, bound = A.axpy64(y, x, A.f32(alpha))
        assert A.ratio(y + _t(alpha) * x, want, bound) <= 1.0 and A.ratio(torch.add(y, x, alpha=A.f32(alpha)), want, bound) <= 1.0
        assert A.ratio(y + _t(alpha) * x * _t(1.0001), want, bound) > 10.0


def test_cast_specials_round_to_nearest_even_on_the_cpu():
    s = A.cast_specials()
    b = s.bfloat16().view(torch.int16).int() & 0xFFFF
    want = [0x0000, 0x8000, 0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x3F81, 0x3F80, 0x7F80, 0xFF80, 0x7F80, 0xFF80]
    assert b[:12].tolist() == want
    assert bool(torch.isnan(s.bfloat16()[12:15]).all())
    assert b[15:].tolist() == [0x0000, 0x0000, 0x0002, 0x0080, 0x8001, 0x0040]     # denormals: the same rule on the same bits
    a, c = torch.tensor([1.5, -3.0], dtype=torch.bfloat16), torch.tensor([1.0078125, 0.33203125], dtype=torch.bfloat16)
    assert torch.equal((a.float() * c.float()).double(), a.double() * c.double())    # the fp32 product of two bf16 values is exact


# ------------------------------------------------------------------------------------------------ host arithmetic
def test_every_chunk_of_the_narrow_walk_is_owned_exactly_once():
    for nch in sorted({c.nch for c in A.ADAM_CASES}):
        for ncus in A.NCUS:
            seen = A.narrow_owner(nch, ncus)
            assert seen == [1] * nch, (nch, ncus, [i for i, s in enumerate(seen) if s != 1][:8])


def test_the_first_level_groups_cover_every_chunk_sum_exactly_once():
    for total in sorted({_resolve(c) for c in A.NORM_CASES}):
        r = A.group_ranges(total)
        assert len(r) == A.SQ_GROUPS and r[0][0] == 0 and max(hi for _, hi in r) == total
        assert all(lo <= hi for lo, hi in r) and sum(hi - lo for lo, hi in r) == total
        assert all(a[1] == b[0] or b[0] == b[1] == total for a, b in zip(r, r[1:]))
