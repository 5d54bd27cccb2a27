"""csrc/heads.hip through the C ABI against plain float64 torch and the oracle: the labelled-row compaction, row gather / scatter-add,
the masked-LM / ITM cross entropy, kl_1601, the loss finalisation and the additive attention mask.

Gates (u = 2^-24, the fp32 unit roundoff; gamma_n = n u / (1 - n u) bounds any fp32 summation tree of depth n, Higham 4.2):
  * lse of a row.  The kernels take exp and log as __expf / __logf: exp2(y log2 e) and log2(s) ln 2, each ~1 ulp, and the rounding of
    y log2 e makes the relative error of exp(y) about u |y|.  Over a row this gives |d lse| <= u (2 Rg + 2 |lse| + D) with Rg the row's
    logit range (max - min: the largest |y| met, rescales of the running sum included), and D = 5 ceil(V / 1024) + 8 the depth of the
    sum of exponentials (per-thread running sums over V / 1024 float4 pieces with a rescale each, a wave and a block tree) plus the
    exp / log ulps.  The gate takes twice that: u (4 Rg + 4 |lse| + 2 D).
  * the loss sum.  Row losses are accumulated with fp32 atomics in arrival order: gamma_{n+1} (|seed| + sum|row loss|) plus the row
    errors above.
  * dlogits (bf16).  p = exp(x - lse) carries u (2 |x - lse| + 4) relative plus the row's lse error; the onehot subtraction and the g / n
    scale round once each: eps = |g / n| (p (u (2 |x - lse| + 4) + d lse) + 2 u |p - onehot|), then one bf16 ulp."""
import ctypes as C
import math

import pytest
import torch

from oracle import volta_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DEV = "cuda"


def _lib():
    from volta_amd import _lib as L
    return L


def _p(t):
    """Raw pointer of a device tensor.  Keep the tensor referenced until the launch: the pointer of a temporary (`_p(x.to(DEV))`)
    can be handed to the next allocation, and two arguments would then alias."""
    return None if t is None else C.c_void_p(t.data_ptr())


def _gamma(n):
    return n * U / (1 - n * U)


def _bf16_ulp(x):
    _, e = torch.frexp(x.abs())
    e = torch.where(x == 0, torch.full_like(e, -125), e.clamp_min(-125))
    return torch.ldexp(torch.ones_like(x), e - 8)


def _bf16_close(got, ref, eps):
    got, ref = got.double(), ref.double()
    return (got - ref).abs() <= _bf16_ulp(ref.abs() + eps) + eps


def _lse_gate(x64, lse64, V):
    D = 5 * math.ceil(V / 1024) + 8
    rg = x64.max(1).values - x64.min(1).values
    return U * (4 * rg + 4 * lse64.abs() + 2 * D)


# ------------------------------------------------------------------------------------------------ compaction
@pytest.mark.parametrize("N", [0, 1, 1023, 1024, 1025, 5120])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("fill", ["random", "none", "all"])
@pytest.mark.parametrize("inner,outer,off", [(20, 20, 0), (36, 37, 1)])
def test_select_rows(N, mode, fill, inner, outer, off):
    """Exact against torch.nonzero: pos = flagged indices in order, rows = (i / inner) * outer + i % inner + off (the vision grid maps
    region r of image b to row b (R + 1) + r + 1, past the global feature), count on the device; entries past the count untouched."""
    L = _lib()
    g = torch.Generator().manual_seed(N + mode)
    vals = torch.tensor([-1, 0, 1, 3])
    labels = vals[torch.randint(0, 4, (N,), generator=g)]
    if fill == "none":
        labels = torch.full((N,), -1 if mode == 0 else 0, dtype=torch.long)
    elif fill == "all":
        labels = torch.ones(N, dtype=torch.long)
    cap = max(N, 1) + 8
    rows, pos = torch.full((cap,), -7, dtype=torch.int32, device=DEV), torch.full((cap,), -7, dtype=torch.int32, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    lab = labels.to(DEV) if N else torch.zeros(1, dtype=torch.long, device=DEV)
    L.check(L.lib.vk_select_rows(_p(lab), N, mode, inner, outer, off, _p(rows), _p(pos), _p(count), L.stream_ptr()))
    torch.cuda.synchronize()
    flag = (labels == 1) if mode else (labels != -1)
    want_pos = torch.nonzero(flag).view(-1)
    n = want_pos.numel()
    assert int(count) == n
    assert n == {"none": 0, "all": N}.get(fill, n)
    assert torch.equal(pos.cpu()[:n].long(), want_pos)
    assert torch.equal(rows.cpu()[:n].long(), (want_pos // inner) * outer + want_pos % inner + off)
    assert bool((pos.cpu()[n:] == -7).all()) and bool((rows.cpu()[n:] == -7).all())


# ------------------------------------------------------------------------------------------------ gather / scatter-add
@pytest.mark.parametrize("H", [8, 264, 1024])
def test_gather_and_scatter_rows_add(H):
    """Rows past the device count (< max_rows) are not touched; the gather copies bits, the scatter-add is bf16(float(dst) + float(src))."""
    L = _lib()
    g = torch.Generator().manual_seed(H)
    Msrc, max_rows, n = 700, 300, 211
    rows = torch.randperm(Msrc, generator=g)[:max_rows].int()
    src = torch.randn(Msrc, H, generator=g).bfloat16()
    cnt = torch.tensor([n], dtype=torch.int32, device=DEV)
    rows_d = rows.to(DEV)
    dst = torch.full((max_rows, H), 7.0, dtype=torch.bfloat16, device=DEV)
    srcd = src.to(DEV)
    L.check(L.lib.vk_gather_rows(_p(srcd), _p(rows_d), _p(cnt), _p(dst), H, max_rows, L.stream_ptr()))
    add = torch.randn(max_rows, H, generator=g).bfloat16()
    base = torch.randn(Msrc, H, generator=g).bfloat16()
    acc = base.to(DEV)
    addd = add.to(DEV)
    L.check(L.lib.vk_scatter_rows_add(_p(addd), _p(rows_d), _p(cnt), _p(acc), H, max_rows, L.stream_ptr()))
    torch.cuda.synchronize()
    got = dst.cpu()
    assert torch.equal(got[:n].view(torch.int16), src[rows[:n].long()].view(torch.int16))
    assert bool((got[n:] == 7.0).all())
    want = base.clone()
    r = rows[:n].long()
    want[r] = (base[r].float() + add[:n].float()).bfloat16()
    assert torch.equal(acc.cpu().view(torch.int16), want.view(torch.int16))
    # sensitivity: one row more than the count (an off-by-one on the device count) is a different result
    more = want.clone()
    more[rows[n].long()] = (base[rows[n].long()].float() + add[n].float()).bfloat16()
    assert not torch.equal(acc.cpu().view(torch.int16), more.view(torch.int16))


# ------------------------------------------------------------------------------------------------ cross entropy
def _xent_logits(g, n, V, ld, scale):
    """n rows of logits (pad columns NaN: never read into a softmax), with rows shifted by +-80 (exp overflows without the max
    subtraction), one row with a single dominant logit at its label (loss ~ 0), and labels 0 and V - 1."""
    x = torch.randn(n, V, generator=g, dtype=torch.float64) * scale
    labels = torch.randint(0, V, (n,), generator=g)
    labels[:4] = torch.tensor([0, V - 1, V - 1, 0])
    x[2] += 80.0
    x[3] -= 80.0
    x[1, V - 1] = 60.0                                                          # dominant, at the last column (the scalar tail)
    x = x.float()
    full = torch.full((n, ld), float("nan"))
    full[:, :V] = x
    return full, x.double(), labels


def _xent_run(L, logits, labels, pos, count, max_rows, V, ld, ldd, seed_loss, gscale):
    dev = lambda t: None if t is None else t.to(DEV)
    lg, lb, ps, ct = dev(logits), dev(labels), dev(pos), dev(count)
    lse = torch.full((max_rows,), 7.0, device=DEV)
    loss = torch.tensor([seed_loss], device=DEV)
    dlog = torch.full((max_rows, ldd), 7.0, dtype=torch.bfloat16, device=DEV)
    gs = torch.tensor([gscale], device=DEV)
    a = L.XentArgs(_p(lg), _p(lb), _p(ps), _p(ct), _p(lse), _p(loss), V, ld, max_rows)
    L.check(L.lib.vk_xent_fwd(C.byref(a), L.stream_ptr()))
    L.check(L.lib.vk_xent_bwd(C.byref(a), _p(dlog), ldd, _p(gs), L.stream_ptr()))
    torch.cuda.synchronize()
    return lse, float(loss), dlog


def _xent_check(lse, loss, dlog, x64, lab, n, V, seed_loss, gscale):
    """Every gate of the module docstring on rows [0, n); returns (loss gate, reference loss sum, dlogits reference, eps)."""
    lse_ref = torch.logsumexp(x64, 1)
    gate = _lse_gate(x64, lse_ref, V)
    got_lse = lse[:n].double()
    assert bool(((got_lse - lse_ref).abs() <= gate).all()), float(((got_lse - lse_ref).abs() / gate).max())
    rl = lse_ref - x64[torch.arange(n, device=x64.device), lab]
    ref_loss = seed_loss + float(rl.sum())
    lgate = _gamma(n + 1) * (abs(seed_loss) + float(rl.abs().sum())) + float(gate.sum()) + U * float(rl.abs().sum())
    assert abs(loss - ref_loss) <= lgate, (loss, ref_loss, lgate)
    gn = gscale / n
    p = torch.exp(x64 - lse_ref[:, None])
    oh = torch.nn.functional.one_hot(lab, V).double()
    ref_d = (p - oh) * gn
    eps = abs(gn) * (p * (U * (2 * (x64 - lse_ref[:, None]).abs() + 4) + gate[:, None]) + 2 * U * (p - oh).abs())
    ok = _bf16_close(dlog[:n, :V], ref_d, eps)
    assert bool(ok.all()), int((~ok).sum())
    return lgate, rl, ref_d, eps


@pytest.mark.parametrize("ld", [30528, 30522])
def test_xent_mlm(ld):
    """Masked LM: V = 30522, ~768 labelled rows of max_rows 5120 through pos and the device count.  ld = 30522 makes every other row
    16-byte misaligned (the forward's scalar path; the backward's vector path needs ld >= the padded ldd)."""
    L = _lib()
    V, max_rows, N = 30522, 5120, 5120
    g = torch.Generator().manual_seed(ld)
    flagged = torch.randperm(N, generator=g)[:768].sort().values
    n = flagged.numel()
    full, x32, lab_rows = _xent_logits(g, n, V, ld, 3.0)
    labels = torch.full((N,), -1, dtype=torch.long)
    labels[flagged] = lab_rows
    pos = torch.zeros(max_rows, dtype=torch.int32)
    pos[:n] = flagged.int()
    logits = torch.full((max_rows, ld), float("nan"))
    logits[:n] = full
    ldd = ld
    seed_loss, gscale = 3.25, 0.7
    lse, loss, dlog = _xent_run(L, logits, labels, pos, torch.tensor([n], dtype=torch.int32), max_rows, V, ld, ldd, seed_loss, gscale)
    x64 = x32.to(DEV)
    lab = lab_rows.to(DEV)
    lgate, rl, ref_d, eps = _xent_check(lse, loss, dlog, x64, lab, n, V, seed_loss, gscale)
    assert bool((dlog[:n, V:] == 0).all()) and bool((dlog[n:] == 7.0).all()) and bool((lse[n:] == 7.0).all())
    assert float(rl[1]) < 1e-12                                                # the dominant row's loss is ~0
    # sensitivity: a label shifted by one misses the loss gate; a dlogits reference without 1 / count misses the dlogits gate
    shifted = seed_loss + float((torch.logsumexp(x64, 1) - x64[torch.arange(n, device=DEV), (lab + 1) % V]).sum())
    assert abs(loss - shifted) > lgate
    assert not bool(_bf16_close(dlog[:n, :V], ref_d * n, eps * n).all())


def test_xent_itm():
    """ITM: V = 2, ld = ldd = 64, count NULL (max_rows rows), labels indexed directly.  The row lse is held to a few u (|lse| + range):
    ~1e-6 relative, where the end-to-end test can only gate the bf16 step at 1e-2."""
    L = _lib()
    V, B, ld = 2, 256, 64
    g = torch.Generator().manual_seed(2)
    full, x32, lab = _xent_logits(g, B, V, ld, 2.0)
    seed_loss, gscale = -1.5, 1.0
    lse, loss, dlog = _xent_run(L, full, lab, None, None, B, V, ld, ld, seed_loss, gscale)
    x64 = x32.to(DEV)
    lgate, rl, ref_d, eps = _xent_check(lse, loss, dlog, x64, lab.to(DEV), B, V, seed_loss, gscale)
    lse_ref = torch.logsumexp(x64, 1)
    assert bool((dlog[:, V:] == 0).all())
    shifted = seed_loss + float((lse_ref - x64[torch.arange(B, device=DEV), (lab.to(DEV) + 1) % V]).sum())
    assert abs(loss - shifted) > lgate
    assert float(rl[1]) < 1e-12
    assert not bool(_bf16_close(dlog[:, :V], ref_d * B, eps * B).all())


# ------------------------------------------------------------------------------------------------ kl_1601
@pytest.mark.parametrize("weight", [1.0, 0.5])
def test_kl_1601(weight):
    """Against oracle.kl_1601 and float64 autograd: targets with exact zeros, a one-hot target and one that sums to 0.6.  The kernel
    accumulates weight x row KL (no mean): the oracle's value times max(n, 1)."""
    L = _lib()
    V, ld, B, Rn = 1601, 1664, 6, 36
    g = torch.Generator().manual_seed(int(weight * 10))
    label = torch.where(torch.rand(B, Rn, generator=g) < 0.3, 1, -1)
    label[0, :3] = 1
    pos = torch.nonzero(label.view(-1) == 1).view(-1)
    n, max_rows = pos.numel(), B * Rn
    tgt = torch.softmax(torch.randn(B * Rn, V, generator=g, dtype=torch.float64) * 2, 1)
    tgt[torch.rand(B * Rn, V, generator=g) < 0.5] = 0.0
    tgt = tgt / tgt.sum(1, keepdim=True)
    tgt[pos[0]] = 0.0
    tgt[pos[0], 7] = 1.0                                                       # one-hot
    tgt[pos[1]] *= 0.6                                                         # sums to < 1
    tgt = tgt.float()
    x = (torch.randn(n, V, generator=g) * 2).float()
    x[2] += 80.0
    logits = torch.full((max_rows, ld), float("nan"))
    logits[:n, :V] = x
    pos_d = torch.zeros(max_rows, dtype=torch.int32)
    pos_d[:n] = pos.int()
    seed_loss, gscale = 2.0, 0.7
    d = dict(logits=logits.to(DEV), tgt=tgt.to(DEV), pos=pos_d.to(DEV), cnt=torch.tensor([n], dtype=torch.int32, device=DEV),
             lse=torch.full((max_rows,), 7.0, device=DEV), tsum=torch.full((max_rows,), 7.0, device=DEV), loss=torch.tensor([seed_loss], device=DEV),
             dlog=torch.full((max_rows, ld), 7.0, dtype=torch.bfloat16, device=DEV), g=torch.tensor([gscale], device=DEV))
    a = L.KlArgs(_p(d["logits"]), _p(d["tgt"]), _p(d["pos"]), _p(d["cnt"]), _p(d["lse"]), _p(d["tsum"]), _p(d["loss"]), weight, V, ld, max_rows)
    L.check(L.lib.vk_kl_fwd(C.byref(a), L.stream_ptr()))
    L.check(L.lib.vk_kl_bwd(C.byref(a), _p(d["dlog"]), ld, _p(d["g"]), L.stream_ptr()))
    torch.cuda.synchronize()
    x64 = x.double().requires_grad_(True)
    t64 = tgt.double()[pos]
    pred = torch.zeros(B * Rn, V, dtype=torch.float64).index_add(0, pos, x64).view(B, Rn, V)
    want = R.kl_1601(pred, weight, label, tgt.double().view(B, Rn, V))
    (want * gscale).backward()
    lse_ref = torch.logsumexp(x64.detach(), 1)
    ts_ref = t64.sum(1)
    gate = _lse_gate(x64.detach(), lse_ref, V)
    assert bool(((d["lse"].cpu()[:n].double() - lse_ref).abs() <= gate).all())
    assert bool(((d["tsum"].cpu()[:n].double() - ts_ref).abs() <= _gamma(V) * ts_ref).all())
    # a row: sum_c t (log t - x) + lse sum_c t.  __logf, the subtraction and the product round a few times per term and the sum is a
    # tree of depth ~V / 256 + 8: 32 u A with A = sum_c t (|log t| + |x|) + |lse| sum_c t, plus sum_c t times the lse error
    safe = t64.clamp_min(1e-38)
    A = (t64 * (safe.log().abs() + x64.detach().abs())).sum(1) + lse_ref.abs() * ts_ref
    row_gate = weight * (32 * U * A + ts_ref * gate)
    rows = weight * torch.where(t64 > 0, t64 * (safe.log() - torch.log_softmax(x64.detach(), 1)), torch.zeros_like(t64)).sum(1)
    ref_loss = seed_loss + float(want.detach()) * max(n, 1)
    lgate = _gamma(n + 1) * (abs(seed_loss) + float(rows.abs().sum())) + float(row_gate.sum())
    got_loss = float(d["loss"])
    assert abs(got_loss - ref_loss) <= lgate, (got_loss, ref_loss, lgate)
    assert abs(float(rows.sum()) + seed_loss - ref_loss) <= 1e-9 * abs(ref_loss)     # the row form is the oracle's form
    # dlogits = (p ts - t) g, g = gscale weight / n: as for xent, with the kernel's tsum (gamma_V) folded into 24 u
    gn = gscale * weight / max(n, 1)
    p = torch.exp(x64.detach() - lse_ref[:, None])
    ref_d = x64.grad
    assert torch.allclose(ref_d, (p * ts_ref[:, None] - t64) * gn, rtol=1e-9, atol=1e-15)
    eps = abs(gn) * (p * ts_ref[:, None] * (U * (2 * (x64.detach() - lse_ref[:, None]).abs() + 24) + gate[:, None]) + 2 * U * (p * ts_ref[:, None] - t64).abs())
    dl = d["dlog"].cpu()
    assert bool(_bf16_close(dl[:n, :V], ref_d, eps).all())
    assert bool((dl[:n, V:] == 0).all()) and bool((dl[n:] == 7.0).all())
    # sensitivity: a loss without the weight, and a gradient without 1 / count
    if weight != 1.0:
        assert abs(got_loss - (seed_loss + float(rows.sum()) / weight)) > lgate
    assert not bool(_bf16_close(dl[:n, :V], ref_d * n, eps * n).all())


def test_kl_count_zero_writes_nothing():
    L = _lib()
    V, ld, max_rows = 1601, 1664, 8
    d = dict(logits=torch.randn(max_rows, ld, device=DEV), tgt=torch.rand(max_rows, V, device=DEV), pos=torch.zeros(max_rows, dtype=torch.int32, device=DEV),
             cnt=torch.zeros(1, dtype=torch.int32, device=DEV), lse=torch.full((max_rows,), 7.0, device=DEV), tsum=torch.full((max_rows,), 7.0, device=DEV),
             loss=torch.tensor([1.25], device=DEV), dlog=torch.full((max_rows, ld), 7.0, dtype=torch.bfloat16, device=DEV), g=torch.ones(1, device=DEV))
    a = L.KlArgs(_p(d["logits"]), _p(d["tgt"]), _p(d["pos"]), _p(d["cnt"]), _p(d["lse"]), _p(d["tsum"]), _p(d["loss"]), 1.0, V, ld, max_rows)
    L.check(L.lib.vk_kl_fwd(C.byref(a), L.stream_ptr()))
    L.check(L.lib.vk_kl_bwd(C.byref(a), _p(d["dlog"]), ld, _p(d["g"]), L.stream_ptr()))
    torch.cuda.synchronize()
    assert float(d["loss"]) == 1.25
    assert bool((d["lse"] == 7.0).all()) and bool((d["tsum"] == 7.0).all()) and bool((d["dlog"] == 7.0).all())


# ------------------------------------------------------------------------------------------------ finalize, mask prep
@pytest.mark.parametrize("n_t,n_v", [(0, 0), (5, 1), (7, 13)])
def test_loss_finalize(n_t, n_v):
    """losses = [sum_t / n_t (NaN at n_t = 0 with an empty sum, the reference's mean over nothing), w sum_v / max(n_v, 1), sum_itm / B].
    Held to one fp32 ulp (the division)."""
    L = _lib()
    B, w = 37, 0.75
    sums = torch.tensor([0.0 if n_t == 0 else 41.3, 17.9, 25.6])
    out = torch.full((3,), 7.0, device=DEV)
    sums_d, nt_d, nv_d = sums.to(DEV), torch.tensor([n_t], dtype=torch.int32, device=DEV), torch.tensor([n_v], dtype=torch.int32, device=DEV)
    L.check(L.lib.vk_loss_finalize(_p(sums_d), _p(nt_d), _p(nv_d), B, w, _p(out), L.stream_ptr()))
    torch.cuda.synchronize()
    got = out.cpu()
    want = torch.stack([sums[0] / n_t if n_t else torch.tensor(float("nan")), torch.tensor(w) * sums[1] / max(n_v, 1), sums[2] / B])
    if n_t == 0:
        assert math.isnan(float(got[0]))
    else:
        assert abs(float(got[0]) - float(want[0])) <= 2.0 ** -23 * abs(float(want[0]))
    assert torch.allclose(got[1:], want[1:], rtol=2.0 ** -23, atol=0)
    assert not torch.allclose(got[1:2], torch.tensor([w]) * sums[1:2] / (max(n_v, 1) + 1), rtol=2.0 ** -23, atol=0)      # sensitivity: count off by one


def test_mask_prep_exact():
    L = _lib()
    n = 4 * 1000 + 3
    m = torch.randint(0, 2, (n,))
    out = torch.full((n + 5,), 7.0, device=DEV)
    md = m.to(DEV)
    L.check(L.lib.vk_mask_prep(_p(md), _p(out), n, L.stream_ptr()))
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(got[:n], (1.0 - m.float()) * -10000.0)
    assert bool((got[n:] == 7.0).all())
