"""vk_task_loss_fwd / vk_task_loss_bwd (csrc/taskloss.hip) on synthetic logits against float64 and against torch's own fp32 criteria.

Inputs: fp32 logits of scale 4 with +-30, +-88 and the -10000 mask value planted in them, in a buffer whose pad columns are NaN (a kernel
that read them would return NaN); targets as the datasets produce them (a few soft scores of {0.3, 0.6, 0.9, 1} per row, one-hot rows,
all-zero rows; option indices).  Every group's maximum is asserted unique on the host: with ties torch's arg-max is unspecified.

Bounds.  Loss: |kernel - float64| <= max(4 x |torch fp32 criterion - float64|, 16 fp32 ulp of the loss) -- both are fp32 evaluations of
the same terms summed in another order.  Arg-max and the per-group score: exact against torch.  The score sum of the soft scores is an
fp32 sum whose bits depend on the order of the additions, torch's included; the kernel accumulates in double and rounds once, so it must
equal the float64 sum rounded to fp32 and be no further from it than torch's fp32 sum is; counts (regions, options) are exact.
dlogits: every element within one bf16 ulp of the float64 gradient rounded to bf16, every pad column exactly zero; the share of elements
that are not the exactly rounded value is printed.  Two runs give the same bits.

Measured on an MI355X over the 140 cases below: worst loss error 1.14 fp32 ulp (torch's own 1.54); at most 0.021 % of a case's dlogits
elements not the exactly rounded value, none further than one bf16 ulp."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = [1, 3, 64, 256, 1000]
WIDTHS = [1, 2, 3, 4, 37, 101, 1533, 3129]
CASES = [(k, r, c) for k in ("bce_scaled", "bce_mean") for r in ROWS for c in WIDTHS] + \
        [(k, r, c) for k in ("bce_regions", "ce_options") for r in ROWS for c in WIDTHS if c <= 101]
KIND = {"bce_scaled": 0, "bce_mean": 1, "bce_regions": 2, "ce_options": 3}
SOFT = [0.3, 0.6, 0.9, 1.0]
GSCALE = 0.37


def make_inputs(kind, groups, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(groups, n, generator=g) * 4
    for i, val in enumerate([30.0, -30.0, 88.0, -88.0, -10000.0]):
        x[(i * 7 + 1) % groups, (i * 3) % n] = val
    mask = None
    if kind == "bce_regions":
        mask = (torch.rand(groups, n, generator=g) > 0.25).long()
        mask[:, 0] = 1
    xe = x if mask is None else x + (1.0 - mask.float()) * -10000.0          # what the loss sees (fp32, as the model computes it)
    top = xe.max(dim=1, keepdim=True)[0]
    assert bool(((xe == top).sum(dim=1) == 1).all()), "every group's maximum must be unique"
    am = xe.argmax(dim=1)
    if kind == "ce_options":
        target = torch.randint(0, n, (groups,), generator=g)
        hit = torch.rand(groups, generator=g) < 0.5
        target[hit] = am[hit]
    else:
        target = torch.zeros(groups, n)
        for r in range(groups):
            if r % 3 == 0:                        # several soft scores
                for c in torch.randperm(n, generator=g)[:3].tolist():
                    target[r, c] = SOFT[int(torch.randint(0, 4, (1,), generator=g))]
            elif r % 3 == 1:                      # one-hot
                target[r, int(torch.randint(0, n, (1,), generator=g))] = 1.0
            if r % 2 == 0 and r % 3 != 2:         # the predicted label carries a score
                target[r, int(am[r])] = SOFT[r % 4]
    return x, xe, mask, target


def reference64(kind, xe, target):
    """(loss, d loss / d x) in float64 from the fp32 logits the loss sees"""
    x = xe.double()
    groups, n = x.shape
    if kind == "ce_options":
        lse = torch.logsumexp(x, dim=1)
        loss = (lse - x.gather(1, target.view(-1, 1)).squeeze(1)).sum() / groups
        p, hot = torch.exp(x - lse.unsqueeze(1)), torch.nn.functional.one_hot(target, n).bool()
        others = p.masked_fill(hot, 0.0).sum(dim=1, keepdim=True)       # softmax - 1 at the target, without the cancellation of 1 - 1
        return loss, torch.where(hot, -others, p) / groups
    t = target.double()
    div = groups * n if kind == "bce_mean" else groups
    loss = (x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))).sum() / div
    e = torch.exp(-x.abs())                                             # sigmoid(x) - t, again without 1 - 1 (x = 88 with t = 1)
    return loss, torch.where(x >= 0, (1 - t) - t * e, e * (1 - t) - t) / (1 + e) / div


def torch32(kind, xe, target):
    """(loss, score sum, arg-max, per-group score) as the reference's torch code computes them in fp32 on the GPU"""
    x, t = xe.cuda(), target.cuda()
    am = torch.max(x, 1)[1]
    if kind == "ce_options":
        per = (am == t).float()
        return torch.nn.CrossEntropyLoss()(x, t), per.sum(), am, per
    loss = torch.nn.BCEWithLogitsLoss(reduction="mean")(x, t)
    if kind == "bce_regions":
        per = (t.gather(1, am.view(-1, 1)).squeeze(1) > 0.5).float()
        return loss.mean() * x.size(1), per.sum(), am, per
    one_hots = torch.zeros_like(t)
    one_hots.scatter_(1, am.view(-1, 1), 1)
    scores = one_hots * t
    return (loss.mean() * x.size(1) if kind == "bce_scaled" else loss.mean()), scores.sum(), am, scores.sum(1)


def run_kernels(kind, x, mask, target):
    from volta_amd import _lib as L
    groups, n = x.shape
    dev = "cuda"
    if kind in ("bce_scaled", "bce_mean"):
        ld = -(-n // 64) * 64
        buf = torch.full((groups, ld), float("nan"))
        buf[:, :n] = x
    else:
        ld = 64
        buf = torch.full((groups * n, ld), float("nan"))
        buf[:, 0] = x.reshape(-1)
    buf, tg = buf.to(dev), target.contiguous().to(dev)
    mk = None if mask is None else mask.contiguous().to(dev)
    work = torch.zeros(L.lib.vk_task_loss_work_bytes(groups), dtype=torch.uint8, device=dev)
    out = torch.full((2,), float("nan"), device=dev)
    amax = torch.full((groups,), -7, dtype=torch.int32, device=dev)
    dlog = torch.full(buf.shape, float("nan"), dtype=torch.bfloat16, device=dev)
    gs = torch.tensor([GSCALE], device=dev)
    args = L.TaskLossArgs(L.ptr(buf), L.ptr(tg), L.ptr(mk), L.ptr(work), L.ptr(out), L.ptr(amax), KIND[kind], groups, n, ld)
    L.check(L.lib.vk_task_loss_fwd(C.byref(args), L.stream_ptr()))
    L.check(L.lib.vk_task_loss_bwd(C.byref(args), L.ptr(gs), L.ptr(dlog), L.stream_ptr()))
    torch.cuda.synchronize()
    per = work[groups * 8: groups * 12].clone().view(torch.float32)
    return out.cpu(), amax.cpu(), per.cpu(), dlog.cpu()


def ordered(bits16):
    """bf16 bit patterns -> integers in value order (+0 and -0 coincide)"""
    b = bits16.view(torch.int16).to(torch.int32) & 0xFFFF
    return torch.where(b >= 0x8000, -(b & 0x7FFF), b)


@pytest.mark.parametrize("kind,groups,n", CASES)
def test_task_loss_kernels(kind, groups, n):
    x, xe, mask, target = make_inputs(kind, groups, n, seed=groups * 10007 + n)
    out, amax, per, dlog = run_kernels(kind, x, mask, target)
    out2, amax2, per2, dlog2 = run_kernels(kind, x, mask, target)
    want_loss, want_grad = reference64(kind, xe, target)
    t_loss, t_score, t_amax, t_per = torch32(kind, xe, target)
    # loss
    want = float(want_loss)
    err_k, err_t = abs(float(out[0].double()) - want), abs(float(t_loss.double()) - want)
    ulp = float(np.spacing(np.float32(abs(want))))
    print("%s %dx%d loss %.9g: kernel error %.3g (%.2f ulp), torch fp32 error %.3g (%.2f ulp)" % (kind, groups, n, want, err_k, err_k / ulp, err_t, err_t / ulp))
    assert np.isfinite(float(out[0])) and err_k <= max(4 * err_t, 16 * ulp), (kind, groups, n, float(out[0]), want, err_k, err_t, ulp)
    # arg-max and score
    assert torch.equal(amax.long(), t_amax.cpu()), (kind, groups, n)
    assert torch.equal(per, t_per.cpu()), (kind, groups, n)
    s64 = float(t_per.double().sum())
    assert float(out[1]) == float(np.float32(s64)), (kind, groups, n, float(out[1]), s64)
    assert abs(float(out[1]) - s64) <= abs(float(t_score) - s64), (kind, groups, n, float(out[1]), float(t_score), s64)
    if kind in ("bce_regions", "ce_options"):
        assert float(out[1]) == float(t_score), (kind, groups, n)
    # gradient
    gs64 = float(np.float32(GSCALE))
    want_bf = (want_grad * gs64).to(torch.bfloat16)
    if kind in ("bce_scaled", "bce_mean"):
        got, pad = dlog[:, :n], dlog[:, n:]
    else:
        got, pad = dlog[:, 0].reshape(groups, n), dlog[:, 1:]
    assert bool((pad.view(torch.int16) == 0).all()), "pad columns of dlogits must be exactly zero"
    assert not bool(torch.isnan(got.float()).any())
    steps = (ordered(got.contiguous()) - ordered(want_bf.contiguous())).abs()
    inexact = float((steps != 0).float().mean())
    print("%s %dx%d dlogits: %.4f%% of the elements are not the exactly rounded value, worst %d bf16 ulp" % (kind, groups, n, 100 * inexact, int(steps.max())))
    assert int(steps.max()) <= 1, (kind, groups, n, int(steps.max()))
    # the same bits on a second run
    assert out.view(torch.int32).tolist() == out2.view(torch.int32).tolist() and torch.equal(amax, amax2)
    assert torch.equal(dlog.view(torch.int16), dlog2.view(torch.int16)) and torch.equal(per.view(torch.int32), per2.view(torch.int32))


def test_masked_regions_give_the_values_torch_gives():
    """x = -10000 (a padded region): loss 10000 t and gradient -t, no NaN / inf"""
    groups, n = 2, 4
    x = torch.tensor([[1.0, -2.0, 0.5, 3.0], [0.25, 2.0, -1.0, 0.0]])
    mask = torch.tensor([[1, 0, 1, 0], [1, 1, 1, 0]])
    target = torch.tensor([[0.9, 0.6, 1.0, 0.0], [0.0, 0.0, 0.0, 0.3]])
    out, amax, per, dlog = run_kernels("bce_regions", x, mask, target)
    xe = x + (1.0 - mask.float()) * -10000.0
    t_loss = torch.nn.BCEWithLogitsLoss()(xe, target) * n
    assert torch.isfinite(out).all() and abs(float(out[0]) - float(t_loss)) <= 4 * float(np.spacing(np.float32(float(t_loss))))
    g = dlog[:, 0].reshape(groups, n).float() * groups / float(np.float32(GSCALE))
    for (r, c) in ((0, 1), (0, 3), (1, 3)):
        assert abs(float(g[r, c]) + float(target[r, c])) <= 2 ** -8 * float(target[r, c]), (r, c, float(g[r, c]))
    assert amax.tolist() == [0, 1] and float(out[1]) == 1.0
