"""Fused RAdam against fused AdamW on the ctrl_vilbert_base arena (242 M fp32 elements), in one run, plus a per-tensor torch RAdam over the
same parameters (the reference's shape of update: ~10 ATen launches per parameter) for context.  Both fused kernels move the same 30 bytes
per element (p, g, m, v read; p, m, v written; bf16 copy written).  Kernel times are the launch alone (hipEvents around one call, median of
REPS after WARMUP); `step()` times include the host side (classes, chunk map, clip hand-off).
usage: python tools/bench_radam.py [--reps 20]"""
import argparse
import ctypes as C
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from volta_amd import _lib as L  # noqa: E402
from volta_amd.config import BertConfig  # noqa: E402
from volta_amd.modeling import BertForVLPreTraining  # noqa: E402
from volta_amd.optimization import AdamW, RAdam  # noqa: E402

NO_DECAY = ["bias", "LayerNorm.bias", "LayerNorm.weight"]


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e-3)
    return statistics.median(out), min(out), max(out)


def torch_radam_step(params, grads, state, lr, betas=(0.9, 0.999), eps=1e-8, wd=0.01):
    """A per-tensor RAdam step as a Python optimizer loop issues it (moments, step size, decay, update: one ATen call each)."""
    b1, b2 = betas
    for p, g in zip(params, grads):
        st = state.setdefault(id(p), [0, torch.zeros_like(p), torch.zeros_like(p)])
        st[0] += 1
        t, m, v = st
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        m.mul_(b1).add_(g, alpha=1 - b1)
        b2t = b2 ** t
        nmax = 2 / (1 - b2) - 1
        n = nmax - 2 * t * b2t / (1 - b2t)
        p.add_(p, alpha=-wd * lr)
        if n >= 5:
            ss = lr * math.sqrt((1 - b2t) * (n - 4) / (nmax - 4) * (n - 2) / n * nmax / (nmax - 2)) / (1 - b1 ** t)
            p.addcdiv_(m, v.sqrt().add_(eps), value=-ss)
        else:
            p.add_(m, alpha=-lr / (1 - b1 ** t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    model = BertForVLPreTraining(BertConfig.from_json_file(os.path.join(root, "config", "ctrl_vilbert_base.json"))).cuda()
    arena = model.materialize()
    named = list(model.named_parameters())
    arena.grad.normal_().mul_(0.01)
    for n, p in named:
        p.grad = arena.view(n, "grad")
    groups = [{"params": [p], "lr": 2e-5, "weight_decay": 0.0 if any(k in n for k in NO_DECAY) else 0.01} for n, p in named]
    radam = RAdam(groups, lr=2e-5)
    adamw = AdamW([dict(g) for g in groups], lr=2e-5, eps=1e-6)
    for _ in range(7):                      # past rectification (step 6): the rectified update is the steady state
        radam.step()
    adamw.step()
    n = arena.total
    bytes_ = n * 30
    print("arena: %d elements (%.1f M), %d parameters; %.2f GB per update" % (n, n / 1e6, len(named), bytes_ / 1e9))

    # the kernels alone, with the arguments the optimizers built for their last step
    ra = L.RadamArgs()
    ra.p, ra.g, ra.m, ra.v = arena.master.data_ptr(), arena.grad.data_ptr(), radam._fused["m"].data_ptr(), radam._fused["v"].data_ptr()
    ra.shadow, ra.n = arena.shadow.data_ptr(), n
    cmap = next(iter(radam._fused["masks"].values()))
    ra.chunk_class = cmap.data_ptr()
    for c in range(2):
        ra.cls_decay[c], ra.cls_step[c], ra.cls_rect[c] = (0.01 * 2e-5 if c == 0 else 0.0), 2e-5, 1
    ra.beta1, ra.beta2, ra.one_minus_beta1, ra.one_minus_beta2, ra.eps, ra.grad_scale = 0.9, 0.999, 1 - 0.9, 1 - 0.999, 1e-8, 1.0
    aa = L.AdamwArgs()
    aa.p, aa.g, aa.m, aa.v = arena.master.data_ptr(), arena.grad.data_ptr(), adamw._fused["m"].data_ptr(), adamw._fused["v"].data_ptr()
    aa.shadow, aa.chunk_class, aa.n = arena.shadow.data_ptr(), adamw._fused["chunk_class"].data_ptr(), n
    for c in range(2):
        aa.cls_lr_mult[c], aa.cls_wd[c] = 2e-5, (0.01 if c == 0 else 0.0)
    aa.lr, aa.beta1, aa.beta2, aa.eps, aa.step_mult, aa.grad_scale = 1.0, 0.9, 0.999, 1e-6, 0.5, 1.0
    rows = []
    for name, fn in (("vk_radam_step", lambda: L.check(L.lib.vk_radam_step(C.byref(ra), L.stream_ptr()))),
                     ("vk_adamw_step", lambda: L.check(L.lib.vk_adamw_step(C.byref(aa), L.stream_ptr()))),
                     ("vk_radam_step (again)", lambda: L.check(L.lib.vk_radam_step(C.byref(ra), L.stream_ptr()))),
                     ("RAdam.step()", radam.step),
                     ("AdamW.step()", adamw.step)):
        med, lo, hi = timed(fn, args.warmup, args.reps)
        rows.append((name, med))
        print("%-24s median %8.3f ms  (min %.3f, max %.3f)  %.2f TB/s" % (name, med * 1e3, lo * 1e3, hi * 1e3, bytes_ / med / 1e12))
    params = [p.detach() for _, p in named]
    grads = [arena.view(n_, "grad") for n_, _ in named]
    state = {}
    med, lo, hi = timed(lambda: torch_radam_step(params, grads, state, 2e-5), 2, max(3, args.reps // 4))
    print("%-24s median %8.3f ms  (min %.3f, max %.3f)  %.2f TB/s at the fused kernels' byte count" % ("per-tensor torch RAdam", med * 1e3, lo * 1e3, hi * 1e3, bytes_ / med / 1e12))


if __name__ == "__main__":
    main()
