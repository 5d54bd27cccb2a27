"""Fused LAMB against fused AdamW on the benchmark model's arena (ctrl_vilbert_base, 242 M fp32 elements), in one process, unprofiled,
after warm-up.  AdamW is the yardstick: its single launch moves 30 bytes per element (p, g, m, v read; p, m, v written; bf16 copy written).
LAMB's two-stage form moves 46:
  gradient sums   4   g read                                              (only when a group clips)
  stage 1        24   g, p, m, v read; m, v written
  stage 2        18   p, m, v read; p and the bf16 copy written
and three small launches (group sums, clip divisors, per-tensor finish) that read a few floats per 1024 elements.  `step()` times are
hipEvents around the whole call, host side included (median of --reps after --warmup); the per-launch times come from
vk_lamb_step_timed (hipEvents between the launches of one call).  A tool, not a gate.
usage: python tools/bench_lamb.py [--reps 20] [--warmup 5] [--config ctrl_vilbert_base]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from volta_amd import _lib as L  # noqa: E402
from volta_amd.config import BertConfig  # noqa: E402
from volta_amd.modeling import BertForVLPreTraining  # noqa: E402
from volta_amd.optimization import LAMB, AdamW  # noqa: E402

NO_DECAY = ["bias", "LayerNorm.bias", "LayerNorm.weight"]
LAUNCHES = (("gradient sums", 4), ("group sums", 0), ("clip divisors", 0), ("stage 1", 24), ("finish", 0), ("stage 2", 18))
ADAMW_BYTES = 30


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


def lamb_args(opt):
    """The vk_lamb_args of the optimizer's last step, rebuilt from its cached tables (what step() passes)."""
    t = opt._fused["last"]
    T, P, G = t["host"]
    a = L.LambArgs()
    a.tensors, a.pieces, a.groups = T.ctypes.data, P.ctypes.data, G.ctypes.data
    a.d_tensors, a.d_pieces, a.d_groups = (x.data_ptr() for x in t["dev"])
    a.work, a.work_bytes, a.table = t["work"].data_ptr(), t["nbytes"], t["table"].data_ptr()
    a.ntensors, a.npieces, a.ngroups = len(T), len(P), len(G)
    a.flags = L.LAMB_ADAM_W_MODE | L.LAMB_GRAD_AVERAGING
    for c in range(L.LAMB_CLASSES):
        a.cls_lr[c], a.cls_wd[c], a.cls_bc1[c], a.cls_bc2[c] = 2e-5, (0.01 if c == 0 else 0.0), 0.5, 0.01
    a.beta1, a.beta2, a.eps, a.grad_scale = 0.9, 0.999, 1e-6, 1.0
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="ctrl_vilbert_base")
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    model = BertForVLPreTraining(BertConfig.from_json_file(os.path.join(root, "config", args.config + ".json"))).cuda()
    arena = model.materialize()
    named = list(model.named_parameters())
    arena.grad.normal_().mul_(0.01)
    for n, p in named:
        p.grad = arena.view(n, "grad")
    dec = [p for n, p in named if not any(k in n for k in NO_DECAY)]
    nod = [p for n, p in named if any(k in n for k in NO_DECAY)]
    groups = [{"params": dec, "weight_decay": 0.01}, {"params": nod, "weight_decay": 0.0}]
    lamb = LAMB([dict(g) for g in groups], lr=2e-5, max_grad_norm=1.0)
    adamw = AdamW([dict(g) for g in groups], lr=2e-5, eps=1e-6)
    lamb.step()
    adamw.step()
    live = sum(p.numel() for _, p in named)
    t = lamb._fused["last"]
    print("%s arena: %d elements (%.1f M, %d in parameters), %d tensors, %d pieces, %d groups" %
          (args.config, arena.total, arena.total / 1e6, live, len(t["host"][0]), len(t["host"][1]), len(t["host"][2])))
    lamb_bytes = sum(b for _, b in LAUNCHES)
    print("bytes per element: AdamW %d, LAMB %d (ratio %.3f)" % (ADAMW_BYTES, lamb_bytes, lamb_bytes / ADAMW_BYTES))

    med_a, lo, hi = timed(adamw.step, args.warmup, args.reps)
    bw_a = arena.total * ADAMW_BYTES / med_a / 1e12
    print("%-22s median %8.3f ms  (min %.3f, max %.3f)  %5.2f TB/s over the arena" % ("AdamW.step()", med_a * 1e3, lo * 1e3, hi * 1e3, bw_a))
    med_l, lo, hi = timed(lamb.step, args.warmup, args.reps)
    print("%-22s median %8.3f ms  (min %.3f, max %.3f)  %5.2f TB/s over the parameters" %
          ("LAMB.step()", med_l * 1e3, lo * 1e3, hi * 1e3, live * lamb_bytes / med_l / 1e12))
    print("LAMB / AdamW step time %.3f; by the byte ratio alone %.3f" % (med_l / med_a, lamb_bytes * live / (ADAMW_BYTES * arena.total)))
    for name, fn in (("AdamW.step()", adamw.step), ("LAMB.step()", lamb.step)):       # the host side alone: how long the call keeps the CPU
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        host = (time.perf_counter() - t0) / args.reps
        torch.cuda.synchronize()
        print("%-22s host %8.3f ms per call" % (name, host * 1e3))

    # AdamW's launch alone, with the arguments its last step used: the yardstick for the LAMB launches below
    aa = L.AdamwArgs()
    aa.p, aa.g, aa.m, aa.v = arena.master.data_ptr(), arena.grad.data_ptr(), adamw._fused["m"].data_ptr(), adamw._fused["v"].data_ptr()
    aa.shadow, aa.chunk_class, aa.n = arena.shadow.data_ptr(), adamw._fused["chunk_class"].data_ptr(), arena.total
    for c in range(2):
        aa.cls_lr_mult[c], aa.cls_wd[c] = 2e-5, (0.01 if c == 0 else 0.0)
    aa.lr, aa.beta1, aa.beta2, aa.eps, aa.step_mult, aa.grad_scale = 1.0, 0.9, 0.999, 1e-6, 0.5, 1.0
    med_k, lo, hi = timed(lambda: L.check(L.lib.vk_adamw_step(C.byref(aa), L.stream_ptr())), args.warmup, args.reps)
    bw_a = arena.total * ADAMW_BYTES / med_k / 1e12
    print("  %-20s median %8.3f ms  %2d B/element  %5.2f TB/s" % ("vk_adamw_step", med_k * 1e3, ADAMW_BYTES, bw_a))
    a = lamb_args(lamb)
    ms = (C.c_float * 6)()
    rows = [[] for _ in LAUNCHES]
    for i in range(args.warmup + args.reps):
        L.check(L.lib.vk_lamb_step_timed(C.byref(a), L.stream_ptr(), ms))
        if i >= args.warmup:
            for k in range(6):
                rows[k].append(ms[k] * 1e-3)
    total = 0.0
    for (name, nbytes), r in zip(LAUNCHES, rows):
        med = statistics.median(r)
        total += med
        bw = "%5.2f TB/s (%.2f of AdamW's)" % (live * nbytes / med / 1e12, live * nbytes / med / 1e12 / bw_a) if nbytes else "   -"
        print("  %-20s median %8.3f ms  %2d B/element  %s" % (name, med * 1e3, nbytes, bw))
    print("  %-20s        %8.3f ms  (vk_adamw_step x byte ratio: %.3f ms)" % ("sum of the launches", total * 1e3, med_k * 1e3 * lamb_bytes * live / (ADAMW_BYTES * arena.total)))


if __name__ == "__main__":
    main()
