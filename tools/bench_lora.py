"""Fine-tuning step with LoRA adapters against full fine-tuning and a frozen encoder, same process:

  python tools/bench_lora.py [--steps 20] [--out profiles/lora.md]

The VQA-shaped step of tools/bench_task_step.py (ctrl_vilbert_base, B = 256, T = 23, 36 + 1 regions, 3129 labels; forward, fused task loss,
backward, clip, AdamW over the trainable parameters) in six variants:
  full      every parameter trains
  head      the encoder frozen, only the task head trains
  lora8     LoRA r = 8 on query and value + the head
  lora16    LoRA r = 16 on query, key and value + the head
  lora8_all LoRA r = 8 on all six targets (query, key, value, attn_out, ffn_up, ffn_down), both streams + the head
  lora8_drop lora8 with LoRA dropout 0.1: the masked kernels (vk_lora_fwd_drop / vk_lora_bwd_drop)
The variants alternate step by step after a warm-up of all of them; every step is timed between device synchronisations and the report gives
the median of `steps` steps per variant, as tools/bench_backbone.py does.  A second pass runs both lists of each LoRA variant through
vk_run_ops_timed and reports the time per LoRA launch (the Q|K|V ops and the whole-projection ops of attn_out / ffn_up / ffn_down) against the bytes the launch moves at the 6.3 TB/s copy rate of VERDICT.md item 10.
Needs an MI355X; random weights and data (the step time does not depend on them)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

VARIANTS = ("full", "head", "lora8", "lora16", "lora8_all", "lora8_drop")
COPY_RATE = 6.3e12


def make(variant):
    import bench_task_step as BT
    from volta_amd import lora
    from volta_amd.optimization import AdamW
    cfg, task_cfg, batch, model, _, crit = BT.make("vqa")
    if variant == "lora8":
        lora.add_lora(model, r=8, alpha=16, targets=("query", "value"))
    elif variant == "lora16":
        lora.add_lora(model, r=16, alpha=32, targets=("query", "key", "value"))
    elif variant == "lora8_all":
        lora.add_lora(model, r=8, alpha=16, targets=lora.TARGETS)
    elif variant == "lora8_drop":
        lora.add_lora(model, r=8, alpha=16, targets=("query", "value"), dropout=0.1)
    if variant.startswith("lora"):
        lora.mark_only_lora_trainable(model, also=("clfs_dict.",))
    elif variant == "head":
        for n, p in model.named_parameters():
            p.requires_grad_(n.startswith("clfs_dict."))
    opt = AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-5)
    return cfg, task_cfg, batch, model, opt, crit


def lora_bytes(eng):
    """(forward, backward) bytes per step that the LoRA launches of a plan read and write: X, T, the qkv / dqkv columns (read and written
    where updated, dqkv read twice: for dT and for dB), dxn where live, the partial records and the gradients."""
    from volta_amd import _lib as L
    fwd = bwd = 0
    for k in eng.keep:
        if isinstance(k, C.Array) and k._type_ is L.LoraProblem:
            for p in k:
                fwd += 2 * (p.M * p.K + 2 * p.M * p.r + 2 * p.M * p.N + p.r * (p.K + p.N))
        if isinstance(k, C.Array) and k._type_ is L.LoraBwdProblem:
            for p in k:
                nblk = -(-p.M // L.LORA_ROW_BLOCK)
                bwd += 2 * (p.M * p.N + 2 * p.M * p.r + p.r * (p.K + p.N))
                if p.dA:
                    bwd += 2 * (p.M * p.N + p.M * p.K + 2 * p.M * p.r) + 4 * (2 * nblk + 1) * p.r * (p.K + p.N)
                if p.dX:
                    bwd += 2 * (2 * p.M * p.K + p.M * p.r)
    return fwd, bwd


def lora_proj_bytes(eng):
    """The same for the whole-projection launches (attn_out, ffn_up, ffn_down): with the GELU the forward also writes gelu' (M N), with R
    the input gradient also reads it (M K)."""
    from volta_amd import _lib as L
    fwd = bwd = 0
    for k in eng.keep:
        if isinstance(k, C.Array) and k._type_ is L.LoraProjProblem:
            for p in k:
                fwd += 2 * (p.M * p.K + 2 * p.M * p.r + (3 if p.act else 2) * p.M * p.N + p.r * (p.K + p.N))
        if isinstance(k, C.Array) and k._type_ is L.LoraProjBwdProblem:
            for p in k:
                nblk = -(-p.M // L.LORA_ROW_BLOCK)
                bwd += 2 * (p.M * p.N + 2 * p.M * p.r + p.r * (p.K + p.N))
                if p.dA:
                    bwd += 2 * (p.M * p.N + p.M * p.K + 2 * p.M * p.r) + 4 * (2 * nblk + 1) * p.r * (p.K + p.N)
                if p.dX:
                    bwd += 2 * ((3 if p.R else 2) * p.M * p.K + p.M * p.r)
    return fwd, bwd


def launch_times(state, steps, fns=None):
    """ms per LoRA launch (forward, backward) and the launches per list, from vk_run_ops_timed over `steps` steps.  fns: the (forward,
    backward) generic functions counted, the Q|K|V ops by default."""
    import bench_task_step as BT
    from volta_amd import _lib as L
    model = state[3]
    BT.run_steps(1, *state)
    eng = model._last[0]
    out = []
    fns = fns or (L.FN_LORA_FWD, L.FN_LORA_BWD)
    for plan, fn in ((eng.fwd, fns[0]), (eng.bwd, fns[1])):
        plan.timing = (C.c_float * max(1, len(plan.ops)))()
    BT.run_steps(steps, *state)
    torch.cuda.synchronize()
    for plan, fn in ((eng.fwd, fns[0]), (eng.bwd, fns[1])):
        idx = [i for i, o in enumerate(plan.ops) if o[0] == L.OP_GENERIC and o[4].fn == fn]
        out.append((sum(plan.timing[i] for i in idx) / steps / max(1, len(idx)), len(idx), sum(plan.timing) / steps))
        plan.timing = None
    return out, eng


def main():
    import bench_task_step as BT
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lora needs the GPU: a step time measured elsewhere says nothing")
    states = {v: make(v) for v in VARIANTS}
    for v in VARIANTS:
        BT.run_steps(5, *states[v])
    torch.cuda.synchronize()
    times = {v: [] for v in VARIANTS}
    for _ in range(args.steps):
        for v in VARIANTS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            BT.run_steps(1, *states[v])
            torch.cuda.synchronize()
            times[v].append((time.perf_counter() - t0) * 1e3)
    med = {v: statistics.median(t) for v, t in times.items()}
    lines = ["## Step time", "", "`tools/bench_lora.py --steps %d` on %s; ms per step (forward, fused task loss, backward, clip, AdamW over the trainable" % (args.steps, torch.cuda.get_device_name(0)),
             "parameters), VQA shape (ctrl_vilbert_base, B = 256, T = 23, 37 region rows); the %d variants alternate step by step." % len(VARIANTS), "",
             "| variant | median | min | max | trainable parameters | backward ops |", "|---|---|---|---|---|---|"]
    for v in VARIANTS:
        model = states[v][3]
        n_train = sum(p.numel() for p in model.parameters() if p.requires_grad)
        lines.append("| %s | %.3f | %.3f | %.3f | %d | %d |" % (v, med[v], min(times[v]), max(times[v]), n_train, len(model._last[0].bwd.ops)))
    lines += ["", "lora8 - full = %+.3f ms (%+.1f %%); lora8 - head = %+.3f ms; lora16 - lora8 = %+.3f ms" %
              (med["lora8"] - med["full"], 100 * (med["lora8"] - med["full"]) / med["full"], med["lora8"] - med["head"], med["lora16"] - med["lora8"]),
              "lora8_all - full = %+.3f ms (%+.1f %%); lora8_all - head = %+.3f ms; lora8_all - lora8 = %+.3f ms" %
              (med["lora8_all"] - med["full"], 100 * (med["lora8_all"] - med["full"]) / med["full"], med["lora8_all"] - med["head"], med["lora8_all"] - med["lora8"]),
              "lora8_drop - lora8 = %+.3f ms (%+.1f %%)" % (med["lora8_drop"] - med["lora8"], 100 * (med["lora8_drop"] - med["lora8"]) / med["lora8"]), "",
              "## LoRA launches", "", "Per-op times from vk_run_ops_timed (side-stream blocks inline), averaged over %d steps; bytes: what a launch reads and writes;" % args.steps,
              "floor: those bytes at the 6.3 TB/s streaming-copy rate of VERDICT.md item 10.", "",
              "| variant | list | LoRA ops | ms per op | MB per op | floor, ms | time / floor | LoRA share of the list |", "|---|---|---|---|---|---|---|---|"]
    from volta_amd import _lib as L
    for v, fns, count, tag in (("lora8", None, lora_bytes, ""), ("lora16", None, lora_bytes, ""), ("lora8_all", None, lora_bytes, " (Q|K|V ops)"),
                               ("lora8_all", (L.FN_LORA_PROJ_FWD, L.FN_LORA_PROJ_BWD), lora_proj_bytes, " (whole-projection ops)"),
                               ("lora8_drop", (L.FN_LORA_FWD_DROP, L.FN_LORA_BWD_DROP), lora_bytes, " (masked)")):
        res, eng = launch_times(states[v], args.steps, fns)
        nbytes = count(eng)
        for (ms, n, total), b, name in zip(res, nbytes, ("forward", "backward")):
            per = b / max(1, n)
            floor = per / COPY_RATE * 1e3
            lines.append("| %s | %s | %d | %.4f | %.1f | %.4f | %.1f | %.1f %% |" % (v, name + tag, n, ms, per / 1e6, floor, ms / floor if floor else 0.0, 100 * ms * n / total if total else 0.0))
    text = "\n".join(lines)
    print(text)
    head = open(args.out).read().split("## Step time")[0] if os.path.exists(args.out) else "# LoRA fine-tuning: measured\n\n"
    with open(args.out, "w") as f:
        f.write(head + text + "\n")


if __name__ == "__main__":
    main()
