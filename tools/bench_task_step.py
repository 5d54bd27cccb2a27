"""Whole fine-tuning step (forward, loss, backward, clip, AdamW) with the fused task loss against the torch path, same process:

  python tools/bench_task_step.py [--steps 20] [--rounds 6] [--out profiles/task_loss_step.md]

Shapes: VQA (ctrl_vilbert_base, B = 256, T = 23, 36 + 1 regions, 3129 labels, VL-classifier) and retrieval (64 x 4 options, T = 30,
VL-logit).  The two paths alternate round by round (VOLTA_TASK_LOSS is read per call), each round times `steps` steps between device
synchronisations after a warm-up of both; the report gives every round, the medians and the spread.  Needs an MI355X; random weights and
data (the step time does not depend on them)."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(shape):
    from volta_amd import task_utils as TU
    from volta_amd.config import BertConfig
    from volta_amd.modeling import BertForVLTasks
    from volta_amd.optimization import AdamW
    cfg = BertConfig.from_json_file(os.path.join(ROOT, "config", "ctrl_vilbert_base.json"))
    g = torch.Generator().manual_seed(0)
    if shape == "vqa":
        B, T, Rv, task = 256, 23, 37, {"type": "VL-classifier", "num_labels": 3129, "process": "normal", "loss": "BCEWithLogitLoss"}
        target = torch.zeros(B, 3129)
        target[torch.arange(B), torch.randint(0, 3129, (B,), generator=g)] = 1.0
        lead = (B,)
    else:
        B, T, Rv, task = 64, 30, 37, {"type": "VL-logit", "process": "retrieval", "loss": "CrossEntropyLoss"}
        target = torch.randint(0, 4, (B,), generator=g)
        lead = (B, 4)
    batch = (torch.randn(*lead, Rv, cfg.v_feature_size, generator=g), torch.rand(*lead, Rv, cfg.num_locs, generator=g),
             torch.ones(*lead, Rv, dtype=torch.int64), torch.randint(1000, cfg.vocab_size, (*lead, T), generator=g), target,
             torch.ones(*lead, T, dtype=torch.int64), torch.zeros(*lead, T, dtype=torch.int64), torch.arange(B))
    batch = tuple(t.cuda() for t in batch)
    task_cfg = {"TASK1": task}
    model = BertForVLTasks(cfg, task_cfg, ["TASK1"]).cuda().train()
    model.set_dropout_seed(1)
    opt = AdamW(model.parameters(), lr=1e-5)
    return cfg, task_cfg, batch, model, opt, TU.LoadLoss(task_cfg, "1")


def run_steps(n, cfg, task_cfg, batch, model, opt, crit):
    from volta_amd import task_utils as TU
    from volta_amd.optimization import clip_grad_norm_
    dev = torch.device("cuda")
    for _ in range(n):
        loss, _ = TU.ForwardModelsTrain(cfg, task_cfg, dev, "TASK1", batch, model, crit)
        loss.backward()
        clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
        opt.zero_grad()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "task_loss_step.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_task_step needs the GPU: a step time measured elsewhere says nothing")
    lines = ["# Fine-tuning step: fused task loss against the torch path", "",
             "`tools/bench_task_step.py --steps %d --rounds %d` on %s; ms per step (forward, loss, backward, clip, AdamW), the two paths" % (args.steps, args.rounds, torch.cuda.get_device_name(0)),
             "alternating round by round in one process after a warm-up of both.", ""]
    for shape in ("vqa", "retrieval"):
        state = make(shape)
        times = {"fused": [], "torch": []}
        for mode in ("fused", "torch"):
            os.environ["VOLTA_TASK_LOSS"] = "" if mode == "fused" else "torch"
            run_steps(5, *state)
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for mode in ("fused", "torch"):
                os.environ["VOLTA_TASK_LOSS"] = "" if mode == "fused" else "torch"
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run_steps(args.steps, *state)
                torch.cuda.synchronize()
                times[mode].append((time.perf_counter() - t0) * 1e3 / args.steps)
        med = {m: statistics.median(v) for m, v in times.items()}
        lines += ["## %s" % shape, "", "| path | median | min | max | rounds |", "|---|---|---|---|---|"]
        for m in ("fused", "torch"):
            lines.append("| %s | %.3f | %.3f | %.3f | %s |" % (m, med[m], min(times[m]), max(times[m]), " ".join("%.3f" % t for t in times[m])))
        lines += ["", "fused - torch = %+.3f ms per step (%+.2f %%); spread of one path across rounds: %.3f ms" %
                  (med["fused"] - med["torch"], 100 * (med["fused"] - med["torch"]) / med["torch"], max(max(v) - min(v) for v in times.values())), ""]
        del state
        torch.cuda.empty_cache()
    os.environ.pop("VOLTA_TASK_LOSS", None)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
