"""Fine-tuning step of VQA (config_tasks/ctrl_trainval_tasks.yml TASK1: 3129 labels, 23 tokens, 36 + 1 regions) on ctrl_vilbert_base at full
depth, B = 256, in two forms, alternated step by step:

  (a) BertForVLTasks with the task's SimpleClassifier on the engine;
  (b) a standalone BertModel under an equivalent torch head (dropout -> Linear -> GELU -> LayerNorm -> Linear).

Each step: forward, BCE-with-logits loss, backward, clip_grad_norm_, AdamW.  Device-event timing of every step; prints the median and
spread of both and the overhead of (b) over (a) as one JSON line.

  python tools/bench_backbone.py [--warmup 5] [--steps 20]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch
from torch import nn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq-len", type=int, default=23)
    ap.add_argument("--regions", type=int, default=36)
    a = ap.parse_args()
    from volta_amd.config import BertConfig
    from volta_amd.data import synthetic_batch
    from volta_amd.modeling import BertForVLTasks, BertModel
    from volta_amd.optimization import AdamW, clip_grad_norm_

    cfg = BertConfig.from_json_file(os.path.join(ROOT, "config", "ctrl_vilbert_base.json"))
    C = 3129
    task_cfg = {"TASK1": {"type": "VL-classifier", "num_labels": C}}
    torch.manual_seed(1234)
    tasks = BertForVLTasks(cfg, task_cfg, ["TASK1"]).cuda().train()

    class Backbone(nn.Module):
        def __init__(self):
            super().__init__()
            self.bert = BertModel(cfg)
            self.head = nn.Sequential(nn.Dropout(0.1), nn.Linear(cfg.pooler_size, cfg.clf_hidden_size), nn.GELU(),
                                      nn.LayerNorm(cfg.clf_hidden_size, eps=1e-12), nn.Linear(cfg.clf_hidden_size, C))

        def forward(self, *batch):
            _, _, pt, pv, _ = self.bert(*batch)
            return self.head(pt * pv)

    backbone = Backbone().cuda().train()
    no_decay = ("bias", "LayerNorm.bias", "LayerNorm.weight")

    def groups(model):          # one group per parameter, the task head at its own lr (train_task.py:208-218)
        return [{"params": [p], "lr": 1e-4 if ("clfs_dict" in n or n.startswith("head.")) else 2e-5,
                 "weight_decay": 0.0 if any(nd in n for nd in no_decay) else 0.01} for n, p in model.named_parameters()]

    opt_a, opt_b = AdamW(groups(tasks), lr=2e-5), AdamW(groups(backbone), lr=2e-5)
    batch = synthetic_batch(cfg, a.batch, a.seq_len, a.regions, seed=1234)      # + the global image feature
    args = (batch["input_ids"], batch["image_feat"], batch["image_loc"], batch["segment_ids"], batch["input_mask"], batch["image_mask"])
    target = (torch.rand(a.batch, C, device="cuda") < 0.002).float()
    bce = nn.BCEWithLogitsLoss(reduction="mean")

    def step_a():
        pred = tasks(args[0], args[1], args[2], "TASK1", args[3], args[4], args[5])[0]
        (bce(pred, target) * C).backward()
        clip_grad_norm_(tasks.parameters(), 1.0)
        opt_a.step()
        opt_a.zero_grad()

    def step_b():
        (bce(backbone(*args), target) * C).backward()
        clip_grad_norm_(backbone.parameters(), 1.0)
        opt_b.step()
        opt_b.zero_grad()

    times = {"a": [], "b": []}
    for i in range(a.warmup + a.steps):
        for k, fn in (("a", step_a), ("b", step_b)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times[k].append(e0.elapsed_time(e1))
    out = {"workload": "vqa_finetune_ctrl_vilbert_base", "batch": a.batch, "seq_len": a.seq_len, "regions": a.regions + 1, "steps": a.steps}
    for k, name in (("a", "tasks_engine_head"), ("b", "backbone_torch_head")):
        t = sorted(times[k])
        out[name] = {"median_ms": round(statistics.median(t), 3), "min_ms": round(t[0], 3), "max_ms": round(t[-1], 3),
                     "stdev_ms": round(statistics.pstdev(t), 3)}
    out["overhead_b_over_a"] = round(out["backbone_torch_head"]["median_ms"] / out["tasks_engine_head"]["median_ms"] - 1.0, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
