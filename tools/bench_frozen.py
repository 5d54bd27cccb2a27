"""What freezing parameters buys on the VQA fine-tuning step of tools/bench_task_step.py (ctrl_vilbert_base, B = 256, T = 23, 36 + 1
regions, 3129 labels; forward, loss, backward, clip, AdamW):

  python tools/bench_frozen.py [--steps 20] [--rounds 3] [--warmup 5] [--tree PATH] [--label NAME] [--json FILE]

Four cases in one process, alternating round by round: nothing frozen; both embeddings frozen; the embeddings and the lower half of
the sub-layers frozen; every `bert.` parameter frozen.  A round of a case sets requires_grad, runs `warmup` steps (the first one builds
the case's plan: a model keeps one plan per mode), then times `steps` steps between two device synchronisations.  A case's figure is the
median of its rounds' ms per step, its spread their max - min.

`--tree` imports volta_amd from another checkout (the `.base` worktree of tools/ab_bench.sh holding the parent commit): there the backward
list is the full static one whatever is frozen, so its four cases are the baseline a pruned list is measured against.  `--json` appends
one result line to FILE; tools/bench_frozen_report.py turns the lines of alternated runs into profiles/frozen_backward.md."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("none", "embeddings", "embeddings+lower half", "all of bert.")


def frozen_names(model, case):
    from volta_amd.modules import sublayer_schedule
    names = [n for n, _ in model.named_parameters()]
    subs = [n for n, _ in sublayer_schedule(model.config)]
    under = lambda pre: {n for n in names if n.startswith(pre)}
    emb = under("bert.embeddings.") | under("bert.v_embeddings.")
    if case == "none":
        return set()
    if case == "embeddings":
        return emb
    if case == "embeddings+lower half":
        return emb.union(*[under("bert.encoder.layer.%d." % n) for n in subs[:len(subs) // 2]])
    return under("bert.")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tree", metavar="PATH")
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--json", metavar="FILE")
    args = ap.parse_args()
    tree = os.path.abspath(args.tree) if args.tree else ROOT
    sys.path.insert(0, tree)
    sys.path.insert(1, os.path.join(tree, "tools"))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_frozen needs the GPU: a step time measured elsewhere says nothing")
    import bench_task_step as S
    state = S.make("vqa")
    model = state[3]
    times = {c: [] for c in CASES}
    ops = {}
    for _ in range(args.rounds):
        for case in CASES:
            off = frozen_names(model, case)
            for n, p in model.named_parameters():
                p.requires_grad_(n not in off)
                p.grad = None
            S.run_steps(args.warmup, *state)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            S.run_steps(args.steps, *state)
            torch.cuda.synchronize()
            times[case].append((time.perf_counter() - t0) * 1e3 / args.steps)
            ops[case] = len(model._last[0].bwd.ops)
    res = dict(label=args.label, device=torch.cuda.get_device_name(0), steps=args.steps, rounds=args.rounds, warmup=args.warmup,
               cases={c: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), rounds_ms=v, backward_ops=ops[c]) for c, v in times.items()})
    for c in CASES:
        r = res["cases"][c]
        print("%-12s %-24s median %8.3f ms  spread %6.3f ms  backward ops %4d" % (args.label, c, r["median_ms"], r["max_ms"] - r["min_ms"], r["backward_ops"]))
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
