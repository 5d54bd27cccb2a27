"""profiles/frozen_backward.md from the result lines of alternated tools/bench_frozen.py runs (--json FILE; labels `parent` and `this`):

  python tools/bench_frozen_report.py FILE [--out profiles/frozen_backward.md]

Per label and case: every run's median, then the mean of the runs' medians.  The spread of the parent is the largest difference between
two of its figures for ONE case (across its runs and rounds).  The four conditions of the change are evaluated against that spread and
printed, each with `holds` or `FAILS`, and a failing one with the reason."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("none", "embeddings", "embeddings+lower half", "all of bert.")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("file")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frozen_backward.md"))
    args = ap.parse_args()
    runs = [json.loads(l) for l in open(args.file) if l.strip().startswith("{")]
    by = {}
    for r in runs:
        by.setdefault(r["label"], []).append(r)
    if not {"parent", "this"} <= set(by):
        sys.exit("need runs labelled `parent` and `this`")
    r0 = runs[0]
    out = ["# Backward pruned to the trainable parameters: the VQA fine-tuning step", "",
           "`tools/bench_frozen.py --steps %d --rounds %d --warmup %d` on %s: ctrl_vilbert_base, B = 256, T = 23, 37 region rows, 3129 labels;" % (r0["steps"], r0["rounds"], r0["warmup"], r0["device"]),
           "ms per step (forward, loss, backward, clip, AdamW).  The parent commit and this one ran alternately in one GPU session, %d runs each," % len(by["this"]),
           "in the order %s; inside a run the four cases alternate round by round, each round timing %d steps after %d warm-up steps." % (" / ".join(r["label"] for r in runs), r0["steps"], r0["warmup"]), ""]
    mean = {}
    for label in ("parent", "this"):
        out += ["## %s" % label, "", "| case | backward ops | run medians | mean of medians | min .. max of all rounds |", "|---|---|---|---|---|"]
        for c in CASES:
            meds = [r["cases"][c]["median_ms"] for r in by[label]]
            allr = [t for r in by[label] for t in r["cases"][c]["rounds_ms"]]
            mean[(label, c)] = statistics.mean(meds)
            out.append("| %s | %d | %s | %.3f | %.3f .. %.3f |" % (c, by[label][0]["cases"][c]["backward_ops"], " ".join("%.3f" % m for m in meds), mean[(label, c)], min(allr), max(allr)))
        out.append("")
    spread = max(max(t for r in by["parent"] for t in r["cases"][c]["rounds_ms"]) - min(t for r in by["parent"] for t in r["cases"][c]["rounds_ms"]) for c in CASES)
    run_spread = max(abs(a["cases"][c]["median_ms"] - b["cases"][c]["median_ms"]) for c in CASES for a in by["parent"] for b in by["parent"])
    base = [mean[("parent", c)] for c in CASES]
    this = [mean[("this", c)] for c in CASES]
    ok = lambda b: "holds" if b else "FAILS"
    out += ["## Conditions", "",
            "Spread of the parent: %.3f ms between the rounds of one case, %.3f ms between the medians of its two runs." % (spread, run_spread), "",
            "1. Baseline: on the parent the four cases cost the same: %s ms, max - min %.3f ms -- %s.%s" % (
                " / ".join("%.3f" % x for x in base), max(base) - min(base), ok(max(base) - min(base) <= spread),
                "" if max(base) - min(base) <= spread else "  Its backward list is the same %d ops in every case; what differs is the clip and AdamW, which"
                % by["parent"][0]["cases"][CASES[0]]["backward_ops"]),
            "" if max(base) - min(base) <= spread else "   pass over the chunks of parameters without a gradient already: that part of the saving is not this change's.",
            "   Per case, this tree against the parent (what pruning the backward list adds): %s." % ", ".join("%+.3f ms" % (t - b) for t, b in zip(this, base)),
            "2. Nothing frozen: this %.3f ms against the parent's %.3f ms, %+.3f ms: within the parent's spread -- %s." % (this[0], base[0], this[0] - base[0], ok(abs(this[0] - base[0]) <= spread)),
            "3. Every frozen case is below the unfrozen one by more than that spread: %s -- %s." % (", ".join("%+.3f ms" % (x - this[0]) for x in this[1:]), ok(all(this[0] - x > spread for x in this[1:]))),
            "4. The four cases are ordered as listed: %s ms -- %s." % (" > ".join("%.3f" % x for x in this), ok(all(a > b for a, b in zip(this, this[1:])))), ""]
    text = "\n".join(out)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
