"""Times the hard-negative pool search on an MI355X:

  python tools/bench_hard_pool.py [--sizes 29000,113287] [--reps 3] [--images 2000] [--out profiles/hard_pool.json]

Per size N (D = 2048, k = 100), on synthetic ReLU-style vectors (non-negative, 64 scene centres plus per-image variation, generated on the
device from a seed):
  knn_pool   `ops.knn_pool`: norms, fp32-MFMA screen with fused selection, float64 refinement, float64 fallback -- exact
  screen     the same call stopped after the screen; its 2 N^2 D flop over that time is compared with the fp32-MFMA peak (157.3 TFLOP/s)
  torch      what a user would write: chunked fp32 `mm` + `topk` on |x_j|^2 - 2 x_i . x_j -- inexact (fp32), the floor to beat
and the certified / fallback row counts of knn_pool, and how many rows of the torch result differ from the exact one.
Every figure is the median (min .. max) of `--reps` calls after one warm-up call, each between two device synchronisations, the three
alternating.  Then `generate_hard_pool` end to end over a synthetic LMDB store of `--images` images x 36 regions x 2048 (host decode
included), run twice."""
import argparse
import base64
import json
import os
import pickle
import statistics
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.lmdb_writer import write_lmdb  # noqa: E402

PEAK_F32_MFMA = 157.3e12


def make_vectors(N, D, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.randn(64, D, generator=g, device="cuda")
    which = torch.randint(0, 64, (N,), generator=g, device="cuda")
    return torch.relu(0.6 * centres[which] + torch.randn(N, D, generator=g, device="cuda")).contiguous()


def torch_topk(X, k, chunk=4096):
    n = (X * X).sum(1)
    out = torch.empty(X.shape[0], k, dtype=torch.int64, device=X.device)
    for i0 in range(0, X.shape[0], chunk):
        s = torch.addmm(n[None, :], X[i0:i0 + chunk], X.t(), alpha=-2.0)
        out[i0:i0 + chunk] = torch.topk(s, k, dim=1, largest=False, sorted=True)[1]
    return out


def timed(fns, reps):
    for f in fns:
        f()
    times = [[] for _ in fns]
    for _ in range(reps):
        for f, ts in zip(fns, times):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
    return [(statistics.median(ts), min(ts), max(ts)) for ts in times]


def bench_size(N, D, k, reps):
    from volta_amd import ops
    X = make_vectors(N, D)
    exact, stats = ops.knn_pool(X, k, return_stats=True)
    approx = torch_topk(X, k)
    differ = int((exact.long() != approx).any(1).sum())
    full, screen, base = timed([lambda: ops.knn_pool(X, k), lambda: ops.knn_pool(X, k, screen_only=True), lambda: torch_topk(X, k)], reps)
    flop = 2.0 * N * N * D
    return dict(N=N, D=D, k=k, certified=stats["certified"], fallback=stats["fallback"], torch_rows_differing=differ, knn_pool_s=full, screen_s=screen,
                torch_s=base, screen_tflops=flop / screen[0] / 1e12, screen_share_of_peak=flop / screen[0] / PEAK_F32_MFMA)


def bench_generate(images, regions=36, F=2048):
    from volta_amd.readers import ImageFeaturesH5Reader
    from volta_amd.retrieval import generate_hard_pool
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as root:
        recs = {}
        boxes = base64.b64encode((rng.uniform(0, 1, (regions, 4)) * 400).astype(np.float32).tobytes()).decode()
        for i in range(images):
            feats = np.maximum(rng.standard_normal((regions, F)), 0).astype(np.float32)
            recs[str(i).encode()] = pickle.dumps(dict(img_id=str(i), img_h=480, img_w=640, num_boxes=regions, boxes=boxes, features=base64.b64encode(feats.tobytes()).decode()))
        recs[b"keys"] = pickle.dumps([str(i).encode() for i in range(images)])
        store = os.path.join(root, "features.lmdb")
        write_lmdb(store, recs)
        ann = os.path.join(root, "train.jsonline")
        with open(ann, "w") as f:
            for i in range(images):
                f.write(json.dumps(dict(img_path="%d.jpg" % i, sentences=["a"])) + "\n")
        reader = ImageFeaturesH5Reader(store, types.SimpleNamespace(v_feature_size=F, num_locs=5, add_global_imgfeat=None))
        times = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            generate_hard_pool(reader, ann, "RetrievalFlickr30k", k=100)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
    return dict(images=images, regions=regions, F=F, seconds=times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="29000,113287")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hard_pool.py measures on an MI355X; no GPU found")
    res = dict(sizes=[], generate=None)
    for N in (int(v) for v in args.sizes.split(",")):
        r = bench_size(N, 2048, 100, args.reps)
        res["sizes"].append(r)
        print("N = %6d: knn_pool %.3f s (%.3f .. %.3f), screen alone %.3f s (%.3f .. %.3f) = %.1f TFLOP/s, %.0f %% of the fp32-MFMA peak; torch mm + topk %.3f s "
              "(%.3f .. %.3f); certified %d, fallback %d; torch differs from the exact pool in %d rows" % (
                  N, *r["knn_pool_s"], *r["screen_s"], r["screen_tflops"], 100 * r["screen_share_of_peak"], *r["torch_s"], r["certified"], r["fallback"],
                  r["torch_rows_differing"]), flush=True)
    if args.images > 0:
        res["generate"] = g = bench_generate(args.images)
        print("generate_hard_pool over %d images x %d regions x %d: %s s (runs in order)" % (g["images"], g["regions"], g["F"], ", ".join("%.2f" % v for v in g["seconds"])))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
