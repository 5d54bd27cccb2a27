"""Times the ranking step and the image load of the retrieval evaluation:

  python tools/bench_retrieval_eval.py [--reps 20] [--images 1000] [--out profiles/retrieval_eval.json]

Ranks, at 5000 x 1000 (Flickr30k's test set) and 25000 x 5000 (COCO's 5k test set) on random scores, five captions per image:
  kernel   `ops.retrieval_ranks` (csrc/ranks.hip: the CSR build in torch, three launches and a memset), top-20
  torch    the same outputs restated on the device with one `torch.argsort(..., stable=True)` per direction
  numpy    the driver's loop (eval_retrieval.py:200-263: one np.argsort per row, one per column) after the device-to-host copy of the matrix
The three are checked to agree before anything is timed (the 5000 x 1000 scores are distinct values, so the driver's unstable sort is
defined; the larger matrix has ties, which the kernel and the stable device sort resolve alike).  Device figures: the median of `--reps` timed calls after a
warm-up call, each call between two device synchronisations, alternating kernel and torch; the spread (min, max) is printed beside them.
The numpy loop is timed once.

Image load: `RetrievalDatasetVal.device_arrays()` on a synthetic store of `--images` images of 36 regions x 2048 features (lookup, base64
decode on the host threads, copy, `vk_task_batch` into the resident arrays), in images per second, cold (first call over a fresh dataset)."""
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


def torch_ranks(S, caption_image, topk):
    """the contract of ops.retrieval_ranks by sorting (untied scores without NaN): positions from two stable argsorts"""
    Nc, Ni = S.shape
    ci = caption_image.long()
    order = torch.argsort(S, dim=1, descending=True, stable=True)
    pos = torch.empty_like(order).scatter_(1, order, torch.arange(Ni, device=S.device).expand(Nc, Ni))
    rank_ir = pos.gather(1, ci[:, None])[:, 0].int()
    corder = torch.argsort(S, dim=0, descending=True, stable=True)
    cpos = torch.empty_like(corder).scatter_(0, corder, torch.arange(Nc, device=S.device)[:, None].expand(Nc, Ni))
    mine = cpos.gather(1, ci[:, None])[:, 0]
    rank_tr = torch.full((Ni,), Nc, dtype=torch.int64, device=S.device).scatter_reduce_(0, ci, mine, "amin").int()
    return rank_ir, order[:, :topk].int(), rank_tr


def numpy_loop(S, caption_image):
    score_matrix = S.cpu().numpy().astype(np.float64)
    ci = caption_image.cpu().numpy()
    Nc, Ni = score_matrix.shape
    rank_ir, results = np.zeros(Nc), []
    for c in range(Nc):
        o = np.argsort(-score_matrix[c])
        rank_ir[c] = np.where(o == ci[c])[0][0]
        results.append(o.tolist()[:20])
    rank_tr = np.zeros(Ni)
    for i in range(Ni):
        o = np.argsort(-score_matrix[:, i])
        rank_tr[i] = min(np.where(o == c)[0][0] for c in np.where(ci == i)[0])
    return rank_ir, results, rank_tr


def timed_pair(fa, fb, reps):
    """alternating timed calls of two functions -> (median, min, max) of each, seconds"""
    fa(), fb()
    ta, tb = [], []
    for _ in range(reps):
        for f, ts in ((fa, ta), (fb, tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
    return tuple((statistics.median(ts), min(ts), max(ts)) for ts in (ta, tb))


def bench_ranks(Nc, Ni, reps, with_numpy):
    from volta_amd import ops
    g = torch.Generator().manual_seed(Nc)
    if Nc * Ni < 1 << 24:                        # distinct values: the unstable np.argsort of the driver is defined everywhere
        S = (torch.randperm(Nc * Ni, generator=g).float().view(Nc, Ni) - 0.5 * Nc * Ni).cuda()
    else:                                        # ties occur; kernel and stable torch sort resolve them alike
        S = torch.randn(Nc, Ni, generator=g).cuda()
    ci = (torch.arange(Nc) % Ni)[torch.randperm(Nc, generator=g)].int().cuda()
    got, want = ops.retrieval_ranks(S, ci, 20), torch_ranks(S, ci, 20)
    assert all(torch.equal(a, b) for a, b in zip(got, want)), "kernel and torch restatement disagree"
    (k, t) = timed_pair(lambda: ops.retrieval_ranks(S, ci, 20), lambda: torch_ranks(S, ci, 20), reps)
    row = dict(Nc=Nc, Ni=Ni, kernel_ms=[1e3 * v for v in k], torch_ms=[1e3 * v for v in t], matrix_mb=Nc * Ni * 4 / 1e6)
    if with_numpy:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rank_ir, results, rank_tr = numpy_loop(S, ci)
        row["numpy_ms"] = 1e3 * (time.perf_counter() - t0)
        assert np.array_equal(rank_ir, got[0].cpu().numpy()) and np.array_equal(rank_tr, got[2].cpu().numpy()) and results == got[1].cpu().tolist()
    return row


def bench_load(images, regions=36, F=2048):
    from volta_amd.datasets import RetrievalDatasetVal
    from volta_amd.readers import ImageFeaturesH5Reader
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as root:
        recs = {}
        for i in range(images):
            feats = rng.standard_normal((regions, F)).astype(np.float32)
            boxes = (rng.uniform(0, 1, (regions, 4)) * 400).astype(np.float32)
            recs[str(i).encode()] = pickle.dumps(dict(img_id=str(i), img_h=480, img_w=640, num_boxes=regions, boxes=base64.b64encode(boxes.tobytes()).decode(),
                                                       features=base64.b64encode(feats.tobytes()).decode()))
        recs[b"keys"] = pickle.dumps([str(i).encode() for i in range(images)])
        store = os.path.join(root, "features.lmdb")
        write_lmdb(store, recs)
        words = ["w%d" % i for i in range(200)]
        with open(os.path.join(root, "vocab.txt"), "w") as f:
            f.write("\n".join(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + words) + "\n")
        with open(os.path.join(root, "test.jsonline"), "w") as f:
            for i in range(images):
                f.write(json.dumps(dict(img_path="%d.jpg" % i, sentences=[" ".join(rng.choice(words, 12)) for _ in range(5)])) + "\n")
        from volta_amd.readers import WordPieceTokenizer
        cfg = types.SimpleNamespace(v_feature_size=F, num_locs=5, add_global_imgfeat="first")
        times = []
        for rep in range(3):                     # a fresh dataset each time: nothing is resident, the store's pages are warm after the first
            ds = RetrievalDatasetVal(task="RetrievalFlickr30k", dataroot=root, annotations_jsonpath=os.path.join(root, "test.jsonline"), split="test",
                                     image_features_reader=ImageFeaturesH5Reader(store, cfg), gt_image_features_reader=None,
                                     tokenizer=WordPieceTokenizer(os.path.join(root, "vocab.txt")), bert_model="bert-base-uncased", max_seq_length=38)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            arr = ds.device_arrays()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        nbytes = sum(arr[k].numel() * arr[k].element_size() for k in ("features", "spatials", "image_mask"))
    return dict(images=images, regions=regions + 1, resident_mb=nbytes / 1e6, seconds=times, images_per_s=[images / t for t in times])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_retrieval_eval.py measures on an MI355X; no GPU found")
    res = dict(ranks=[bench_ranks(5000, 1000, args.reps, True), bench_ranks(25000, 5000, max(3, args.reps // 4), False)], load=bench_load(args.images))
    for r in res["ranks"]:
        print("ranks %5d x %4d (%.0f MB): kernel %.3f ms (%.3f .. %.3f), torch argsort %.3f ms (%.3f .. %.3f)%s" % (
            r["Nc"], r["Ni"], r["matrix_mb"], *r["kernel_ms"], *r["torch_ms"], ", numpy loop %.0f ms" % r["numpy_ms"] if "numpy_ms" in r else ""))
    ld = res["load"]
    print("device_arrays: %d images x %d rows (%.0f MB resident): %s images/s (runs in order)" % (
        ld["images"], ld["regions"], ld["resident_mb"], ", ".join("%.0f" % v for v in ld["images_per_s"])))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
