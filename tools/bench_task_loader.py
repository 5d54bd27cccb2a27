"""Throughput of the fine-tuning loader at the VQA shape (batch 256, 101 regions, 2048 features, T = 16) on a synthetic feature store the tool
writes itself:

  python tools/bench_task_loader.py [--images 512] [--batch 256] [--out profiles/task_loader.json]

Reports samples per second of `TaskLoader` cold (lookup + base64 decode on the host threads + copy + assembly), with `in_memory` on the
second epoch (copies from the pinned pool + assembly), the host's base64 decode rate on its own, and the assembler (`vk_task_batch`) alone with
the bytes it moves (read + written) per second.  Compare the in_memory rate with tools/bench_task_step.py on the same machine, and the
assembler with the copy rate quoted for a streaming kernel in VERDICT.md.  Each figure is the median of `--reps` timed runs after one
warm-up run; the spread is printed beside it."""
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


def write_store(root, images, regions, F, questions, T):
    rng = np.random.default_rng(0)
    recs, words = {}, ["w%d" % i for i in range(200)]
    for i in range(images):
        feats = rng.standard_normal((regions, F)).astype(np.float32)
        boxes = (rng.uniform(0, 1, (regions, 4)) * 400).astype(np.float32)
        recs[str(i).encode()] = pickle.dumps(dict(img_id=str(i), img_h=480, img_w=640, num_boxes=regions, boxes=base64.b64encode(boxes.tobytes()).decode(),
                                                   features=base64.b64encode(feats.tobytes()).decode()))
    recs[b"keys"] = pickle.dumps([str(i).encode() for i in range(images)])
    write_lmdb(os.path.join(root, "features.lmdb"), recs)
    os.makedirs(os.path.join(root, "cache"))
    qs = [dict(question_id=i, image_id=i % images, question=" ".join(rng.choice(words, T - 4))) for i in range(questions)]
    ans = [dict(question_id=i, image_id=i % images, labels=sorted(int(x) for x in rng.choice(3129, 3, replace=False)), scores=[1.0, 0.6, 0.3]) for i in range(questions)]
    for split in ("train", "val"):
        json.dump(dict(questions=qs), open(os.path.join(root, "v2_OpenEnded_mscoco_%s2014_questions.json" % split), "w"))
        pickle.dump(ans, open(os.path.join(root, "cache", "%s_target.pkl" % split), "wb"))
    labels = ["a%d" % i for i in range(3129)]
    pickle.dump({a: i for i, a in enumerate(labels)}, open(os.path.join(root, "trainval_ans2label.pkl"), "wb"))
    pickle.dump(labels, open(os.path.join(root, "trainval_label2ans.pkl"), "wb"))
    with open(os.path.join(root, "vocab.txt"), "w") as f:
        f.write("\n".join(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + words) + "\n")


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--regions", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from volta_amd import datasets as D, ops
    from volta_amd.readers import ImageFeaturesH5Reader, WordPieceTokenizer, b64_to_array
    F, T = 2048, 16
    res = dict(shape=dict(batch=a.batch, regions=a.regions + 1, features=F, T=T, images=a.images), device=torch.cuda.get_device_name(0))
    with tempfile.TemporaryDirectory() as root:
        write_store(root, a.images, a.regions, F, a.images, T)
        cfg = types.SimpleNamespace(v_feature_size=F, num_locs=5, add_global_imgfeat="first")
        tok = WordPieceTokenizer(os.path.join(root, "vocab.txt"))

        def dataset():
            rd = ImageFeaturesH5Reader(os.path.join(root, "features.lmdb"), cfg)
            return D.VQAClassificationDataset("VQA", root, "", "train", rd, None, tok, "bert-base-uncased", max_seq_length=T, max_region_num=a.regions,
                                              num_locs=5, add_global_imgfeat="first")

        def epoch(ld):
            n = 0
            for batch in ld:
                n += batch[0].shape[0]
            return n

        ds = dataset()
        cold = D.TaskLoader(ds, a.batch)
        med, lo, hi = timed(lambda: epoch(cold), a.reps)
        res["cold_samples_per_s"] = dict(median=len(ds) / med, min=len(ds) / hi, max=len(ds) / lo, threads=cold.threads)
        warm = D.TaskLoader(ds, a.batch, in_memory=True)
        epoch(warm)                                                          # fills the pool
        med, lo, hi = timed(lambda: epoch(warm), a.reps)
        res["in_memory_samples_per_s"] = dict(median=len(ds) / med, min=len(ds) / hi, max=len(ds) / lo, pool_bytes=warm.pool_bytes_used)
        text = pickle.loads(ds._image_features_reader.env.get(b"0"))["features"].encode()
        t0 = time.perf_counter()
        for _ in range(20):
            b64_to_array(text)
        res["b64_decode_one_thread_MB_text_per_s"] = 20 * len(text) / (time.perf_counter() - t0) / 1e6
        # the assembler alone, on one staged batch that stays on the device
        h = cold._stage(list(range(min(a.batch, len(ds)))), 0)
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        S, Rcap = h["S"], h["Rcap"]
        feat, boxes = h["stage"]["feat"][:S].cuda().contiguous(), h["stage"]["boxes"][:S].cuda().contiguous()
        args = (feat, boxes, dev(h["n"]), dev(h["wh"]), dev(h["segs"]), dev(h["counts"]), ds.block_rows, 5, "first")
        scatter = (dev(h["csr"]), dev(h["labels"]), dev(h["scores"]), ds.num_labels)
        out = ops.task_batch(*args, scatter=scatter)
        mean = torch.empty(S, F, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        times = []
        for i in range(3 + 20):
            ev[0].record()
            ops.task_batch(*args, scatter=scatter, out=out, mean=mean)
            ev[1].record()
            torch.cuda.synchronize()
            if i >= 3:
                times.append(ev[0].elapsed_time(ev[1]) * 1e-3)
        N, R = h["segs"].shape[0], ds.block_rows
        assert S == N, "the byte count below takes one distinct image per sample (%d images, %d blocks): raise --images" % (S, N)
        rows = int(np.minimum(h["n"] + 1, R).sum())
        moved = rows * F * 4 * 2 + (N * R - rows) * F * 4 + int(h["n"].sum()) * F * 4 + S * F * 4 + out["target"].numel() * 4   # copied rows twice, zero rows, mean pass
        med = statistics.median(times)
        res["assembler"] = dict(seconds_median=med, seconds_min=min(times), seconds_max=max(times), bytes_moved=moved, TB_per_s=moved / med / 1e12,
                                samples_per_s=N / med)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
