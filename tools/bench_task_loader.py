"""Throughput of the fine-tuning loader at the VQA shape (batch 256, 101 regions, 2048 features, T = 16) on a synthetic feature store the tool
writes itself:

  python tools/bench_task_loader.py [--images 512] [--batch 256] [--resident-bytes N] [--out profiles/task_loader.json]

Reports samples per second of `TaskLoader` cold (lookup + base64 decode on the host threads + copy + assembly), with `in_memory` on the
second epoch (copies from the pinned pool + assembly), the host's base64 decode rate on its own, and the assembler (`vk_task_batch`) alone with
the bytes it moves (read + written) per second.  Compare the in_memory rate with tools/bench_task_step.py on the same machine, and the
assembler with the copy rate quoted for a streaming kernel in VERDICT.md.  Each figure is the median of `--reps` timed runs after one
warm-up run; the spread is printed beside it.

`--resident-bytes N` (N must hold the whole store: 512 images of 100 regions need about 425 MB) adds the device-resident path: four epoch
variants timed ALTERNATELY in one loop -- cold with host decode, cold with device decode (a pool too small to hold anything), warm `in_memory`,
warm all-resident -- the device decoder alone (`vk_b64_decode_device`, GB of text per second) and the pool assembler alone
(`vk_task_batch_pool`, bytes moved per second, checked equal to `vk_task_batch` on the same batch first)."""
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


def kernel_times(fn, warm=3, reps=20):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for i in range(warm + reps):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        if i >= warm:
            times.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    return statistics.median(times), min(times), max(times)


def resident_rows(res, a, ds, cold, warm, epoch, h, dense_args, scatter, out, dense_moved, F):
    """The rows of the device-resident path.  The epoch variants ALTERNATE inside one loop (cold host decode / cold device decode / warm
    in_memory / warm resident), one timed epoch each per repetition, so drift of the box lands on all of them alike."""
    from volta_amd import datasets as D, ops
    device_cold = D.TaskLoader(ds, a.batch, resident_bytes=16)                     # a pool too small to hold anything: every image is decoded
    resident = D.TaskLoader(ds, a.batch, resident_bytes=a.resident_bytes)
    variants = dict(cold_host_decode=cold, cold_device_decode=device_cold, warm_in_memory=warm, warm_resident=resident)
    for ld in variants.values():                                                    # warm-up: fills the pinned pool and the resident pool
        epoch(ld)
    assert resident.resident_images == a.images and resident.stats["scratch_images"] == 0, "--resident-bytes does not hold the store"
    ts = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, ld in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            epoch(ld)
            torch.cuda.synchronize()
            ts[k].append(time.perf_counter() - t0)
    res["alternating_epochs_samples_per_s"] = {k: dict(median=len(ds) / statistics.median(v), min=len(ds) / max(v), max=len(ds) / min(v)) for k, v in ts.items()}
    res["resident"] = dict(stats=resident.stats, bytes_used=resident.resident_bytes_used, cold_device_stats=device_cold.stats)
    # the decoder alone: the text of one batch on the device, decoded into scratch
    hr = device_cold._stage_resident(list(range(min(a.batch, len(ds)))), 0)
    text = hr["arena"][:hr["arena_bytes"]].cuda()
    jobs, at = [], 0
    for k, s in enumerate(hr["fresh"]):
        rows = int(hr["n"][s])
        fo, bo, _, size = D._ResidentPool.layout(at, rows, F)
        jobs += [(hr["fields"][2 * k][1], fo, hr["fields"][2 * k][0], rows * F * 4), (hr["fields"][2 * k + 1][1], bo, hr["fields"][2 * k + 1][0], rows * 16)]
        at += size
    tab, mx = ops.b64_jobs(jobs)
    tab, dst = tab.cuda(), torch.empty(at, dtype=torch.uint8, device="cuda")
    status = ops.b64_decode_device(text, dst, tab, mx)
    assert not status.any().item()
    med, lo, hi = kernel_times(lambda: ops.b64_decode_device(text, dst, tab, mx, status=status))
    chars = sum(j[2] for j in jobs)
    res["b64_decode_device"] = dict(seconds_median=med, seconds_min=lo, seconds_max=hi, text_bytes=chars, GB_text_per_s=chars / med / 1e9, jobs=len(jobs))
    # the pool assembler alone on the same batch: the images where the decoder above put them (region 1), stored global rows
    S = hr["S"]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    offs = np.zeros((3, S), np.int64)
    at = 0
    for s in range(S):
        fo, bo, mo, size = D._ResidentPool.layout(at, int(hr["n"][s]), F)
        offs[:, s] = fo, bo, mo
        at += size
    slots = ((None, dst), torch.ones(S, dtype=torch.int32, device="cuda"), dev(offs[0]), dev(offs[1]), dev(offs[2]), dev(hr["n"]), dev(hr["wh"]), F)
    ops.task_pool_means(*slots, torch.arange(S, dtype=torch.int32, device="cuda"))
    tail = (dev(hr["segs"]), dev(hr["counts"]), ds.block_rows, 5, "first")
    pout = ops.task_batch_pool(*slots, *tail, scatter=scatter)
    want = ops.task_batch(*dense_args, scatter=scatter)
    assert all(torch.equal(pout[k], want[k]) for k in want), "the pool assembler and the dense assembler disagree"
    med, lo, hi = kernel_times(lambda: ops.task_batch_pool(*slots, *tail, scatter=scatter, out=pout))
    moved = dense_moved - (int(hr["n"].sum()) + S) * F * 4                           # no mean pass: the global rows are stored
    res["assembler_pool"] = dict(seconds_median=med, seconds_min=lo, seconds_max=hi, bytes_moved=moved, TB_per_s=moved / med / 1e12,
                                 samples_per_s=hr["segs"].shape[0] / med)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--regions", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resident-bytes", type=int, default=0,
                    help="> 0: also measure the device-resident path with a pool of this size (it must hold every image of the store)")
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
        if a.resident_bytes:
            resident_rows(res, a, ds, cold, warm, epoch, h, args, scatter, out, moved, F)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
