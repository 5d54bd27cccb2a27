"""Runs and times the retrieval evaluation with the captions sharded over W ranks (`evaluate_retrieval(..., group=True)`):

  python tools/eval_retrieval_sharded.py [--world W] [--images 1000] [--config ctrl_vilbert_base] [--dtype bf16|fp8] [--reps 2] [--timeout 900] [--out FILE.json]
  python tools/eval_retrieval_sharded.py --kernels [--reps 20] [--out FILE.json]

Default mode.  Writes the synthetic store of tools/bench_retrieval_eval.py (`--images` images of 36 regions x 2048 features, five 12-word
captions each) into a temporary directory, then starts W ranks (1..16, default: the number of visible GPUs) as fresh child processes of this
file, each under its own time limit of `--timeout` seconds, and stops all of them when the first one fails.  Rank r runs on GPU r modulo the
GPU count; the group is nccl when every rank has a GPU of its own and gloo otherwise (several ranks on one GPU: a functional run, not a
speed-up).  Every rank builds the same randomly initialised task model (one seed), loads the test set, and calls the evaluation `--reps`
times; the first call builds the scorer's plans and is reported apart.  Per rank and call it prints the seconds of three phases, taken by a
`phase_hook` that synchronises the device: encode (all images and the rank's captions), score (the rank's block of the matrix), ranks +
exchange (three launches and four all_reduce calls), and inside the last the seconds spent in `all_reduce` itself.  The parent checks
that every rank reports the same metrics and prints one JSON line.  `--dtype fp8` scores on the e4m3 projection path
(`evaluate_retrieval(..., projection_dtype="fp8")`): the metrics are then the fp8 model's.

--kernels.  One process, one GPU, no model: `ops.retrieval_ranks` against the W = 1 sharded sequence (`retrieval_ranks_shard`,
`retrieval_ranks_shard_counts`, `retrieval_ranks_finish`) on the matrices of tools/bench_retrieval_eval.py, 5000 x 1000 and 25000 x 5000,
top-20.  The outputs are checked to be equal first.  Figures: the median of `--reps` (a quarter of them at the larger size) timed calls
after a warm-up call, each between two device synchronisations, the two paths alternating; minimum and maximum beside them."""
import argparse
import base64
import datetime
import json
import os
import pickle
import statistics
import subprocess
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TASK_CFG = {"TASK8": {"type": "VL-logit"}}
REGIONS, F, WORDS, SENTENCES = 36, 2048, 200, 5


# ------------------------------------------------------------------------------------------------ the synthetic test set
def write_store(root, images):
    """the store, vocabulary and annotations of tools/bench_retrieval_eval.py:bench_load"""
    from tests.lmdb_writer import write_lmdb
    rng = np.random.default_rng(0)
    recs = {}
    for i in range(images):
        feats = rng.standard_normal((REGIONS, F)).astype(np.float32)
        boxes = (rng.uniform(0, 1, (REGIONS, 4)) * 400).astype(np.float32)
        recs[str(i).encode()] = pickle.dumps(dict(img_id=str(i), img_h=480, img_w=640, num_boxes=REGIONS, boxes=base64.b64encode(boxes.tobytes()).decode(),
                                                   features=base64.b64encode(feats.tobytes()).decode()))
    recs[b"keys"] = pickle.dumps([str(i).encode() for i in range(images)])
    write_lmdb(os.path.join(root, "features.lmdb"), recs)
    words = ["w%d" % i for i in range(WORDS)]
    with open(os.path.join(root, "vocab.txt"), "w") as f:
        f.write("\n".join(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + words) + "\n")
    with open(os.path.join(root, "test.jsonline"), "w") as f:
        for i in range(images):
            f.write(json.dumps(dict(img_path="%d.jpg" % i, sentences=[" ".join(rng.choice(words, 12)) for _ in range(SENTENCES)])) + "\n")


def open_dataset(root):
    from volta_amd.datasets import RetrievalDatasetVal
    from volta_amd.readers import ImageFeaturesH5Reader, WordPieceTokenizer
    cfg = types.SimpleNamespace(v_feature_size=F, num_locs=5, add_global_imgfeat="first")
    return RetrievalDatasetVal(task="RetrievalFlickr30k", dataroot=root, annotations_jsonpath=os.path.join(root, "test.jsonline"), split="test",
                               image_features_reader=ImageFeaturesH5Reader(os.path.join(root, "features.lmdb"), cfg), gt_image_features_reader=None,
                               tokenizer=WordPieceTokenizer(os.path.join(root, "vocab.txt")), bert_model="bert-base-uncased", max_seq_length=38)


# ------------------------------------------------------------------------------------------------ one rank
def child(args):
    import torch.distributed as dist
    from volta_amd.config import BertConfig
    from volta_amd.modeling import BertForVLTasks
    from volta_amd.retrieval import evaluate_retrieval
    torch.cuda.set_device(args.rank % torch.cuda.device_count())
    dist.init_process_group(args.backend, init_method="file://" + os.path.join(args.root, "rendezvous"), rank=args.rank, world_size=args.world,
                            timeout=datetime.timedelta(seconds=args.timeout))
    try:
        cfg = BertConfig.from_json_file(os.path.join(ROOT, "config", args.config + ".json"))
        torch.manual_seed(0)                                                  # the same weights on every rank
        model = BertForVLTasks(cfg, TASK_CFG, list(TASK_CFG)).cuda().eval()
        ds = open_dataset(args.root)
        ds.device_arrays()
        spent, reduce_s, all_reduce = {}, [0.0], dist.all_reduce

        def timed_all_reduce(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = all_reduce(*a, **kw)
            torch.cuda.synchronize()
            reduce_s[0] += time.perf_counter() - t0
            return out

        def hook(name):
            torch.cuda.synchronize()
            now = time.perf_counter()
            spent[name], spent["_t"] = now - spent["_t"], now

        dist.all_reduce = timed_all_reduce
        calls = []
        for rep in range(args.reps):
            dist.barrier()
            torch.cuda.synchronize()
            reduce_s[0], spent["_t"] = 0.0, time.perf_counter()
            res = evaluate_retrieval(model, ds, task_id="TASK8", pair_chunk=args.pair_chunk, topk=20, group=True, phase_hook=hook, projection_dtype=args.dtype)
            calls.append(dict(encode=spent["encode"], score=spent["score"], ranks=spent["ranks"], all_reduce=reduce_s[0]))
            print("rank %d call %d: captions [%d, %d): encode %.3f s, score %.3f s, ranks + exchange %.4f s (all_reduce %.4f s)%s" % (
                args.rank, rep, *res.caption_range, *[calls[-1][k] for k in ("encode", "score", "ranks", "all_reduce")], "  [builds the plans]" if rep == 0 else ""), flush=True)
        dist.all_reduce = all_reduce
        with open(os.path.join(args.root, "rank%d.json" % args.rank), "w") as f:
            json.dump(dict(rank=args.rank, caption_range=list(res.caption_range), calls=calls, image_retrieval=res.image_retrieval, text_retrieval=res.text_retrieval), f)
    finally:
        dist.destroy_process_group()


def parent(args):
    ngpu = torch.cuda.device_count()
    if ngpu < 1:
        raise SystemExit("eval_retrieval_sharded.py runs on MI355X GPUs; none found")
    W = args.world or ngpu
    if not 1 <= W <= 16:
        raise SystemExit("--world %d: 1 to 16 ranks" % W)
    backend = "nccl" if W <= ngpu else "gloo"
    with tempfile.TemporaryDirectory() as root:
        write_store(root, args.images)
        procs = [subprocess.Popen(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--rank", str(r), "--world", str(W),
                                   "--root", root, "--backend", backend, "--config", args.config, "--reps", str(args.reps), "--timeout", str(args.timeout),
                                   "--pair-chunk", str(args.pair_chunk), "--dtype", args.dtype]) for r in range(W)]
        pending, failed = set(range(W)), None
        while pending and failed is None:
            for r in sorted(pending):
                try:
                    rc = procs[r].wait(timeout=0.1)
                except subprocess.TimeoutExpired:
                    continue
                pending.discard(r)
                if rc != 0:
                    failed = (r, rc)
                    break
        for r in pending:                                                     # the first failure ends the run: the others would wait for it
            procs[r].kill()
            procs[r].wait()
        if failed is not None:
            raise SystemExit("rank %d ended with status %d; the other ranks were stopped" % failed)
        ranks = [json.load(open(os.path.join(root, "rank%d.json" % r))) for r in range(W)]
    for r in ranks[1:]:
        assert r["image_retrieval"] == ranks[0]["image_retrieval"] and r["text_retrieval"] == ranks[0]["text_retrieval"], "the ranks disagree"
    res = dict(world=W, gpus=ngpu, backend=backend, images=args.images, captions=args.images * SENTENCES, config=args.config, dtype=args.dtype, ranks=ranks)
    print(json.dumps(res))
    return res


# ------------------------------------------------------------------------------------------------ the kernels alone
def timed_pair(fa, fb, reps):
    """alternating timed calls of two functions -> (median, min, max) of each, milliseconds"""
    fa(), fb()
    ta, tb = [], []
    for _ in range(reps):
        for f, ts in ((fa, ta), (fb, tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
    return tuple([statistics.median(ts), min(ts), max(ts)] for ts in (ta, tb))


def kernels(args):
    from volta_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("eval_retrieval_sharded.py --kernels measures on an MI355X; no GPU found")
    rows = []
    for Nc, Ni, reps in ((5000, 1000, args.reps), (25000, 5000, max(3, args.reps // 4))):
        g = torch.Generator().manual_seed(Nc)
        S = ((torch.randperm(Nc * Ni, generator=g).float().view(Nc, Ni) - 0.5 * Nc * Ni) if Nc * Ni < 1 << 24 else torch.randn(Nc, Ni, generator=g)).cuda()
        ci = (torch.arange(Nc) % Ni)[torch.randperm(Nc, generator=g)].int().cuda()

        def sharded():
            sh = ops.retrieval_ranks_shard(S, 0, Nc, ci, 20)
            count = ops.retrieval_ranks_shard_counts(sh, sh.target_key)
            return sh.rank_ir, sh.topk_ir, ops.retrieval_ranks_finish(count, sh.image_ptr, Ni)

        assert all(torch.equal(a, b) for a, b in zip(ops.retrieval_ranks(S, ci, 20), sharded())), "the sharded sequence and ops.retrieval_ranks disagree"
        whole, shard = timed_pair(lambda: ops.retrieval_ranks(S, ci, 20), sharded, reps)
        rows.append(dict(Nc=Nc, Ni=Ni, reps=reps, retrieval_ranks_ms=whole, sharded_w1_ms=shard))
        print("ranks %5d x %4d: ops.retrieval_ranks %.3f ms (%.3f .. %.3f), W = 1 sharded sequence %.3f ms (%.3f .. %.3f), %d alternated calls each" % (
            Nc, Ni, *whole, *shard, reps), flush=True)
    return dict(kernels=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=0)
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--config", default="ctrl_vilbert_base")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp8"], help="projection precision of the scorer")
    ap.add_argument("--reps", type=int, default=0)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--pair-chunk", type=int, default=1000)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--rank", type=int, default=0)
    ap.add_argument("--root", default="")
    ap.add_argument("--backend", default="gloo")
    args = ap.parse_args()
    args.reps = args.reps or (20 if args.kernels else 2)
    if args.child:
        return child(args)
    res = kernels(args) if args.kernels else parent(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
