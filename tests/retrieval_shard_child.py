"""Shared by tests/test_retrieval_eval_sharded_gpu.py and run by it as the program of one rank:

    python tests/retrieval_shard_child.py --rank R --world W --store FILE --root DIR --out FILE.npz [--zero-shot]

The tiny ViLBERT of tests/test_retrieval_eval_gpu.py and a 20-caption test set over the six images of the retrieval-eval fixture
(tests/retrieval_eval_fixture.py: its Flickr annotations with every sentence once more in reverse word order).  As a program: joins the gloo
group that `--store` (a file) names, runs `evaluate_retrieval(..., group=True)` on GPU 0 and writes what it returned to `--out`."""
import argparse
import datetime
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.dirname(os.path.abspath(__file__)), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
from tests.retrieval_eval_fixture import F, EvalFixture  # noqa: E402

TASK_CFG = {"TASK8": {"type": "VL-logit"}}
METRICS = ("r1", "r5", "r10", "medr", "meanr")


def tiny_model(zero_shot, seed=4):
    from test_engine_gpu import CONFIGS
    from oracle import volta_ref as R
    from volta_amd.config import BertConfig
    from volta_amd.modeling import BertForVLPreTraining, BertForVLTasks
    cd = dict(CONFIGS["vilbert"], clf_hidden_size=1536, v_feature_size=F)
    rcfg = R.RefConfig(cd)
    if zero_shot:
        model = BertForVLPreTraining(BertConfig.from_dict(cd))
        model.load_state_dict(R.make_weights(rcfg, seed=seed, std=0.04), strict=True)
    else:
        model = BertForVLTasks(BertConfig.from_dict(cd), TASK_CFG, list(TASK_CFG))
        model.load_state_dict(R.make_task_weights(rcfg, TASK_CFG, list(TASK_CFG), seed=seed, std=0.04), strict=True)
    return model.cuda().eval()


def dataset20(fx):
    """20 captions over the fixture's 6 images (the sixth has none): flickr_plain's reader and tokenizer over a doubled annotation file"""
    from volta_amd import datasets as D
    path = os.path.join(fx.root, "flickr20_test.jsonline")
    with open(fx.jsonpath("RetrievalFlickr30k")) as f, open(path, "w") as out:
        for line in f:
            ann = json.loads(line)
            ann["sentences"] = ann["sentences"] + [" ".join(reversed(s.split())) for s in ann["sentences"]]
            out.write(json.dumps(ann) + "\n")
    kind, kw = fx.cases["flickr_plain"]
    ds = D.RetrievalEvalMap[kind](task=kind, dataroot=fx.root, annotations_jsonpath=path, image_features_reader=fx.reader("flickr_plain"),
                                  gt_image_features_reader=None, tokenizer=fx.tokenizer("words"), bert_model="bert-base-uncased", padding_index=0, **kw)
    assert len(ds) == 40 and len(ds._image_entries) == 6
    return ds


def pack(res):
    """a RetrievalResult as a dict of numpy arrays (np.savez)"""
    K = max([len(r) for r in res.results] + [0])
    top = np.full((len(res.results), K), -1, np.int64)
    for c, r in enumerate(res.results):
        top[c, :len(r)] = r
    return dict(rank_ir=res.rank_ir.cpu().numpy(), rank_tr=res.rank_tr.cpu().numpy(), results=top, score_matrix=res.score_matrix.cpu().numpy(),
                caption_range=np.asarray(res.caption_range, np.int64), image_retrieval=np.asarray([res.image_retrieval[k] for k in METRICS], np.float64),
                text_retrieval=np.asarray([res.text_retrieval[k] for k in METRICS], np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, required=True)
    ap.add_argument("--store", required=True)
    ap.add_argument("--root", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--zero-shot", action="store_true")
    args = ap.parse_args()
    import torch.distributed as dist
    from volta_amd.retrieval import evaluate_retrieval
    os.makedirs(args.root, exist_ok=True)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="file://" + args.store, rank=args.rank, world_size=args.world, timeout=datetime.timedelta(seconds=60))
    try:
        model, ds = tiny_model(args.zero_shot), dataset20(EvalFixture(args.root))
        res = evaluate_retrieval(model, ds, task_id=None if args.zero_shot else "TASK8", pair_chunk=1000, topk=20, group=True)
        np.savez(args.out, **pack(res))
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
