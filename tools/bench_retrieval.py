"""Retrieval scoring throughput: the reference driver's loop (eval_retrieval.py:168-198: per caption, two `model(...)` calls on 500 pairs --
the caption repeated, 500 images -- each followed by `.cpu()`) against volta_amd.retrieval.RetrievalScorer (image encoding once, caption
encoding, score_matrix; one `.cpu()` at the end), on random weights, in VL-logit and zero-shot mode.  In zero-shot mode the loop also pays for
the [B, T, 30522] MLM and region scores that BertForVLPreTraining's score branch computes and the driver throws away; the scorer skips them.
That share is reported on its own ("heads"): the loop's time minus the same loop over `encode()` + the ITM linear, so it is not credited to
the prefix reuse.  Timed with torch.cuda.Event after one warm-up pass over a few captions (every shape of the timed window).
usage: python tools/bench_retrieval.py --config ctrl_vilbert_base [--captions 64] [--images 1000] [--modes logit,zeroshot]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from volta_amd.config import BertConfig  # noqa: E402
from volta_amd.modeling import BertForVLPreTraining, BertForVLTasks  # noqa: E402
from volta_amd.retrieval import RetrievalScorer, split_plan  # noqa: E402

TASK_CFG = {"TASK8": {"type": "VL-logit"}}


def inputs(cfg, Nc, Ni, T, Rv, seed=0):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(T // 2, T + 1, (Nc,), generator=g)
    mask = (torch.arange(T)[None] < lens[:, None]).long()
    ids = torch.randint(1000, cfg.vocab_size, (Nc, T), generator=g) * mask
    ids[:, 0] = 101
    nreg = torch.randint(10, Rv + 1, (Ni,), generator=g)
    imask = (torch.arange(Rv)[None] < nreg[:, None]).long()
    feat = torch.rand(Ni, Rv, cfg.v_feature_size, generator=g) * imask[..., None]
    loc = torch.rand(Ni, Rv, cfg.num_locs, generator=g) * imask[..., None]
    return [t.cuda() for t in (ids, torch.zeros_like(ids), mask)], [t.cuda() for t in (feat, loc, imask)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def loop(model, zero_shot, caps, imgs, ncap, encode_only=False, block=500):
    ids, seg, mask = caps
    feat, loc, imask = imgs
    Ni = feat.shape[0]
    W = model.cls.bi_seq_relationship if zero_shot else None
    with torch.no_grad():
        for c in range(ncap):
            for i0 in range(0, Ni, block):
                n = min(block, Ni - i0)
                q, s, m = ids[c:c + 1].repeat(n, 1), seg[c:c + 1].repeat(n, 1), mask[c:c + 1].repeat(n, 1)
                args = (q, feat[i0:i0 + n], loc[i0:i0 + n])
                if not zero_shot:
                    out = model(*args, "TASK8", s, m, imask[i0:i0 + n])[0].view(-1)
                elif encode_only:                   # the encoder and poolers of the score branch, then the ITM linear in torch
                    _, _, pt, pv, _ = model.encode(*args, s, m, imask[i0:i0 + n])
                    out = torch.softmax(torch.nn.functional.linear(pt * pv, W.weight, W.bias), dim=1)[:, 0]
                else:
                    out = torch.softmax(model(*args, s, m, imask[i0:i0 + n])[2], dim=1)[:, 0]
                out.cpu()


def scorer_run(sc, caps, imgs):
    S = sc.score_matrix(sc.encode_captions(*caps), sc.encode_images(*imgs))
    S.cpu()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="ctrl_vilbert_base")
    ap.add_argument("--captions", type=int, default=64)
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--T", type=int, default=38)
    ap.add_argument("--regions", type=int, default=37, help="rows per image, the global feature included")
    ap.add_argument("--pair-chunk", type=int, default=1000)
    ap.add_argument("--modes", default="logit,zeroshot")
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = BertConfig.from_json_file(os.path.join(root, "config", args.config + ".json"))
    caps, imgs = inputs(cfg, args.captions, args.images, args.T, args.regions)
    pairs = args.captions * args.images
    text, vision, per_mod = split_plan(cfg)
    print("%s: text prefix %s, vision prefix %s, per-modality embeddings %s" % (args.config, text, vision, per_mod))
    for mode in args.modes.split(","):
        zs = mode == "zeroshot"
        torch.manual_seed(0)
        model = (BertForVLPreTraining(cfg) if zs else BertForVLTasks(cfg, TASK_CFG, list(TASK_CFG))).cuda().eval()
        sc = RetrievalScorer(model, None if zs else "TASK8", pair_chunk=args.pair_chunk)
        warm = min(2, args.captions)
        loop(model, zs, caps, imgs, warm)
        if zs:
            loop(model, zs, caps, imgs, warm, encode_only=True)
        scorer_run(sc, [t[:warm] for t in caps], imgs)
        scorer_run(sc, caps, imgs)
        t_loop = timed(lambda: loop(model, zs, caps, imgs, args.captions))
        t_enc = timed(lambda: loop(model, zs, caps, imgs, args.captions, encode_only=True)) if zs else None
        t_sc = timed(lambda: scorer_run(sc, caps, imgs))
        res = dict(config=args.config, mode=mode, captions=args.captions, images=args.images, T=args.T, regions=args.regions, pair_chunk=args.pair_chunk,
                   loop_s=round(t_loop, 4), scorer_s=round(t_sc, 4), loop_pairs_per_s=round(pairs / t_loop), scorer_pairs_per_s=round(pairs / t_sc),
                   speedup=round(t_loop / t_sc, 3))
        if zs:
            res.update(loop_encode_itm_s=round(t_enc, 4), heads_share_of_loop=round(1.0 - t_enc / t_loop, 4),
                       speedup_vs_encode_itm_loop=round(t_enc / t_sc, 3))
        print(json.dumps(res), flush=True)
        del sc, model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
