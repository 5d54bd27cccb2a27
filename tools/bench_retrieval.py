"""Retrieval scoring throughput: the reference driver's loop (eval_retrieval.py:168-198: per caption, two `model(...)` calls on 500 pairs --
the caption repeated, 500 images -- each followed by `.cpu()`) against volta_amd.retrieval.RetrievalScorer (image encoding once, caption
encoding, score_matrix; one `.cpu()` at the end), on random weights, in VL-logit and zero-shot mode.  In zero-shot mode the loop also pays for
the [B, T, 30522] MLM and region scores that BertForVLPreTraining's score branch computes and the driver throws away; the scorer skips them.
That share is reported on its own ("heads"): the loop's time minus the same loop over `encode()` + the ITM linear, so it is not credited to
the prefix reuse.  Timed with torch.cuda.Event after one warm-up pass over a few captions (every shape of the timed window).
usage: python tools/bench_retrieval.py --config ctrl_vilbert_base [--captions 64] [--images 1000] [--modes logit,zeroshot] [--dtype bf16|fp8|both]

--dtype fp8: the same comparison with the projections on the e4m3 path on both sides (the model after set_projection_dtype("fp8") in the
loop, RetrievalScorer(projection_dtype="fp8")).
--dtype both: no driver loop.  One model, a bf16 and an fp8 scorer on it; after a warm-up call of each, `--reps` timed calls of each, the two
alternating call by call, every call split into three phases that are timed apart between device synchronisations: encode (captions and
images), the pair gathers alone (the vk_pair_gather launches of score_matrix without the suffix lists) and score_matrix.  Per precision:
median, minimum and maximum of each phase, pairs/s from the median score_matrix time, and the gathers' share of it."""
import argparse
import json
import os
import statistics
import sys
import time

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


def wall(fn):
    """seconds of fn between two device synchronisations, and its result"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def gathers_only(sc, c, i):
    with torch.no_grad():
        for c0, nc, i0, ni in sc._matrix_blocks(c.n, i.n):
            sc._gather_pairs(c, i, nc * ni, cross=(c0, nc, i0, ni))


def gather_bytes(sc):
    """bytes one pair's segments take in a vk_pair_gather launch"""
    a = next(e for k, e in sc._engines.items() if k[0] == "pair").pair_args
    return sum(int(a.bytes[k]) for k in range(a.nseg))


def both(args, cfg, caps, imgs, mode):
    """bf16 against fp8 scorer on one model, alternated timed calls"""
    zs = mode == "zeroshot"
    torch.manual_seed(0)
    model = (BertForVLPreTraining(cfg) if zs else BertForVLTasks(cfg, TASK_CFG, list(TASK_CFG))).cuda().eval()
    scorers = {d: RetrievalScorer(model, None if zs else "TASK8", pair_chunk=args.pair_chunk, projection_dtype=d) for d in ("bf16", "fp8")}
    encode = lambda sc: (sc.encode_captions(*caps), sc.encode_images(*imgs))
    times = {d: dict(encode=[], gather=[], score=[]) for d in scorers}
    for rep in range(-1, args.reps):                       # call -1 builds the plans and warms up: not recorded
        for d, sc in scorers.items():
            t_enc, (c, i) = wall(lambda: encode(sc))
            t_gat, _ = wall(lambda: gathers_only(sc, c, i))
            t_sc, S = wall(lambda: sc.score_matrix(c, i))
            if rep >= 0:
                for k, t in (("encode", t_enc), ("gather", t_gat), ("score", t_sc)):
                    times[d][k].append(t)
    pairs = args.captions * args.images
    res = dict(config=args.config, mode=mode, captions=args.captions, images=args.images, T=args.T, regions=args.regions, pair_chunk=args.pair_chunk, reps=args.reps)
    for d in scorers:
        med = {k: statistics.median(v) for k, v in times[d].items()}
        res[d] = dict({k + "_s": [round(med[k], 5), round(min(v), 5), round(max(v), 5)] for k, v in times[d].items()},
                      pairs_per_s=round(pairs / med["score"]), gather_share=round(med["gather"] / med["score"], 4),
                      gather_bytes_per_pair=gather_bytes(scorers[d]))
    res["fp8_over_bf16"] = round(res["fp8"]["pairs_per_s"] / res["bf16"]["pairs_per_s"], 4)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="ctrl_vilbert_base")
    ap.add_argument("--captions", type=int, default=64)
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--T", type=int, default=38)
    ap.add_argument("--regions", type=int, default=37, help="rows per image, the global feature included")
    ap.add_argument("--pair-chunk", type=int, default=1000)
    ap.add_argument("--modes", default="logit,zeroshot")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp8", "both"], help="projection precision; both: bf16 against fp8 scorer, no driver loop")
    ap.add_argument("--reps", type=int, default=7, help="--dtype both: timed calls per precision")
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = BertConfig.from_json_file(os.path.join(root, "config", args.config + ".json"))
    caps, imgs = inputs(cfg, args.captions, args.images, args.T, args.regions)
    pairs = args.captions * args.images
    text, vision, per_mod = split_plan(cfg)
    print("%s: text prefix %s, vision prefix %s, per-modality embeddings %s" % (args.config, text, vision, per_mod))
    for mode in args.modes.split(","):
        if args.dtype == "both":
            both(args, cfg, caps, imgs, mode)
            torch.cuda.empty_cache()
            continue
        zs = mode == "zeroshot"
        torch.manual_seed(0)
        model = (BertForVLPreTraining(cfg) if zs else BertForVLTasks(cfg, TASK_CFG, list(TASK_CFG))).cuda().eval()
        model.set_projection_dtype(args.dtype)
        sc = RetrievalScorer(model, None if zs else "TASK8", pair_chunk=args.pair_chunk, projection_dtype=args.dtype)
        warm = min(2, args.captions)
        loop(model, zs, caps, imgs, warm)
        if zs:
            loop(model, zs, caps, imgs, warm, encode_only=True)
        scorer_run(sc, [t[:warm] for t in caps], imgs)
        scorer_run(sc, caps, imgs)
        t_loop = timed(lambda: loop(model, zs, caps, imgs, args.captions))
        t_enc = timed(lambda: loop(model, zs, caps, imgs, args.captions, encode_only=True)) if zs else None
        t_sc = timed(lambda: scorer_run(sc, caps, imgs))
        res = dict(config=args.config, mode=mode, dtype=args.dtype, captions=args.captions, images=args.images, T=args.T, regions=args.regions, pair_chunk=args.pair_chunk,
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
