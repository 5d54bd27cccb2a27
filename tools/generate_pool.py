"""Writes the `hard_negative.pkl` that `RetrievalDataset(split="train")` reads: per training image its k nearest training images by mean region
feature (the product of the reference's scripts/generate_pool.py; volta_amd.retrieval.generate_hard_pool).

    python tools/generate_pool.py --features_h5path data/flickr30k/resnet101_faster_rcnn_genome_imgfeats/volta/flickr30k_feat.lmdb \\
        --annotations_jsonpath data/flickr30k/annotations/train_ann.jsonl --task RetrievalFlickr30k

`--out` defaults to hard_negative.pkl beside the annotation file."""
import argparse
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--features_h5path", required=True, help="the LMDB feature store (file, or directory holding data.mdb)")
    ap.add_argument("--annotations_jsonpath", required=True, help="training annotations, one JSON object per line")
    ap.add_argument("--task", default="RetrievalFlickr30k", choices=["RetrievalFlickr30k", "RetrievalCOCO"])
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--out", default=None, help="output pickle (default: hard_negative.pkl beside the annotations)")
    ap.add_argument("--feature_size", type=int, default=2048)
    ap.add_argument("--chunk", type=int, default=256, help="images decoded and reduced per step")
    args = ap.parse_args(argv)
    from volta_amd.readers import ImageFeaturesH5Reader
    from volta_amd.retrieval import generate_hard_pool
    reader = ImageFeaturesH5Reader(args.features_h5path, types.SimpleNamespace(v_feature_size=args.feature_size, num_locs=5, add_global_imgfeat=None))
    t0 = time.time()
    res = generate_hard_pool(reader, args.annotations_jsonpath, args.task, k=args.k, out=args.out if args.out else True, chunk=args.chunk)
    path = args.out or os.path.join(os.path.dirname(os.path.abspath(args.annotations_jsonpath)), "hard_negative.pkl")
    print("%d images, %d neighbours each, %.1f s -> %s" % (len(res["train_image_list"]), res["train_hard_pool"].shape[1], time.time() - t0, path))


if __name__ == "__main__":
    main()
