"""Writes tests/golden/hard_pool_reference.npz: a small synthetic feature store and the hard-negative pool that the arithmetic of the
reference's scripts/generate_pool.py gives for it -- per image the fp32 mean `features[:num_boxes].sum(0) / num_boxes` stored into a float64
array, then `sklearn.neighbors.BallTree(metric="euclidean").query(k=100)` over those rows.  Runs on the CPU (needs scikit-learn).

    python tools/make_hard_pool_golden.py

Contents: features [sum of num_boxes, F] fp32 (the images' regions one after another), num_boxes [N] int32, image_list [N] int64 (the ids, in
annotation order), means [N, F] fp32, pool [N, 100] int32 (the script stores it as float64; the values are positions in image_list).
The script checks that the pool is also what the (distance, index) order of tests/knn_restate.py gives and prints the smallest relative gap
between neighbouring distances."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import knn_restate as KR  # noqa: E402

N, F, K, MAX_REGIONS = 300, 64, 100, 6


def main():
    from sklearn.neighbors import BallTree
    rng = np.random.default_rng(20240)
    num_boxes = rng.integers(1, MAX_REGIONS + 1, N).astype(np.int32)
    num_boxes[:4] = (1, 2, MAX_REGIONS, MAX_REGIONS)
    # detector-like features: non-negative, a scene vector per group of images plus per-region variation
    scene = np.maximum(rng.standard_normal((12, F)), 0)
    group = rng.integers(0, 12, N)
    feats = [np.maximum(scene[group[i]] + 0.7 * rng.standard_normal((num_boxes[i], F)), 0).astype(np.float32) for i in range(N)]
    image_list = rng.permutation(np.arange(1000, 9000))[:N].astype(np.int64)
    train_image_feature = np.zeros((N, F))                                   # float64, as pymp.shared.array
    for i in range(N):
        train_image_feature[i] = feats[i][:num_boxes[i]].sum(0) / int(num_boxes[i])
    means = train_image_feature.astype(np.float32)
    assert np.array_equal(means.astype(np.float64), train_image_feature)
    kdt = BallTree(train_image_feature, metric="euclidean")
    pool = np.zeros((N, K))
    for i in range(N):
        pool[i] = kdt.query(train_image_feature[i:i + 1], k=K, return_distance=False)
    want = KR.knn(train_image_feature, K)
    assert np.array_equal(pool, want.astype(np.float64)), "BallTree and the (distance, index) order disagree: %d positions" % int((pool != want).sum())
    assert np.array_equal(pool[:, 0], np.arange(N))
    print("min relative gap of neighbouring distances: %.3g" % KR.min_relative_gap(train_image_feature, K))
    path = os.path.join(ROOT, "tests", "golden", "hard_pool_reference.npz")
    np.savez_compressed(path, features=np.concatenate(feats), num_boxes=num_boxes, image_list=image_list, means=means, pool=pool.astype(np.int32))
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
