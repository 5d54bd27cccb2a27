"""Numpy float64 restatement of `vk_knn_pool` (csrc/knn.hip): per row the first k indices under the total order (squared Euclidean distance
in float64 ascending, then index ascending); the row itself is a candidate.  The yardstick of tests/test_knn_kernel_gpu.py and
tests/test_hard_pool_*.py."""
import numpy as np


def distances(X, i):
    X = np.asarray(X, np.float64)
    return ((X - X[i]) ** 2).sum(-1)


def knn(X, k, return_gap=False):
    """int32 [N, k]; with `return_gap` also the smallest relative difference between consecutive unequal distances among each row's first
    k + 1 (inf when there is none): what a test asserts about its own input before it demands equality"""
    X = np.asarray(X, np.float64)
    N = X.shape[0]
    if not 1 <= k <= N:
        raise ValueError("k = %d neighbours of N = %d vectors" % (k, N))
    idx = np.arange(N)
    out, worst = np.empty((N, k), np.int32), np.inf
    for i in range(N):
        d = distances(X, i)
        order = np.lexsort((idx, d))
        out[i] = order[:k]
        head = d[order[:min(k + 1, N)]]
        lo, hi = head[:-1], head[1:]
        differ = hi != lo
        if differ.any():
            worst = min(worst, float(((hi - lo)[differ] / hi[differ]).min()))
    return (out, worst) if return_gap else out


def min_relative_gap(X, k):
    return knn(X, k, True)[1]


def image_means(feat, n):
    """np.sum(features, 0) / num_boxes per image, fp32: feat [S, Rcap, F], n [S]"""
    return np.stack([np.sum(feat[s, :n[s]], 0) / int(n[s]) for s in range(feat.shape[0])]).astype(np.float32)
