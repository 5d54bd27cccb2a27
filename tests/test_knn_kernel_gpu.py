"""`vk_knn_pool` and `vk_image_means` (csrc/knn.hip) on the GPU against tests/knn_restate.py.  Every nearest-neighbour case first asserts its
own precondition on the CPU -- consecutive float64 distances among a row's first k + 1 are exactly equal or more than 1e-10 apart (relative;
summation-order noise is about 2e-13 at D = 2048) -- and then demands equality of the whole index matrix: no tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import knn_restate as KR  # noqa: E402

pytestmark = pytest.mark.gpu


def _gauss():
    return np.random.default_rng(0).standard_normal((1000, 64))


def _relu():
    rng = np.random.default_rng(0)
    return np.maximum(rng.standard_normal((777, 2048)), 0).cumsum(0)[rng.permutation(777)] / 50


def _cluster():
    rng = np.random.default_rng(0)
    return 10 + rng.standard_normal((1, 256)) + 1e-3 * rng.standard_normal((513, 256))


def _ties():
    X = np.random.default_rng(0).integers(0, 3, (300, 8)).astype(np.float64)
    X[[7, 19, 250]] = X[3]
    return X


def _edge(N, D):
    return lambda: np.random.default_rng(0).standard_normal((N, D))


# name -> (input, k, shortlist)
CASES = {
    "gauss": (_gauss, 100, None),
    "relu": (_relu, 100, None),
    "cluster": (_cluster, 100, None),
    "no_margin": (_gauss, 100, 100),
    "ties": (_ties, 100, None),
    "edge_1_1": (_edge(1, 5), 1, None),
    "edge_2_2": (_edge(2, 3), 2, None),
    "edge_100_100": (_edge(100, 16), 100, None),
    "edge_257_37_5": (_edge(257, 37), 5, None),
    "edge_65_4_65": (_edge(65, 4), 65, None),
}
_REF = {}


def _reference(name):
    """(X fp32, expected indices, smallest relative gap), computed once per input"""
    make, k, _ = CASES[name]
    key = (make.__name__ if not name.startswith("edge") else name, k)
    if key not in _REF:
        X = np.ascontiguousarray(make().astype(np.float32))
        want, gap = KR.knn(X, k, return_gap=True)
        _REF[key] = (X, want, gap)
    return _REF[key]


@pytest.mark.parametrize("name", list(CASES))
def test_knn_pool_equals_the_float64_restatement(name):
    from volta_amd import ops
    _, k, shortlist = CASES[name]
    X, want, gap = _reference(name)
    N = X.shape[0]
    print("%s: N = %d, D = %d, k = %d, smallest relative gap %.3g" % (name, N, X.shape[1], k, gap))
    assert gap > 1e-10, "the input has near-ties that float64 summation order could flip"
    Xd = torch.from_numpy(X).cuda()
    got, stats = ops.knn_pool(Xd, k, shortlist=shortlist, return_stats=True)
    torch.cuda.synchronize()
    print("%s: certified %d, fallback %d" % (name, stats["certified"], stats["fallback"]))
    assert got.dtype == torch.int32 and tuple(got.shape) == (N, k)
    assert stats["certified"] + stats["fallback"] == N
    got = got.cpu().numpy()
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, "%d rows differ, first %d: got %s, want %s" % (bad.size, bad[0], got[bad[0]][:12], want[bad[0]][:12])
    if name == "gauss":
        assert stats["certified"] == N                                  # the bound is ~5e-4 against gaps of order 1
    if name in ("cluster", "no_margin"):
        assert stats["fallback"] > 0                                    # the screen is blind / has no margin: the float64 path answers
    if name == "ties":
        assert want[3][:4].tolist() == [3, 7, 19, 250] and want[250][:4].tolist() == [3, 7, 19, 250]    # a duplicate with a lower index precedes the row itself
    again, stats2 = ops.knn_pool(Xd, k, shortlist=shortlist, return_stats=True)
    assert torch.equal(again.cpu(), torch.from_numpy(got)) and stats2 == stats


def test_knn_pool_refuses_non_finite_input():
    from volta_amd import ops
    X = torch.randn(40, 8, device="cuda")
    X[17, 3] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        ops.knn_pool(X, 5)
    X[17, 3] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        ops.knn_pool(X, 5)


@pytest.mark.parametrize("F", [64, 2048])
def test_image_means_equal_numpy_bit_for_bit(F):
    from volta_amd import ops
    rng = np.random.default_rng(F)
    n = np.asarray([1, 2, 36, 37, 100], np.int32)
    Rcap = 101
    feat = np.full((5, Rcap, F), np.nan, np.float32)
    for s in range(5):
        feat[s, :n[s]] = np.maximum(rng.standard_normal((n[s], F)), 0).astype(np.float32) * rng.uniform(0.1, 30)
    want = np.stack([np.sum(feat[s, :n[s]], 0) / int(n[s]) for s in range(5)])
    assert want.dtype == np.float32 and np.isfinite(want).all()
    got = ops.image_means(torch.from_numpy(feat).cuda(), torch.from_numpy(n).cuda()).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (5, F)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
