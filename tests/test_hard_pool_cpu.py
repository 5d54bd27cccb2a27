"""The hard-negative pool on the host: the golden fixture (tests/golden/hard_pool_reference.npz, written by tools/make_hard_pool_golden.py with
the arithmetic of the reference's scripts/generate_pool.py and sklearn's BallTree) against the float64 restatement of tests/knn_restate.py,
argument checks of `ops.knn_pool` / `generate_hard_pool`, and the C boundary of `vk_knn_pool` / `vk_image_means`.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import knn_restate as KR  # noqa: E402
from tests.hard_pool_fixture import PoolFixture, golden  # noqa: E402


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    return PoolFixture(tmp_path_factory.mktemp("hard_pool"))


def test_golden_pool_equals_the_restatement():
    z = golden()
    N = len(z["image_list"])
    assert z["pool"].shape == (N, 100) and z["means"].dtype == np.float32 and len(set(z["image_list"].tolist())) == N
    want, gap = KR.knn(z["means"], 100, return_gap=True)
    assert gap > 1e-10
    assert np.array_equal(z["pool"], want)
    assert np.array_equal(z["pool"][:, 0], np.arange(N))                 # no duplicate image in the fixture: every row starts with itself


def test_golden_means_equal_numpy_sum_over_regions():
    z = golden()
    ends = np.cumsum(z["num_boxes"])
    assert z["num_boxes"].min() == 1 and ends[-1] == z["features"].shape[0]
    for i, (e, n) in enumerate(zip(ends, z["num_boxes"])):
        f = z["features"][e - n:e]
        assert np.array_equal(z["means"][i], np.sum(f, 0) / int(n)), i
    Rcap = int(z["num_boxes"].max())
    feat = np.full((4, Rcap, z["features"].shape[1]), np.nan, np.float32)
    for s in range(4):
        feat[s, :z["num_boxes"][s]] = z["features"][ends[s] - z["num_boxes"][s]:ends[s]]
    assert np.array_equal(KR.image_means(feat, z["num_boxes"][:4]), z["means"][:4])


def test_reader_row_zero_is_the_golden_mean(fx):
    reader = fx.reader("first")
    for pos in (0, 1, 2, 3, 150, fx.N - 1):
        assert np.array_equal(reader[fx.image_list[pos]][0][0], fx.z["means"][pos])


def test_restatement_order_rules():
    X = np.asarray([[0, 0], [3, 4], [0, 0], [3, 4], [1, 0]], np.float32)
    assert KR.knn(X, 5).tolist() == [[0, 2, 4, 1, 3], [1, 3, 4, 0, 2], [0, 2, 4, 1, 3], [1, 3, 4, 0, 2], [4, 0, 2, 1, 3]]
    assert KR.min_relative_gap(X, 4) == pytest.approx((20 - 16) / 20)
    with pytest.raises(ValueError):
        KR.knn(X, 6)


def test_knn_pool_refuses_bad_arguments_by_name():
    from volta_amd import ops
    X = torch.zeros(10, 4)
    with pytest.raises(ValueError, match="k = 11 neighbours of N = 10"):
        ops.knn_pool(X, 11)
    with pytest.raises(ValueError, match="k = 0"):
        ops.knn_pool(X, 0)
    with pytest.raises(ValueError, match="shortlist = 4"):
        ops.knn_pool(X, 5, shortlist=4)
    with pytest.raises(ValueError, match="shortlist = 257"):
        ops.knn_pool(X, 5, shortlist=257)
    with pytest.raises(AssertionError, match="fp32"):
        ops.knn_pool(X.double(), 5)
    with pytest.raises(AssertionError, match="contiguous"):
        ops.knn_pool(torch.zeros(4, 10).t(), 5)
    with pytest.raises(AssertionError, match=r"\[N, D\]"):
        ops.knn_pool(torch.zeros(10), 5)
    with pytest.raises(AssertionError, match="cuda"):
        ops.knn_pool(X, 5)
    with pytest.raises(AssertionError, match="cuda"):
        ops.image_means(torch.zeros(2, 3, 4), torch.ones(2, dtype=torch.int32))
    with pytest.raises(AssertionError, match="int32"):
        ops.image_means(torch.zeros(2, 3, 4), torch.ones(2, dtype=torch.int64))
    assert ops.knn_default_shortlist(100) == 128 and ops.knn_default_shortlist(1) == 2 and ops.knn_default_shortlist(250) == 256


def test_generate_hard_pool_refuses_bad_arguments_by_name(fx):
    from volta_amd.retrieval import generate_hard_pool, train_image_list
    for task in ("RetrievalFlickr30k", "RetrievalCOCO"):
        assert train_image_list(fx.jsonpath(task), task) == fx.image_list
    with pytest.raises(ValueError, match="k = 301 neighbours of 300 training images"):
        generate_hard_pool(None, fx.jsonpath("RetrievalCOCO"), "RetrievalCOCO", k=fx.N + 1)
    with pytest.raises(ValueError, match="k = 0"):
        generate_hard_pool(None, fx.jsonpath("RetrievalCOCO"), "RetrievalCOCO", k=0)
    with pytest.raises(ValueError, match="RetrievalFlickr30k or RetrievalCOCO"):
        generate_hard_pool(None, fx.jsonpath("RetrievalCOCO"), "VQA")
    with pytest.raises(ValueError, match="out"):
        generate_hard_pool(None, fx.jsonpath("RetrievalCOCO"), "RetrievalCOCO", out=3)
    assert not os.path.exists(os.path.join(fx.root, "hard_negative.pkl"))


# ------------------------------------------------------------------------------------------------ the C boundary
def test_entries_are_exported_and_declared():
    from volta_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "volta_hip.h")).read(), flags=re.S)
    for name in ("vk_knn_pool", "vk_knn_pool_work_bytes", "vk_image_means"):
        assert name in L.EXPORTS and hasattr(L.lib, name)
    assert re.search(r"\bint\s+vk_knn_pool\s*\(\s*const\s+vk_knn_pool_args\s*\*", text)
    assert re.search(r"\bint\s+vk_image_means\s*\(\s*const\s+vk_image_means_args\s*\*", text)
    assert "#define VK_KNN_MAX_SHORTLIST %d" % L.KNN_MAX_SHORTLIST in text and "#define VK_KNN_SCREEN_ONLY %d" % L.KNN_SCREEN_ONLY in text


@pytest.mark.parametrize("name", ["vk_knn_pool_args", "vk_image_means_args"])
def test_struct_layouts_match_the_header(tmp_path, name):
    from volta_amd import _lib as L
    mirror = {"vk_knn_pool_args": L.KnnPoolArgs, "vk_image_means_args": L.ImageMeansArgs}[name]
    fields = [n for n, _ in mirror._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "volta_hip.h"\nint main(void){printf("%%zu\\n", sizeof(%s));' % name + "".join(
        'printf("%%zu\\n", offsetof(%s, %s));' % (name, n) for n in fields) + "return 0;}"
    c, exe = str(tmp_path / "s.c"), str(tmp_path / "s")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert ctypes.sizeof(mirror) == out[0]
    assert [getattr(mirror, n).offset for n in fields] == out[1:]


def test_knn_pool_host_validation_errors_without_gpu():
    """argument checks happen on the host before any launch and report through vk_last_error()"""
    from volta_amd import _lib as L
    buf = (ctypes.c_int32 * 1024)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)

    def call(**kw):
        v = dict(X=p, out=p, work=p, stats=p, work_bytes=1 << 40, N=50, D=8, k=5, M=8, flags=0, reserved_=0)
        v.update(kw)
        a = L.KnnPoolArgs(*[v[n] for n, _ in L.KnnPoolArgs._fields_])
        rc = L.lib.vk_knn_pool(ctypes.byref(a), None)
        return rc, L.lib.vk_last_error().decode()

    for name in ("X", "out", "work", "stats"):
        rc, msg = call(**{name: None})
        assert rc != 0 and "null pointer" in msg, name
    assert L.lib.vk_knn_pool(None, None) != 0 and "null argument struct" in L.lib.vk_last_error().decode()
    rc, msg = call(k=0)
    assert rc != 0 and "k = 0 neighbours" in msg
    rc, msg = call(k=51)
    assert rc != 0 and "k = 51 neighbours of N = 50" in msg
    rc, msg = call(M=4)
    assert rc != 0 and "shortlist M = 4" in msg and "k = 5 <= M" in msg
    for M in (257, 51):
        rc, msg = call(M=M)
        assert rc != 0 and "shortlist M = %d" % M in msg
    for kw in (dict(N=0), dict(D=0), dict(N=-1)):
        rc, msg = call(**kw)
        assert rc != 0 and "must be positive" in msg, kw
    rc, msg = call(work_bytes=16)
    assert rc != 0 and "work_bytes = 16" in msg
    rc, msg = call(work=ctypes.c_void_p(p.value + 8))
    assert rc != 0 and "256-byte aligned" in msg
    rc, msg = call(flags=6)
    assert rc != 0 and "unknown flags" in msg
    assert L.lib.vk_knn_pool_work_bytes(50, 8, 5, 4) == -1 and L.lib.vk_knn_pool_work_bytes(50, 8, 5, 8) > 50 * 8 * 8
    # O(N M) + one slab of KNN_FB rows: far from N x N x D
    assert L.lib.vk_knn_pool_work_bytes(113287, 2048, 100, 128) < 1 << 29
    with pytest.raises(L.VoltaHipError, match="shortlist"):
        L.check(call(M=4)[0])


def test_image_means_host_validation_errors_without_gpu():
    from volta_amd import _lib as L
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(**kw):
        v = dict(feat=p, n=p, mean=p, S=2, Rcap=3, F=4, reserved_=0)
        v.update(kw)
        a = L.ImageMeansArgs(*[v[n] for n, _ in L.ImageMeansArgs._fields_])
        rc = L.lib.vk_image_means(ctypes.byref(a), None)
        return rc, L.lib.vk_last_error().decode()

    for name in ("feat", "n", "mean"):
        rc, msg = call(**{name: None})
        assert rc != 0 and "null pointer" in msg, name
    for kw in (dict(Rcap=0), dict(F=0), dict(S=-1)):
        rc, msg = call(**kw)
        assert rc != 0 and "vk_image_means: S =" in msg, kw
    assert L.lib.vk_image_means(None, None) != 0
    assert call(S=0)[0] == 0                                            # nothing to do, nothing launched
