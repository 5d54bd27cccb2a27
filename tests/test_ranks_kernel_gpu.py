"""`ops.retrieval_ranks` (csrc/ranks.hip) against the numpy restatement of its contract (tests/ranks_restate.py), exact equality of every
integer output.  GPU only.

The (Nc, Ni) shapes are the smallest at which each mechanism can break: (1, 1); (7, 5) less than a wave and top-k past Ni; (70, 64) exactly one
wave; (130, 257) odd Ni -- unaligned rows, a tail after the 16-byte part; (300, 1031) more than one element per lane and a ragged tail;
(64, 9001) a row longer than the 8192 elements a workgroup keeps in LDS; (2100, 100) columns deeper than one workgroup's 256 rows.  Each
with scores that are untied (rows `ld == Ni` apart), drawn from four values so that nearly everything ties, and holding NaN, +-inf and
+-0.0 (both as a column slice of a wider tensor, `ld > Ni`, starting at an odd column); K in {0, 1, 20, 64}; targets at index 0 and
Ni - 1, an image without a caption, an image owning 70 captions (the shapes with at least 74 captions: four captions are spoken for),
caption_image entries outside [0, Ni)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import ranks_restate as RR  # noqa: E402

SHAPES = [(1, 1), (7, 5), (70, 64), (130, 257), (300, 1031), (64, 9001), (2100, 100)]
KINDS = ["untied", "four_values", "special"]
TOPKS = [0, 1, 20, 64]


def _inputs(Nc, Ni, kind, seed):
    """-> S (numpy fp32 [Nc, Ni]), caption_image (numpy int32 [Nc]), what the caption table holds"""
    rng = np.random.default_rng(seed)
    if kind == "untied":
        S = rng.standard_normal((Nc, Ni)).astype(np.float32)
    elif kind == "four_values":
        S = rng.choice(np.asarray([-1.5, 0.25, 0.25 + 2.0 ** -20, 3.0], np.float32), size=(Nc, Ni))
    else:
        S = rng.standard_normal((Nc, Ni)).astype(np.float32)
        special = np.asarray([np.nan, np.inf, -np.inf, 0.0, -0.0, -np.nan], np.float32)
        hit = rng.random((Nc, Ni)) < 0.3
        S[hit] = rng.choice(special, size=int(hit.sum()))
        S[0, :] = np.nan if Nc > 1 else S[0, :]                          # a row of nothing but NaN: ordered by index
    ci = rng.integers(0, Ni, size=Nc).astype(np.int32)
    has = dict(first=False, last=False, empty_image=False, crowded=False, outside=False)
    if Ni > 2:                                                           # image 1 has no caption
        ci[ci == 1] = 2
        has["empty_image"] = True
    if Nc >= 74 and Ni > 3:                                              # image 3 owns 70 captions (more than one register chunk),
        ci[ci == 3] = 2                                                  # none of them among captions 0..3, which are set below
        ci[4 + rng.permutation(Nc - 4)[:70]] = 3
        has["crowded"] = True
    ci[0], has["first"] = 0, True
    if Nc > 1:
        ci[1], has["last"] = Ni - 1, True
    if Nc > 3:
        ci[2], ci[3], has["outside"] = Ni, -5, True
    return np.ascontiguousarray(S.astype(np.float32)), ci, has


@pytest.fixture(scope="module")
def expected():
    cache = {}

    def get(Nc, Ni, kind):
        key = (Nc, Ni, kind)
        if key not in cache:
            S, ci, has = _inputs(Nc, Ni, kind, seed=17 * Nc + Ni)
            cache[key] = (S, ci, has, RR.ranks(S, ci, 64))
        return cache[key]
    return get


def _device_scores(S, sliced):
    t = torch.from_numpy(S)
    if not sliced:
        return t.cuda()
    wide = torch.full((S.shape[0], S.shape[1] + 7), float("nan"), dtype=torch.float32)      # NaN around the slice: reading past it would show
    wide[:, 3:3 + S.shape[1]] = t
    return wide.cuda()[:, 3:3 + S.shape[1]]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_ranks_equal_the_restatement(expected, shape, kind):
    from volta_amd import ops
    Nc, Ni = shape
    S, ci, has, (want_ir, want_top, want_tr) = expected(Nc, Ni, kind)
    Sd, cid = _device_scores(S, sliced=kind != "untied"), torch.from_numpy(ci).cuda()
    assert (Sd.stride(0) > Ni) == (kind != "untied")
    if has["outside"]:
        assert want_ir[2] == -1 and want_ir[3] == -1
    if has["empty_image"]:
        assert want_tr[1] == -1
    if has["crowded"]:
        assert int((ci == 3).sum()) == 70
    assert ci[0] == 0 and (Nc == 1 or ci[1] == Ni - 1)
    for K in TOPKS:
        rank_ir, topk_ir, rank_tr = ops.retrieval_ranks(Sd, cid, topk=K)
        assert rank_ir.dtype == topk_ir.dtype == rank_tr.dtype == torch.int32 and rank_ir.is_cuda and topk_ir.is_cuda and rank_tr.is_cuda
        assert tuple(rank_ir.shape) == (Nc,) and tuple(topk_ir.shape) == (Nc, K) and tuple(rank_tr.shape) == (Ni,)
        got_ir, got_top, got_tr = rank_ir.cpu().numpy(), topk_ir.cpu().numpy(), rank_tr.cpu().numpy()
        assert np.array_equal(got_ir, want_ir), (K, np.flatnonzero(got_ir != want_ir)[:8])
        assert np.array_equal(got_tr, want_tr), (K, np.flatnonzero(got_tr != want_tr)[:8])
        assert np.array_equal(got_top, want_top[:, :K]), (K, np.argwhere(got_top != want_top[:, :K])[:8])
        if K > Ni:
            assert (got_top[:, Ni:] == -1).all()


def test_two_calls_give_identical_bytes(expected):
    from volta_amd import ops
    S, ci, _, _ = expected(300, 1031, "four_values")
    Sd, cid = _device_scores(S, sliced=True), torch.from_numpy(ci).cuda()
    a = [t.cpu().numpy().tobytes() for t in ops.retrieval_ranks(Sd, cid, topk=20)]
    b = [t.cpu().numpy().tobytes() for t in ops.retrieval_ranks(Sd, cid, topk=20)]
    assert a == b


def test_wrapper_refuses_what_the_kernel_cannot_read():
    from volta_amd import _lib as L
    from volta_amd import ops
    S, ci = torch.zeros(4, 6, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    with pytest.raises(AssertionError):
        ops.retrieval_ranks(S.t(), torch.zeros(6, dtype=torch.int32, device="cuda"))      # columns are not adjacent
    with pytest.raises(AssertionError):
        ops.retrieval_ranks(S, ci.long())
    with pytest.raises(AssertionError):
        ops.retrieval_ranks(S.double(), ci)
    with pytest.raises(L.VoltaHipError, match="top-k of 65"):
        ops.retrieval_ranks(S, ci, topk=65)
