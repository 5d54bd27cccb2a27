"""`ops.retrieval_ranks_shard` / `retrieval_ranks_shard_counts` / `retrieval_ranks_finish` (csrc/ranks.hip) as a serial simulation of W ranks
on one device: the row call on every shard's slice of one matrix, the target words added, the column call per shard, the counts added, the
finish call.  rank_ir, topk_ir and rank_tr must equal `ops.retrieval_ranks` on the whole matrix, the definition (tests/ranks_restate.py) and
the numpy restatement of the steps (tests/ranks_shard_restate.py), exactly.  GPU only.

Inputs (tests/ranks_shard_restate.py, CASES): 37 x 13 with scores from {-1, 0, 1} and ties across the shard boundaries of W = 2 and 3 with
the target on either side; the same shape with NaN, +-inf, +-0.0 in targets and elsewhere; 41 x 70, two column blocks with a dead lane
tail; 600 x 9, shards of 300 rows (two 256-row blocks) and the uneven split of W = 7.  All of them: an image with 11 captions in three
shards, an image without a caption, captions with an image outside the set; W = Nc + 2 gives empty and one-row shards.  Every case runs
with rows `ld == Ni` apart and as a column slice of a wider tensor at an odd offset (`ld > Ni`, unaligned row starts); K in {0, 20, 64}."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import ranks_restate as RR  # noqa: E402
from tests import ranks_shard_restate as SR  # noqa: E402

TOPKS = [0, 20, 64]


@pytest.fixture(scope="module")
def expected():
    """name -> (S, caption_image, definition at K = 64), computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            S, ci = SR.CASES[name][0]()
            cache[name] = (S, ci, RR.ranks(S, ci, 64))
        return cache[name]
    return get


def _device_scores(S, sliced):
    t = torch.from_numpy(S)
    if not sliced:
        return t.cuda()
    wide = torch.full((S.shape[0], S.shape[1] + 7), float("nan"), dtype=torch.float32)      # NaN around the slice: reading past it would show
    wide[:, 3:3 + S.shape[1]] = t
    return wide.cuda()[:, 3:3 + S.shape[1]]


def _simulate(ops, Sd, cid, W, K):
    """the sequence of evaluate_retrieval(group=...) with the W ranks run one after the other and `+` in place of all_reduce"""
    Nc, Ni = Sd.shape
    shards = [ops.retrieval_ranks_shard(Sd[a:b], a, Nc, cid, topk=K) for a, b in (SR.shard_range(Nc, W, r) for r in range(W))]
    target_key = torch.stack([sh.target_key for sh in shards]).sum(0, dtype=torch.int32)
    count = torch.stack([ops.retrieval_ranks_shard_counts(sh, target_key) for sh in shards]).sum(0, dtype=torch.int32)
    rank_tr = ops.retrieval_ranks_finish(count, shards[0].image_ptr, Ni)
    rank_ir = torch.stack([sh.rank_ir for sh in shards]).sum(0, dtype=torch.int32)
    topk_ir = torch.stack([sh.topk_ir for sh in shards]).sum(0, dtype=torch.int32)
    return rank_ir, topk_ir, rank_tr, shards, count


@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "sliced"])
@pytest.mark.parametrize("name", list(SR.CASES))
def test_simulated_shards_equal_the_whole_matrix(expected, name, sliced):
    from volta_amd import ops
    S, ci, (want_ir, want_top, want_tr) = expected(name)
    Nc, Ni = S.shape
    Sd, cid = _device_scores(S, sliced), torch.from_numpy(ci).cuda()
    if sliced:
        assert Sd.stride(0) == Ni + 7 and Sd.storage_offset() == 3 and any((Sd[a:].data_ptr() & 15) != 0 for a in range(Nc))
    assert want_ir[2] == -1 and want_ir[3] == -1 and want_tr[1] == -1 and int((ci == 4).sum()) == 11
    for K in TOPKS:
        whole = [t.cpu().numpy() for t in ops.retrieval_ranks(Sd, cid, topk=K)]
        for W in SR.CASES[name][1]:
            rank_ir, topk_ir, rank_tr, shards, _ = _simulate(ops, Sd, cid, W, K)
            assert rank_ir.dtype == topk_ir.dtype == rank_tr.dtype == torch.int32
            assert tuple(rank_ir.shape) == (Nc,) and tuple(topk_ir.shape) == (Nc, K) and tuple(rank_tr.shape) == (Ni,)
            got = [rank_ir.cpu().numpy(), topk_ir.cpu().numpy(), rank_tr.cpu().numpy()]
            for g, w, d, what in zip(got, whole, (want_ir, want_top[:, :K], want_tr), ("rank_ir", "topk_ir", "rank_tr")):
                assert np.array_equal(g, w), (K, W, what, "against ops.retrieval_ranks", np.argwhere(g != w)[:8])
                assert np.array_equal(g, d), (K, W, what, "against the definition", np.argwhere(g != d)[:8])
            if K > Ni:
                assert (got[1][:, Ni:] == -1).all()
            if W > Nc:
                assert sorted(sh.nrows for sh in shards)[:2] == [0, 0] and max(sh.nrows for sh in shards) == 1


@pytest.mark.parametrize("name", ["ties_37x13", "special_37x13"])
def test_each_step_equals_its_restatement(expected, name):
    """the parts themselves, not only their merge: what a shard writes and where, and its counts"""
    from volta_amd import ops
    S, ci, _ = expected(name)
    Nc, Ni = S.shape
    Sd, cid = _device_scores(S, True), torch.from_numpy(ci).cuda()
    image_ptr, image_captions = SR.csr(ci, Ni)
    for W in (3, Nc + 2):
        _, _, _, shards, count = _simulate(ops, Sd, cid, W, 20)
        parts = [SR.shard_rows(S[sh.row0:sh.row0 + sh.nrows], sh.row0, Nc, ci, 20) for sh in shards]
        tk_all = sum(p[2] for p in parts)
        for sh, (w_ir, w_top, w_tk) in zip(shards, parts):
            assert np.array_equal(sh.rank_ir.cpu().numpy(), w_ir) and np.array_equal(sh.topk_ir.cpu().numpy(), w_top)
            assert np.array_equal(sh.target_key.cpu().numpy().view(np.uint32), w_tk)
            assert np.array_equal(sh.image_ptr.cpu().numpy(), image_ptr)
            assert np.array_equal(sh.image_captions.cpu().numpy()[:image_ptr[-1]], image_captions)
            got = ops.retrieval_ranks_shard_counts(sh, torch.from_numpy(tk_all.view(np.int32)).cuda()).cpu().numpy()
            assert np.array_equal(got, SR.shard_counts(S[sh.row0:sh.row0 + sh.nrows], sh.row0, tk_all, image_ptr, image_captions, Nc)), (W, sh.row0)
        want = sum(SR.shard_counts(S[sh.row0:sh.row0 + sh.nrows], sh.row0, tk_all, image_ptr, image_captions, Nc) for sh in shards)
        assert np.array_equal(count.cpu().numpy(), want)


def test_accumulate_flag_two_blocks_on_one_device(expected):
    """two local blocks counted into one array give the counts of two shards added, and of the whole matrix as one shard"""
    from volta_amd import ops
    S, ci, _ = expected("ties_37x13")
    Nc, Ni = S.shape
    Sd, cid = _device_scores(S, True), torch.from_numpy(ci).cuda()
    a = ops.retrieval_ranks_shard(Sd[:18], 0, Nc, cid, topk=0)
    b = ops.retrieval_ranks_shard(Sd[18:], 18, Nc, cid, topk=0)
    one = ops.retrieval_ranks_shard(Sd, 0, Nc, cid, topk=0)
    tk = a.target_key + b.target_key
    assert torch.equal(tk, one.target_key)
    separate = ops.retrieval_ranks_shard_counts(a, tk) + ops.retrieval_ranks_shard_counts(b, tk)
    acc = ops.retrieval_ranks_shard_counts(a, tk)
    assert ops.retrieval_ranks_shard_counts(b, tk, out=acc) is acc
    assert torch.equal(acc, separate) and torch.equal(acc, ops.retrieval_ranks_shard_counts(one, tk))
    again = torch.full((Nc,), 77, dtype=torch.int32, device="cuda")               # `out` is added to, a fresh array is cleared by the call
    fresh = ops.retrieval_ranks_shard_counts(a, tk)
    ops.retrieval_ranks_shard_counts(a, tk, out=again)
    assert torch.equal(again - 77, fresh)


def test_an_empty_shard_writes_nothing(expected):
    from volta_amd import _lib as L
    from volta_amd import ops
    S, ci, _ = expected("ties_37x13")
    Nc, Ni = S.shape
    Sd, cid = _device_scores(S, False), torch.from_numpy(ci).cuda()
    sh = ops.retrieval_ranks_shard(Sd[5:5], 5, Nc, cid, topk=20)
    assert sh.nrows == 0 and not sh.rank_ir.any() and not sh.topk_ir.any() and not sh.target_key.any()
    for t in (sh.rank_ir, sh.topk_ir, sh.target_key):                             # the call itself on buffers that are not zero
        t.fill_(-9)
    a = sh.args(caption_image=L.ptr(cid), rank_ir=L.ptr(sh.rank_ir), topk_ir=L.ptr(sh.topk_ir), target_key=L.ptr(sh.target_key))
    L.check(L.lib.vk_retrieval_ranks_shard_rows(ctypes.byref(a), L.stream_ptr()))
    assert (sh.rank_ir == -9).all() and (sh.topk_ir == -9).all() and (sh.target_key == -9).all()
    tk = torch.zeros(Nc, dtype=torch.int32, device="cuda")
    kept = torch.full((Nc,), 5, dtype=torch.int32, device="cuda")
    ops.retrieval_ranks_shard_counts(sh, tk, out=kept)
    assert (kept == 5).all() and not ops.retrieval_ranks_shard_counts(sh, tk).any()     # accumulate: untouched; otherwise cleared


def test_two_runs_give_identical_bytes(expected):
    from volta_amd import ops
    S, ci, _ = expected("deep_600x9")
    Sd, cid = _device_scores(S, True), torch.from_numpy(ci).cuda()
    a = [t.cpu().numpy().tobytes() for t in _simulate(ops, Sd, cid, 7, 20)[:3]]
    b = [t.cpu().numpy().tobytes() for t in _simulate(ops, Sd, cid, 7, 20)[:3]]
    assert a == b


def test_wrappers_refuse_what_the_kernels_cannot_read():
    from volta_amd import _lib as L
    from volta_amd import ops
    S, ci = torch.zeros(4, 6, device="cuda"), torch.zeros(9, dtype=torch.int32, device="cuda")
    with pytest.raises(AssertionError):
        ops.retrieval_ranks_shard(S.t()[:, :4], 0, 9, ci)                          # columns are not adjacent
    with pytest.raises(AssertionError):
        ops.retrieval_ranks_shard(S, 6, 9, ci)                                     # rows 6..9 of 9 captions
    with pytest.raises(AssertionError):
        ops.retrieval_ranks_shard(S, -1, 9, ci)
    with pytest.raises(AssertionError):
        ops.retrieval_ranks_shard(S, 0, 9, ci.long())
    with pytest.raises(AssertionError):
        ops.retrieval_ranks_shard(S.double(), 0, 9, ci)
    with pytest.raises(L.VoltaHipError, match="vk_retrieval_ranks_shard_rows: top-k of 65"):
        ops.retrieval_ranks_shard(S, 0, 9, ci, topk=65)
    sh = ops.retrieval_ranks_shard(S, 2, 9, ci, topk=3)
    with pytest.raises(AssertionError):
        ops.retrieval_ranks_shard_counts(sh, sh.target_key[:5])
    with pytest.raises(AssertionError):
        ops.retrieval_ranks_shard_counts(sh, sh.target_key.long())
    with pytest.raises(AssertionError):
        ops.retrieval_ranks_finish(torch.zeros(9, dtype=torch.int32, device="cuda"), sh.image_ptr, 5)
