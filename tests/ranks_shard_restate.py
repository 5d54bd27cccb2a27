"""numpy restatement of the sharded rank calls (include/volta_hip.h: vk_retrieval_ranks_shard_rows / _shard_cols / _finish, csrc/ranks.hip)
and the inputs that the CPU and GPU tests of those calls share.

A shard owns the captions [row0, row0 + nrows) and sees their rows of the score matrix only.  `shard_rows` is row-local and writes at
global positions; `shard_counts` counts the shard's rows against the targets of all captions, comparing (sortable word, GLOBAL caption
index); `finish` takes the minimum per image over the SUM of the shards' counts.  `merged` runs the sequence for W shards.  The key order is
restated from the header -- sortable words, not np.argsort -- so tests/test_ranks_shard_cpu.py can hold it against the definition
(tests/ranks_restate.py)."""
import numpy as np


def sortable(s):
    """fp32 -> uint32, monotone, -0.0 == +0.0, every NaN lowest"""
    u = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32)
    mag = u & np.uint32(0x7FFFFFFF)
    out = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    out = np.where(mag == 0, np.uint32(0x80000000), out)
    return np.where(mag > np.uint32(0x7F800000), np.uint32(0), out).astype(np.uint32)


def shard_range(Nc, W, r):
    return r * Nc // W, (r + 1) * Nc // W


def csr(caption_image, Ni):
    """captions of each image, captions with an image outside [0, Ni) left out -> image_ptr [Ni + 1], image_captions [entries]"""
    ci = np.asarray(caption_image)
    image_captions = [c for i in range(Ni) for c in np.flatnonzero(ci == i)]
    image_ptr = np.concatenate([[0], np.cumsum([(ci == i).sum() for i in range(Ni)])])
    return image_ptr.astype(np.int32), np.asarray(image_captions, np.int32)


def shard_rows(S_local, row0, Nc, caption_image, topk):
    """-> rank_ir int32 [Nc], topk_ir int32 [Nc, topk], target_key uint32 [Nc]: written at the shard's rows, zero elsewhere"""
    nrows, Ni = S_local.shape
    rank_ir, topk_ir, target_key = np.zeros(Nc, np.int32), np.zeros((Nc, topk), np.int32), np.zeros(Nc, np.uint32)
    j = np.arange(Ni)
    for r in range(nrows):
        c, sk = row0 + r, sortable(S_local[r])
        tj = int(caption_image[c])
        if 0 <= tj < Ni:
            target_key[c] = sk[tj]
            rank_ir[c] = int(((sk > sk[tj]) | ((sk == sk[tj]) & (j < tj))).sum())
        else:
            rank_ir[c] = -1
        first = np.lexsort((j, -sk.astype(np.int64)))                    # larger word first, then lower index
        topk_ir[c] = -1
        topk_ir[c, :min(topk, Ni)] = first[:topk]
    return rank_ir, topk_ir, target_key


def shard_counts(S_local, row0, target_key_all, image_ptr, image_captions, Nc):
    """-> count int32 [Nc]: per CSR entry e (caption c of image i) the local rows r with (sortable(S_local[r, i]), row0 + r) above
    (target_key_all[c], c)"""
    nrows = S_local.shape[0]
    count = np.zeros(Nc, np.int32)
    if nrows == 0:
        return count
    sk, rows = sortable(S_local).reshape(S_local.shape), row0 + np.arange(nrows)
    for i in range(len(image_ptr) - 1):
        for e in range(image_ptr[i], image_ptr[i + 1]):
            c = int(image_captions[e])
            tk = target_key_all[c]
            count[e] = int(((sk[:, i] > tk) | ((sk[:, i] == tk) & (rows < c))).sum())
    return count


def finish(count_sum, image_ptr):
    Ni = len(image_ptr) - 1
    return np.asarray([count_sum[image_ptr[i]:image_ptr[i + 1]].min() if image_ptr[i + 1] > image_ptr[i] else -1 for i in range(Ni)], np.int32)


def merged(S, caption_image, topk, W):
    """the three steps over W shards of the whole matrix S, parts added as the exchange adds them -> rank_ir, topk_ir, rank_tr"""
    Nc, Ni = S.shape
    image_ptr, image_captions = csr(caption_image, Ni)
    ranges = [shard_range(Nc, W, r) for r in range(W)]
    parts = [shard_rows(S[a:b], a, Nc, caption_image, topk) for a, b in ranges]
    rank_ir, topk_ir, target_key = (sum(p[k] for p in parts) for k in range(3))
    count = sum(shard_counts(S[a:b], a, target_key, image_ptr, image_captions, Nc) for a, b in ranges)
    return rank_ir.astype(np.int32), topk_ir.astype(np.int32), finish(count, image_ptr)


# ------------------------------------------------------------------------------------------------ the shared inputs
NAN, INF = np.float32("nan"), np.float32("inf")


def _caption_table(Nc, Ni, rng):
    """image 1 without a caption, captions 2 and 3 with an image outside [0, Ni), image 4 with 11 captions in three runs (rows 5-8, 13-16
    and 25-27: one run in each of W = 3's shards of 37 captions)"""
    ci = rng.integers(0, Ni, size=Nc).astype(np.int32)
    ci[ci == 1] = 2
    ci[ci == 4] = 5
    ci[[5, 6, 7, 8, 13, 14, 15, 16, 25, 26, 27]] = 4
    ci[0], ci[1], ci[2], ci[3] = 0, Ni - 1, Ni, -1
    return ci


def case_ties():
    """37 x 13, scores from {-1, 0, 1}: ties everywhere.  Captions 17 and 18 -- either side of W = 2's boundary, 18 -- belong to image 7 and
    tie there with each other and with rows 16 and 19; captions 11 and 12 the same at W = 3's first boundary, 12."""
    rng = np.random.default_rng(3713)
    Nc, Ni = 37, 13
    S = rng.choice(np.asarray([-1.0, 0.0, 1.0], np.float32), size=(Nc, Ni))
    ci = _caption_table(Nc, Ni, rng)
    ci[[17, 18]], ci[[11, 12]] = 7, 9
    S[16:20, 7], S[10:14, 9] = 0.0, 1.0
    return np.ascontiguousarray(S, np.float32), ci


def case_special():
    """37 x 13 with NaN, +-inf and +-0.0 in targets and elsewhere, a row and a column of nothing but NaN"""
    rng = np.random.default_rng(1337)
    Nc, Ni = 37, 13
    S = rng.standard_normal((Nc, Ni)).astype(np.float32)
    hit = rng.random((Nc, Ni)) < 0.4
    S[hit] = rng.choice(np.asarray([NAN, INF, -INF, 0.0, -0.0, -NAN], np.float32), size=int(hit.sum()))
    ci = _caption_table(Nc, Ni, rng)
    S[9, :], S[:, 6] = NAN, NAN
    for c, v in ((0, NAN), (1, INF), (5, -INF), (6, np.float32(-0.0)), (13, np.float32(0.0)), (25, NAN)):     # targets
        S[c, ci[c]] = v
    return np.ascontiguousarray(S, np.float32), ci


def case_two_column_blocks():
    """41 x 70: two 64-column blocks, the second with 58 dead lanes"""
    rng = np.random.default_rng(4170)
    Nc, Ni = 41, 70
    S = np.round(rng.standard_normal((Nc, Ni)) * 2).astype(np.float32) / 2          # a few dozen values: many ties
    ci = _caption_table(Nc, Ni, rng)
    ci[30:41] = np.arange(59, 70)                                                   # targets in the tail block
    return np.ascontiguousarray(S, np.float32), ci


def case_deep():
    """600 x 9: W = 2 gives shards of 300 rows, more than one 256-row block; W = 7 splits unevenly (85 or 86 rows)"""
    rng = np.random.default_rng(6009)
    Nc, Ni = 600, 9
    S = rng.choice(np.asarray([-1.5, 0.25, 0.25 + 2.0 ** -20, 3.0], np.float32), size=(Nc, Ni))
    ci = _caption_table(Nc, Ni, rng)
    return np.ascontiguousarray(S, np.float32), ci


# name -> (builder, shard counts for the device simulation); the host test runs every case at W in {1, 2, 3, 5, Nc + 2}
CASES = {"ties_37x13": (case_ties, [1, 2, 3, 5, 39]), "special_37x13": (case_special, [1, 2, 3, 5, 39]),
         "two_column_blocks_41x70": (case_two_column_blocks, [1, 2, 3, 43]), "deep_600x9": (case_deep, [1, 2, 7])}
