"""numpy restatement of the contract of `vk_retrieval_ranks` (include/volta_hip.h, csrc/ranks.hip) and of the driver's metric arithmetic.

One total order: element (score s, index j) ranks before (s', j') when s > s', or s == s' and j < j'; -0.0 == +0.0 and every NaN ranks
after everything else (NaNs among themselves by index).  That is np.argsort(-s, kind="stable") once NaN is made the largest value of -s
(numpy already sorts NaN last) and the signed zeros are merged.  The driver's np.argsort(-s) (eval_retrieval.py:203,222,253) is quicksort:
its result is only defined where the target's score is untied, and there it is the same position."""
import numpy as np


def order(s):
    """indices of the 1-D score vector `s`, best first"""
    neg = -np.asarray(s, dtype=np.float32)
    neg = np.where(neg == 0, np.float32(0), neg)            # -0.0 and +0.0 alike
    return np.argsort(neg, kind="stable")                   # NaN last, ties by index


def ranks(S, caption_image, topk):
    """-> rank_ir int32 [Nc] (-1 for a caption_image outside [0, Ni)), topk_ir int32 [Nc, topk] (-1 past Ni), rank_tr int32 [Ni] (-1 for an
    image without a caption)"""
    S = np.asarray(S, dtype=np.float32)
    Nc, Ni = S.shape
    rank_ir = np.full(Nc, -1, np.int32)
    topk_ir = np.full((Nc, topk), -1, np.int32)
    for c in range(Nc):
        o = order(S[c])
        if 0 <= caption_image[c] < Ni:
            rank_ir[c] = np.where(o == caption_image[c])[0][0]
        k = min(topk, Ni)
        topk_ir[c, :k] = o[:k]
    rank_tr = np.full(Ni, -1, np.int32)
    for i in range(Ni):
        mine = np.where(np.asarray(caption_image) == i)[0]
        if len(mine):
            o = order(S[:, i])
            rank_tr[i] = min(np.where(o == c)[0][0] for c in mine)
    return rank_ir, topk_ir, rank_tr


def metrics(rank):
    """eval_retrieval.py:225-230 (image retrieval) and :258-263 (text retrieval): r1, r5, r10, medr, meanr of a vector of 0-based ranks"""
    rank_matrix = np.asarray(rank, dtype=np.float64)
    r1 = 100.0 * np.sum(rank_matrix < 1) / len(rank_matrix)
    r5 = 100.0 * np.sum(rank_matrix < 5) / len(rank_matrix)
    r10 = 100.0 * np.sum(rank_matrix < 10) / len(rank_matrix)
    medr = np.floor(np.median(rank_matrix) + 1)
    meanr = np.mean(rank_matrix) + 1
    return dict(r1=r1, r5=r5, r10=r10, medr=medr, meanr=meanr)
