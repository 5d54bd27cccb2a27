"""Float64 restatement of the LoRA dropout entry points (include/volta_hip.h: vk_lora_fwd_drop / vk_lora_bwd_drop / vk_lora_proj_fwd_drop /
vk_lora_proj_bwd_drop, csrc/lora.hip), on top of tests/lora_restate.py.  CPU only (numpy).

The contract, where it differs from lora_restate's (keep [M, K] = oracle.volta_ref.philox_keep_mask(seed, site, (M, K), p), the mask of
the problem's site on the rows of X as passed; c = fp32(1 / (1 - p))):
    T   = bf16(c sum_k keep[m,k] X[m,k] A[j,k])
    dA  = sum over the problems that name it of  c sum_m keep[m,k] dT[m,j] X[m,k]            (+ the previous dA with `accumulate`)
    dX  = bf16(dX + rho[m,k] sum_c keep_c[m,k] c_c sum_j dT_c[m,j] A_c[j,k])
Y, dT and dB are lora_restate's: they read the T the kernel stored, which carries the mask.

The bounds are lora_restate's e_acc and bound_bf16, nothing new: a dropped element contributes an exact zero and no addition's rounding,
so the sum length Kc is the number of KEPT terms of each output (kept k of row m for T; kept rows m of column k, over every source, for
dA; r times the adapters that keep element (m, k) for dX), and every magnitude carries the factor c.  The single multiplication by c is
the "multiplication by s" among the 4 spare roundings of e_acc (the unmasked T, dA and dX multiply by 1).

At p = 0.5, c = 2 is a power of two: the integer family of lora_restate.family stays exact (|T| <= 8, |s T B^T| <= 128, |dT| <= 16,
|sum_c 2 dT_c A_c| <= 192, all integers of magnitude <= 256 and sums below 2^24), so the outputs are bitwise the float64 results."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lora_restate as R  # noqa: E402

from oracle import volta_ref as VR  # noqa: E402


def threshold(p):
    return min(int(p * 4294967296.0), 0xFFFFFFFF)


def scale(p):
    """c as the kernels hold it: 1 / (1 - p) rounded to fp32"""
    return float(np.float32(1.0 / (1.0 - p)))


def keep_mask(seed, site, M, K, p):
    """float64 0 / 1 [M, K]; p = 0 keeps everything"""
    if p <= 0.0:
        return np.ones((M, K))
    return VR.philox_keep_mask(int(seed), int(site), (M, K), p).numpy().astype(np.float64)


def ref_T(X, A, keep, c):
    Xk = keep * X
    return c * (Xk @ A.T), R.e_acc(keep.sum(axis=1)[:, None], c * (np.abs(Xk) @ np.abs(A).T))


def ref_dA(sources, prev=None):
    """sources: [(dT values [M, r], X [M, K], keep [M, K], c)] of every problem that names this dA, in list order"""
    ref = sum(c * (dT.T @ (keep * X)) for dT, X, keep, c in sources)
    mag = sum(c * (np.abs(dT).T @ np.abs(keep * X)) for dT, X, keep, c in sources)
    if prev is not None:
        ref, mag = ref + prev, mag + np.abs(prev)
    return ref, R.e_acc(sum(keep.sum(axis=0)[None, :] for _, _, keep, _ in sources), mag)


def ref_dX_term(members):
    """members: [(dT values [M, r], A [r, K], keep [M, K], c)] of the problems that name one dX -> the adapters' share (before rho and the
    previous dX), its accumulation bound"""
    ref = sum(keep * c * (dT @ A) for dT, A, keep, c in members)
    mag = sum(keep * c * (np.abs(dT) @ np.abs(A)) for dT, A, keep, c in members)
    return ref, R.e_acc(sum(keep * A.shape[0] for _, A, keep, _ in members), mag)


def ref_dX(dXprev, members):
    ref = dXprev + sum(keep * c * (dT @ A) for dT, A, keep, c in members)
    mag = np.abs(dXprev) + sum(keep * c * (np.abs(dT) @ np.abs(A)) for dT, A, keep, c in members)
    return ref, R.e_acc(sum(keep * A.shape[0] for _, A, keep, _ in members), mag)
