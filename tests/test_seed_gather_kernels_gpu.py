"""vk_grad_seed (csrc/backbone.hip) and vk_pair_gather (csrc/pairs.hip) through the C ABI, bit for bit against the numpy restatements of
tests/vis_restate.py.  Neither kernel had a direct test: tests/ named them for struct layout and the hosts' refusals only.
  * vk_grad_seed: at most one fp32 add and one round to nearest even to bf16, so the expected bits are fp32 numpy's.  Shapes from one
    8-element piece to one whose piece count exceeds 2048 x 256 (the grid-stride loop goes round); contiguous, stride-0 and padded
    sources (NaN in the source pad); row0, ld > H, the ReLU gate on y (positive, negative, +0, -0, NaN: !(y > 0) closes it), write and
    accumulate, src = NULL in both forms; rows before row0, rows past the last one and the pad columns keep their canary.
  * vk_pair_gather: byte-exact.  One launch carries eight segments of both sides whose sizes take every path: the 4-byte path alone (4,
    12, a source offset by 4 bytes), the 16-byte path alone (16), with a tail (20), across the four-in-flight loop once (16400), that loop
    plus the single loop plus the tail (16 (1024 + 300) + 8), and 8 x 37, where every other item is misaligned and both paths run in one
    launch.  Cross products and explicit indices (repeats, -1 and n_items: all-zero blocks); guard bands behind every dst."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vis_restate as VR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
CAN = np.uint16(0xFFA5)
Y_VALUES = np.array([0x3F80, 0xBF80, 0x0000, 0x8000, 0x7FC0, 0x3C00, 0xC2C8, 0x4120], np.uint16)    # 1, -1, +0, -0, NaN, 2^-7, -100, 10


def _lib():
    from volta_amd import _lib as L
    return L


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _strides(kind, L_, H):
    """(stride_b, stride_l, number of source floats for B samples)"""
    if kind == "contiguous":
        return L_ * H, H, lambda B: B * L_ * H
    if kind == "expand_bl":
        return 0, 0, lambda B: H
    if kind == "expand_l":
        return H, 0, lambda B: B * H
    return L_ * (H + 4), H + 4, lambda B: B * L_ * (H + 4)


def _seed_case(L, rng, B, L_, H, stride, row0, ld, with_y, accumulate, null_src=False):
    sb, sl, size = _strides(stride, L_, H)
    n = B * L_
    src = rng.standard_normal(size(B)).astype(np.float32)
    if stride == "padded":
        src.reshape(n, H + 4)[:, H:] = np.nan
    ldy = H + 8
    dst = np.full((row0 + n + 2, ld), CAN, np.uint16)
    if accumulate:
        dst[row0:row0 + n, :H] = VR.bf16_bits(rng.standard_normal((n, H)))
    y = None
    if with_y:
        y = np.full((n, ldy), 0x7FC0, np.uint16)
        y[:, :H] = Y_VALUES[rng.integers(0, len(Y_VALUES), (n, H))]
    want = VR.grad_seed_restate(None if null_src else src, sb, sl, B, L_, H, dst, row0, ld, y, ldy, accumulate)
    s_d, d_d = _dev(src), _dev(dst.view(np.int16))
    y_d = _dev(y.view(np.int16)) if with_y else None
    a = L.GradSeedArgs(None if null_src else s_d.data_ptr(), sb, sl, d_d.data_ptr(), y_d.data_ptr() if with_y else None, B, L_, H, row0, ld, ldy if with_y else 0,
                       accumulate, 0)
    L.check(L.lib.vk_grad_seed(C.byref(a), L.stream_ptr()))
    torch.cuda.synchronize()
    got = d_d.cpu().numpy().view(np.uint16)
    tag = (B, L_, H, stride, row0, ld, with_y, accumulate, null_src)
    assert (got[:row0] == CAN).all() and (got[row0 + n:] == CAN).all() and (got[:, H:] == CAN).all(), "canary lost: %r" % (tag,)
    bad = got != want
    assert not bad.any(), "%r: %d element(s) differ, first at %r" % (tag, int(bad.sum()), tuple(np.argwhere(bad)[0]))
    if not (null_src and accumulate):
        assert not (got[row0:row0 + n, :H] == CAN).any(), "not written: %r" % (tag,)


@pytest.mark.parametrize("B,L_,H", [(1, 1, 8), (3, 5, 24), (2, 7, 768)])
def test_grad_seed_bit_exact(B, L_, H):
    L = _lib()
    rng = np.random.default_rng(B * 1000 + H)
    for stride in ("contiguous", "expand_bl", "expand_l", "padded"):
        for row0 in (0, 3):
            for ld in (H, H + 16):
                for with_y in (False, True):
                    for accumulate in (0, 1):
                        _seed_case(L, rng, B, L_, H, stride, row0, ld, with_y, accumulate)
    for accumulate in (0, 1):                                  # src = NULL: the write form zero-fills, the accumulate form changes no byte
        for with_y in (False, True):
            _seed_case(L, rng, B, L_, H, "contiguous", 3, H + 16, with_y, accumulate, null_src=True)


@pytest.mark.parametrize("stride,with_y,accumulate", [("contiguous", True, 1), ("expand_l", False, 0)])
def test_grad_seed_grid_stride_loop(stride, with_y, accumulate):
    """8 x 700 x 768 / 8 = 537600 pieces > 2048 blocks x 256 threads: the loop goes round once for the first 13312 threads."""
    B, L_, H = 8, 700, 768
    assert B * L_ * H // 8 > 2048 * 256
    _seed_case(_lib(), np.random.default_rng(7), B, L_, H, stride, 3, H + 16, with_y, accumulate)


# ------------------------------------------------------------------------------------------------ pair gather
SEG_BYTES = (4, 12, 16, 20, 16400, 16 * (1024 + 300) + 8, 8 * 37, 32)
SEG_OFFSET = (0, 0, 0, 0, 0, 0, 0, 4)           # the last segment's src starts 4 bytes past an aligned address: the 4-byte path for 32 bytes
GUARD = 64


def _gather(L, n_items, npairs, cap=None, img=None, cross=None):
    rng = np.random.default_rng(npairs * 31 + n_items[0])
    a = L.PairGatherArgs()
    keep, srcs, dsts = [], [], []
    for k, (nb, off) in enumerate(zip(SEG_BYTES, SEG_OFFSET)):
        side = k % 2
        src = rng.integers(1, 256, n_items[side] * nb + off, dtype=np.uint8)          # no zero byte: a zero block can only be a refusal
        s_d = _dev(src)
        d_d = torch.full((npairs * nb + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        keep += [s_d, d_d]
        srcs.append(src[off:])
        dsts.append(d_d)
        a.src[k], a.dst[k], a.bytes[k], a.side[k] = s_d.data_ptr() + off, d_d.data_ptr(), nb, side
    a.nseg, a.npairs = len(SEG_BYTES), npairs
    a.n_items[0], a.n_items[1] = n_items
    if cross is None:
        c_d, i_d = _dev(np.asarray(cap, np.int64)), _dev(np.asarray(img, np.int64))
        keep += [c_d, i_d]
        a.cap_idx, a.img_idx = c_d.data_ptr(), i_d.data_ptr()
        items = (np.asarray(cap), np.asarray(img))
    else:
        a.c0, a.nc, a.i0, a.ni = cross
        pr = np.arange(npairs)
        items = (cross[0] + pr // cross[3], cross[2] + pr % cross[3])
    L.check(L.lib.vk_pair_gather(C.byref(a), L.stream_ptr()))
    torch.cuda.synchronize()
    for k, nb in enumerate(SEG_BYTES):
        got = dsts[k].cpu().numpy()
        assert (got[npairs * nb:] == 0xA5).all(), "segment %d: the guard band was written" % k
        want = VR.pair_gather_restate(srcs[k], nb, items[k % 2])
        bad = got[:npairs * nb] != want
        assert not bad.any(), "segment %d (%d bytes): %d byte(s) differ, first at %d" % (k, nb, int(bad.sum()), int(np.argwhere(bad)[0][0]))
    return items


@pytest.mark.parametrize("nc,ni", [(1, 1), (3, 5)])
def test_pair_gather_cross_product(nc, ni):
    c0, i0 = 1, 2
    _gather(_lib(), (c0 + nc + 1, i0 + ni + 1), nc * ni, cross=(c0, nc, i0, ni))


def test_pair_gather_explicit_indices():
    """Repeated indices; -1 and n_items zero-fill their block of that side only."""
    n_items = (4, 6)
    cap = [0, 0, 3, -1, 4, 1, 1, 3, 2]
    img = [5, 5, -1, 2, 0, 6, 1, 1, 4]
    _gather(_lib(), n_items, len(cap), cap=cap, img=img)
