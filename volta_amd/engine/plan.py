"""The command list (`Plan`), the constructors of its ops and the names of the side-stream events."""
import ctypes as C

import torch

from .. import _lib as L
from .._lib import check

# Side-stream events (VK_OP_SIDE_END records, VK_OP_WAIT_SIDE makes the main stream wait).  The one place that says who does which:
#   k % EV_WGRAD_RING   sub-layer k's weight-gradient block records (_wgrad); the backward of sub-layer k first waits for the event of
#                       sub-layer k + 2, the previous user of its set (k % 2) of backward temporaries (_build)
#   EV_HEAD_REGIONS     forward: the heads' masked-region chain records, the loss finalisation waits
#   EV_DECODER_WGRAD    backward: the weight gradients of the heads' main chains record, the tied LM decoder's among them, which initialises
#                       the word table's gradient: the text tables' backward waits before it adds to that gradient
#   EV_HEAD_REGIONS_BWD backward: the heads' region chain records, the end of the heads' backward waits (dX[1] complete)
#   EV_IMAGE_EMB_FWD    forward: the image embedding's block records, the first sub-layer that touches the vision stream waits
#   EV_IMAGE_EMB_BWD    backward: the image embedding's block behind that sub-layer records; the VK_OP_JOIN that ends the list joins it
EV_WGRAD_RING, EV_HEAD_REGIONS, EV_DECODER_WGRAD, EV_HEAD_REGIONS_BWD, EV_IMAGE_EMB_BWD, EV_IMAGE_EMB_FWD = 8, 11, 12, 13, 14, 15
NODROP = L.dropout_cfg(None, 0, 0.0)          # "no dropout here" of the argument structures (copied into them)


def op(kind, a=None, b=None, c=None, i0=0, i1=0, i2=0):
    """One entry of Plan.ops: (kind, i0, i1, i2, a, b, c) -- structures, tensors or addresses behind a / b / c (_addr)."""
    return (kind, i0, i1, i2, a, b, c)


def side_begin():
    return op(L.OP_SIDE_BEGIN)


def side_end(event):
    return op(L.OP_SIDE_END, i0=event)


def wait_side(event):
    return op(L.OP_WAIT_SIDE, i0=event)


def _round_up(x, m):
    return (x + m - 1) // m * m


class Plan:
    def __init__(self):
        self.ops, self.keep = [], []
        self.c_ops = None
        self.timing = None

    def freeze(self):
        arr = (L.Op * max(1, len(self.ops)))()
        for i, (kind, i0, i1, i2, a, b, c) in enumerate(self.ops):
            arr[i] = L.Op(kind, i0, i1, i2, _addr(a), _addr(b), _addr(c))
        self.c_ops = arr
        return self

    def run(self, start=0, end=None):
        end = len(self.ops) if end is None else end
        if end > start:
            base = C.cast(C.byref(self.c_ops, start * C.sizeof(L.Op)), C.POINTER(L.Op))
            if self.timing is not None:
                ms = C.cast(C.byref(self.timing, start * C.sizeof(C.c_float)), C.POINTER(C.c_float))
                check(L.lib.vk_run_ops_timed(base, end - start, L.stream_ptr(), ms))
            else:
                check(L.lib.vk_run_ops(base, end - start, L.stream_ptr()))

    def join_side(self, owner=None):
        """Make the current stream wait for the side-stream work (weight gradients) issued so far by lists run on stream `owner`
        (a raw stream handle; default: the current stream itself)."""
        if owner is None:
            check(L.lib.vk_side_join(L.stream_ptr()))
        else:
            check(L.lib.vk_side_join_from(C.c_void_p(owner), L.stream_ptr()))

    def enable_timing(self, on=True):
        """Per-op HIP-event timing (synchronises the stream on every run; profiling passes only)."""
        self.timing = (C.c_float * max(1, len(self.ops)))() if on else None


def _addr(o):
    if o is None:
        return None
    if isinstance(o, int):
        if 0 < o < (1 << 16):        # a count or an index handed over where a buffer was meant: never a device address
            raise ValueError("engine: %d is not a device address" % o)
        return o
    if isinstance(o, torch.Tensor):
        return o.data_ptr()
    return C.addressof(o)


def _mk_segs(drop, segs):
    arr = (L.DropRows * 2)()
    if segs is None:
        segs = [(drop.site, 0, 0, 0), (drop.site + 1, 0, 0, 0)]
    for i, sg in enumerate(segs):
        arr[i] = L.DropRows(*sg)
    return arr
