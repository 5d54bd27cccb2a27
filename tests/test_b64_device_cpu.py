"""The numpy restatement of the device base64 decoder (tests/b64_restate.py) against Python's base64 module and against the host decoder
`vk_b64_decode`, on canonical input; its status words on the offending inputs the GPU test uses; and the Python-side length check of
`ops.b64_jobs`.  No GPU needed."""
import base64
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import b64_restate as RS  # noqa: E402

SIZES = [16 * k for k in range(1, 14)] + [12288 - 16, 12288, 12288 + 16, 0]


def _payload(nbytes, seed):
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8).tobytes()


def _host_decode(text, cap):
    from volta_amd import _lib as L
    out, got = (C.c_uint8 * max(cap, 1))(), C.c_size_t()
    L.check(L.lib.vk_b64_decode(text, len(text), out, cap, C.byref(got)))
    return bytes(out[:got.value])


@pytest.mark.parametrize("urlsafe", [False, True])
@pytest.mark.parametrize("padded", [True, False])
def test_restatement_equals_python_and_the_host_decoder(padded, urlsafe):
    for nbytes in SIZES:
        raw = _payload(nbytes, nbytes)
        full = (base64.urlsafe_b64encode if urlsafe else base64.b64encode)(raw)
        text = full if padded else full.rstrip(b"=")
        nsig = RS.nsig_of(text) if text else 0
        assert nsig == len(full.rstrip(b"=")) and nsig * 3 // 4 == nbytes
        arena, (off,) = RS.pack([text[:nsig]])
        dst = np.full(nbytes + 64, 0xA5, np.uint8)
        out, status, defined, touchable = RS.decode(arena, dst, [(off, 32, nsig, nbytes)])
        assert status[0] == 0 and defined.sum() == nbytes == touchable.sum()
        assert out[32:32 + nbytes].tobytes() == raw == (base64.urlsafe_b64decode if urlsafe else base64.b64decode)(full)
        assert out[32:32 + nbytes].tobytes() == _host_decode(text, nbytes)
        assert (out[:32] == 0xA5).all() and (out[32 + nbytes:] == 0xA5).all()


def test_unused_low_bits_of_the_last_character_are_ignored_as_on_the_host():
    for nbytes in (16, 32):                                    # nbytes mod 3 = 1, 2: four and two unused bits
        raw = _payload(nbytes, 5)
        text = base64.b64encode(raw).rstrip(b"=")
        last = RS.STD[RS.LUT[text[-1]] | (0xF if nbytes % 3 == 1 else 0x3)]
        dirty = text[:-1] + bytes([last])
        assert dirty != text
        arena, (off,) = RS.pack([dirty])
        out, status, _, _ = RS.decode(arena, np.zeros(nbytes, np.uint8), [(off, 0, len(dirty), nbytes)])
        assert status[0] == 0 and out.tobytes() == raw == _host_decode(dirty, nbytes)


def test_status_words_of_the_restatement():
    raw = _payload(480, 1)
    text = bytearray(base64.b64encode(raw))
    nsig = len(text)
    for where, byte in ((0, b"\n"), (nsig - 1, b"="), (100, b" "), (321, b"=")):
        t = bytearray(text)
        t[where:where + 1] = byte
        arena, (off,) = RS.pack([bytes(t)])
        _, status, defined, touchable = RS.decode(arena, np.zeros(480, np.uint8), [(off, 0, nsig, 480)])
        assert status[0] == where + 1 and not defined.any() and touchable.all()
    t = bytearray(text)
    t[400:401], t[77:78] = b"\r", b"*"
    arena, (off,) = RS.pack([bytes(t)])
    assert RS.decode(arena, np.zeros(480, np.uint8), [(off, 0, nsig, 480)])[1][0] == 78           # the smaller offset
    arena, (off,) = RS.pack([bytes(text)])
    for job in ((off, 0, nsig, 476), (off, 0, nsig + 1, 480), (off, 8, nsig, 480), (off + 32, 0, nsig, 480), (off, 16, nsig, 480), (off, 0, nsig - 2, 478)):
        out, status, _, touchable = RS.decode(arena, np.full(480, 0xA5, np.uint8), [job], max_nsig=nsig)
        assert status[0] == RS.REFUSED and not touchable.any() and (out == 0xA5).all(), job


def test_job_table_layout_and_the_wrapper_length_check():
    from volta_amd import _lib as L, ops
    assert C.sizeof(L.B64Job) == 24 and L.B64_REFUSED == RS.REFUSED
    jobs = [(0, 16, 64, 48), (80, 64, 22, 16)]
    tab, mx = ops.b64_jobs(jobs)
    assert mx == 64 and np.array_equal(tab.numpy(), RS.job_table(jobs))
    rec = L.B64Job.from_buffer_copy(tab.numpy()[1].tobytes())
    assert (rec.text_off, rec.dst_off, rec.nsig, rec.want_bytes) == jobs[1]
    for bad in ((0, 16, 64, 44), (0, 16, 23, 17), (8, 16, 64, 48), (0, 4, 64, 48)):
        with pytest.raises(ValueError):
            ops.b64_jobs([bad])
    assert ops.b64_jobs([])[1] == 0
