"""`vk_b64_decode_device` (csrc/b64.hip) against its numpy restatement (tests/b64_restate.py, tied to Python's base64 and the host decoder by
tests/test_b64_device_cpu.py): equal bytes and equal status words.  The destination handed to the kernel is the middle of a larger tensor
filled with 0xA5, so a write outside a job's destination -- inside or outside the region -- shows, and lands in memory the test owns.
GPU only."""
import base64
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import b64_restate as RS  # noqa: E402

SLACK = 4096
CHUNK = 12288                                                  # bytes one workgroup decodes (256 lanes x 48 bytes)


def _payload(nbytes, seed):
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8).tobytes()


def _layout(wants, gap=32):
    """16-byte aligned destination offsets with untouched bytes between the jobs"""
    offs, at = [], 16
    for w in wants:
        offs.append(at)
        at += -(-w // 16) * 16 + gap
    return offs, at


def _run(arena, jobs, dst_bytes, max_nsig=None):
    """-> (the kernel's dst region, the slack around it, status) and the restatement's (dst, status, defined, touchable)"""
    from volta_amd import ops
    if max_nsig is None:
        max_nsig = max([int(j[2]) for j in jobs] + [0])
    whole = torch.full((SLACK + dst_bytes + SLACK,), 0xA5, dtype=torch.uint8, device="cuda")
    text_whole = torch.full((SLACK + arena.size + SLACK,), ord("!"), dtype=torch.uint8, device="cuda")
    text_whole[SLACK:SLACK + arena.size] = torch.from_numpy(arena).cuda()
    status = torch.full((len(jobs) + 2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")         # uninitialised as far as the kernel knows
    got_status = ops.b64_decode_device(text_whole[SLACK:SLACK + arena.size], whole[SLACK:SLACK + dst_bytes], torch.from_numpy(RS.job_table(jobs)).cuda(),
                                       max_nsig, status=status)
    torch.cuda.synchronize()
    assert (status[len(jobs):] == 0x5A5A5A5A).all()
    w = whole.cpu().numpy()
    want = RS.decode(arena, np.full(dst_bytes, 0xA5, np.uint8), jobs, max_nsig)
    return (w[SLACK:SLACK + dst_bytes], np.concatenate([w[:SLACK], w[SLACK + dst_bytes:]]), got_status.cpu().numpy().view(np.uint32)), want


def _check(arena, jobs, dst_bytes, max_nsig=None):
    (got, slack, status), (want, want_status, defined, touchable) = _run(arena, jobs, dst_bytes, max_nsig)
    assert np.array_equal(status, want_status), (status, want_status)
    assert (slack == 0xA5).all()
    assert (got[~touchable] == 0xA5).all(), "bytes outside every accepted job's destination changed"
    assert np.array_equal(got[defined], want[defined]), int((got[defined] != want[defined]).sum())
    return status


SIZES = [16 * k for k in range(1, 14)] + [CHUNK - 16, CHUNK, CHUNK + 16, 2 * CHUNK + 48 + 16]


@pytest.mark.parametrize("urlsafe", [False, True])
@pytest.mark.parametrize("padded", [True, False])
def test_canonical_text_one_job_per_launch(padded, urlsafe):
    """16 * k bytes for k = 1 ... 13 (16, 32, 48: the tail classes nbytes mod 3 = 1, 2, 0), and sizes around one workgroup's chunk"""
    for nbytes in SIZES:
        full = (base64.urlsafe_b64encode if urlsafe else base64.b64encode)(_payload(nbytes, nbytes))
        text = full if padded else full.rstrip(b"=")
        nsig = RS.nsig_of(text)
        arena, (off,) = RS.pack([text[:nsig]])
        (dst_off,), total = _layout([nbytes])
        status = _check(arena, [(off, dst_off, nsig, nbytes)], total)
        assert status[0] == 0


def test_dirty_low_bits_in_the_last_character():
    for nbytes in (16, 32, 12288 + 16):
        raw = _payload(nbytes, 5)
        text = base64.b64encode(raw).rstrip(b"=")
        dirty = text[:-1] + bytes([RS.STD[RS.LUT[text[-1]] | (0xF if nbytes % 3 == 1 else 0x3)]])
        assert dirty != text
        arena, (off,) = RS.pack([dirty])
        (got, _, status), _ = _run(arena, [(off, 16, len(dirty), nbytes)], nbytes + 32)
        assert status[0] == 0 and got[16:16 + nbytes].tobytes() == raw


def _ragged(seed=3):
    rng = np.random.default_rng(seed)
    wants = [int(w) for w in rng.choice([4, 8, 16, 44, 48, 52, 1600, 3072, 12284, 12288, 12292, 40000], 19)] + [0, 576, 2 * CHUNK + 4]
    raws = [_payload(w, 100 + i) for i, w in enumerate(wants)]
    texts = [(base64.urlsafe_b64encode if i % 3 == 0 else base64.b64encode)(r).rstrip(b"=") for i, r in enumerate(raws)]
    return wants, texts


def test_ragged_jobs_in_one_launch():
    """about 20 jobs from 0 to 24580 bytes in one launch, both alphabets, a zero-length job among them"""
    wants, texts = _ragged()
    arena, offs = RS.pack(texts)
    dst_offs, total = _layout(wants)
    status = _check(arena, [(o, d, len(t), w) for o, d, t, w in zip(offs, dst_offs, texts, wants)], total)
    assert not status.any() and 0 in wants


def test_offending_bytes_are_reported_and_the_neighbours_decode():
    """first position, last position, mid-chunk, two offenders in one job (the smaller offset is reported), a line break, an interior '='"""
    wants, texts = _ragged(4)
    texts = [bytearray(t) for t in texts]
    big = [i for i, w in enumerate(wants) if w >= 12284]
    small = [i for i, w in enumerate(wants) if 44 <= w <= 3072]
    marks = {}

    def spoil(i, at, byte):
        texts[i][at] = byte
        marks[i] = min(marks.get(i, at), at)

    spoil(big[0], 0, ord("\n"))
    spoil(big[1], len(texts[big[1]]) - 1, ord("="))
    spoil(big[2], 7000, ord(" "))
    spoil(big[3], 9001, ord("*"))
    spoil(big[3], 1234, ord("\r"))
    spoil(small[0], 30, ord("="))
    spoil(small[1], len(texts[small[1]]) - 1, ord("\n"))
    spoil(small[2], 0, 0xC3)
    arena, offs = RS.pack([bytes(t) for t in texts])
    dst_offs, total = _layout(wants)
    status = _check(arena, [(o, d, len(t), w) for o, d, t, w in zip(offs, dst_offs, texts, wants)], total)
    for i in range(len(wants)):
        assert status[i] == (marks[i] + 1 if i in marks else 0), (i, status[i], marks.get(i))
    assert len(marks) == 7


def test_untrusted_job_table():
    """ranges that leave the text or the destination, lengths that disagree, misaligned offsets: 0xFFFFFFFE and nothing written; the honest
    jobs of the same launch decode"""
    raw = _payload(960, 9)
    text = base64.b64encode(raw)
    nsig = len(text)
    arena, offs = RS.pack([text, text])
    total = 4096
    honest = [(offs[0], 16, nsig, 960), (offs[1], 2048, nsig, 960)]
    rogue = [(arena.size - 16, 1024, nsig, 960),                 # the text range leaves the arena
             (1 << 40, 1024, nsig, 960),
             (offs[0], total - 16, nsig, 960),                   # the destination range leaves the region
             (offs[0], (1 << 63) + 16, nsig, 960),
             (offs[0], 1024, nsig, 956), (offs[0], 1024, nsig, 964), (offs[0], 1024, nsig - 4, 960), (offs[0], 1024, nsig - 2, 958),
             (offs[0], 1024, 0xFFFFFFFF, 960), (offs[0], 1024, 0xFFFFFFF0, 0xBFFFFFF4),
             (offs[0] + 4, 1024, nsig, 960), (offs[0], 1028, nsig, 960),
             (offs[0], 1024, nsig + 64, 1008)]                   # longer than max_nsig says: the grid would not cover it
    jobs = honest[:1] + rogue + honest[1:]
    (got, _, status), _ = _run(arena, jobs, total, max_nsig=nsig)
    status = _check(arena, jobs, total, max_nsig=nsig)
    assert status[0] == 0 and status[-1] == 0 and (status[1:-1] == RS.REFUSED).all()
    assert got[16:976].tobytes() == raw and got[2048:3008].tobytes() == raw
    assert (got[976:2048] == 0xA5).all()


def test_no_jobs_and_empty_jobs():
    from volta_amd import ops
    empty = torch.zeros(16, dtype=torch.uint8, device="cuda")
    assert ops.b64_decode_device(empty, empty.clone(), torch.zeros(0, 6, dtype=torch.int32, device="cuda"), 0).numel() == 0
    status = _check(np.full(16, ord("!"), np.uint8), [(0, 0, 0, 0), (0, 16, 0, 0)], 64)
    assert not status.any()
