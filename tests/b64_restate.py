"""numpy restatement of `vk_b64_decode_device` (include/volta_hip.h; csrc/b64.hip): the canonical base64 subset, the table check and the status
words.  Written from the contract, not from the kernel: a 256-entry table and whole-array arithmetic.

  jobs     list of (text_off, dst_off, nsig, want_bytes)
  decode() -> (dst after the call, status uint32 [njobs], defined, touchable)
             defined    bool mask over dst: bytes the contract pins (the destination of every job with status 0)
             touchable  bool mask over dst: bytes the call may write at all (the destination of every job the table check accepts)
Bytes outside `touchable` must keep their value; bytes inside `defined` must equal the returned dst."""
import numpy as np

REFUSED = 0xFFFFFFFE
STD = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
URL = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_"

LUT = np.full(256, 255, np.uint8)
for _i in range(64):
    LUT[STD[_i]] = _i
    LUT[URL[_i]] = _i


def nsig_of(text):
    """significant characters: the length without up to two trailing '=' (the last two bytes only)"""
    return len(text) - (2 if text[-2:] == b"==" else 1 if text[-1:] == b"=" else 0)


def job_ok(job, text_bytes, dst_bytes, max_nsig):
    text_off, dst_off, nsig, want = (int(v) for v in job)
    if nsig > max_nsig or nsig > 0x7FFFFFFF:
        return False
    if want % 4 or want != nsig * 3 // 4:
        return False
    if text_off % 16 or dst_off % 16:
        return False
    return text_off + nsig <= text_bytes and dst_off + want <= dst_bytes


def decode_field(chars):
    """significant characters (uint8 array, all inside the alphabets) -> len * 3 // 4 bytes; the unused low bits of the last character drop"""
    v = LUT[chars].astype(np.uint32)
    v = np.concatenate([v, np.zeros(-len(v) % 4, np.uint32)]).reshape(-1, 4)
    w = (v[:, 0] << 18) | (v[:, 1] << 12) | (v[:, 2] << 6) | v[:, 3]
    out = np.stack([(w >> 16) & 255, (w >> 8) & 255, w & 255], 1).astype(np.uint8).reshape(-1)
    return out[:len(chars) * 3 // 4]


def decode(text, dst, jobs, max_nsig=None):
    text, out = np.asarray(text, np.uint8), np.array(dst, np.uint8, copy=True)
    if max_nsig is None:
        max_nsig = max([int(j[2]) for j in jobs] + [0])
    status = np.zeros(len(jobs), np.uint32)
    defined, touchable = np.zeros(out.size, bool), np.zeros(out.size, bool)
    for k, job in enumerate(jobs):
        if not job_ok(job, text.size, out.size, max_nsig):
            status[k] = REFUSED
            continue
        text_off, dst_off, nsig, want = (int(v) for v in job)
        touchable[dst_off:dst_off + want] = True
        chars = text[text_off:text_off + nsig]
        bad = np.flatnonzero(LUT[chars] == 255)
        if bad.size:
            status[k] = 1 + int(bad[0])
            continue
        out[dst_off:dst_off + want] = decode_field(chars)
        defined[dst_off:dst_off + want] = True
    return out, status, defined, touchable


def job_table(jobs):
    """the vk_b64_job records as int32 [njobs, 6], unchecked (the tests of the untrusted table write it themselves)"""
    tab = np.zeros(len(jobs), np.dtype([("text_off", "<u8"), ("dst_off", "<u8"), ("nsig", "<u4"), ("want_bytes", "<u4")]))
    for k, job in enumerate(jobs):
        tab[k] = tuple(int(v) for v in job)
    return tab.view(np.int32).reshape(len(jobs), 6)


def pack(texts, gap=16):
    """significant texts (bytes) -> (arena uint8, offsets): 16-byte aligned, `gap` bytes of '!' (outside both alphabets) between them"""
    offs, at = [], 0
    for t in texts:
        offs.append(at)
        at += -(-len(t) // 16) * 16 + gap
    arena = np.full(max(at, 16), ord("!"), np.uint8)
    for t, o in zip(texts, offs):
        arena[o:o + len(t)] = np.frombuffer(t, np.uint8)
    return arena, offs
