"""csrc/concap.hip (vk_concap_batch: the meta, feature and class kernels) through the C ABI against the op-by-op fp32 restatement of
tests/concap_restate.py, whose case table and preconditions tests/test_concap_restate_cpu.py checks on the CPU.  Every case:
  * read checks: feat, cls and boxes hold NaN in the rows >= num_boxes and in 3 further rows past B * R; the caption table holds a filler
    id beyond cap_len and in the rows [n_caps, n_rows).  One stray read shows as a NaN or as the filler in an output.
  * write checks: each of the ten outputs lies between two guard bands and is prefilled, bands included, with a canary (fp32 bits
    0xFFA5A5A5, a NaN no arithmetic here produces; int64 -0x5A5A5A5A5A5A5A5B).  Inside the contract's shape no element keeps the canary
    and no float is NaN; the bands keep their bits.
  * values: the three float outputs equal the restatement bit for bit -- the copies trivially, image_loc because every operation of it is
    one IEEE fp32 operation, the global feature row because the kernel adds the rows in order r = 0 .. R-1 and divides once; the integer
    outputs equal it exactly."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import concap_restate as CR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64                          # elements of canary in front of and behind every output
XROWS = 3                           # NaN rows behind feat / cls / boxes
CAN32 = 0xFFA5A5A5 - (1 << 32)
CAN64 = -0x5A5A5A5A5A5A5A5B
INPUTS = ("cap_tokens", "cap_len", "cap_index", "feat", "cls", "boxes", "num_boxes", "img_wh")
OUTPUTS = ("input_ids", "input_mask", "segment_ids", "lm_label_ids", "is_match", "image_feat", "image_loc", "image_cls", "image_label", "image_mask")
CASES = CR.cases()
BY_ID = {c.id: c for c in CASES}


def _lib():
    from volta_amd import _lib as L
    return L


def _shapes(B, T, Rl, F, Cn, add_global):
    Rv = Rl + (1 if add_global else 0)
    return dict(input_ids=(B, T), input_mask=(B, T), segment_ids=(B, T), lm_label_ids=(B, T), is_match=(B,), image_feat=(B, Rv, F),
                image_loc=(B, Rv, 5), image_cls=(B, Rl, Cn), image_label=(B, Rl), image_mask=(B, Rv))


def _padded(x):
    """[B, R, k] -> device [B * R + XROWS, k] with NaN rows behind the batch."""
    flat = x.reshape(-1, x.shape[-1])
    return torch.from_numpy(np.concatenate([flat, np.full((XROWS, x.shape[-1]), np.nan, np.float32)])).to(DEV)


def _launch(L, inp, launches=1, **over):
    """One (or more) vk_concap_batch launches into fresh canaried buffers.  -> (return code, {output: host array with its guard bands})."""
    B, Rl, F = inp["feat"].shape
    Cn = inp["cls"].shape[2]
    dev = {k: (_padded(inp[k]) if k in ("feat", "cls", "boxes") else torch.from_numpy(np.ascontiguousarray(inp[k])).to(DEV)) for k in INPUTS}
    geo = dict(B=B, T=inp["T"], R=Rl, F=F, C=Cn, n_caps=inp["n_caps"], cap_ld=inp["cap_tokens"].shape[1], vocab_size=inp["V"], cls_id=inp["cls_id"],
               sep_id=inp["sep_id"], mask_id=inp["mask_id"], add_global=inp["add_global"], objective=inp["objective"], visualization=inp["visualization"])
    shapes = _shapes(B, inp["T"], Rl, F, Cn, inp["add_global"])          # the buffers keep the case's shape whatever `over` asks the host to refuse
    geo.update(over)
    out = {}
    for k in OUTPUTS:
        size = int(np.prod(shapes[k]))
        is_f = k in CR.FLOAT_KEYS
        out[k] = torch.full((GUARD + size + GUARD,), CAN32 if is_f else CAN64, dtype=torch.int32 if is_f else torch.int64, device=DEV)
    ptr = {k: C.c_void_p(t.data_ptr()) for k, t in dev.items()}
    ptr.update({k: C.c_void_p(t.data_ptr() + GUARD * t.element_size()) for k, t in out.items()})
    a = L.ConcapArgs(seed=int(inp["seed"]), **ptr, **geo)
    rc = 0
    for _ in range(launches):
        rc = L.lib.vk_concap_batch(C.byref(a), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, {k: t.cpu().numpy() for k, t in out.items()}


def _split(host, shapes):
    """-> ({output: interior in its shape, floats as uint32 bits}, [outputs whose guard bands changed])."""
    inner, broken = {}, []
    for k, raw in host.items():
        can = np.int32(CAN32) if raw.dtype == np.int32 else np.int64(CAN64)
        if not ((raw[:GUARD] == can).all() and (raw[len(raw) - GUARD:] == can).all()):
            broken.append(k)
        body = raw[GUARD:len(raw) - GUARD].reshape(shapes[k])
        inner[k] = body.view(np.uint32) if raw.dtype == np.int32 else body
    return inner, broken


def _run_case(case, **kw):
    L = _lib()
    inp, ref = CR.reference(case)
    rc, host = _launch(L, inp, **kw)
    assert rc == 0, L.lib.vk_last_error().decode()
    B, Rl, F = inp["feat"].shape
    inner, broken = _split(host, _shapes(B, inp["T"], Rl, F, inp["cls"].shape[2], inp["add_global"]))
    return inp, ref, inner, broken


def _check(case, ref, inner, broken):
    assert broken == [], "%s: written outside the contract's shape: %s" % (case.id, broken)
    for k in OUTPUTS:
        got, want = inner[k], CR.bits(ref[k])
        assert got.shape == want.shape, (case.id, k)
        if k in CR.FLOAT_KEYS:
            assert not (got == np.uint32(0xFFA5A5A5)).any(), "%s: %s elements of the write set were not written" % (case.id, k)
            assert not np.isnan(got.view(np.float32)).any(), "%s: %s holds NaN (a read of the padding)" % (case.id, k)
        else:
            assert not (got == np.int64(CAN64)).any(), "%s: %s elements of the write set were not written" % (case.id, k)
            assert not (got == CR.SENT).any(), "%s: %s holds the caption-table filler" % (case.id, k)
        bad = np.argwhere(got != want)
        if len(bad):
            i = tuple(bad[0])
            gv, wv = (got.view(np.float32)[i], ref[k][i]) if k in CR.FLOAT_KEYS else (got[i], want[i])
            pytest.fail("%s: %s differs from the restatement in %d of %d elements (pairs %s), first at %s: got %r, want %r"
                        % (case.id, k, len(bad), got.size, sorted(set(int(x) for x in bad[:, 0])), tuple(int(x) for x in i), gv, wv))


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_kernels_equal_restatement(case):
    inp, ref, inner, broken = _run_case(case)
    _check(case, ref, inner, broken)
    if case.visualization:
        assert (inner["lm_label_ids"] == -1).all() and (inner["image_label"] == -1).all() and (inner["is_match"] == 0).all()
        off = 1 if case.add_global == 1 else 0
        for b in range(case.B):
            n = int(inp["num_boxes"][b])
            assert np.array_equal(inner["image_feat"][b, off:off + n], inp["feat"][b, :n].view(np.uint32))
    if case.id == "threshold_word":
        assert inner["image_label"][0, 0] == 1        # word 644245094: 644245094 / 2^32 < 0.15


def test_refusals_write_nothing():
    L = _lib()
    inp, _ = CR.reference(BY_ID["cls_C1"])
    for over in (dict(R=257), dict(R=0), dict(T=2), dict(F=0), dict(C=0), dict(n_caps=0), dict(vocab_size=0), dict(add_global=3), dict(objective=3)):
        rc, host = _launch(L, inp, **over)
        assert rc != 0, over
        assert "vk_concap_batch" in L.lib.vk_last_error().decode(), over
        for k, raw in host.items():
            assert (raw == (CAN32 if raw.dtype == np.int32 else CAN64)).all(), (over, k)


def test_empty_batch_writes_nothing():
    L = _lib()
    inp, _ = CR.reference(BY_ID["cls_C1"])
    rc, host = _launch(L, inp, B=0)
    assert rc == 0
    for k, raw in host.items():
        assert (raw == (CAN32 if raw.dtype == np.int32 else CAN64)).all(), k


def test_two_launches_same_bits():
    L = _lib()
    for cid in ("objective1", "regions_R256"):
        inp, _ = CR.reference(BY_ID[cid])
        _, h1 = _launch(L, inp)
        _, h2 = _launch(L, inp, launches=2)
        for k in OUTPUTS:
            assert np.array_equal(h1[k], h2[k]), (cid, k)


def test_pair_zero_does_not_depend_on_the_batch():
    """The Philox counter holds the pair index, so the statement is made for the record at index 0 of both launches."""
    L = _lib()
    inp, _ = CR.reference(BY_ID["objective0"])

    def first(n):
        d = dict(inp)
        for k in ("feat", "cls", "boxes", "num_boxes", "img_wh", "cap_index"):
            d[k] = np.ascontiguousarray(inp[k][:n])
        rc, host = _launch(L, d)
        assert rc == 0
        Rl, F = d["feat"].shape[1:]
        inner, broken = _split(host, _shapes(n, d["T"], Rl, F, d["cls"].shape[2], d["add_global"]))
        assert broken == []
        return inner

    eight, one = first(8), first(1)
    for k in OUTPUTS:
        assert np.array_equal(eight[k][0], one[k][0]), k


@pytest.mark.parametrize("fault", ["cnt_plus_one", "region_next_slot"])
def test_comparison_is_not_vacuous(fault):
    """The kernels' output does not compare equal to a restatement with the divisor off by one or with the region word of slot r + 1."""
    inp, ref, inner, _ = _run_case(BY_ID["objective0"])
    wrong = CR.restate_inputs(inp, fault=fault)
    assert not np.array_equal(inner["image_feat"], CR.bits(wrong["image_feat"]))
    assert np.array_equal(inner["image_feat"], CR.bits(ref["image_feat"]))
    if fault == "region_next_slot":
        assert not np.array_equal(inner["image_label"], wrong["image_label"])
