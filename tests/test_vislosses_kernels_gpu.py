"""csrc/vislosses.hip (and vk_pool_mul_* of csrc/heads.hip) through the C ABI against the float64 restatements and derived gates of
tests/vis_restate.py.  Every case lays its buffers out the way tests/test_attention_kernels_gpu.py does:
  * read checks: logits has ld > V where the case says so, NaN in its pad columns and in every row at and past the labelled ones;
    target rows that are neither labelled nor drawn as a labelled row's negative hold NaN; labels at unlabelled positions hold 2^40
    and conf holds NaN there; the pooled vectors' gradient has NaN in its pad columns.  One stray read shows as a non-finite result.
  * write checks: dlogits, lse, aux and the fusion outputs are prefilled with the NaN canaries 0xFFA5 / 0xFFA5A5A5.  Columns [V, ldd) of
    rows < n must be exactly +0; rows >= n, the guard rows past max_rows, aux columns past n_neg and the guard bands behind the fusion
    outputs keep their canary; with *count = 0 no byte of dlogits changes and *loss_sum keeps its bits.
  * *loss_sum starts at 3.0; a second forward adds the same amount again (both within the gate; the atomics' order is free and the
    forward is not asserted to be deterministic).  Every backward runs twice into fresh canaried buffers and must give the same bits.
Measured on the MI355X (167 tests with tests/test_seed_gather_kernels_gpu.py, 3 s), worst |got - ref| / gate over the table:
  loss_sum  mse 0.044, huber 0.040, xent 0.066, nce 0.021        lse  xent 0.12, nce 0.035        aux  nce 0.074 (integer family: exact)
  dlogits   mse 1.000, huber 1.000, xent 0.998, nce 0.993 of the whole gate, which half a bf16 ulp -- the output's own rounding -- dominates,
            as it does for every bf16 output of the other suites; what the error exceeds that rounding by takes 0.131 (mse), 0 (huber),
            0.038 (xent) and 0.002 (nce) of the fp32 part of the gate (vis_restate.fp32_share)
  dlogits not the exactly rounded value: at most 0.056 % of a case's elements (mse, xent), none (huber), 0.11 % (nce, Gaussian
            family); nce up to 36 % in the wide and integer families, whose softmax is one-hot to fp32 (p - 1 cancels: 1e-20 in
            float64, 0 in fp32) -- inside the gate, which carries 4u |p - onehot| for exactly that
  fusions   p = 0 and p = 0.5: every element the exactly rounded value; p = 0.1: out 0.31 % (mul) and 0.39 % (sum) of the elements one
            step away, dyt / dyv of mul 0.10 % / 0.08 %, text none -- each exactly the share numpy fp32 leaves (the cap is twice that)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from oracle import volta_ref as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vis_restate as VR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
CAN16 = -91                         # bf16 canary bits 0xFFA5: a negative NaN no bf16 conversion produces
CAN32 = 0xFFA5A5A5 - (1 << 32)      # fp32 / int32 canary bits
CASES = VR.loss_cases()
_REF = {}


def _lib():
    from volta_amd import _lib as L
    return L


def _p(t):
    """Raw pointer of a device tensor; the caller keeps the tensor referenced until the launch has run."""
    return None if t is None else C.c_void_p(t.data_ptr())


def _canary16(shape):
    return torch.full(shape, CAN16, dtype=torch.int16, device=DEV)


def _canary32(shape):
    return torch.full(shape, CAN32, dtype=torch.int32, device=DEV)


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ref(case):
    if case.id not in _REF:
        inp = VR.make_inputs(case)
        _REF[case.id] = (inp, VR.restate(inp))
    return _REF[case.id]


def _launch(L, inp, forwards=2):
    """Two forwards over *loss_sum = 3.0 and two backwards into fresh canaried buffers.  -> dict of host arrays."""
    c = inp["case"]
    rows = c.max_rows + VR.XR
    d = {k: _dev(inp[k]) for k in ("logits", "target", "labels", "conf", "pos", "neg")}
    count = torch.tensor([c.count], dtype=torch.int32, device=DEV)
    lse, aux = _canary32((rows,)), _canary32((rows, VR.NCE_MAX_SAMPLES))
    loss = torch.tensor([VR.LOSS_START], dtype=torch.float32, device=DEV)
    g = torch.tensor([c.gscale], dtype=torch.float32, device=DEV)
    a = L.VisLossArgs(_p(d["logits"]), _p(d["target"]), _p(d["labels"]), _p(d["conf"]), _p(d["pos"]), _p(count), _p(d["neg"]), _p(lse), _p(aux), _p(loss),
                      c.weight, c.V, c.ld, c.max_rows, c.kind, c.n_neg)
    losses = []
    for _ in range(forwards):
        L.check(L.lib.vk_vis_loss_fwd(C.byref(a), L.stream_ptr()))
        torch.cuda.synchronize()
        losses.append(loss.cpu().numpy().copy())
    dl = [_canary16((rows, c.ldd)) for _ in range(2)]
    for t in dl:
        L.check(L.lib.vk_vis_loss_bwd(C.byref(a), _p(t), c.ldd, _p(g), L.stream_ptr()))
    torch.cuda.synchronize()
    return dict(losses=losses, lse=lse.cpu().numpy(), aux=aux.cpu().numpy(), dl=[_u16(t) for t in dl])


def _check_case(case, inp, ref, out):
    """The write set, the read poison (through finiteness), the gates and the exact cases.  -> {output: worst ratio}."""
    n, V, kind = ref["n"], case.V, case.kind
    can16, can32 = np.uint16(0xFFA5), np.int32(CAN32)
    dl, dl2 = out["dl"]
    assert np.array_equal(dl, dl2), "%s: two backwards differ" % case.id
    assert (dl[n:] == can16).all(), "%s: dlogits rows at and past n = %d were written" % (case.id, n)
    assert (dl[:n, V:] == 0).all(), "%s: dlogits pad columns are not +0" % case.id
    assert not (dl[:n, :V] == can16).any(), "%s: dlogits elements of the write set were not written" % case.id
    has_lse = kind in (VR.XENT, VR.NCE)
    assert (out["lse"][n if has_lse else 0:] == can32).all(), "%s: lse outside the write set was written" % case.id
    ns = case.n_neg + 1 if kind == VR.NCE else 0
    assert (out["aux"][n:] == can32).all() and (out["aux"][:, ns:] == can32).all(), "%s: aux outside the write set was written" % case.id
    got = dict(dlogits=VR.bf16_value(dl[:n, :V]), lse=out["lse"][:n].view(np.float32), aux=out["aux"][:n, :ns].view(np.float32))
    worst = {}
    for k, l in enumerate(out["losses"], 1):
        got["loss"] = float(l[0])
        if n == 0:
            assert l.view(np.int32)[0] == np.float32(VR.LOSS_START).view(np.int32), "%s: loss_sum changed with no rows" % case.id
        res = VR.check_loss(ref, got, case, k=k)
        for name, r in res.items():
            worst[name] = max(worst.get(name, 0.0), r)
        assert VR.exact_checks(ref, got, case, k=k) == [], case.id
    print("%s: %s" % (case.id, " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert all(r <= 1.0 for r in worst.values()), (case.id, worst)
    if n:
        inexact = dl[:n, :V] != VR.bf16_bits(ref["dlogits"])
        print("%s dlogits: %.4f%% of the elements are not the exactly rounded value; beyond its own bf16 round the error takes %.3f of the fp32 gate"
              % (case.id, 100 * float(inexact.mean()), VR.fp32_share(got["dlogits"], ref)))
    return worst


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_vis_loss_against_float64(case):
    L = _lib()
    inp, ref = _ref(case)
    _check_case(case, inp, ref, _launch(L, inp))


@pytest.mark.parametrize("case", VR.over_count_cases(), ids=[c.id for c in VR.over_count_cases()])
def test_count_above_max_rows_writes_nothing_past_max_rows(case):
    """*count > max_rows is outside the contract (the header requires count <= max_rows; vk_select_rows cannot give more): only the
    write set is pinned -- the guard rows past max_rows of dlogits, lse and aux keep their canary."""
    L = _lib()
    inp = VR.make_inputs(case)
    out = _launch(L, inp, forwards=1)
    mr = case.max_rows
    assert (out["dl"][0][mr:] == np.uint16(0xFFA5)).all() and (out["dl"][1][mr:] == np.uint16(0xFFA5)).all()
    assert (out["lse"][mr:] == np.int32(CAN32)).all() and (out["aux"][mr:] == np.int32(CAN32)).all()


@pytest.mark.parametrize("conf", [False, True])
def test_xent_out_of_range_labels_are_clamped_in_both_directions(conf):
    """Labels -1 and V at two labelled rows: the forward charges lse - x[clamped] and the backward must put the one-hot at the same
    clamped column (0 and V - 1).  Before this test the backward compared the raw label and subtracted no one-hot at all."""
    L = _lib()
    case = VR._case(VR.XENT, 257, 1, conf=conf)
    inp = VR.make_inputs(case)
    inp["labels"][VR.LABELLED[1]], inp["labels"][VR.LABELLED[4]] = -1, case.V
    ref = VR.restate(inp)
    out = _launch(L, inp)
    _check_case(case, inp, ref, out)
    dl = VR.bf16_value(out["dl"][0])
    assert dl[1, 0] < 0 and dl[4, case.V - 1] < 0                     # p - 1 at the clamped class
    assert (np.delete(dl[1, :case.V], 0) >= 0).all() and (dl[4, :case.V - 1] >= 0).all()


# ------------------------------------------------------------------------------------------------ negatives
def _negatives(L, B, Rn, seed, site):
    nneg = L.NCE_ACROSS + L.NCE_INSIDE
    seed_t = torch.tensor([seed], dtype=torch.int64, device=DEV)
    buf = _canary32((B * Rn * nneg + 64,))
    L.check(L.lib.vk_nce_negatives(L.rng_cfg(seed_t.data_ptr(), site), B, Rn, _p(buf), L.stream_ptr()))
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[B * Rn * nneg:] == np.int32(CAN32)).all(), "the canary past B * R * 127 was written"
    return out[:B * Rn * nneg].reshape(B, Rn, nneg)


@pytest.mark.parametrize("B,Rn", [(2, 2), (2, 3), (3, 2), (4, 7), (5, 37)])
def test_nce_negatives_bit_for_bit(B, Rn):
    L = _lib()
    seed, site = 0x5EEDF00D1234 + B, 17 + Rn
    got = _negatives(L, B, Rn, seed, site)
    want = R.nce_negative_index(R.nce_draws(seed, site, B, Rn), B, Rn).numpy()
    assert np.array_equal(got, want)
    na = L.NCE_ACROSS
    b, r = np.arange(B)[:, None, None], np.arange(Rn)[None, :, None]
    assert (got >= 0).all() and (got < B * Rn).all()
    assert (got[..., :na] // Rn != b).all()                           # across: never the region's own image
    assert (got[..., na:] // Rn == b).all() and (got[..., na:] % Rn != r).all()      # inside: the same image, never the region itself


def test_generated_negatives_feed_the_nce_loss():
    """(B, R) = (2, 2): vk_nce_negatives' output, as it stands on the device, is the neg_index of an NCE forward and backward."""
    L = _lib()
    B, Rn, seed, site = 2, 2, 0xABCDEF0123456, 5
    neg = _negatives(L, B, Rn, seed, site).reshape(B * Rn, -1)
    labelled = (0, 3)
    case = VR.Case("nce-e2e-2x2", VR.NCE, 256, neg.shape[1], "gauss", False, 268, 320, len(labelled), len(labelled), 0.7, 1.7)
    inp = VR.make_inputs(case, seed=11, grid=(B, Rn), labelled=labelled, neg=neg.astype(np.int32))
    _check_case(case, inp, VR.restate(inp), _launch(L, inp))


# ------------------------------------------------------------------------------------------------ fusions
GUARD = 64


def _fuse_run(L, pt, pv, dp, B, P, ldp, mode, p, mul_entry=False):
    """-> (out, dyt, dyv) bf16 bits; guard bands behind each output and the NaN pad of dp are checked here."""
    seed_t = torch.tensor([VR.FUSE_SEED], dtype=torch.int64, device=DEV)
    drop = L.dropout_cfg(seed_t.data_ptr(), VR.FUSE_SITE, p)
    a, b = _dev(pt.view(np.int16)), _dev(pv.view(np.int16))
    dpad = np.full((B, ldp), 0x7FC0, np.uint16)
    dpad[:, :P] = dp
    d = _dev(dpad.view(np.int16))
    outs = [_canary16((B * P + GUARD,)) for _ in range(3)]
    text = mode == VR.FUSE_TEXT
    if mul_entry:
        L.check(L.lib.vk_pool_mul_fwd(_p(a), _p(b), _p(outs[0]), B, P, drop, L.stream_ptr()))
        L.check(L.lib.vk_pool_mul_bwd(_p(d), ldp, _p(a), _p(b), _p(outs[1]), _p(outs[2]), B, P, drop, L.stream_ptr()))
    else:
        L.check(L.lib.vk_pool_fuse_fwd(_p(a), None if text else _p(b), _p(outs[0]), B, P, mode, drop, L.stream_ptr()))
        L.check(L.lib.vk_pool_fuse_bwd(_p(d), ldp, _p(a), None if text else _p(b), _p(outs[1]), None if text else _p(outs[2]), B, P, mode, drop, L.stream_ptr()))
    torch.cuda.synchronize()
    res = []
    for i, t in enumerate(outs):
        h = _u16(t)
        assert (h[B * P:] == np.uint16(0xFFA5)).all(), "guard band behind output %d was written" % i
        if text and i == 2:
            assert (h == np.uint16(0xFFA5)).all(), "text mode wrote dyv"
            res.append(None)
        else:
            res.append(h[:B * P].reshape(B, P))
    return res


@pytest.mark.parametrize("p", VR.FUSE_DROP)
@pytest.mark.parametrize("B", VR.FUSE_B)
@pytest.mark.parametrize("P", VR.FUSE_P)
def test_pool_fusions_exact_bits(B, P, p):
    """The three modes of vk_pool_fuse_* and vk_pool_mul_* (bit-equal to mode MUL), ldp = P and P + 8 with NaN in the pad.  p = 0: the
    exactly rounded bits.  p > 0: within one bf16 step, the inexact share under twice what numpy fp32 leaves (vis_restate.check_fused)."""
    L = _lib()
    pt, pv, dp = VR.pooled_inputs(B, P, seed=B * 4096 + P)
    for mode in (VR.FUSE_MUL, VR.FUSE_SUM, VR.FUSE_TEXT):
        ref = VR.fuse_restate(pt, pv, dp, mode, p)
        npb = VR.fuse_fp32(pt, pv, dp, mode, p)
        got = None
        for ldp in (P, P + 8):
            g = _fuse_run(L, pt, pv, dp, B, P, ldp, mode, p)
            if got is not None:
                assert all(x is None or np.array_equal(x, y) for x, y in zip(g, got)), "the result depends on ldp"
            got = g
        for name, gb, r, nb in zip(("out", "dyt", "dyv"), got, ref, npb):
            if r is None:
                continue
            bad, share, steps = VR.check_fused(gb, r, p, nb)
            cap = 2 * float((VR.ordered(nb) != VR.ordered(VR.bf16_bits(r))).mean())
            print("fuse mode %d B %d P %d p %.1f %s: %.4f%% not exactly rounded (cap %.4f%%), worst %d bf16 steps" % (mode, B, P, p, name, 100 * share, 100 * cap, steps))
            assert bad is None, (mode, B, P, p, name, bad)
        dead = ~(VR.bf16_value(pt) > 0)
        assert (got[1][dead] == 0).all(), "a dead element of pt passes gradient (or carries -0)"
        if mode != VR.FUSE_TEXT:
            assert (got[2][~(VR.bf16_value(pv) > 0)] == 0).all(), "a dead element of pv passes gradient (or carries -0)"
        if mode == VR.FUSE_MUL:
            mul = _fuse_run(L, pt, pv, dp, B, P, P + 8, mode, p, mul_entry=True)
            assert all(np.array_equal(x, y) for x, y in zip(mul, got)), "vk_pool_mul_* and vk_pool_fuse_*(MUL) differ"


# ------------------------------------------------------------------------------------------------ text end rows
@pytest.mark.parametrize("T", VR.TEXT_T)
def test_text_end_rows(T):
    """Captions with 0, 1, 2 and T non-zero ids, a ragged one, and one with a zero in its interior (the header says the NUMBER of non-zero
    ids); T on both sides of the kernel's stride of 64; *count = B; the canary behind rows intact."""
    L = _lib()
    ids = VR.text_ids(T)
    B = ids.shape[0]
    idc = _dev(ids)
    rows, cnt = _canary32((B + 8,)), _canary32((2,))
    L.check(L.lib.vk_text_end_rows(_p(idc), B, T, _p(rows), _p(cnt), L.stream_ptr()))
    torch.cuda.synchronize()
    r, c = rows.cpu().numpy(), cnt.cpu().numpy()
    assert np.array_equal(r[:B], VR.text_end_rows_restate(ids)) and (r[B:] == np.int32(CAN32)).all()
    assert c[0] == B and c[1] == np.int32(CAN32)
