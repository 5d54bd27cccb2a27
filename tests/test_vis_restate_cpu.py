"""tests/vis_restate.py checked without a GPU.
  * Acceptance: a plain numpy fp32 evaluation of every formula, written here and independent of the float64 path, passes the derived
    gates with no element excluded, in every family and at every shape of the table -- the gates are not too tight.
  * Rejection: the same evaluation with one planted fault is refused, in every case the fault applies to -- they are not too loose.
  * The hosts' refusals of vk_vis_loss_*, vk_grad_seed, vk_nce_negatives and vk_pool_fuse_* through the loaded library: each is decided
    before any launch, so no GPU is touched.
Worst |fp32 evaluation - float64| / gate over the table, as measured: loss_sum 0.081, lse 0.091, aux 0.075; dlogits 1.000 of the whole
gate (half a bf16 ulp, the output's own rounding, dominates it) and 0.131 of its fp32 part beyond that rounding."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vis_restate as VR  # noqa: E402

f32 = np.float32
CASES = VR.loss_cases()
_REF = {}


def _ref(case):
    if case.id not in _REF:
        inp = VR.make_inputs(case)
        _REF[case.id] = (inp, VR.restate(inp))
    return _REF[case.id]


def _bf(x):
    return VR.bf16_value(VR.f32_to_bf16_bits(x))


def _lse32(s):
    m = s.max(-1, keepdims=True)
    return (m + np.log(np.exp(s - m).sum(-1, keepdims=True, dtype=f32)))[..., 0].astype(f32)


def eval32(inp, bug=None, forwards=1):
    """One forward (x `forwards`) and backward in numpy fp32, laid out like the kernels' outputs.  `bug` plants one fault."""
    c = inp["case"]
    V, kind = c.V, c.kind
    n = min(c.count, c.max_rows, inp["nl"])
    w, g = f32(c.weight), f32(c.gscale)
    if bug == "gscale_dropped":
        g = f32(1.0)
    x = inp["logits"][:n, :V]
    pos = inp["pos"][:n]
    div = f32(max(c.max_rows if bug == "div_max_rows" else n, 1))
    got = {}
    if kind in (VR.MSE, VR.HUBER):
        d = x - inp["target"][pos]
        ad = np.abs(d)
        term = d * d if kind == VR.MSE else np.where(ad < 1, f32(0.5) * d * d, ad - f32(0.5))
        rows = w * term.sum(1, dtype=f32) / f32(V)
        lim = f32(0.5 if bug == "huber_clamp_half" else 1.0)
        dl = g * w / (div * f32(V)) * (f32(2) * d if kind == VR.MSE else np.clip(d, -lim, lim))
    elif kind == VR.XENT:
        lab = np.clip(inp["labels"][pos], 0, V - 1)
        cf = inp["conf"][pos] if (inp["conf"] is not None and bug != "conf_ignored") else np.ones(n, f32)
        lse = _lse32(x) if n else np.zeros(0, f32)
        got["lse"] = lse
        rows = w * cf * (lse - x[np.arange(n), lab])
        oh = np.zeros((n, V), f32)
        oh[np.arange(n), lab] = 1
        if bug == "onehot_missing" and n:
            oh[n // 2] = 0
        dl = (np.exp(x - lse[:, None]) - oh) * (g * w * cf / div)[:, None]
    else:
        nn = c.n_neg
        flat = inp["neg"].reshape(-1)
        j0 = 1 if bug == "nce_off_by_one" else 0
        nidx = np.stack([flat[np.minimum(p * nn + j0 + np.arange(nn), flat.size - 1)] for p in pos]) if n else np.zeros((0, nn), np.int64)
        idx = np.concatenate([pos[:, None].astype(np.int64), nidx.astype(np.int64)], 1)
        smp = inp["target"][idx]
        s = np.einsum("njc,nc->nj", smp, x).astype(f32)
        lse = _lse32(s) if n else np.zeros(0, f32)
        got["lse"], got["aux"] = lse, s
        rows = w * (lse - s[:, 0])
        oh = np.zeros_like(s)
        oh[:, 0] = 1
        if bug == "onehot_missing" and n:
            oh[n // 2] = 0
        q = (np.exp(s - lse[:, None]) - oh) * (g * w / div)
        dl = np.einsum("nj,njc->nc", q, smp).astype(f32)
    if bug == "weight_twice":
        rows, dl = rows * w, dl * w
    dl = dl.astype(f32)
    if bug == "last_col_pad" and n:
        dl[:, V - 1] = 0
    loss = f32(VR.LOSS_START)
    for _ in range(forwards):
        for r in rows.astype(f32):
            loss = f32(loss + r)
    got["loss"], got["dlogits"] = float(loss), _bf(dl)
    return got


# ------------------------------------------------------------------------------------------------ acceptance
WORST = {}


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_fp32_evaluation_passes_the_gates(case):
    inp, ref = _ref(case)
    with np.errstate(all="ignore"):
        for k in (1, 2):
            got = eval32(inp, forwards=k)
            res = VR.check_loss(ref, got, case, k=k)
            for name, r in res.items():
                WORST[name] = max(WORST.get(name, 0.0), r)
            assert all(r <= 1.0 for r in res.values()), (case.id, k, res)
            assert VR.exact_checks(ref, got, case, k=k) == [], case.id
    WORST["dlogits beyond its bf16 round / fp32 gate"] = max(WORST.get("dlogits beyond its bf16 round / fp32 gate", 0.0), VR.fp32_share(got["dlogits"], ref))
    print("%s: %s" % (case.id, " ".join("%s %.3f" % kv for kv in sorted(res.items()))))


def test_zz_worst_ratios_of_the_fp32_evaluation():
    """Printed for the record (after the table above ran); every ratio stays below 1 by the tests above."""
    if not WORST:
        with np.errstate(all="ignore"):
            for case in CASES:
                inp, ref = _ref(case)
                for name, r in VR.check_loss(ref, eval32(inp), case).items():
                    WORST[name] = max(WORST.get(name, 0.0), r)
    print("worst fp32 / gate: " + ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))
    assert all(r <= 1.0 for r in WORST.values())


def test_the_table_covers_what_it_claims():
    by = {}
    for c in CASES:
        by.setdefault(c.kind, []).append(c)
    nl = len(VR.LABELLED)
    for kind in (VR.MSE, VR.HUBER, VR.XENT):
        cs = by[kind]
        assert {c.V for c in cs} >= set(VR.VS)
        assert any(c.V == 1601 and c.ldd == 1601 for c in cs) and any(c.V == 1601 and c.ldd == 1728 for c in cs)
    assert {(c.V, c.n_neg) for c in by[VR.NCE] if c.family == "gauss" and c.count == nl} >= {(V, nn) for V in VR.NCE_VS for nn in VR.NCE_NEGS}
    for kind, cs in by.items():
        assert {c.count for c in cs} >= {0, 1, nl} and {c.max_rows for c in cs} == {nl, nl + 2}
        assert any(c.count == c.max_rows for c in cs)
        assert {c.gscale for c in cs} == {1.0, 0.7, 2.0 ** -10}
        assert any(c.ld == c.V for c in cs) and any(c.ld == c.V + 12 for c in cs)
        assert all(c.ld % 4 == 0 and c.V % 4 == 0 for c in cs if c.kind == VR.NCE)
        fams = {c.family for c in cs}
        assert fams == {VR.XENT: {"gauss", "wide"}, VR.NCE: {"gauss", "wide", "int"}}.get(kind, {"gauss", "int"})
    assert any(c.conf for c in by[VR.XENT]) and any(not c.conf for c in by[VR.XENT])
    for c in by[VR.XENT]:
        if c.V == 1:                                                         # one class: loss 0 and gradient 0
            ref = _ref(c)[1]
            assert ref["n"] and not ref["rows"].any() and not ref["dlogits"].any()
    assert 0 in VR.LABELLED and VR.GRID_B * VR.GRID_R - 1 in VR.LABELLED


def test_makers_poison_everything_outside_the_contract():
    for case in CASES:
        inp = VR.make_inputs(case)
        lg, nl = inp["logits"], inp["nl"]
        assert np.isnan(lg[nl:]).all() and np.isnan(lg[:, case.V:]).all() and np.isfinite(lg[:nl, :case.V]).all()
        lab = np.zeros(VR.GRID_B * VR.GRID_R, bool)
        lab[list(VR.LABELLED)] = True
        if inp["labels"] is not None:
            assert (inp["labels"][~lab] == VR.LABEL_POISON).all()
        if inp["conf"] is not None:
            assert np.isnan(inp["conf"][~lab]).all() and np.isfinite(inp["conf"][lab]).all()
        if inp["target"] is not None:
            used = lab.copy()
            if inp["neg"] is not None:
                used[inp["neg"][lab].reshape(-1)] = True
            assert np.isnan(inp["target"][~used]).all() and np.isfinite(inp["target"][used]).all()


def test_wide_rows_reach_a_hundred_and_integer_sums_are_exact():
    for case in CASES:
        inp, ref = _ref(case)
        if case.family == "wide" and ref["n"] > 1:
            s = ref["aux"][1] if case.kind == VR.NCE else inp["logits"][1, :case.V].astype(np.float64)
            assert s.max() > 80 and s.min() < -80, (case.id, s.max(), s.min())
            assert np.isfinite(ref["dlogits"]).all() and np.isfinite(ref["rows"]).all()
        if case.family == "int" and ref["n"]:
            if case.kind == VR.NCE:
                assert np.array_equal(ref["aux"], ref["aux"].astype(f32).astype(np.float64)) and np.abs(ref["aux"]).max() < 2 ** 24
            else:
                tot = VR.LOSS_START + 2 * ref["rows"].sum()
                assert float(f32(tot)) == tot
    huber = [c for c in CASES if c.kind == VR.HUBER and c.family == "gauss" and c.V >= 63]
    for case in huber:                                                       # both branches of the smooth-l1 are met
        inp, ref = _ref(case)
        if ref["n"]:
            d = np.abs(inp["logits"][:ref["n"], :case.V] - inp["target"][inp["pos"][:ref["n"]]])
            assert (d < 1).any() and (d > 1).any()


# ------------------------------------------------------------------------------------------------ rejection
def _applies(bug, c):
    n = min(c.count, c.max_rows)
    if n == 0 or (c.kind == VR.XENT and c.V == 1):          # one class: the loss and its gradient are 0 whatever the scale
        return False
    return {
        "div_max_rows": c.max_rows != n,
        "onehot_missing": c.kind in (VR.XENT, VR.NCE) and n > 1,
        "last_col_pad": True,
        "huber_clamp_half": c.kind == VR.HUBER,
        "conf_ignored": c.kind == VR.XENT and c.conf,
        "weight_twice": True,
        "nce_off_by_one": c.kind == VR.NCE,
        "gscale_dropped": c.gscale != 1.0,
    }[bug]


LOSS_BUGS = ("div_max_rows", "onehot_missing", "last_col_pad", "huber_clamp_half", "conf_ignored", "weight_twice", "nce_off_by_one", "gscale_dropped")


@pytest.mark.parametrize("bug", LOSS_BUGS)
def test_planted_faults_are_rejected(bug):
    """Every case the fault applies to refuses it (a ratio above 1 or a failed exact check), in every family."""
    seen = {}
    with np.errstate(all="ignore"):
        for case in CASES:
            if not _applies(bug, case):
                continue
            inp, ref = _ref(case)
            got = eval32(inp, bug=bug)
            res = VR.check_loss(ref, got, case)
            caught = any(not r <= 1.0 for r in res.values()) or bool(VR.exact_checks(ref, got, case))
            assert caught, (bug, case.id, res)
            seen.setdefault(case.kind, set()).add(case.family)
    want = {VR.XENT: {"gauss", "wide"}, VR.NCE: {"gauss", "wide", "int"}, VR.MSE: {"gauss", "int"}, VR.HUBER: {"gauss", "int"}}
    kinds = {"huber_clamp_half": (VR.HUBER,), "conf_ignored": (VR.XENT,), "nce_off_by_one": (VR.NCE,), "onehot_missing": (VR.XENT, VR.NCE)}.get(bug, tuple(want))
    for k in kinds:
        assert seen.get(k, set()) >= want[k], (bug, k, seen)


# ------------------------------------------------------------------------------------------------ fusions
def _fuse_cases():
    return [(B, P, mode, p) for B in VR.FUSE_B for P in VR.FUSE_P for mode in (VR.FUSE_MUL, VR.FUSE_SUM, VR.FUSE_TEXT) for p in VR.FUSE_DROP]


def test_fusion_fp32_evaluation_is_exact_without_dropout_and_within_one_step_with_it():
    for B, P, mode, p in _fuse_cases():
        pt, pv, dp = VR.pooled_inputs(B, P, seed=B * 4096 + P)
        ref = VR.fuse_restate(pt, pv, dp, mode, p)
        got = VR.fuse_fp32(pt, pv, dp, mode, p)
        for name, r, gbits in zip(("out", "dyt", "dyv"), ref, got):
            if r is None:
                continue
            bad, _, steps = VR.check_fused(gbits, r, p, gbits)
            assert bad is None and steps <= 1, (B, P, mode, p, name, bad)
        if B * P >= 2:
            assert (pt == 0x8000).any() and (pt == 0).any()
        if B * P >= 256:
            live = VR.bf16_value(pt) > 0
            assert live.any() and (~live).any()
            dyt = VR.bf16_bits(ref[1])
            assert (dyt[~live] == 0).all()                                   # a dead element's gradient is exactly +0


@pytest.mark.parametrize("bug", ["keep_word", "dead_relu_passes", "sum_for_mul", "scale_missing"])
def test_fusion_planted_faults_are_rejected(bug):
    hit = 0
    for B, P, mode, p in _fuse_cases():
        if P < 255 or (bug in ("keep_word", "scale_missing") and p == 0) or (bug == "sum_for_mul" and mode != VR.FUSE_MUL):
            continue
        pt, pv, dp = VR.pooled_inputs(B, P, seed=B * 4096 + P)
        ref = VR.fuse_restate(pt, pv, dp, mode, p)
        honest = VR.fuse_fp32(pt, pv, dp, mode, p)
        if bug == "keep_word":
            got = VR.fuse_fp32(pt, pv, dp, mode, p, keep=VR.keep_scale64(B, P, p, word_bug=True))
        elif bug == "scale_missing":
            got = VR.fuse_fp32(pt, pv, dp, mode, 0.0, keep=VR.keep_scale64(B, P, p))
        elif bug == "sum_for_mul":
            got = VR.fuse_fp32(pt, pv, dp, VR.FUSE_SUM, p)
        else:                                                                # the ReLU gate ignored: gradient flows where pt is dead
            live = np.where(VR.bf16_value(pt) > 0, pt, VR.bf16_bits(np.full(pt.shape, 2.0 ** -6)))
            g = VR.fuse_fp32(live, pv, dp, mode, p)
            got = (honest[0], g[1], honest[2])
        bad = [VR.check_fused(gb, r, p, hb)[0] for gb, r, hb in zip(got, ref, honest) if r is not None]
        assert any(b is not None for b in bad), (bug, B, P, mode, p)
        hit += 1
    assert hit >= 6


def test_small_exact_restatements():
    for T in VR.TEXT_T:
        ids = VR.text_ids(T)
        nz = (ids != 0).sum(1)
        assert list(nz[:4]) == [0, min(1, T), min(2, T), T]
        rows = VR.text_end_rows_restate(ids)
        assert all(rows[b] == b * T + max(int(nz[b]) - 2, 0) for b in range(len(nz)))
        if T >= 3:
            assert ids[5, 1] == 0 and ids[5, 2] != 0 and rows[5] == 5 * T + T - 3   # a zero in the interior: counted, not searched
    src = np.arange(5 * 12, dtype=np.uint8)
    out = VR.pair_gather_restate(src, 12, [4, 0, -1, 5, 4])
    assert np.array_equal(out[:12], src[48:]) and np.array_equal(out[12:24], src[:12]) and not out[24:48].any() and np.array_equal(out[48:], src[48:])
    # grad seed: the gate on y, accumulate, stride-0 sources, canaries kept
    B, L, H, ld, ldy, row0 = 2, 3, 8, 16, 16, 1
    rng = np.random.default_rng(0)
    srcf = rng.standard_normal(H).astype(f32)
    dst = np.full((row0 + B * L + 1, ld), 0xFFA5, np.uint16)
    dst[row0:row0 + B * L, :H] = VR.bf16_bits(rng.standard_normal((B * L, H)))
    y = np.full((B * L, ldy), 0x7FC0, np.uint16)
    y[:, :H] = VR.bf16_bits(np.array([1.0, -1.0, 0.0, -0.0, 2.0, 0.5, -3.0, 1.5]))[None]
    y[0, 0] = 0x7FC0
    out = VR.grad_seed_restate(srcf, 0, 0, B, L, H, dst, row0, ld, y, ldy, 1)
    assert (out[:row0] == 0xFFA5).all() and (out[row0 + B * L:] == 0xFFA5).all() and (out[:, H:] == 0xFFA5).all()
    assert np.array_equal(out[row0:, 1:4][:B * L], dst[row0:, 1:4][:B * L]) and out[row0, 0] == dst[row0, 0]     # closed gates add nothing
    want = VR.f32_to_bf16_bits(srcf[4] + VR.bf16_value(dst[row0 + 1, 4]).astype(f32))
    assert out[row0 + 1, 4] == want
    assert np.array_equal(VR.grad_seed_restate(None, 0, 0, B, L, H, dst, row0, ld, None, 0, 1), dst)
    z = VR.grad_seed_restate(None, 0, 0, B, L, H, dst, row0, ld, None, 0, 0)
    assert (z[row0:row0 + B * L, :H] == 0).all() and (z[:, H:] == 0xFFA5).all()


def test_bf16_helpers_round_to_nearest_even_once():
    import torch
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.standard_normal(4096) * 10.0 ** rng.integers(-30, 30, 4096), [0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 2.0 ** -130]])
    x32 = x.astype(f32)
    t = torch.from_numpy(x32).bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(VR.f32_to_bf16_bits(x32), t) and np.array_equal(VR.bf16_bits(x32.astype(np.float64)), t)
    # a float64 just above a bf16 tie rounds up in one step; through fp32 it would first fall onto the tie and then to even
    v = 1.0 + 2.0 ** -8 + 2.0 ** -40
    assert VR.bf16_bits(np.array([v]))[0] == 0x3F81 and VR.f32_to_bf16_bits(np.array([v], f32))[0] == 0x3F80
    assert VR.ordered(np.array([0x8000, 0x0000, 0x0001, 0x8001], np.uint16)).tolist() == [0, 0, 1, -1]


# ------------------------------------------------------------------------------------------------ host refusals
def _aligned(buf):
    base = ctypes.addressof(buf)
    return base + (-base) % 16


def test_vis_loss_refusals_on_the_host():
    from volta_amd import _lib as L
    buf = (ctypes.c_uint8 * 4096)()
    p = _aligned(buf)

    def args(**kw):
        a = L.VisLossArgs(p, p, p, p, p, p, p, p, p, p, 1.0, 8, 8, 4, L.VIS_XENT, 0)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    nce = dict(kind=L.VIS_NCE, n_neg=3)
    bad = [dict(kind=0), dict(kind=4), dict(kind=6), dict(ld=7), dict(kind=L.VIS_MSE, ld=7), dict(V=6, ld=8, **nce), dict(kind=L.VIS_NCE, n_neg=0),
           dict(kind=L.VIS_NCE, n_neg=128), dict(V=8, ld=10, **nce), dict(labels=None), dict(kind=L.VIS_HUBER, target=None), dict(aux=None, **nce)]
    for kw in bad:
        assert L.lib.vk_vis_loss_fwd(ctypes.byref(args(**kw)), None) != 0, kw
        assert L.lib.vk_last_error().startswith(b"vk_vis_loss_fwd"), kw
        assert L.lib.vk_vis_loss_bwd(ctypes.byref(args(**kw)), p, 64, p, None) != 0, kw
        assert L.lib.vk_last_error().startswith(b"vk_vis_loss_bwd"), kw
    for kw in (dict(), nce, dict(kind=L.VIS_MSE)):
        assert L.lib.vk_vis_loss_bwd(ctypes.byref(args(**kw)), p, 7, p, None) != 0, kw          # ldd < V
        assert L.lib.vk_last_error().startswith(b"vk_vis_loss_bwd: ldd"), kw
    # no rows: accepted without a launch
    assert L.lib.vk_vis_loss_fwd(ctypes.byref(args(max_rows=0)), None) == 0
    assert L.lib.vk_vis_loss_bwd(ctypes.byref(args(max_rows=0)), p, 8, p, None) == 0


def test_grad_seed_refusals_on_the_host():
    from volta_amd import _lib as L
    buf = (ctypes.c_uint8 * 4096)()
    p = _aligned(buf)

    def args(**kw):
        a = L.GradSeedArgs(p, 64, 16, p + 1024, p + 2048, 2, 4, 16, 0, 16, 16, 0, 0)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    bad = [dict(H=12), dict(H=0), dict(B=0), dict(ld=8), dict(ld=20), dict(ldy=8), dict(ldy=20), dict(row0=-1), dict(dst=p + 1024 + 8), dict(dst=None),
           dict(y=p + 2048 + 2), dict(src=p + 4), dict(stride_l=18), dict(stride_b=62)]
    for kw in bad:
        assert L.lib.vk_grad_seed(ctypes.byref(args(**kw)), None) != 0, kw
        assert L.lib.vk_last_error().startswith(b"vk_grad_seed"), kw
    # an absent gradient adds nothing: accepted without a launch
    assert L.lib.vk_grad_seed(ctypes.byref(args(src=None, accumulate=1)), None) == 0


def test_negatives_and_fusion_refusals_on_the_host():
    from volta_amd import _lib as L
    buf = (ctypes.c_uint8 * 4096)()
    p = _aligned(buf)
    rng = L.rng_cfg(p, 3)
    for B, R in ((1, 4), (4, 1), (0, 0), (1, 1)):
        assert L.lib.vk_nce_negatives(rng, B, R, p, None) != 0, (B, R)
        assert L.lib.vk_last_error().startswith(b"vk_nce_negatives"), (B, R)
    assert L.lib.vk_nce_negatives(L.rng_cfg(None, 3), 2, 2, p, None) != 0
    drop = L.dropout_cfg(None, 0, 0.0)
    for mode, pv in ((-1, p), (3, p), (L.FUSE_MUL, None), (L.FUSE_SUM, None)):
        assert L.lib.vk_pool_fuse_fwd(p, pv, p, 2, 8, mode, drop, None) != 0, (mode, pv)
        assert L.lib.vk_last_error().startswith(b"vk_pool_fuse_fwd"), (mode, pv)
        assert L.lib.vk_pool_fuse_bwd(p, 8, p, pv, p, p, 2, 8, mode, drop, None) != 0, (mode, pv)
        assert L.lib.vk_last_error().startswith(b"vk_pool_fuse_bwd"), (mode, pv)
    for mode in (L.FUSE_MUL, L.FUSE_SUM):
        assert L.lib.vk_pool_fuse_bwd(p, 8, p, p, p, None, 2, 8, mode, drop, None) != 0, mode            # dyv missing
