"""tests/concap_restate.py checked without a GPU.
  * The restatement equals oracle.volta_ref.concap_make_batch bit for bit (integers exactly, floats by their bit patterns) on the cases of
    tests/test_concap_gpu.py and on a ragged R = 36 batch for every add_global and objective.  tests/golden/concap_batch.npz pins that
    oracle function to the reference's own code (tests/test_concap_cpu.py), so the restatement inherits the tie.
  * The 15 % threshold as an integer comparison: word / 2^32 < 0.15 in double <=> word < CC_T15.
  * The in-order fp32 row sum equals np.sum(axis=1), the reference's, bit for bit at R = 36 and 256.
  * Every precondition the cases of tests/test_concap_kernels_gpu.py rely on, asserted on the restatement alone."""
import os
import sys

import numpy as np
import pytest

from oracle import volta_ref as R
from oracle.make_golden import concap_records

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import concap_restate as CR  # noqa: E402

f32 = np.float32
CASES = {c.id: c for c in CR.cases()}

ORACLE_CASES = [("first", 1, True, 10, 96, 33, 24), ("last", 0, True, 10, 96, 33, 24), (None, 2, False, 10, 96, 33, 24), ("first", 0, False, 10, 96, 33, 24)] + \
               [(ag, obj, True, 36, 32, 7, 8) for ag in (None, "first", "last") for obj in (0, 1, 2)]


@pytest.mark.parametrize("add_global,objective,ragged,Rl,F,C,B", ORACLE_CASES)
def test_restatement_equals_oracle(add_global, objective, ragged, Rl, F, C, B):
    T, V, seed = 14, 3000, 1234567
    recs, caps = concap_records(B, Rl, seed=5, F=F, C=C, ragged=ragged)
    want = R.concap_make_batch(recs, caps, seed=seed, seq_len=T, region_len=Rl, vocab_size=V, add_global=add_global, num_locs=5, objective=objective)
    got = CR.restate_inputs(CR.from_records(recs, caps, Rl, seed, T, V, add_global, objective))
    assert CR.same_bits(got, want) == []
    assert (got["image_label"] == 1).any() or objective == 1
    assert any(len(c) > T - 2 for c in caps) and any(len(c) < T - 2 for c in caps)


def test_threshold_as_integer_comparison():
    for w in (644245093, 644245094, 644245095):
        assert (w / 2 ** 32 < 0.15) == (w < R.CC_T15), w


def test_threshold_seed_word():
    assert int(R.concap_words(CR.THRESHOLD_SEED, R.CC_SITE_REGION, 1, 1)[0, 0]) == CR.THRESHOLD_WORD
    assert CR.THRESHOLD_WORD / 2 ** 32 < 0.15 <= (CR.THRESHOLD_WORD + 1) / 2 ** 32
    inp, ref = CR.reference(CASES["threshold_word"])
    assert inp["num_boxes"][0] == inp["case"].R and ref["is_match"][0] == 0 and ref["image_label"][0, 0] == 1


@pytest.mark.parametrize("Rl", [36, 256])
def test_inorder_sum_is_numpy_axis_sum(Rl):
    rng = np.random.default_rng(Rl)
    for x in (rng.random((4, Rl, 64), dtype=f32), rng.standard_normal((4, Rl, 64), dtype=f32)):
        want = np.sum(x, axis=1)
        for b in range(4):
            assert np.array_equal(CR.inorder_sum(x[b]).view(np.uint32), want[b].view(np.uint32))


@pytest.mark.parametrize("case", CR.cases(), ids=repr)
def test_restated_outputs_are_clean(case):
    """No NaN of the input padding, no caption-table filler and no out-of-range id reaches a restated output."""
    inp, ref = CR.reference(case)
    for k in CR.FLOAT_KEYS:
        assert np.isfinite(ref[k]).all(), k
    assert (ref["input_ids"] != CR.SENT).all() and (ref["lm_label_ids"] != CR.SENT).all()
    n = np.clip(inp["num_boxes"], 0, case.R)
    assert np.array_equal(ref["image_mask"].sum(1), n + (1 if case.add_global else 0))
    assert ((ref["image_label"] == 1).sum(1) <= n).all()


def test_region_cases_reach_the_second_loop_pass():
    for Rl in (129, 255, 256):
        _, ref = CR.reference(CASES["regions_R%d" % Rl])
        assert (ref["image_label"][:, 128:] == 1).any(), Rl
    c = CASES["cls_grid_loops"]
    assert c.B * c.R * c.C > 4096 * 256


def test_text_case_preconditions():
    inp, ref = CR.reference(CASES["text_lengths_obj2"])
    assert list(inp["cap_len"][:5]) == [0, 1, 12, 13, 40] and list(ref["input_mask"].sum(1)) == [2, 3, 14, 14, 14]
    assert (ref["input_ids"][np.arange(5), ref["input_mask"].sum(1) - 1] == 102).all()
    inp, ref = CR.reference(CASES["text_T3"])
    assert (inp["cap_len"][inp["cap_index"]] > 1).any() and (ref["input_mask"].sum(1) <= 3).all() and (ref["input_mask"].sum(1) == 3).any()
    # a token whose id is 0, selected in an unswapped pair: objective 0 labels it 0, objective 1 must give -1 (and still mask the input)
    inp, ref1 = CR.reference(CASES["text_token0_obj1"])
    ref0 = CR.restate_inputs(inp, objective=0)
    hit = (ref0["lm_label_ids"] == 0) & (ref0["is_match"] == 0)[:, None]
    assert hit.any() and (ref1["lm_label_ids"][hit] == -1).all() and np.array_equal(ref1["input_ids"], ref0["input_ids"])
    assert (ref1["lm_label_ids"][ref1["is_match"] == 0] > 0).any()


@pytest.mark.parametrize("objective", [0, 1, 2])
def test_objective_case_preconditions(objective):
    _, ref = CR.reference(CASES["objective%d" % objective])
    sw = ref["is_match"] == 1
    assert (sw.any() and (~sw).any()) if objective != 2 else not sw.any()
    both = (ref["lm_label_ids"] != -1).any(1) & (ref["image_label"] == 1).any(1) & ~sw
    assert both.any()                                     # a selected token and a selected region in one unswapped pair
    if objective == 1:
        assert (ref["lm_label_ids"][sw] == -1).all() and (ref["image_label"][sw] == -1).all()
    if objective == 0:
        assert (ref["lm_label_ids"][sw] != -1).any() and (ref["image_label"][sw] == 1).any()


@pytest.mark.parametrize("objective", [0, 1])
def test_visualization_case_preconditions(objective):
    inp, ref = CR.reference(CASES["visualization_obj%d" % objective])
    assert (ref["lm_label_ids"] == -1).all() and (ref["image_label"] == -1).all() and (ref["is_match"] == 0).all()
    assert CR.restate_inputs(inp, visualization=0)["is_match"].any()           # the same words would have swapped a caption
    for b in range(inp["case"].B):
        n = int(inp["num_boxes"][b])
        assert np.array_equal(ref["image_feat"][b, 1:1 + n].view(np.uint32), inp["feat"][b, :n].view(np.uint32))


def test_n_caps_case_preconditions():
    inp, ref = CR.reference(CASES["n_caps_below_rows"])
    n_rows, n_caps = inp["cap_tokens"].shape[0], inp["n_caps"]
    w = R.concap_words(inp["seed"], R.CC_SITE_CAPTION, inp["case"].B, 2)
    sw = ref["is_match"] == 1
    assert n_caps < n_rows and sw.any()
    assert (w[sw, 1] % n_rows >= n_caps).any()            # drawing over the whole table would land in a filler row
    assert (inp["cap_tokens"][n_caps:] == CR.SENT).all() and (inp["cap_len"][n_caps:] == inp["cap_tokens"].shape[1]).all()


def test_divisor_floor_preconditions():
    inp, ref = CR.reference(CASES["divisor_floor"])
    c = inp["case"]
    w = R.concap_words(c.seed, R.CC_SITE_REGION, c.B, c.R)
    floors = 0
    for b in range(c.B):
        sel, zero, masked, cnt = CR.region_decisions(inp["boxes"][b], c.R, w[b], c.R)
        assert masked.all() == sel.any() and cnt == (1 if sel.any() else c.R)
        if sel.any():
            floors += 1
            rows = np.where(~zero[:, None], inp["feat"][b], f32(0))
            assert np.array_equal(ref["image_feat"][b, 0].view(np.uint32), CR.inorder_sum(rows).view(np.uint32))      # divided by 1, not by 0
    assert floors >= 1 and floors < c.B


def test_iou_case_preconditions():
    inp, ref = CR.reference(CASES["iou_near_0p4"])
    c = inp["case"]
    plan = CR.iou_plan(c)
    assert [k for _, _, k, _, _, _ in plan] == ["area_i"] * 2 + ["area_j"] * 2 + ["inter"] * 2 + ["exact_0p4_a", "above_0p4_a", "exact_0p4_b", "above_0p4_b"]
    w = R.concap_words(c.seed, R.CC_SITE_REGION, c.B, c.R)
    assert (ref["is_match"] == 0).all()
    for b, s, kind, p, q, dec in plan:
        sel, zero, masked, cnt = CR.region_decisions(inp["boxes"][b], c.R, w[b], c.R)
        assert sel[s] and not sel[1 - s], (b, kind)                               # exactly one of the planted rows is selected
        assert np.array_equal(inp["boxes"][b, s], p) and np.array_equal(inp["boxes"][b, 1 - s], q)
        v = CR._iou_variants(p[None], q[None])
        assert bool(v["plain"][0]) == dec == bool(masked[1 - s])
        # the planted decision alone moves the divisor: every other row is disjoint from the planted ones and masks only itself
        assert cnt == c.R - int(sel.sum()) - int(dec), (b, kind)
        if kind in ("area_i", "area_j", "inter"):
            assert bool(v[kind][0]) != dec and (p != np.round(p)).all() and (q != np.round(q)).all()
        else:
            assert (p == np.round(p)).all() and (q == np.round(q)).all() and all(bool(x[0]) == dec for x in v.values())
            iou = CR.iou_matrix(np.stack([p, q]))[0, 1]
            assert (iou == f32(0.4)) if kind.startswith("exact") else (f32(0.4) < iou < f32(0.42))
        # a flipped decision shows in the global row: n / (n +- 1) is far outside one rounding
        other = CR.inorder_sum(np.where(~zero[:, None], inp["feat"][b], f32(0))) / f32(cnt + (1 if dec else -1))
        assert not np.array_equal(other.view(np.uint32), ref["image_feat"][b, 0].view(np.uint32))


@pytest.mark.parametrize("fault", ["cnt_plus_one", "region_next_slot"])
def test_comparison_is_not_vacuous(fault):
    inp, ref = CR.reference(CASES["objective0"])
    assert CR.same_bits(CR.restate_inputs(inp), ref) == []
    bad = CR.same_bits(CR.restate_inputs(inp, fault=fault), ref)
    assert "image_feat" in bad and ("image_label" in bad) == (fault == "region_next_slot")
