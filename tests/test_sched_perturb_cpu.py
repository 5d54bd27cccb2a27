"""The list rewriting of tests/sched_perturb.py on hand-written op lists, without a GPU: where the holds go, which wait leaves, that every
op-index table of the engine still points at the same op afterwards, and that leaving `perturbed` puts the original objects back."""
import ctypes
import os
import sys
import types

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sched_perturb as SP  # noqa: E402


def _lists():
    """(L, forward list, backward list, {label: op}).  Plain ops are OP_GEMM entries without arguments, told apart by i0."""
    from volta_amd import _lib as L
    from volta_amd.engine.plan import op, side_begin, side_end, wait_side
    named = {}

    def m(label):
        named[label] = op(L.OP_GEMM, i0=len(named))
        return named[label]

    fwd = [m("masks"), side_begin(), m("img_emb"), side_end(15), m("text_emb"),
           m("sub0"), m("sub0b"),                                  # sub-layer 0 starts at "sub0"
           wait_side(15), m("sub1"),                               # sub-layer 1 starts at its wait for the image embedding
           m("sub2"),
           m("heads"), side_begin(), m("regions"), side_end(11), m("itm"), wait_side(11), m("loss")]
    named["wait15"], named["wait11"] = fwd[7], fwd[15]
    bwd = [m("zero"), side_begin(), m("regions_bwd"), side_end(13), m("lm_bwd"), side_begin(), m("head_wgrad"), side_end(12), wait_side(13),
           m("sub2_bwd"), side_begin(), m("sub2_wgrad"), side_end(2),          # stage 1
           m("sub1_bwd"), side_begin(), m("sub1_wgrad"), side_end(1),          # stage 2
           wait_side(2), m("sub0_bwd"), side_begin(), m("sub0_wgrad"), side_end(0), side_begin(), m("img_emb_bwd"), side_end(14),      # stage 3
           wait_side(12), m("text_emb_bwd"),                        # stage 4
           op(L.OP_JOIN)]
    named["wait2"], named["wait12"], named["join"] = bwd[17], bwd[25], bwd[27]
    return L, fwd, bwd, named


def _engine(fwd, bwd, named):
    from volta_amd.engine.plan import Plan
    eng = types.SimpleNamespace(fwd=Plan(), bwd=Plan())
    eng.fwd.ops, eng.bwd.ops = list(fwd), list(bwd)
    eng.fwd.freeze()
    eng.bwd.freeze()
    at = lambda ops, label: next(i for i, o in enumerate(ops) if o is named[label])
    eng.fwd_sub_start = [at(fwd, "sub0"), at(fwd, "wait15"), at(fwd, "sub2")]
    eng.fwd_heads_start = at(fwd, "heads")
    eng.bwd_marks = [at(bwd, "sub2_bwd"), at(bwd, "sub1_bwd"), at(bwd, "wait2"), at(bwd, "wait12"), at(bwd, "join")]
    eng._fwd_segments = {(1, 2): [(1, 0, 5)]}
    return eng


def test_late_side_puts_one_hold_behind_every_side_begin_and_nothing_else():
    L, fwd, bwd, _ = _lists()
    for ops, blocks in ((fwd, 2), (bwd, 6)):
        before = list(ops)
        out = SP.late_side(ops, 250)
        assert ops == before and all(a is b for a, b in zip(ops, before))           # the argument is left alone
        assert len(out) == len(ops) + blocks and SP.count_holds(out) == blocks and SP.count_holds(ops) == 0
        assert [o for o in out if not (o[0] == L.OP_GENERIC and o[4].fn == L.FN_HOLD)] == ops
        for i, o in enumerate(out):
            is_hold = o[0] == L.OP_GENERIC and o[4].fn == L.FN_HOLD
            assert is_hold == (i > 0 and out[i - 1][0] == L.OP_SIDE_BEGIN)
            if is_hold:
                assert tuple(o[4].n[:3]) == (1, 250, 0) and o[5] is None and o[6] is None
        assert len({id(o[4]) for o in out if o[0] == L.OP_GENERIC}) == blocks       # every hold has arguments of its own
    made = []
    out = SP.late_side(fwd, 7, make_hold=lambda us: made.append(us) or ("hold", us))
    assert made == [7, 7] and out.count(("hold", 7)) == 2
    with pytest.raises(AssertionError):
        SP.hold_op(SP.HOLD_MAX_US + 1)                    # asserted, never clamped
    with pytest.raises(AssertionError):
        SP.hold_op(0)


def test_without_wait_takes_out_the_first_wait_of_that_event_only():
    L, fwd, bwd, named = _lists()
    out = SP.without_wait(fwd, 15)
    assert len(out) == len(fwd) - 1 and named["wait15"] not in out and named["wait11"] in out
    assert [o for o in fwd if o is not named["wait15"]] == out
    twice = bwd + [named["wait2"]]
    out = SP.without_wait(twice, 2)
    assert len(out) == len(twice) - 1 and out[-1] is named["wait2"] and out[:17] == bwd[:17] and out[17] is bwd[18]
    with pytest.raises(ValueError):
        SP.without_wait(fwd, 12)
    assert SP.events(bwd) == ([13, 12, 2, 1, 0, 14], {13, 2, 12})


def test_implied_by_finds_the_later_wait_that_makes_a_wait_redundant():
    L, fwd, bwd, named = _lists()
    at = lambda ops, label: next(i for i, o in enumerate(ops) if o is named[label])
    assert SP.implied_by(fwd, 15) is None and SP.implied_by(fwd, 11) is None
    assert SP.implied_by(bwd, 13) is None                 # the head weight-gradient block is opened in between, but nobody waits for it there
    assert SP.implied_by(bwd, 2) is None                  # event 1 is recorded in between and not waited for
    assert SP.implied_by(bwd, 12) == at(bwd, "wait2")     # sub-layer 2's block runs behind the heads' on the one side stream: its wait covers both
    assert SP.implied_by(SP.without_wait(bwd, 2), 12) is None
    assert SP.implied_by([o for o in bwd if o is not named["wait12"]] + [named["wait12"]], 12) == at(bwd, "wait2")
    joined = [o for o in bwd if o not in (named["wait2"], named["wait12"], named["join"])] + [named["join"], named["wait12"]]
    assert SP.implied_by(joined, 12) == len(joined) - 2   # a join waits for every block
    assert SP.implied_by(bwd, 14) == at(bwd, "join")      # recorded, never waited for: the join that ends the list is its edge
    with pytest.raises(ValueError):
        SP.implied_by(bwd[:-1], 14)


def test_boundary_map():
    a, b, c, d, x, y = [("op", i) for i in range(6)]
    assert SP.boundary_map([a, b, c], [a, b, c]) == [0, 1, 2, 3]
    assert SP.boundary_map([a, b, c], [a, x, b, c, y]) == [0, 2, 3, 5]            # the end stays the end
    assert SP.boundary_map([a, b, c, d], [a, c, d]) == [0, 1, 1, 2, 3]            # a boundary at a removed op moves to the next one left
    assert SP.boundary_map([a, b, c, d], [x, a, b, y, c]) == [1, 2, 4, 5, 5]
    assert SP.boundary_map([], [x]) == [1]
    assert SP.boundary_map([a, b, a, c], [a, x, b, a, c]) == [0, 2, 3, 4, 5]      # the same object listed twice: matched in order


def test_perturbed_remaps_every_index_table_and_restores_the_original_objects():
    L, fwd, bwd, named = _lists()
    eng = _engine(fwd, bwd, named)
    orig = dict(fwd_ops=eng.fwd.ops, fwd_c=eng.fwd.c_ops, bwd_ops=eng.bwd.ops, bwd_c=eng.bwd.c_ops, marks=eng.bwd_marks, sub=eng.fwd_sub_start,
                heads=eng.fwd_heads_start, segs=eng._fwd_segments)
    assert {a for a, _ in SP.INDEX_TABLES} == {"bwd_marks", "fwd_sub_start", "fwd_heads_start"}
    new_f = SP.late_side(SP.without_wait(fwd, 15), 300)
    new_b = SP.late_side(SP.without_wait(bwd, 12), 300)

    def check_inside():
        assert eng.fwd.ops == new_f and eng.bwd.ops == new_b and eng._fwd_segments == {}
        assert len(eng.fwd.c_ops) == len(new_f) and len(eng.bwd.c_ops) == len(new_b)
        assert [o.kind for o in eng.fwd.c_ops] == [o[0] for o in new_f] and [o.i0 for o in eng.bwd.c_ops] == [o[1] for o in new_b]
        for i, o in enumerate(new_f):                     # the frozen array points at the holds' arguments
            if o[0] == L.OP_GENERIC:
                assert eng.fwd.c_ops[i].a == ctypes.addressof(o[4])
        # every table entry stands in front of the op it stood in front of; where that op is the removed wait, in front of the next one
        want_sub = [named["sub0"], named["sub1"], named["sub2"]]
        assert [eng.fwd.ops[i] for i in eng.fwd_sub_start] == want_sub
        assert eng.fwd.ops[eng.fwd_heads_start] is named["heads"]
        want_marks = [named["sub2_bwd"], named["sub1_bwd"], named["wait2"], named["text_emb_bwd"], named["join"]]
        assert [eng.bwd.ops[i] for i in eng.bwd_marks] == want_marks
        assert eng.bwd_marks[-1] == len(new_b) - 1 and eng.bwd_marks == sorted(eng.bwd_marks)
        # a hold goes with the block it opens: no table entry points at one, and none points into a side block
        for table, ops in ((eng.fwd_sub_start + [eng.fwd_heads_start], eng.fwd.ops), (eng.bwd_marks, eng.bwd.ops)):
            for i in table:
                depth = sum((o[0] == L.OP_SIDE_BEGIN) - (o[0] == L.OP_SIDE_END) for o in ops[:i])
                assert depth == 0 and ops[i][0] != L.OP_GENERIC

    def check_restored():
        assert eng.fwd.ops is orig["fwd_ops"] and eng.fwd.c_ops is orig["fwd_c"] and eng.bwd.ops is orig["bwd_ops"] and eng.bwd.c_ops is orig["bwd_c"]
        assert eng.bwd_marks is orig["marks"] and eng.fwd_sub_start is orig["sub"] and eng.fwd_heads_start == orig["heads"]
        assert eng._fwd_segments is orig["segs"] and eng._fwd_segments == {(1, 2): [(1, 0, 5)]}
        assert eng.fwd.ops == fwd and eng.bwd.ops == bwd

    with SP.perturbed(eng, new_f, new_b) as got:
        assert got is eng
        check_inside()
    check_restored()
    with pytest.raises(RuntimeError):                    # leaving by an exception restores as well
        with SP.perturbed(eng, new_f, new_b):
            check_inside()
            raise RuntimeError("step failed")
    check_restored()
    with SP.perturbed(eng, None, new_b):                 # one list only: the other list and its tables stay the objects they were
        assert eng.fwd.ops is orig["fwd_ops"] and eng.fwd.c_ops is orig["fwd_c"] and eng.fwd_sub_start is orig["sub"]
        assert eng.bwd.ops == new_b and eng.bwd.ops[eng.bwd_marks[3]] is named["text_emb_bwd"]
    check_restored()


def test_fwd_segments_of_a_real_plan_follow_the_remap():
    """On a plan built on the CPU (ViLBERT of tests/test_engine_gpu.py): the segments the pipelined forward cuts the perturbed list into
    begin at the same ops as those of the original list, cover the whole list, and none begins inside a side block."""
    import torch
    from test_engine_gpu import CONFIGS
    from volta_amd import _lib as L
    from volta_amd.config import BertConfig
    from volta_amd.engine import ParamArena, StepEngine
    from volta_amd.engine.plan import EV_IMAGE_EMB_FWD
    from volta_amd.modeling import BertForVLPreTraining
    cfg = BertConfig.from_dict(CONFIGS["vilbert"])
    model = BertForVLPreTraining(cfg)
    arena = ParamArena(model, torch.device("cpu"), prefix=model._arena_prefix)
    eng = StepEngine(cfg, arena, 2, 20, 36, True)
    nch = arena.total // 1024
    bounds = [nch * (i + 1) // 5 for i in range(5)]
    old_ops = eng.fwd.ops
    old = eng.fwd_segments(bounds)
    for new_f in (SP.late_side(old_ops, 100), SP.late_side(SP.without_wait(old_ops, EV_IMAGE_EMB_FWD), 100)):
        with SP.perturbed(eng, new_f, SP.late_side(eng.bwd.ops, 100)):
            new = eng.fwd_segments(bounds)
            assert [nd for nd, _, _ in new] == [nd for nd, _, _ in old]
            assert new[0][1] == 0 and new[-1][2] == len(new_f) and all(a[2] == b[1] for a, b in zip(new, new[1:]))
            for (_, s_old, _), (_, s_new, _) in zip(old, new):
                a, b = old_ops[s_old], new_f[s_new]
                assert a is b or (a[0] == L.OP_WAIT_SIDE and a[1] == EV_IMAGE_EMB_FWD and b is old_ops[s_old + 1])
                assert sum((o[0] == L.OP_SIDE_BEGIN) - (o[0] == L.OP_SIDE_END) for o in new_f[:s_new]) == 0
            assert SP.count_holds(new_f) == sum(o[0] == L.OP_SIDE_BEGIN for o in old_ops) >= 2
        assert eng.fwd.ops is old_ops and eng.fwd_segments(bounds) is old


def test_serial_switches_the_side_stream_back_on_however_the_block_leaves(monkeypatch):
    from volta_amd import _lib as L
    calls = []
    monkeypatch.setattr(L, "lib", types.SimpleNamespace(vk_side_enable=calls.append))
    with SP.serial():
        assert calls == [0]
    with pytest.raises(KeyError):
        with SP.serial():
            raise KeyError("x")
    assert calls == [0, 1, 0, 1]
