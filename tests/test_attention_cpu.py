"""Host side of the gated attention tests, no GPU: the float64 restatement of tests/attn_restate.py against autograd, its gates against
an fp32/bf16 emulation of the MFMA kernels (not too tight) and against planted bugs (not too loose), and the dispatch of every case of
the GPU table (tests/test_attention_kernels_gpu.py) through vk_gated_attn_lds_bytes."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_restate as A  # noqa: E402


def _lib():
    from volta_amd import _lib as L
    return L


def test_closed_form_matches_autograd():
    """The closed-form backward of the restatement equals float64 autograd through the joint softmax, mask, dropout and block sum."""
    inp = A.make_inputs(4, 3, 16, 7, 11, "mid", seed=3)
    for gname in A.GATES:
        gate, p = A.GATES[gname], 0.25
        keep = A.keeps(inp, gate, p)
        ref = A.restate(inp, gate, p, keep)
        B, nh, dh, Ls = 4, 3, 16, inp["L"]
        q = [A.heads(inp["q"][m], B, Ls[m], nh, dh).clone().requires_grad_(True) for m in range(2)]
        k = [A.heads(inp["k"][m], B, Ls[m], nh, dh).clone().requires_grad_(True) for m in range(2)]
        v = [A.heads(inp["v"][m], B, Ls[m], nh, dh).clone().requires_grad_(True) for m in range(2)]
        loss = 0
        for mq in range(2):
            bl = A.blocks(gate, mq)
            if not bl:
                continue
            sc = [q[mq] @ k[mk].transpose(-1, -2) / math.sqrt(dh) + inp["mask"][mk].double()[:, None, None, :] for mk in bl]
            pr = torch.softmax(torch.cat(sc, -1), -1).split([Ls[mk] for mk in bl], -1)
            ctx = sum((pb * keep[mq][mk].double() / (1 - p)) @ v[mk] for pb, mk in zip(pr, bl))
            torch.testing.assert_close(A.rows(ctx), ref["ctx"][mq], rtol=1e-12, atol=1e-12)
            torch.testing.assert_close(torch.logsumexp(torch.cat(sc, -1), -1).reshape(-1), ref["lse"][mq], rtol=1e-12, atol=1e-12)
            loss = loss + (A.rows(ctx) * inp["do"][mq].double()).sum()
        loss.backward()
        for m in range(2):
            for key, leaf in (("dq", q[m]), ("dk", k[m]), ("dv", v[m])):
                if leaf.grad is None:
                    assert ref[key][m] is None, (gname, key, m)
                else:
                    torch.testing.assert_close(ref[key][m], A.rows(leaf.grad), rtol=1e-9, atol=1e-10)


def _emulation_ok(case):
    sh = case.shape
    inp = A.make_inputs(sh.B, sh.nh, sh.dh, sh.T, sh.R, case.dist, seed=A.case_seed(case))
    gate = A.GATES[case.gname]
    ref = A.restate(inp, gate, case.p)
    emu = A.emulate(inp, gate, case.p)
    for key, r in A.worst_ratio(emu, ref).items():
        assert r <= 1.0, (case.id, key, r)


@pytest.mark.parametrize("shape", A.SHAPES, ids=lambda s: s.name)
def test_emulated_kernel_passes_every_gate(shape):
    """Not too tight: the kernels' rounding points emulated in fp32 / bf16 pass every gate at every shape, gate pattern and dropout
    setting of the GPU table."""
    for case in A.table_cases():
        if case.shape == shape:
            _emulation_ok(case)


def test_emulated_kernel_passes_every_gate_extra_cases():
    """... and at the GPU table's other cases: p = 0.5, B = 1, the attention-map shapes, the largest backward shapes (the 256-batch
    bench shape at gate 'all' only: the other patterns are subsets of its arithmetic)."""
    cases = [c for c in A.table_cases() if not any(c.shape == s for s in A.SHAPES) and not c.fwd_only]
    cases = [c for c in cases if c.shape.B < 256 or c.gname == "all"] + A.largest_cases(_lib().lib)
    for case in cases:
        _emulation_ok(case)


# (bug, argument, T, R, gate, p, input distribution, outputs that must fail).  Ragged batch element 1 has one valid key of each modality.
PLANTED = [
    ("drop_key", (0, 16), 17, 37, "tt", 0.0, "uniform", ("ctx", "lse", "dv")),          # last key of a partial 16-key tile
    ("drop_key", (0, 64), 65, 37, "tt", 0.0, "uniform", ("ctx", "lse", "dv")),          # first generic text length
    ("drop_key", (1, 64), 20, 65, "tt+vv", 0.1, "uniform", ("ctx", "lse", "dv")),
    ("mask_ignored", 1, 20, 37, "all", 0.0, "mid", ("ctx", "lse", "dq", "dk", "dv")),
    ("per_block_softmax", None, 20, 37, "all", 0.0, "mid", ("ctx", "dq", "dk")),
    ("per_block_softmax", None, 20, 37, "tt+tv", 0.1, "uniform", ("ctx", "dq", "dk")),
    ("drow_shift", None, 20, 37, "all", 0.1, "uniform", ("ctx", "dq", "dk", "dv")),
    ("drow_shift", None, 38, 101, "tt+tv", 0.1, "mid", ("ctx", "dq", "dk", "dv")),
    ("site_shift", None, 20, 37, "all", 0.1, "uniform", ("ctx", "dq", "dk", "dv")),
    ("no_keep_scale", None, 20, 37, "all", 0.1, "mid", ("ctx", "dq", "dv")),
    ("no_keep_scale", None, 20, 37, "tt", 0.1, "uniform", ("ctx", "dq", "dv")),
    ("other_scale", None, 20, 37, "all", 0.0, "mid", ("ctx", "lse", "dq", "dk", "dv")),
    ("other_scale", None, 20, 37, "tt+vv", 0.1, "peaked", ("ctx", "lse", "dq", "dk", "dv")),
    ("lse_row_shift", None, 20, 37, "all", 0.0, "mid", ("dq", "dk", "dv")),
    ("lse_row_shift", None, 17, 64, "tv+vt", 0.1, "mid", ("dq", "dk", "dv")),
    ("dk_no_scale", None, 20, 37, "all", 0.0, "mid", ("dk",)),
    ("dq_no_scale", None, 20, 37, "all", 0.0, "mid", ("dq",)),
    ("dk_no_scale", None, 20, 37, "tt", 0.1, "uniform", ("dk",)),
    ("dq_no_scale", None, 20, 37, "tt", 0.1, "uniform", ("dq",)),
    ("delta_row_shift", None, 20, 37, "all", 0.0, "mid", ("dq", "dk")),
    ("delta_row_shift", None, 20, 37, "tt+tv", 0.1, "uniform", ("dq", "dk")),
]
MARGIN = 3.0


@pytest.mark.parametrize("bug,arg,T,R,gname,p,dist,outputs", PLANTED, ids=["%s-T%dR%d-%s-p%g" % (s[0], s[2], s[3], s[4], s[5]) for s in PLANTED])
def test_planted_bug_fails_its_gate(bug, arg, T, R, gname, p, dist, outputs):
    """Not too loose: the emulated kernel with one planted defect misses the gate of every output the defect reaches by MARGIN x."""
    inp = A.make_inputs(4, 12, 64, T, R, dist, seed=5)
    gate = A.GATES[gname]
    ref = A.restate(inp, gate, p)
    bad = A.worst_ratio(A.emulate(inp, gate, p, bug, arg), ref)
    for key in outputs:
        r = max(v for (k, _), v in bad.items() if k == key)
        assert r >= MARGIN, (bug, key, r)


# ------------------------------------------------------------------------------------------------ dispatch of the GPU table
def _args(sh, gname, probs):
    L = _lib()
    aa = L.AttnArgs()
    aa.B, aa.nh, aa.dh, aa.scale = sh.B, sh.nh, sh.dh, 1.0 / math.sqrt(sh.dh)
    aa.L[0], aa.L[1] = sh.T, sh.R
    for i in range(2):
        for j in range(2):
            aa.gate[i][j] = A.GATES[gname][i][j]
            aa.probs[i][j] = 8 if (probs and A.GATES[gname][i][j]) else None     # only tested against NULL on the host
    return aa


def test_every_case_runs_on_its_claimed_path():
    """vk_gated_attn_lds_bytes (host arithmetic) returns 0 exactly for the cases the restated dispatch puts on the MFMA kernels and puts
    every generic case within the LDS; with every gate open each case runs where the table claims; the MFMA cases cover all six template
    instances and all three backward launch branches of attention.hip:552-569."""
    L = _lib()
    instances, branches = set(), set()
    for case in A.table_cases() + A.largest_cases(L.lib):
        sh, gate = case.shape, A.GATES[case.gname]
        aa = _args(sh, case.gname, case.probs)
        fwd, bwd = L.lib.vk_gated_attn_lds_bytes(C.byref(aa), 0), L.lib.vk_gated_attn_lds_bytes(C.byref(aa), 1)
        path = A.case_path(sh.T, sh.R, sh.dh, gate, case.probs)
        if case.gname == "all":
            assert path == sh.path.replace("generic-fwd", "generic"), (case.id, path)
        if path.startswith("mfma"):
            assert fwd == 0 and bwd == 0, (case.id, fwd, bwd)
            instances.add(path)
            branches.add(A.bwd_branch(sh.T, sh.R, sh.dh, gate))
        elif sh.path == "generic-fwd":
            assert 0 < fwd <= A.LDS_LIMIT < bwd, (case.id, fwd, bwd)
        else:
            assert 0 < fwd <= bwd <= A.LDS_LIMIT, (case.id, fwd, bwd)
    assert instances == {"mfma<32,64,64>", "mfma<64,64,64>", "mfma<32,128,64>", "mfma<64,128,64>", "mfma<32,64,128>", "mfma<64,64,128>"}
    assert {b for b, _ in branches} == {"occ3", "occ2", "occ2-1wg"}
    assert ("occ2-1wg", 8) in branches                   # the 8-wave workgroup


def test_largest_backward_shape_is_the_edge():
    """The search of largest_bwd_shape stops at the LDS edge: one more region would not fit (the GPU table runs the shape it finds)."""
    L = _lib()
    for dh in (64, 128):
        R = A.largest_bwd_shape(L.lib, dh)
        assert R is not None and R > 129
        sh = A.Shape("x", 1, 1, dh, 65, R + 1, "generic")
        assert L.lib.vk_gated_attn_lds_bytes(C.byref(_args(sh, "all", False)), 1) > A.LDS_LIMIT
