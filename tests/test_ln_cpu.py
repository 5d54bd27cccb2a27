"""Host side of the LayerNorm kernel tests, no GPU: the float64 restatement of tests/ln_restate.py against autograd, its gates against
an fp32/bf16 emulation of the kernels (not too tight) and against planted bugs (not too loose), the dispatch of every case of the GPU
table (tests/test_ln_kernels_gpu.py) against the switch statements of csrc/layernorm.hip, and the partial-record arithmetic."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ln_restate as A  # noqa: E402


def _lib():
    from volta_amd import _lib as L
    return L


def _run(case, bug=None):
    """(forward ratios, backward ratios) of the emulation against the restatement; the backward is fed the restated inputs."""
    inp = A.make_inputs(case)
    n = A.case_rows(case)
    fwd = A.restate_fwd(inp, n, case.y8)
    zb, mean, rstd = A.backward_inputs(A.restate_fwd(inp))         # every row of the inputs exists, whatever dyn says
    bwd = A.restate_bwd(inp, zb, mean, rstd, n, case.dd, case.acc)
    ef = A.emulate_fwd(inp, n, case.y8, bug)
    eb = A.emulate_bwd(inp, zb, mean, rstd, n, case.dd, case.acc, bug)
    res = A.ratios(ef, fwd, A.FWD_KEYS + (("y8", "sc") if case.y8 else ()))
    res.update(A.ratios(eb, bwd, A.BWD_KEYS))
    return res, ef, eb


@pytest.mark.parametrize("case", A.CASES, ids=[c.id for c in A.CASES])
def test_emulated_kernel_passes_every_gate(case):
    """Not too tight: the kernels' arithmetic emulated in fp32 / bf16 passes every gate at every case of the GPU table."""
    res, ef, eb = _run(case)
    if case.profile == "const":             # ill-conditioned on purpose (ln_restate.CASES): finiteness and the gate of mean only
        n = A.case_rows(case)
        for out in (ef, eb):
            for key, t in out.items():
                assert t is None or bool(torch.isfinite(t[:n] if t.shape[0] == case.M else t).all()), key
        res = {"mean": res["mean"]}
    assert res and all(r <= 1.0 for r in res.values()), (case.id, res)


@pytest.mark.parametrize("bug", A.BUGS)
def test_planted_bug_fails_its_gate(bug):
    """Not too loose: with one planted defect the emulation misses the gate of at least one of the outputs the defect reaches, on every
    case named for it in ln_restate.PLANTED; without the defect the same outputs pass (test_emulated_kernel_passes_every_gate)."""
    ids, outputs = A.PLANTED[bug]
    for cid in ids:
        res, _, _ = _run(A.CASE[cid], bug)
        hit = {k: res[k] for k in outputs if k in res}
        assert hit and max(hit.values()) > 1.0, (bug, cid, res)


def test_closed_form_matches_autograd():
    """The closed-form backward of the restatement equals float64 autograd through dropout, the add chain, LayerNorm and out_scale,
    when it is fed the forward's unrounded z, mean and rstd."""
    for cid in ("M33-H260-pre-offset-addvec", "M33-H516-post-randn-split-addvec", "M33-H256-post05-wide-split", "M17-H1284-none-randn-xnull-zalias"):
        case = A.CASE[cid]
        inp = A.make_inputs(case)
        fwd = A.restate_fwd(inp)
        d = inp["d"].double().requires_grad_(True)
        x = inp["x"].double().requires_grad_(True) if inp["x"] is not None else None
        gamma, beta = inp["gamma"].double().requires_grad_(True), inp["beta"].double().requires_grad_(True)
        km = inp["keep"].double() * inp["scale"] if inp["p"] > 0 else torch.ones(case.M, case.H, dtype=torch.float64)
        z = d * km if (inp["p"] > 0 and not inp["post"]) else d * 1.0
        if x is not None:
            z = z + x
        if inp["addvec"] is not None:
            z = z + inp["addvec"].double()
        y = torch.nn.functional.layer_norm(z, (case.H,), gamma, beta, eps=A.EPS)
        y = (y * km if (inp["p"] > 0 and inp["post"]) else y) * inp["out_scale"]
        torch.testing.assert_close(y, fwd["y"], rtol=1e-11, atol=1e-11)
        y.backward(inp["dy"].double())
        # restate_bwd takes bf16 z / fp32 stats as given; here they are passed unrounded so that the closed form itself is checked
        M, H = case.M, case.H
        mean, rstd = fwd["mean"][:, None], fwd["rstd"][:, None]
        xh = (fwd["z"] - mean) * rstd
        gy = inp["dy"].double() * inp["out_scale"] * (km if (inp["p"] > 0 and inp["post"]) else 1.0)
        gx = gy * inp["gamma"].double()
        dz = rstd * (gx - gx.mean(-1, keepdim=True) - xh * (gx * xh).mean(-1, keepdim=True))
        if x is not None:
            torch.testing.assert_close(dz, x.grad, rtol=1e-8, atol=1e-9)
        torch.testing.assert_close(dz * (km if (inp["p"] > 0 and not inp["post"]) else 1.0), d.grad, rtol=1e-8, atol=1e-9)
        torch.testing.assert_close((gy * xh).sum(0), gamma.grad, rtol=1e-8, atol=1e-9)
        torch.testing.assert_close(gy.sum(0), beta.grad, rtol=1e-8, atol=1e-9)
        # and restate_bwd is that closed form on the rounded inputs: identical when the inputs need no rounding
        ref = A.restate_bwd(inp, fwd["z"], fwd["mean"], fwd["rstd"])
        torch.testing.assert_close(ref["dz"], dz, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(ref["dgamma"], gamma.grad, rtol=1e-8, atol=1e-9)


def test_row_mapping_matches_the_engine_form():
    """The single-stream tuples (site, T, T + R, 0) / (site, R, T + R, T) number the rows of a per-sample concatenation [T text | R
    vision]: text row b T + t -> b (T + R) + t, vision row b R + r -> b (T + R) + T + r; segment 1 starts again at split_row."""
    B, T, R = 4, 5, 3
    prow, site = A.drop_rows(B * (T + R), B * T, [(21, T, T + R, 0), (21, R, T + R, T)])
    want = [b * (T + R) + t for b in range(B) for t in range(T)] + [b * (T + R) + T + r for b in range(B) for r in range(R)]
    assert prow.tolist() == want and set(site.tolist()) == {21}
    assert sorted(want) == list(range(B * (T + R)))
    prow, site = A.drop_rows(10, 6, [(11, 0, 0, 0), (12, 0, 0, 0)])
    assert prow.tolist() == [0, 1, 2, 3, 4, 5, 0, 1, 2, 3] and site.tolist() == [11] * 6 + [12] * 4


def test_dispatch_matches_the_switch_statements():
    """fwd_template / bwd_template against the `switch (nch)` statements of layernorm.hip for every admissible H, and the table reaches
    every instantiation, each with a full and (where one exists) a partly filled last chunk."""
    sw = A.parse_switches()
    assert sw["fwd"] == ({1: 1, 2: 2, 3: 3, 4: 4}, 8), sw["fwd"]
    assert sw["bwd"] == ({1: 1, 2: 2, 3: 3, 4: 4, 5: 6, 6: 6}, 8), sw["bwd"]
    for H in range(4, 2049, 4):
        for kind, fn in (("fwd", A.fwd_template), ("bwd", A.bwd_template)):
            cases, default = sw[kind]
            assert fn(H) == cases.get(A.nch(H), default), (kind, H)
            assert fn(H) * 256 >= H, (kind, H)             # the instantiation's registers / LDS row cover the row
    Hs = {c.H for c in A.CASES}
    assert Hs >= {4, 64, 252, 256, 260, 516, 768, 1024, 1284, 1536, 1792, 2048}
    assert {A.fwd_template(H) for H in Hs} == {1, 2, 3, 4, 8}
    assert {A.bwd_template(H) for H in Hs} == {1, 2, 3, 4, 6, 8}
    for kind, fn, insts in (("fwd", A.fwd_template, (1, 2, 3, 4, 8)), ("bwd", A.bwd_template, (1, 2, 3, 4, 6, 8))):
        for t in insts:
            mine = [H for H in Hs if fn(H) == t]
            assert any(H % 256 == 0 for H in mine), (kind, t, "no full last chunk")
            assert any(H % 256 != 0 for H in mine), (kind, t, "no partly filled last chunk")


def test_table_covers_what_the_issue_lists():
    Ms = {c.M for c in A.CASES}
    assert Ms >= {1, 3, 4, 5, 15, 16, 17, 33, 1000} and any(c.M == 14592 and c.H == 768 for c in A.CASES)
    assert {c.mode for c in A.CASES} == set(A.MODES)
    assert {c.profile for c in A.CASES} == {"randn", "offset", "wide", "spike", "const"}
    assert sum(c.profile == "const" for c in A.CASES) == 1
    assert {c.seg for c in A.CASES} == {"rows", "single", "single_v"}
    assert {c.z for c in A.CASES} == {"own", "null", "alias"}
    for field in ("split", "addvec", "x", "dd", "y8", "acc"):
        assert {bool(getattr(c, field)) for c in A.CASES} == {True, False}, field
    M = 33
    assert {c.dyn for c in A.CASES if c.M == M and c.dyn is not None} == {0, 1, M - 1, M, M + 5}
    assert 40 <= len(A.CASES) <= 60
    for ids, _ in A.PLANTED.values():
        assert all(cid in A.CASE for cid in ids)


def test_partial_rows_arithmetic():
    """vk_ln_bwd_partial_rows (host arithmetic): one record per 16-row workgroup, at the table's row counts and around them."""
    L = _lib()
    for M in sorted({c.M for c in A.CASES} | {0, 2, 31, 32, 48, 49, 14591, 14593}):
        assert L.lib.vk_ln_bwd_partial_rows(M) == A.partial_rows(M) == math.ceil(M / 16), M
