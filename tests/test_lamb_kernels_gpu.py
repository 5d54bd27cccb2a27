"""vk_lamb_step (csrc/lamb.hip) through the C ABI against the float64 restatement of tests/lamb_restate.py, under the gates derived there, on
the layout of its case table: tensors of 1 .. 2 * 1024 + 5 elements, three tensors sharing one chunk, a skipped tensor between live ones,
an all-zero p, an all-zero update, tensors outside the arena (one off a 16-byte boundary), two groups.
  * gradients of skipped tensors and every gap hold NaN; p / m / v / shadow gaps, the floats behind the scratch and behind the ratio table
    hold canary bits: results inside their gates show nothing outside the contract's inputs was used, and everything the contract does not
    assign keeps its bits -- `.grad`, skipped tensors, the pads between tensors, the scratch's surroundings;
  * the bf16 shadow equals round-to-nearest-even of the p written; two runs give equal bits; a tensor's results do not change with its
    chunk neighbour's data; refusals launch nothing; a tensor placed beyond element 2^31 of its allocations.
tests/test_lamb_cpu.py checks the gates themselves.  GPU only."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lamb_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
CAN16 = -91                         # bf16 canary bits 0xFFA5
CAN32 = 0xFFA5A5A5 - (1 << 32)      # fp32 canary bits
PAD = 64
NAN = float("nan")
CLS = (5, 63)                       # the classes groups 0 and 1 use: not 0 and 1, and the last one


def _lib():
    from volta_amd import _lib as L
    return L


def _can32(n):
    return torch.full((n,), CAN32, dtype=torch.int32, device=DEV).view(torch.float32)


def _can16(n):
    return torch.full((n,), CAN16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


class Bench:
    """Device buffers of one case.  Arena tensors are views of p / m / v / g / shadow arenas filled with canaries (NaN for g); tensors
    outside the arena have buffers of their own, FOREIGN_SHIFT floats off a 16-byte boundary, with the same surroundings."""

    def __init__(self, case, inp, mutate=None):
        self.case = case
        n = R.ARENA_TOTAL + PAD
        self.p, self.m, self.v, self.shadow = _can32(n), _can32(n), _can32(n), _can16(n)
        self.g = [torch.full((n,), NAN, device=DEV) for _ in range(R.NSTEPS)]
        self.foreign = {}
        self.views = {}
        for s in R.LAYOUT:
            d = inp[s.name] if mutate is None or s.name not in mutate else mutate[s.name]
            if s.offset is None:
                sh = R.FOREIGN_SHIFT[s.name]
                bufs = dict(p=_can32(s.numel + 2 * PAD), m=_can32(s.numel + 2 * PAD), v=_can32(s.numel + 2 * PAD),
                            g=[torch.full((s.numel + 2 * PAD,), NAN, device=DEV) for _ in range(R.NSTEPS)])
                self.foreign[s.name] = bufs
                lo = PAD + sh
                vw = dict(p=bufs["p"][lo:lo + s.numel], m=bufs["m"][lo:lo + s.numel], v=bufs["v"][lo:lo + s.numel],
                          g=[x[lo:lo + s.numel] for x in bufs["g"]], shadow=None)
            else:
                lo = s.offset
                vw = dict(p=self.p[lo:lo + s.numel], m=self.m[lo:lo + s.numel], v=self.v[lo:lo + s.numel],
                          g=[x[lo:lo + s.numel] for x in self.g], shadow=self.shadow[lo:lo + s.numel])
            for k in "pmv":
                vw[k].copy_(d[k])
            if vw["shadow"] is not None:
                vw["shadow"].copy_(d["p"].bfloat16())
            for k in range(R.NSTEPS):
                if d["gs"][k] is not None:
                    vw["g"][k].copy_(d["gs"][k])
            self.views[s.name] = vw
        self.live = [[s for s in R.LAYOUT if inp[s.name]["gs"][k] is not None] for k in range(R.NSTEPS)]
        self.clip = None if case.clip is None else torch.tensor([NAN, case.clip, NAN, NAN], dtype=torch.float32, device=DEV)
        self.steps = [case.step0, case.step0]
        self.tables = {}

    def buffers(self):
        out = [self.p, self.m, self.v, self.shadow] + self.g
        for b in self.foreign.values():
            out += [b["p"], b["m"], b["v"]] + b["g"]
        return out

    def args(self, k):
        """(vk_lamb_args, keep-alive) of step k; the tables are built once per liveness pattern, as the optimizer does."""
        from volta_amd.optimization import lamb_tables
        L = _lib()
        case, live = self.case, self.live[k]
        key = tuple(s.name for s in live)
        if key not in self.tables:
            rows = []
            for s in live:
                vw = self.views[s.name]
                rows.append((vw["p"].data_ptr(), vw["g"][k].data_ptr(), vw["m"].data_ptr(), vw["v"].data_ptr(),
                             vw["shadow"].data_ptr() if vw["shadow"] is not None else 0, s.numel, CLS[s.group], s.group))
            T, P, G = lamb_tables(rows, case.max_norm)
            nbytes = L.lib.vk_lamb_work_bytes(T.ctypes.data, len(T), P.ctypes.data, len(P), G.ctypes.data, len(G))
            assert nbytes > 0, L.lib.vk_last_error()
            assert nbytes % 4 == 0
            dev = [torch.from_numpy(x.view(np.uint8).reshape(-1).copy()).to(DEV) for x in (T, P, G)]
            self.tables[key] = dict(host=(T, P, G), dev=dev, nbytes=nbytes, work=_can32(nbytes // 4 + PAD), table=_can32(4 * len(T) + PAD))
        else:                                              # the gradients of another step: the same tables with other g pointers
            T = self.tables[key]["host"][0]
            T["g"] = [self.views[s.name]["g"][k].data_ptr() for s in live]
            self.tables[key]["dev"][0] = torch.from_numpy(T.view(np.uint8).reshape(-1).copy()).to(DEV)
        t = self.tables[key]
        T, P, G = t["host"]
        a = L.LambArgs()
        a.tensors, a.pieces, a.groups = T.ctypes.data, P.ctypes.data, G.ctypes.data
        a.d_tensors, a.d_pieces, a.d_groups = (x.data_ptr() for x in t["dev"])
        a.work, a.work_bytes, a.table = t["work"].data_ptr(), t["nbytes"], t["table"].data_ptr()
        a.clip = self.clip.data_ptr() if self.clip is not None else None
        a.ntensors, a.npieces, a.ngroups = len(T), len(P), len(G)
        h = case.h
        a.flags = (L.LAMB_ADAM_W_MODE if h.adam_w else 0) | (L.LAMB_GRAD_AVERAGING if h.grad_averaging else 0) | (L.LAMB_GLOBAL_NORM if h.global_norm else 0)
        for c in range(L.LAMB_CLASSES):
            a.cls_lr[c] = a.cls_wd[c] = a.cls_bc1[c] = a.cls_bc2[c] = NAN
        for gi in range(2):
            a.cls_lr[CLS[gi]], a.cls_wd[CLS[gi]] = case.lr[gi], case.wd[gi]
            a.cls_bc1[CLS[gi]], a.cls_bc2[CLS[gi]] = R.bias_corrections(h, self.steps[gi] + 1)
        a.beta1, a.beta2, a.eps, a.grad_scale = h.b1, h.b2, h.eps, case.grad_scale
        return a, t

    def step(self, k):
        L = _lib()
        a, t = self.args(k)
        L.check(L.lib.vk_lamb_step(C.byref(a), L.stream_ptr()))
        torch.cuda.synchronize()
        self.steps = [x + 1 for x in self.steps]
        return t


def _live_mask(bench, k, foreign=None):
    """True where step k may write: the elements of its live tensors (arena), or of one tensor outside it."""
    if foreign is not None:
        n = [s for s in R.LAYOUT if s.name == foreign][0].numel
        m = torch.zeros(n + 2 * PAD, dtype=torch.bool, device=DEV)
        if foreign in [s.name for s in bench.live[k]]:
            lo = PAD + R.FOREIGN_SHIFT[foreign]
            m[lo:lo + n] = True
        return m
    m = torch.zeros(R.ARENA_TOTAL + PAD, dtype=torch.bool, device=DEV)
    for s in bench.live[k]:
        if s.offset is not None:
            m[s.offset:s.offset + s.numel] = True
    return m


def _run(case, inp, check=True, mutate=None):
    """NSTEPS steps; with `check`, every statement of the module docstring after each.  Returns the final bits of every buffer and table."""
    b = Bench(case, inp, mutate)
    W = R.restated(case, inp) if check else None
    tabs = []
    for k in range(R.NSTEPS):
        before = [x.clone() for x in b.buffers()]
        t = b.step(k)
        tabs.append(t["table"].clone())
        if not check:
            continue
        W.step(R.step_grads(inp, k), case.grad_scale, case.clip)
        live = b.live[k]
        assert set(W.last) == {s.name for s in live}
        worst = 0.0
        rows = t["table"][:4 * len(live)].view(-1, 4).cpu()
        for s in R.LAYOUT:
            vw = b.views[s.name]
            worst = max(worst, W.excess(s.name, vw["p"].cpu(), vw["m"].cpu(), vw["v"].cpu()))
        for i, s in enumerate(live):
            worst = max(worst, W.excess_table(s.name, rows[i].tolist()))
            if s.offset is not None:
                assert _same(b.views[s.name]["shadow"], b.views[s.name]["p"].bfloat16()), s.name          # RNE of the p written
        assert worst <= 1.0, (case.id, k, worst)
        # what the contract does not assign keeps its bits
        after = b.buffers()
        amask = _live_mask(b, k)
        for x0, x1 in zip(before[:4], after[:4]):
            assert _same(x0[~amask], x1[~amask])
        for x0, x1 in zip(before[4:4 + R.NSTEPS], after[4:4 + R.NSTEPS]):
            assert _same(x0, x1)                                                                           # g: every bit, NaN gaps included
        at = 4 + R.NSTEPS
        for name, bufs in b.foreign.items():
            fmask = _live_mask(b, k, name)
            for x0, x1 in zip(before[at:at + 3], after[at:at + 3]):
                assert _same(x0[~fmask], x1[~fmask]), name
            for x0, x1 in zip(before[at + 3:at + 3 + R.NSTEPS], after[at + 3:at + 3 + R.NSTEPS]):
                assert _same(x0, x1), name
            at += 3 + R.NSTEPS
        assert bool((_bits(t["work"][t["nbytes"] // 4:]) == CAN32).all()) and bool((_bits(t["table"][4 * len(live):]) == CAN32).all())
        assert bool(torch.isfinite(t["table"][:4 * len(live)]).all())
    return [x.clone() for x in b.buffers()] + tabs, b


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_lamb_step_against_the_restatement(case):
    inp = R.lamb_inputs(case)
    first, b = _run(case, inp)
    again, _ = _run(case, inp, check=False)
    assert len(first) == len(again) and all(_same(x, y) for x, y in zip(first, again))                     # two runs: equal bits
    rows = {s.name: first[-1][4 * i:4 * i + 4].tolist() for i, s in enumerate(b.live[-1])}
    assert len({rows[n][1] for n in ("w_q", "w_k", "w_v")}) == 3 and len({rows[n][1] for n in ("b_q", "b_k", "b_v")}) == 3
    if "zero_u" in rows:
        assert rows["zero_u"][0] == R.f32(case.lr[1]) and rows["zero_u"][1] == 1.0 and rows["zero_u"][3] == 0.0    # all-zero update: ratio = lr
    for n in case.skip:
        assert all(_same(b.views[n][k], inp[n][k].to(DEV)) for k in "pmv")


def test_first_step_of_an_all_zero_p_takes_ratio_lr():
    case = R.CASES[0]
    inp = R.lamb_inputs(case)
    b = Bench(case, inp)
    t = b.step(0)
    i = [s.name for s in b.live[0]].index("zero_p")
    row = t["table"][4 * i:4 * i + 4].tolist()
    assert row[0] == R.f32(case.lr[0]) and row[1] == 1.0 and row[2] == 0.0 and row[3] > 0.0
    assert bool((b.views["zero_p"]["p"] != 0).any())


def test_a_tensor_does_not_depend_on_its_chunk_neighbour():
    """b_k and w_k get other p, g, m, v (no clipping in this case, so the group's gradient norm plays no part): b_q, b_v, w_q, w_v -- in the
    same chunk -- keep every bit of p, m, v, shadow and of their table rows."""
    case = [c for c in R.CASES if c.id == "biglr-bigwd-noclip"][0]
    inp = R.lamb_inputs(case)
    other = R.lamb_inputs(case._replace(seed=case.seed + 1000))
    _, b0 = _run(case, inp, check=False)
    _, b1 = _run(case, inp, check=False, mutate={"b_k": other["b_k"], "w_k": other["w_k"]})
    names = [s.name for s in b0.live[-1]]
    t0, t1 = list(b0.tables.values())[0]["table"], list(b1.tables.values())[0]["table"]
    for n in ("b_q", "b_v", "w_q", "w_v"):
        for k in ("p", "m", "v", "shadow"):
            assert _same(b0.views[n][k], b1.views[n][k]), (n, k)
        i = names.index(n)
        assert _same(t0[4 * i:4 * i + 4], t1[4 * i:4 * i + 4]), n
    for n in ("b_k", "w_k"):
        assert not _same(b0.views[n]["p"], b1.views[n]["p"])


def test_refusals_launch_nothing():
    L = _lib()
    case = R.CASES[0]
    b = Bench(case, R.lamb_inputs(case))
    a, t = b.args(0)
    T, P, G = t["host"]
    before = [x.clone() for x in b.buffers()] + [t["work"].clone(), t["table"].clone()]

    def refused():
        assert L.lib.vk_lamb_step(C.byref(a), L.stream_ptr()) != 0 and L.lib.vk_last_error()
        torch.cuda.synchronize()
        assert all(_same(x, y) for x, y in zip(before, b.buffers() + [t["work"], t["table"]]))

    keep = int(P["count"][0]); P["count"][0] = 1025; refused(); P["count"][0] = keep
    last = int(T["piece0"][5]) + int(T["npieces"][5]) - 1                     # t2053's last piece: 5 elements
    keep = int(P["count"][last]); P["count"][last] = 6; refused(); P["count"][last] = keep
    keep = int(T["numel"][2]); T["numel"][2] = -1; refused(); T["numel"][2] = keep
    for field in ("p", "g", "m", "v"):
        keep = int(T[field][3]); T[field][3] = keep + 2; refused(); T[field][3] = keep
    keep = int(T["shadow"][3]); T["shadow"][3] = keep + 1; refused(); T["shadow"][3] = keep
    a.work_bytes = t["nbytes"] - 4; refused(); a.work_bytes = t["nbytes"]
    a.work = t["work"].data_ptr() + 4; refused(); a.work = t["work"].data_ptr()
    L.check(L.lib.vk_lamb_step(C.byref(a), L.stream_ptr()))                   # restored: accepted
    torch.cuda.synchronize()
    assert not _same(before[0], b.p)


def test_a_tensor_beyond_element_2_to_the_31():
    """A 1025-element tensor whose p, g, m, v and shadow all start beyond element 2^31 of one large allocation that is otherwise never
    touched: the address arithmetic is 64-bit.  Same results, bit for bit, as the same data in small buffers."""
    L = _lib()
    from volta_amd.optimization import lamb_tables
    n, big = 1025, (1 << 31) + 7 * 4096
    gen = torch.Generator().manual_seed(9)
    data = dict(p=torch.randn(n, generator=gen), g=torch.randn(n, generator=gen) * 0.1, m=torch.randn(n, generator=gen) * 0.01,
                v=torch.rand(n, generator=gen) * 1e-3 + 1e-8)
    results = []
    for large in (False, True):
        buf = torch.empty(big if large else 7 * 4096, dtype=torch.float32, device=DEV)
        base = buf.numel() - 7 * 4096                                           # 0, or 2^31
        region = buf[base:]
        _bits(region).fill_(CAN32)
        vw = {k: region[4096 * (i + 1):4096 * (i + 1) + n] for i, k in enumerate("pgmv")}
        shadow = region[5 * 4096:6 * 4096].view(torch.bfloat16)[:n]            # a bf16 element offset beyond 2^32 in the large buffer
        for k in "pgmv":
            vw[k].copy_(data[k])
        T, P, G = lamb_tables([(vw["p"].data_ptr(), vw["g"].data_ptr(), vw["m"].data_ptr(), vw["v"].data_ptr(), shadow.data_ptr(), n, 0, 0)], [1.0])
        if large:
            assert (int(T["p"][0]) - buf.data_ptr()) // 4 > 1 << 31
        nbytes = L.lib.vk_lamb_work_bytes(T.ctypes.data, 1, P.ctypes.data, len(P), G.ctypes.data, 1)
        dev = [torch.from_numpy(x.view(np.uint8).reshape(-1).copy()).to(DEV) for x in (T, P, G)]
        work, table = _can32(nbytes // 4 + PAD), _can32(4 + PAD)
        a = L.LambArgs()
        a.tensors, a.pieces, a.groups = T.ctypes.data, P.ctypes.data, G.ctypes.data
        a.d_tensors, a.d_pieces, a.d_groups = (x.data_ptr() for x in dev)
        a.work, a.work_bytes, a.table = work.data_ptr(), nbytes, table.data_ptr()
        a.ntensors, a.npieces, a.ngroups, a.flags = 1, len(P), 1, L.LAMB_ADAM_W_MODE | L.LAMB_GRAD_AVERAGING
        a.cls_lr[0], a.cls_wd[0] = 1e-3, 0.01
        a.cls_bc1[0], a.cls_bc2[0] = R.bias_corrections(R.hyper(), 1)
        a.beta1, a.beta2, a.eps, a.grad_scale = 0.9, 0.999, 1e-6, 1.0
        L.check(L.lib.vk_lamb_step(C.byref(a), L.stream_ptr()))
        torch.cuda.synchronize()
        assert _same(shadow, vw["p"].bfloat16()) and _same(vw["g"], data["g"].to(DEV))
        results.append([region.clone(), table.clone()])
        del buf, region, vw, shadow
    assert all(_same(x, y) for x, y in zip(*results))
    region = results[0][0]
    touched = torch.zeros(7 * 4096, dtype=torch.bool, device=DEV)
    for i in range(5):
        touched[4096 * (i + 1):4096 * (i + 1) + n] = True
    assert bool((_bits(region)[~touched] == CAN32).all())
    h = R.hyper()
    W = R.Lamb64([("t", data["p"], data["m"], data["v"], 0, "t")], [dict(lr=1e-3, wd=0.01, max_norm=1.0, step=0)], h)
    W.step({"t": data["g"]})
    assert W.excess("t", region[4096:4096 + n].cpu(), region[3 * 4096:3 * 4096 + n].cpu(), region[4 * 4096:4 * 4096 + n].cpu()) <= 1.0
    assert W.excess_table("t", results[0][1][:4].tolist()) <= 1.0
