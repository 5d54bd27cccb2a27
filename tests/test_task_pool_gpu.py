"""`vk_task_batch_pool` / `vk_task_pool_means` (csrc/taskbatch.hip) against `vk_task_batch` on the same images: the images and segment lists
of every dataset case of tests/task_data_fixture.py, the images laid into two byte regions through per-slot offsets.  Every output tensor and
every stored global row must be `torch.equal`.  The slot tables are untrusted: a slot with a bad `where`, offset or row count must feed no row
and leave the rows of the other slots alone.  Both regions are the middle of larger tensors, so an unchecked offset would land in memory the
test owns.  GPU only."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.task_data_fixture import F, Fixture  # noqa: E402

CASES = ["vqa_plain", "vqa_first_cut_sep", "vqa_last_cut", "vqa_test", "gqa_last", "gqa_cut", "gqa_test", "nlvr_plain", "nlvr_first_over", "nlvr_last_over",
         "refer_plain", "refer_first_cut", "refer_last_cut_g", "refer_testA", "retr_flickr_train", "retr_coco_val"]
SLACK = 1 << 16
NAMES = ("features", "spatials", "image_mask", "target")


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    return Fixture(tmp_path_factory.mktemp("task_pool"))


_staged = {}


def staged(fx, case):
    """one staged batch of the case (the default host path), its tables on the device; computed once per case"""
    if case not in _staged:
        from volta_amd.datasets import TaskLoader
        ds = fx.dataset(case)
        ld = TaskLoader(ds, 4, prefetch=0)
        h = ld._stage(list(range(min(len(ds), 6))), 0)
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        S = h["S"]
        t = dict(feat=h["stage"]["feat"][:S].cuda().contiguous(), boxes=h["stage"]["boxes"][:S].cuda().contiguous(),
                 **{k: dev(h[k]) for k in ("n", "wh", "segs", "counts", "csr", "labels", "scores", "ref_box")})
        _staged[case] = (ds, h, t)
    return _staged[case]


def target_args(ds, t):
    if ds.target_kind == "scatter":
        return dict(scatter=(t["csr"], t["labels"], t["scores"], ds.num_labels))
    return dict(ref_box=t["ref_box"]) if ds.target_kind == "iou" else {}


def lay_out(h, t, split):
    """the staged images packed into two regions: `split(s)` names the region of slot s -> (regions, where, feat_off, box_off, mean_off)"""
    from volta_amd.datasets import _ResidentPool
    S, n = h["S"], h["n"]
    at = [16, 48]                                              # neither region starts its first image at offset 0
    where, offs = np.zeros(S, np.int32), np.zeros((3, S), np.int64)
    for s in range(S):
        w = split(s)
        fo, bo, mo, size = _ResidentPool.layout(at[w], int(n[s]), F)
        where[s], offs[:, s] = w, (fo, bo, mo)
        at[w] += size + 16 * (s % 3)
    whole = [torch.full((SLACK + a + SLACK,), 0xFF, dtype=torch.uint8, device="cuda") for a in at]      # 0xFF...: NaN as fp32
    regions = [wh[SLACK:SLACK + a] for wh, a in zip(whole, at)]
    for s in range(S):
        r, rows = regions[where[s]], int(n[s])
        r[offs[0, s]:offs[0, s] + rows * F * 4] = t["feat"][s, :rows].contiguous().view(torch.uint8).view(-1)
        r[offs[1, s]:offs[1, s] + rows * 16] = t["boxes"][s, :rows].contiguous().view(torch.uint8).view(-1)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return regions, dev(where), dev(offs[0]), dev(offs[1]), dev(offs[2])


def run_both(ds, h, t, split, num_locs, add_global):
    from volta_amd import ops
    S = h["S"]
    mean = torch.full((S, F), float("nan"), device="cuda")
    want = ops.task_batch(t["feat"], t["boxes"], t["n"], t["wh"], t["segs"], t["counts"], ds.block_rows, num_locs, add_global, mean=mean, **target_args(ds, t))
    regions, where, fo, bo, mo = lay_out(h, t, split)
    slots = (regions, where, fo, bo, mo, t["n"], t["wh"], F)
    if add_global is not None:
        ops.task_pool_means(*slots, torch.arange(S, dtype=torch.int32, device="cuda"))
    got = ops.task_batch_pool(*slots, t["segs"], t["counts"], ds.block_rows, num_locs, add_global, **target_args(ds, t))
    torch.cuda.synchronize()
    return want, got, mean, slots


def stored_means(slots, S):
    regions, where, _, _, mo = slots[:5]
    return torch.stack([regions[int(where[s])][int(mo[s]):int(mo[s]) + F * 4].view(torch.float32) for s in range(S)])


@pytest.mark.parametrize("case", CASES)
def test_pool_equals_the_dense_assembler_on_every_dataset_case(fx, case):
    """the case's own num_locs and global row; odd slots in the scratch region, even slots in the pool"""
    ds, h, t = staged(fx, case)
    want, got, mean, slots = run_both(ds, h, t, lambda s: s & 1, ds._num_locs, ds._add_global_imgfeat)
    assert set(got) == set(want)
    for name in want:
        assert got[name].dtype == want[name].dtype and torch.equal(got[name], want[name]), (case, name)
    if ds._add_global_imgfeat is not None:
        assert torch.equal(stored_means(slots, h["S"]).view(torch.int32), mean.view(torch.int32)), case


@pytest.mark.parametrize("split", ["pool", "scratch", "mixed"])
@pytest.mark.parametrize("num_locs", [4, 5])
@pytest.mark.parametrize("add_global", [None, "first", "last"])
@pytest.mark.parametrize("case", ["vqa_plain", "nlvr_first_over", "refer_plain", "retr_flickr_train"])
def test_global_row_and_box_coordinate_variants(fx, case, add_global, num_locs, split):
    ds, h, t = staged(fx, case)
    where = {"pool": lambda s: 0, "scratch": lambda s: 1, "mixed": lambda s: (s // 2) & 1}[split]
    want, got, mean, slots = run_both(ds, h, t, where, num_locs, add_global)
    for name in want:
        assert torch.equal(got[name], want[name]), (case, name)
    assert got["spatials"].shape[-1] == num_locs
    if add_global is not None:
        assert torch.equal(stored_means(slots, h["S"]).view(torch.int32), mean.view(torch.int32))


@pytest.mark.parametrize("add_global", [None, "first"])
@pytest.mark.parametrize("case", ["vqa_plain", "nlvr_first_over"])
def test_untrusted_slot_tables(fx, case, add_global):
    """one slot spoiled at a time: its rows come out as if no segment named it, the other slots' rows are unchanged, nothing outside the
    regions is read into the outputs (the slack is NaN) and the mean launch writes nothing for it"""
    from volta_amd import ops
    ds, h, t = staged(fx, case)
    S, n = h["S"], h["n"]
    k = int(np.argmax(n > 0))
    segs_without = t["segs"].clone()
    segs_without[..., 3] = torch.where(segs_without[..., 0] == k, torch.zeros_like(segs_without[..., 3]), segs_without[..., 3])
    want = ops.task_batch(t["feat"], t["boxes"], t["n"], t["wh"], segs_without, t["counts"], ds.block_rows, 5, add_global, **target_args(ds, t))
    regions, where, fo, bo, mo = lay_out(h, t, lambda s: s & 1)
    honest = (regions, where, fo, bo, mo, t["n"], t["wh"], F)
    every = torch.arange(S, dtype=torch.int32, device="cuda")
    ops.task_pool_means(*honest, every)
    clean = ops.task_batch_pool(*honest, t["segs"], t["counts"], ds.block_rows, 5, add_global, **target_args(ds, t))
    assert not torch.equal(clean["features"], want["features"])             # slot k does feed rows
    size = regions[int(where[k])].numel()
    spoils = [("where", 2), ("where", -1), ("feat_off", size - 64), ("feat_off", size + (1 << 20)), ("feat_off", 1 << 62), ("feat_off", int(fo[k]) + 4),
              ("box_off", size - 16 * int(n[k]) + 16), ("box_off", int(bo[k]) + 8), ("n", int(n[k]) + (size // (F * 4)) + 1), ("n", -3)]
    if add_global is not None:
        spoils += [("mean_off", size - 4 * F + 16), ("mean_off", int(mo[k]) + 4)]
    for field, value in spoils:
        tabs = dict(where=where.clone(), feat_off=fo.clone(), box_off=bo.clone(), mean_off=mo.clone(), n=t["n"].clone())
        tabs[field][k] = value
        slots = (regions, tabs["where"], tabs["feat_off"], tabs["box_off"], tabs["mean_off"], tabs["n"], t["wh"], F)
        before = [r.clone() for r in regions]
        ops.task_pool_means(*slots, every)
        assert all(torch.equal(a, b) for a, b in zip(before, regions)), (field, value)          # same rows rewritten, nothing for slot k
        got = ops.task_batch_pool(*slots, t["segs"], t["counts"], ds.block_rows, 5, add_global, **target_args(ds, t))
        torch.cuda.synchronize()
        assert not torch.isnan(got["features"]).any()
        for name in want:
            assert torch.equal(got[name], want[name]), (case, field, value, name)


def test_pool_entry_points_refuse_bad_arguments():
    from volta_amd import _lib as L
    a = L.TaskPoolArgs()
    a.S, a.F, a.N, a.R, a.num_locs = 1, 6, 1, 4, 5
    assert L.lib.vk_task_batch_pool(a, None) != 0 and b"multiple of 4" in L.lib.vk_last_error()
    a.F, a.num_locs = 8, 3
    assert L.lib.vk_task_batch_pool(a, None) != 0 and b"num_locs" in L.lib.vk_last_error()
    a.num_locs = 5
    assert L.lib.vk_task_pool_means(a, None, 1, None) != 0
