"""volta_amd.datasets and the loaders of volta_amd.task_utils on the host: every dataset's `__getitem__` against outputs recorded from the
reference's own classes (tests/golden/task_data_reference.npz, tools/make_task_data_golden.py), the segment lists the datasets emit for the
device assembler (through the numpy restatement of `vk_task_batch`, tests/taskbatch_restate.py), the native staging call, the samplers and
LoadDataset / LoadDatasetEval.  No GPU needed."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.task_data_fixture import F, Fixture  # noqa: E402
from tests import taskbatch_restate as RS  # noqa: E402

CASES = ["vqa_plain", "vqa_first_cut_sep", "vqa_last_cut", "vqa_test", "gqa_last", "gqa_cut", "gqa_test", "nlvr_plain", "nlvr_first_over", "nlvr_last_over",
         "refer_plain", "refer_first_cut", "refer_last_cut_g", "refer_testA", "retr_flickr_train", "retr_coco_val"]

# Global feature row: |fp32 row - float64 mean| over every image of the fixture.  Observed: reference 4.768e-08, ours 4.768e-08 (the fixture's
# features are multiples of 0.25, so the fp32 sums are exact and what is left is the rounding of the division); bound = 2 x the larger.
GLOBAL_ROW_BOUND = 2 * 4.768371586472142e-08


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    return Fixture(tmp_path_factory.mktemp("task_data"))


def test_fixture_lists_the_cases(fx):
    assert sorted(fx.cases) == sorted(CASES)


@pytest.mark.parametrize("tokenizer", ["words", "wordpiece"])
@pytest.mark.parametrize("case", CASES)
def test_getitem_equals_the_reference(fx, case, tokenizer):
    """shapes, dtypes and every value bit for bit: features (global row included -- both sides add the rows in the same order), spatials,
    masks, tokens, targets, ids; with a plain `tokenizer.encode` object and with the native WordPieceTokenizer (one call per split)"""
    ds = fx.dataset(case, tokenizer)
    assert len(ds) == fx.length(case) and ds.num_labels == int(fx.z["%s::num_labels" % case])
    for i in range(len(ds)):
        got = ds[i]
        want, dtypes = fx.sample(case, i)
        assert len(got) == 8
        for j, (g, w, dt) in enumerate(zip(got, want, dtypes)):
            if dt is None:
                assert not torch.is_tensor(g) and g == w.item(), (i, j)
                continue
            assert str(g.dtype) == dt and tuple(g.shape) == w.shape, (i, j, g.dtype, dt, tuple(g.shape), w.shape)
            assert np.array_equal(g.numpy(), w), (i, j, float(np.abs(g.numpy().astype(np.float64) - w).max()))


def test_collate_of_the_host_path_is_what_the_drivers_unpack(fx):
    ds = fx.dataset("vqa_first_cut_sep")
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=4)))
    assert [tuple(t.shape) for t in batch] == [(4, 9, F), (4, 9, 4), (4, 9), (4, 14), (4, 7), (4, 14), (4, 14), (4,)]
    assert batch[7].dtype == torch.int64 and ds.label2ans[ds.ans2label["red"]] == "red"


def test_global_row_within_the_measured_bound_of_the_float64_mean(fx):
    rd = fx.reader("vqa_test")                                           # add_global_imgfeat = first
    worst_ref = worst_ours = 0.0
    for key in fx.image_keys:
        m64 = fx.z["img::%s::mean64" % key]
        worst_ref = max(worst_ref, float(np.abs(fx.z["img::%s::global_ref32" % key].astype(np.float64) - m64).max()))
        worst_ours = max(worst_ours, float(np.abs(rd[key][0][0].astype(np.float64) - m64).max()))
    print("global row error: reference %.4g, ours %.4g" % (worst_ref, worst_ours))
    assert worst_ref <= GLOBAL_ROW_BOUND and worst_ours <= GLOBAL_ROW_BOUND


def _staged(fx, ds, indices):
    """what TaskLoader stages for `indices`, as numpy"""
    from volta_amd.datasets import TaskLoader
    ld = TaskLoader(ds, len(indices), prefetch=0, device="cpu")
    h = ld._stage(list(indices), 0)
    S, Rcap = h["S"], h["Rcap"]
    feat, boxes = np.zeros((S, Rcap, F), np.float32), np.zeros((S, Rcap, 4), np.float32)
    for s, (f, b) in enumerate(h["src"]):
        feat[s, :f.shape[0]], boxes[s, :b.shape[0]] = f.numpy(), b.numpy()
    return h, feat, boxes


@pytest.mark.parametrize("case", CASES)
def test_segment_lists_reproduce_the_reference_through_the_restatement(fx, case):
    """The datasets' plans (segments, mask counts, CSR targets) over natively staged images, run through the numpy restatement of
    vk_task_batch, give the reference's features / spatials / image_mask / target: this is what ties the device test to the reference."""
    ds = fx.dataset(case)
    idx = list(range(len(ds)))
    h, feat, boxes = _staged(fx, ds, idx)
    kw = dict(scatter=(h["csr"], h["labels"], h["scores"], ds.num_labels)) if ds.target_kind == "scatter" else \
        dict(ref_box=h["ref_box"]) if ds.target_kind == "iou" else {}
    out = RS.task_batch(feat, boxes, h["n"], h["wh"], h["segs"], h["counts"], ds.block_rows, ds._num_locs, ds._add_global_imgfeat, **kw)
    k = ds.options
    assert h["segs"].shape == (len(ds) * k, 2, 4) and h["text_rows"].shape == (len(ds) * k,)
    for i in idx:
        want, _ = fx.sample(case, i)
        blk = slice(i, i + 1) if k == 1 else slice(k * i, k * i + k)
        for j, name in enumerate(("features", "spatials", "image_mask")):
            got = out[name][blk]
            assert np.array_equal(got[0] if k == 1 else got, want[j]), (i, name)
        if ds.target_kind == "zero":
            assert int(want[4]) == 0
        else:
            assert np.array_equal(out["target"][i], want[4]), i
        for j, t in zip((3, 5, 6), ds._text):                            # the token rows the loader gathers on the device
            got = t[h["text_rows"][blk]]
            assert np.array_equal(got[0] if k == 1 else got, want[j]), (i, j)
        assert int(h["ids"][i]) == int(want[7])


def test_retrieval_draws_and_the_region_limit(fx):
    """own draws: seedable, never the sample's own image, hard negatives from the pool on the train split; an image above the block length is
    the ValueError the class documents (the reference fails in torch.stack there)"""
    a, b, c = (fx.dataset("retr_flickr_train", seed=s) for s in (5, 5, 6))
    da, db, dc = ([d.draw(i) for i in range(len(d)) for _ in range(3)] for d in (a, b, c))
    assert da == db and da != dc
    for v, (e2, img3, e4) in enumerate(da):
        own = a._entries[v // 3]["image_id"]
        assert a._entries[e2]["image_id"] != own and img3 != own and img3 in a.imgid2entry
        pool = [a.train_image_list[int(p)] for p in a.train_hard_pool[a.train_imgId2pool[own]][1:]]
        assert a._entries[e4]["image_id"] in pool
    got = a[0]
    assert [tuple(t.shape) for t in got[:4]] == [(4, 16, 2048), (4, 16, 5), (4, 16), (4, 12)] and got[4] == 0
    kind, kw = fx.cases["retr_coco_val"]
    from volta_amd import datasets as D
    kw2 = {k: v for k, v in kw.items() if k not in ("max_region_num", "split")}
    small = D.RetrievalDataset(task=kind, dataroot=fx.dataroot(kind), annotations_jsonpath=fx.jsonpath(kind), split="val", image_features_reader=fx.reader("retr_coco_val"),
                               gt_image_features_reader=None, tokenizer=fx.tokenizer(), bert_model="bert-base-uncased", max_region_num=6,
                               negatives=lambda i: (0, 12, 0), **kw2)
    with pytest.raises(ValueError, match="max_region_num"):
        small[0]


@pytest.mark.parametrize("in_memory", [False, True])
def test_native_staging_equals_the_reader(fx, in_memory):
    from volta_amd.datasets import ImageStager
    rd = fx.reader("vqa_plain")                                          # no global row, 5 locations: loc_ori[:, :4] are the pixel boxes
    st = ImageStager(rd, threads=3, in_memory=in_memory, pin_memory=False)
    for _ in range(2):                                                   # the second pass comes from the pool when in_memory
        h = st.stage(fx.image_keys)
        assert h["S"] == len(fx.image_keys) and h["Rcap"] == 14 and h["staged_all"] == (not in_memory)
        for s, key in enumerate(fx.image_keys):
            feats, n, _, ori = rd[key]
            hw = fx.z["img::%s::hw" % key]
            assert int(h["n"][s]) == n and tuple(h["wh"][s]) == (int(hw[1]), int(hw[0]))
            assert np.array_equal(h["src"][s][0].numpy(), feats) and np.array_equal(h["src"][s][1].numpy(), ori[:, :4])
    assert (st.pool_bytes_used > 0) == in_memory
    with pytest.raises(ValueError, match="is not in list"):             # what ImageFeaturesH5Reader.__getitem__ raises today
        st.stage(["11", "no-such-image"])
    with pytest.raises(ValueError, match="is not in list"):
        rd["no-such-image"]
    assert ImageStager(rd, threads=64, pin_memory=False).threads == 16  # never more than 16 host threads


def test_pool_is_bounded(fx):
    from volta_amd.datasets import ImageStager
    rd = fx.reader("vqa_plain")
    st = ImageStager(rd, in_memory=True, pool_bytes=200_000, pin_memory=False)       # room for the 3- and 4-region images only
    h = st.stage(fx.image_keys)
    assert 0 < st.pool_bytes_used <= 200_000 and 0 < len(st._pool.items) < len(fx.image_keys)
    for s, key in enumerate(fx.image_keys):
        assert np.array_equal(h["src"][s][0].numpy(), rd[key][0])


def test_corrupt_record_is_an_error_not_a_short_read(fx):
    from volta_amd import _lib as L
    import ctypes as C
    text = b"AAAA" * 8
    out = np.zeros(64, np.float32)
    job = (L.TaskImage * 1)(L.TaskImage(C.cast(C.c_char_p(text), C.c_void_p), len(text), C.cast(C.c_char_p(text), C.c_void_p), len(text),
                                        C.c_void_p(out.ctypes.data), C.c_void_p(out.ctypes.data), 2, 4))
    assert L.lib.vk_task_images_stage(job, 1, 2, None) != 0 and b"features decode to 24 bytes" in L.lib.vk_last_error()


def test_samplers():
    from volta_amd import datasets as D
    assert list(D.SequentialSampler(5)) == [0, 1, 2, 3, 4]
    a, b = D.RandomSampler(23, seed=4), D.RandomSampler(23, seed=4)
    e0, e1 = list(a), list(a)
    assert sorted(e0) == list(range(23)) == sorted(e1) and e0 != e1      # one epoch visits every index once, two epochs differ
    assert list(b) == e0 and list(b) == e1                               # the same seed repeats
    assert list(D.RandomSampler(23, seed=5)) != e0
    shards = [D.DistributedSampler(23, 3, r, seed=1) for r in range(3)]
    got = [list(s) for s in shards]
    assert all(len(g) == 8 == len(s) for g, s in zip(got, shards))       # padded to a multiple of the world size
    flat = sorted(sum(got, []))
    assert set(flat) == set(range(23)) and len(flat) == 24
    order = [got[k % 3][k // 3] for k in range(24)]                      # rank-strided shards of one permutation, padded with its head
    assert order[23] == order[0] and sorted(order[:23]) == list(range(23))
    for s in shards:
        s.set_epoch(1)
    again = [list(s) for s in shards]
    assert again != got and set(sum(again, [])) == set(range(23))
    for s in shards:
        s.set_epoch(0)
    assert [list(s) for s in shards] == got
    assert list(D.DistributedSampler(5, 2, 1, shuffle=False)) == [1, 3, 0]


def test_loader_batching_without_a_device(fx):
    from volta_amd import datasets as D
    ds = fx.dataset("vqa_plain")
    assert len(D.TaskLoader(ds, 4, device="cpu")) == 2 and len(D.TaskLoader(ds, 4, drop_last=True, device="cpu")) == 1
    ld = D.TaskLoader(ds, 4, D.RandomSampler(len(ds), 3), device="cpu")
    assert ld.dataset is ds and ld.batch_size == 4 and sorted(sum(ld._index_batches(), [])) == list(range(6))
    assert D.DatasetMapTrain["refcoco+"] is D.ReferExpressionDataset and D.DatasetMapTrain["RetrievalCOCO"] is D.RetrievalDataset
    with pytest.raises(KeyError, match="VCRDataset"):
        D.DatasetMapTrain["VCR_Q-A"]
    with pytest.raises(KeyError, match="RetrievalDatasetVal"):
        D.DatasetMapEval["RetrievalFlickr30k"]


def _args(fx, **kw):
    base = dict(bert_model=fx.vocab_file, do_lower_case=True, in_memory=False, grad_acc_steps=1, local_rank=-1, num_workers=2, drop_last=False,
                batch_size=3, split="", seed=0)
    base.update(kw)
    return types.SimpleNamespace(**base)


def _task_cfg(fx, name="VQA", **kw):
    cfg = dict(name=name, dataroot=fx.dataroot(name), features_h5path1=fx.store, features_h5path2="", train_annotations_jsonpath="",
               val_annotations_jsonpath="", train_split="train", val_split="val" if name != "NLVR2" else "dev", max_seq_length=12, max_region_num=16,
               batch_size=4, type="VL-classifier", process="normal")
    cfg.update(kw)
    return {"TASK1": cfg}


def test_load_dataset_and_load_dataset_eval(fx, monkeypatch):
    from volta_amd import datasets as D
    from volta_amd import task_utils as TU
    config = types.SimpleNamespace(v_feature_size=F, num_locs=5, add_global_imgfeat="first", fusion_method="mul")
    bs, iters, dtr, dva, ltr, lva = TU.LoadDataset(_args(fx), config, _task_cfg(fx), "1")
    assert bs == 4 and iters == {"TASK1": 2} and len(dtr) == 6 and len(dva) == 6 and len(ltr) == 2 and len(lva) == 2
    assert isinstance(ltr, D.TaskLoader) and isinstance(ltr.sampler, D.RandomSampler) and isinstance(lva.sampler, D.SequentialSampler)
    assert ltr.dataset is dtr and dtr.block_rows == 17 and dtr.split == "train" and dva.split == "val" and dtr._text[0].shape == (6, 12)
    bs, iters, dtr, dva, ltr, lva = TU.LoadDataset(_args(fx, grad_acc_steps=2, drop_last=True), config, _task_cfg(fx, batch_size=8), "1", split="train")
    assert bs == 4 and iters == {"TASK1": 1} and dva is None and lva is None and len(ltr) == 1
    bs, iters, dtr, dva, ltr, lva = TU.LoadDataset(_args(fx), config, _task_cfg(fx), "1", split="val")
    assert iters == {} and dtr is None and ltr is None and len(lva) == 2
    # vl-bert_vqa appends [MASK] [CLS]
    cfg2 = types.SimpleNamespace(v_feature_size=F, num_locs=5, add_global_imgfeat=None, fusion_method="vl-bert_vqa")
    assert TU.LoadDataset(_args(fx), cfg2, _task_cfg(fx), "1", split="train")[2]._text[0].shape == (6, 14)
    # a faked world of 3 ranks
    import torch.distributed as dist
    monkeypatch.setattr(dist, "get_world_size", lambda: 3)
    monkeypatch.setattr(dist, "get_rank", lambda: 2)
    bs, iters, dtr, _, ltr, _ = TU.LoadDataset(_args(fx, local_rank=2), config, _task_cfg(fx, batch_size=6), "1", split="train")
    assert bs == 2 and isinstance(ltr.sampler, D.DistributedSampler) and (ltr.sampler.world, ltr.sampler.rank) == (3, 2)
    assert len(ltr.sampler) == 2 and iters == {"TASK1": 1}
    bs, iters, dva, lva = TU.LoadDatasetEval(_args(fx, local_rank=2, batch_size=9), config, _task_cfg(fx), "1")
    assert bs == 3 and iters == {"TASK1": 2} and dva.split == "val"
    monkeypatch.undo()
    bs, iters, dva, lva = TU.LoadDatasetEval(_args(fx, split="minval"), config, _task_cfg(fx, eval_batch_size=5), "1")
    assert bs == 5 and iters == {"TASK1": 2} and dva.split == "minval" and len(dva) == 6
    bs, _, dva, lva = TU.LoadDatasetEval(_args(fx), config, _task_cfg(fx, "NLVR2"), "1")
    assert bs == 3 and isinstance(dva, D.NLVR2Dataset) and len(lva) == 2 and dva.block_rows == 34
    with pytest.raises(FileNotFoundError, match="does not download"):
        TU.LoadDataset(_args(fx, bert_model="bert-base-uncased"), config, _task_cfg(fx), "1")
    with pytest.raises(KeyError, match="volta.datasets.VCRDataset"):
        TU.LoadDataset(_args(fx), config, {"TASK1": dict(_task_cfg(fx)["TASK1"], name="VCR_Q-A")}, "1")
