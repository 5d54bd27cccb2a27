"""Retrieval evaluation on the host: `RetrievalDatasetVal` against outputs recorded from the reference's own class
(tests/golden/retrieval_eval_reference.npz, tools/make_retrieval_eval_golden.py), LoadDatasetEval for the retrieval names, the numpy
restatement of the ranking contract (tests/ranks_restate.py) against the driver's literal loops, and the C boundary of `vk_retrieval_ranks`
(export, struct layout, host validation).  Integer outputs are compared for equality.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.retrieval_eval_fixture import CASES, F, EvalFixture  # noqa: E402
from tests import ranks_restate as RR  # noqa: E402


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    return EvalFixture(tmp_path_factory.mktemp("retrieval_eval"))


def test_fixture_lists_the_cases(fx):
    assert sorted(fx.cases) == sorted(CASES)
    kinds = {(k, kw["add_global_imgfeat"], kw["num_locs"]) for k, kw in fx.cases.values()}
    assert {k for k, _, _ in kinds} == {"RetrievalCOCO", "RetrievalFlickr30k"} and {g for _, g, _ in kinds} == {None, "first", "last"}
    assert {n for _, _, n in kinds} == {4, 5}


@pytest.mark.parametrize("tokenizer", ["words", "wordpiece"])
@pytest.mark.parametrize("case", CASES)
def test_getitem_equals_the_reference(fx, case, tokenizer):
    """every index of every case: the 9-tuple's shapes, dtypes and values bit for bit, the `[:500]` / `[500:]` halves included"""
    ds = fx.dataset(case, tokenizer)
    z = fx.z
    assert len(ds) == int(z["%s::len" % case]) and ds.num_labels == 1
    want_all, dtypes_all = fx.arrays(case)
    for i in range(len(ds)):
        got = ds[i]
        assert len(got) == 9
        half = slice(0, 500) if i % 2 == 0 else slice(500, None)
        for j in range(3):
            w = want_all[j][half]
            assert str(got[j].dtype) == dtypes_all[j] and tuple(got[j].shape) == tuple(z["%s::%d::%d::shape" % (case, i, j)]) == w.shape, (i, j)
            assert np.array_equal(got[j].numpy(), w), (i, j)
        for j in range(3, 9):
            w = z["%s::%d::%d" % (case, i, j)]
            name = "%s::%d::%d::dtype" % (case, i, j)
            if name not in z.files:
                assert not torch.is_tensor(got[j]) and type(got[j]) is int and got[j] == w.item(), (i, j)
                continue
            assert str(got[j].dtype) == str(z[name]) and tuple(got[j].shape) == w.shape, (i, j, got[j].dtype, tuple(got[j].shape))
            assert np.array_equal(got[j].numpy(), w), (i, j)


@pytest.mark.parametrize("case", CASES)
def test_host_tables_equal_the_reference(fx, case):
    """what device_arrays uploads: the image index of every caption, the image ids in first-seen order, the token tables"""
    ds = fx.dataset(case)
    z, t = fx.z, ds.host_tables()
    assert t["caption_image"].dtype == np.int32 and np.array_equal(t["caption_image"], z["%s::caption_image" % case])
    assert t["image_ids"].dtype == np.int64 and np.array_equal(t["image_ids"], z["%s::image_entries" % case])
    Nc = len(ds) // 2
    for j, name in ((3, "input_ids"), (4, "input_mask"), (5, "segment_ids")):
        want = np.stack([z["%s::%d::%d" % (case, 2 * c, j)] for c in range(Nc)])
        assert t[name].dtype == np.int64 and np.array_equal(t[name], want), name
    assert set(range(len(t["image_ids"]))) - set(t["caption_image"].tolist()) == {5}          # the fixture's image without a caption


@pytest.mark.parametrize("case", CASES)
def test_chunked_segment_lists_give_the_reference_arrays(fx, case):
    """what device_arrays hands to `vk_task_batch`, chunk by chunk (three images each), through the numpy restatement of that kernel
    (tests/taskbatch_restate.py): the reference's features_all / spatials_all / image_mask_all bit for bit"""
    from tests import taskbatch_restate as RS
    from volta_amd.datasets import ImageStager
    ds = fx.dataset(case, chunk_images=3)
    stager = ImageStager(ds._image_features_reader, sets=2, pin_memory=False)
    parts = []
    for k, i0 in enumerate(range(0, len(ds._image_entries), ds.chunk_images)):
        h = stager.stage(ds._image_entries[i0:i0 + ds.chunk_images], k % 2)
        S = h["S"]
        assert S == 3 and h["staged_all"]
        feat, boxes = h["stage"]["feat"][:S].numpy().copy(), h["stage"]["boxes"][:S].numpy().copy()
        for s in range(S):                                               # rows past n are uninitialised in staging and must not matter
            feat[s, h["n"][s]:], boxes[s, h["n"][s]:] = np.nan, np.nan
        segs, counts = ds._chunk_blocks(h["n"])
        parts.append(RS.task_batch(feat, boxes, h["n"], h["wh"], segs, counts, ds.block_rows, ds._num_locs, ds._add_global_imgfeat))
    (feat_all, loc_all, mask_all), _ = fx.arrays(case)
    for name, want in (("features", feat_all), ("spatials", loc_all), ("image_mask", mask_all)):
        got = np.concatenate([p[name] for p in parts])
        assert got.dtype == want.dtype and np.array_equal(got, want), name


def test_a_caption_without_its_image_is_refused_and_the_device_surface_needs_a_gpu(fx):
    from volta_amd import datasets as D
    with pytest.raises(ValueError, match=r"caption 1 \('b'\) belongs to image 7"):
        D.RetrievalDatasetVal._index_captions([3, 5], [dict(caption="a", image_id=5), dict(caption="b", image_id=7)])
    assert D.RetrievalDatasetVal._index_captions([3, 5], [dict(caption="a", image_id=5)]).tolist() == [1]
    with pytest.raises(ValueError, match="RetrievalCOCO and RetrievalFlickr30k"):
        D.RetrievalDatasetVal(task="VQA", dataroot=fx.root, annotations_jsonpath=fx.jsonpath("RetrievalCOCO"), split="test", image_features_reader=None,
                              gt_image_features_reader=None, tokenizer=fx.tokenizer(), bert_model="bert-base-uncased")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="MI355X"):
            fx.dataset("coco_last").device_arrays()


def test_target_past_the_500_block_keeps_the_reference_quirk(fx):
    """more than 1000 images: the second half holds more than 500, and a target there raises as the reference's `target_all[i] = 1` does"""
    ds = fx.dataset("coco_last")
    ds.caption_image = np.asarray([499, 500, 999, 1000], np.int32)
    assert [ds._target_pos(0, 0), ds._target_pos(0, 1), ds._target_pos(1, 0), ds._target_pos(1, 1), ds._target_pos(2, 1)] == [499, None, None, 0, 499]
    with pytest.raises(IndexError):
        ds._target_pos(3, 1)


def _args(fx, **kw):
    base = dict(bert_model=fx.vocab_file, do_lower_case=True, in_memory=False, grad_acc_steps=1, local_rank=-1, num_workers=2, drop_last=False,
                batch_size=3, split="", seed=0)
    base.update(kw)
    return types.SimpleNamespace(**base)


@pytest.mark.parametrize("name", ["RetrievalFlickr30k", "RetrievalCOCO"])
def test_load_dataset_eval_serves_retrieval(fx, name):
    from volta_amd import datasets as D
    from volta_amd import task_utils as TU
    config = types.SimpleNamespace(v_feature_size=F, num_locs=5, add_global_imgfeat="first", fusion_method="mul")
    cfg = {"TASK8": dict(name=name, dataroot=fx.root, features_h5path1=fx.store, features_h5path2="", train_annotations_jsonpath="",
                         val_annotations_jsonpath=fx.jsonpath(name), train_split="", val_split="test", max_seq_length=12, max_region_num=16, batch_size=64,
                         eval_batch_size=1, type="VL-logit", process="retrieval")}
    bs, iters, dset, dl = TU.LoadDatasetEval(_args(fx), config, cfg, "8")
    captions = 10
    assert D.RetrievalEvalMap[name] is D.RetrievalDatasetVal and type(dset) is D.RetrievalDatasetVal and isinstance(dl, D.RetrievalEvalLoader)
    assert bs == 1 and iters == {"TASK8": 2 * captions} and len(dset) == 2 * captions == len(dl) and dl.dataset is dset
    assert dset.split == "test" and dset.block_rows == 17 and dset._text[0].shape == (captions, 12)
    cfg["TASK8"].pop("eval_batch_size")
    assert TU.LoadDatasetEval(_args(fx, split="val"), config, cfg, "8")[0] == 3
    with pytest.raises(KeyError, match="RetrievalDatasetVal"):           # the map of TaskLoader's datasets stays as it is
        D.DatasetMapEval[name]


# ------------------------------------------------------------------------------------------------ the restatement
def _driver_loops(S, caption_image):
    """eval_retrieval.py:200-208, 222 and 249-256, literally: np.argsort(-x) without `kind`, target matrix, np.where"""
    Nc, Ni = S.shape
    score_matrix = S.astype(np.float64)                      # the driver's matrix is float64 (np.zeros)
    target_matrix = np.zeros((Nc, Ni))
    target_matrix[np.arange(Nc), caption_image] = 1
    rank_matrix, results = np.ones(Nc) * Ni, []
    for caption_idx in range(Nc):
        rank = np.where((np.argsort(-score_matrix[caption_idx]) == np.where(target_matrix[caption_idx] == 1)[0][0]) == 1)[0][0]
        rank_matrix[caption_idx] = rank
        results.append(np.argsort(-score_matrix[caption_idx]).tolist()[:20])
    rank_tr = np.zeros(Ni)
    for image_idx in range(Ni):
        ranks = []
        tgt_captions = np.where(target_matrix[:, image_idx] == 1)[0]
        sorted_scores = np.argsort(-score_matrix[:, image_idx])
        for tgt_caption in tgt_captions:
            ranks.append(np.where((sorted_scores == tgt_caption) == 1)[0][0])
        rank_tr[image_idx] = min(ranks)
    return rank_matrix, results, rank_tr


@pytest.mark.parametrize("shape", [(35, 7), (60, 30), (200, 40)])
def test_restatement_equals_the_driver_loops_without_ties(shape):
    Nc, Ni = shape
    rng = np.random.default_rng(Nc)
    S = rng.permutation(Nc * Ni).astype(np.float32).reshape(Nc, Ni) - 0.5 * Nc * Ni          # distinct values: no ties anywhere
    caption_image = np.arange(Nc) % Ni                                                       # every image has a caption, as in the driver
    rng.shuffle(caption_image)
    want_ir, want_top, want_tr = _driver_loops(S, caption_image)
    rank_ir, topk_ir, rank_tr = RR.ranks(S, caption_image, 20)
    assert np.array_equal(rank_ir, want_ir.astype(np.int32)) and np.array_equal(rank_tr, want_tr.astype(np.int32))
    assert [[v for v in row if v >= 0] for row in topk_ir.tolist()] == want_top
    for got, want in ((RR.metrics(rank_ir), want_ir), (RR.metrics(rank_tr), want_tr)):
        assert got == dict(r1=100.0 * np.sum(want < 1) / len(want), r5=100.0 * np.sum(want < 5) / len(want), r10=100.0 * np.sum(want < 10) / len(want),
                           medr=np.floor(np.median(want) + 1), meanr=np.mean(want) + 1)


def test_restatement_order_rules():
    nan, inf = np.float32("nan"), np.float32("inf")
    s = np.asarray([0.0, nan, -0.0, inf, 1.0, -inf, 1.0, nan], np.float32)
    assert RR.order(s).tolist() == [3, 4, 6, 0, 2, 5, 1, 7]              # ties by index, signed zeros alike, NaN last
    rank_ir, topk_ir, rank_tr = RR.ranks(s[None], np.asarray([9]), 10)
    assert rank_ir.tolist() == [-1] and topk_ir[0].tolist() == [3, 4, 6, 0, 2, 5, 1, 7, -1, -1] and rank_tr.tolist() == [-1] * 8
    from volta_amd.retrieval import rank_metrics
    r = np.asarray([0, 3, 7, 12, 0, 1], np.int32)
    assert rank_metrics(r) == RR.metrics(r)


# ------------------------------------------------------------------------------------------------ the C boundary
def test_ranks_entry_is_exported_and_declared():
    from volta_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "volta_hip.h")).read(), flags=re.S)
    assert "vk_retrieval_ranks" in L.EXPORTS and hasattr(L.lib, "vk_retrieval_ranks")
    assert re.search(r"\bint\s+vk_retrieval_ranks\s*\(\s*const\s+vk_retrieval_ranks_args\s*\*", text)
    assert "#define VK_RANKS_MAX_TOPK %d" % L.RANKS_MAX_TOPK in text


def test_ranks_struct_layout_matches_the_header(tmp_path):
    """sizeof and the offset of every member of the ctypes mirror against a C translation unit compiled from the header"""
    from volta_amd import _lib as L
    fields = [n for n, _ in L.RetrievalRanksArgs._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "volta_hip.h"\nint main(void){printf("%zu\\n", sizeof(vk_retrieval_ranks_args));' + "".join(
        'printf("%%zu\\n", offsetof(vk_retrieval_ranks_args, %s));' % n for n in fields) + "return 0;}"
    c, exe = str(tmp_path / "s.c"), str(tmp_path / "s")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert ctypes.sizeof(L.RetrievalRanksArgs) == out[0]
    assert [getattr(L.RetrievalRanksArgs, n).offset for n in fields] == out[1:]


def test_ranks_host_validation_errors_without_gpu():
    """argument checks happen on the host before any launch and report through vk_last_error()"""
    from volta_amd import _lib as L
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(**kw):
        v = dict(S=p, caption_image=p, image_ptr=p, image_captions=p, rank_ir=p, topk_ir=p, rank_tr=p, target_key=p, count=p, ld=4, Nc=2, Ni=4, K=2, reserved_=0)
        v.update(kw)
        a = L.RetrievalRanksArgs(*[v[n] for n, _ in L.RetrievalRanksArgs._fields_])
        rc = L.lib.vk_retrieval_ranks(ctypes.byref(a), None)
        return rc, L.lib.vk_last_error().decode()

    for name in ("S", "caption_image", "image_ptr", "image_captions", "rank_ir", "topk_ir", "rank_tr", "target_key", "count"):
        rc, msg = call(**{name: None})
        assert rc != 0 and "null pointer" in msg, name
    rc, msg = call(ld=3)
    assert rc != 0 and "leading dimension 3" in msg
    for k in (-1, 65):
        rc, msg = call(K=k)
        assert rc != 0 and "top-k of %d" % k in msg
    for kw in (dict(Nc=0), dict(Ni=0), dict(Nc=-3), dict(Ni=-1, ld=4)):
        rc, msg = call(**kw)
        assert rc != 0 and "must be positive" in msg, kw
    assert L.lib.vk_retrieval_ranks(None, None) != 0
    with pytest.raises(L.VoltaHipError, match="top-k"):
        L.check(call(K=99)[0])
