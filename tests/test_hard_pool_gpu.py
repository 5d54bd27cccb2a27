"""`volta_amd.retrieval.generate_hard_pool` end to end on the GPU: an LMDB feature store built from tests/golden/hard_pool_reference.npz, the
pool against the golden one (the reference script's arithmetic with sklearn's BallTree) exactly, the pickle, and `RetrievalDataset` over it."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.hard_pool_fixture import VOCAB, PoolFixture, WordTokenizer  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    return PoolFixture(tmp_path_factory.mktemp("hard_pool_gpu"))


def test_means_equal_row_zero_of_the_reader(fx):
    from volta_amd.retrieval import image_mean_features
    reader = fx.reader("first")
    ids = fx.image_list[:70] + fx.image_list[3:5]                        # more than one chunk, an id twice
    got = image_mean_features(reader, ids, chunk=32).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (72, fx.F)
    for row, iid in zip(got, ids):
        assert np.array_equal(row.view(np.uint32), reader[iid][0][0].view(np.uint32)), iid
    assert np.array_equal(got[:70], fx.z["means"][:70])


@pytest.mark.parametrize("task", ["RetrievalFlickr30k", "RetrievalCOCO"])
def test_generate_hard_pool_equals_the_golden_pool(fx, task, tmp_path):
    from volta_amd import datasets as D
    from volta_amd.retrieval import generate_hard_pool
    reader = fx.reader(None)
    out = str(tmp_path / "hard_negative.pkl")
    res = generate_hard_pool(reader, fx.jsonpath(task), task, k=100, out=out, chunk=64)
    assert sorted(res) == ["train_hard_pool", "train_image_list"]
    pool = res["train_hard_pool"]
    assert isinstance(pool, np.ndarray) and pool.dtype == np.float64 and pool.shape == (fx.N, 100)
    assert np.array_equal(pool, fx.z["pool"].astype(np.float64))
    assert type(res["train_image_list"]) is list and res["train_image_list"] == fx.image_list and all(type(v) is int for v in res["train_image_list"])
    with open(out, "rb") as f:
        back = pickle.load(f)
    assert sorted(back) == sorted(res) and back["train_image_list"] == fx.image_list
    assert back["train_hard_pool"].dtype == np.float64 and np.array_equal(back["train_hard_pool"], pool)
    assert not os.path.exists(os.path.join(fx.root, "hard_negative.pkl"))            # nothing is written beside the annotations unasked

    ds = D.RetrievalDataset(task=task, dataroot=str(tmp_path), annotations_jsonpath=fx.jsonpath(task), split="train", image_features_reader=reader,
                            gt_image_features_reader=None, tokenizer=WordTokenizer(VOCAB), bert_model="bert-base-uncased", max_seq_length=12,
                            max_region_num=8, seed=3)
    assert len(ds) == 2 * fx.N and np.array_equal(ds.train_hard_pool, pool) and ds.train_image_list == fx.image_list
    for index in (0, 1, 2 * 17, 2 * 150 + 1, 2 * fx.N - 1):
        _, _, e4 = ds.draw(index)
        row = pool[index // 2]
        allowed = {fx.image_list[int(p)] for p in row[1:]}
        assert ds.entries[e4]["image_id"] in allowed and ds.entries[e4]["image_id"] != fx.image_list[index // 2]


def test_out_true_writes_beside_the_annotations(fx, tmp_path):
    import shutil
    from volta_amd.retrieval import generate_hard_pool
    ann = str(tmp_path / "coco.jsonline")
    shutil.copy(fx.jsonpath("RetrievalCOCO"), ann)
    res = generate_hard_pool(fx.reader(None), ann, "RetrievalCOCO", k=7, out=True)
    with open(str(tmp_path / "hard_negative.pkl"), "rb") as f:
        back = pickle.load(f)
    assert np.array_equal(back["train_hard_pool"], res["train_hard_pool"]) and res["train_hard_pool"].shape == (fx.N, 7)
    assert np.array_equal(res["train_hard_pool"], fx.z["pool"][:, :7].astype(np.float64))
