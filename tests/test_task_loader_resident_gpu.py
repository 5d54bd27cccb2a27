"""`TaskLoader(resident_bytes > 0)` against the default `TaskLoader` over the fixture's stores: every tensor of every batch `torch.equal`, for
every dataset case, sequential and seeded random samplers, two epochs; the pool's bookkeeping (second epoch served from the pool, a pool that
holds about half the images, a record with a line break, a truncated record).  GPU only."""
import base64
import os
import pickle
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.lmdb_writer import write_lmdb  # noqa: E402
from tests.task_data_fixture import F, Fixture  # noqa: E402

CASES = ["vqa_plain", "vqa_first_cut_sep", "vqa_last_cut", "vqa_test", "gqa_last", "gqa_cut", "gqa_test", "nlvr_plain", "nlvr_first_over", "nlvr_last_over",
         "refer_plain", "refer_first_cut", "refer_last_cut_g", "refer_testA", "retr_flickr_train", "retr_coco_val"]
BIG = 64 << 20


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    return Fixture(tmp_path_factory.mktemp("task_resident"))


def sampler(kind, n):
    from volta_amd.datasets import RandomSampler, SequentialSampler
    return SequentialSampler(n) if kind == "sequential" else RandomSampler(n, seed=11)


def epochs(fx, case, kind, reader=None, epochs=2, **kw):
    """-> (the loader, per epoch the list of batches)"""
    from volta_amd.datasets import TaskLoader
    ds = fx.dataset(case, reader=reader)
    smp = sampler(kind, len(ds))
    ld = TaskLoader(ds, 4 if len(ds) > 4 else 3, smp, prefetch=1, **kw)
    out = []
    for e in range(epochs):
        if hasattr(smp, "set_epoch"):
            smp.set_epoch(e)
        out.append([tuple(t.clone() for t in batch) for batch in ld])
    return ld, out


def assert_equal_epochs(got, want, what):
    assert len(got) == len(want)
    for e, (ge, we) in enumerate(zip(got, want)):
        assert len(ge) == len(we) > 0
        for b, (gb, wb) in enumerate(zip(ge, we)):
            assert len(gb) == len(wb) == 8
            for j, (g, w) in enumerate(zip(gb, wb)):
                assert g.dtype == w.dtype and g.shape == w.shape and g.is_cuda, (what, e, b, j)
                same = torch.equal(g.view(torch.int32), w.view(torch.int32)) if g.dtype == torch.float32 else torch.equal(g, w)
                assert same, (what, e, b, j)


def images_staged(fx, case, kind):
    """distinct images per batch, summed over the batches of an epoch (what the loader has to place)"""
    ds = fx.dataset(case)
    bs, total = 4 if len(ds) > 4 else 3, 0
    idx = list(sampler(kind, len(ds)))
    for at in range(0, len(idx), bs):
        total += len({iid for i in idx[at:at + bs] for iid in ds.images(i)})
    return total


@pytest.mark.parametrize("kind", ["sequential", "random"])
@pytest.mark.parametrize("case", CASES)
def test_resident_loader_equals_the_default_loader(fx, case, kind):
    _, want = epochs(fx, case, kind)
    ld, got = epochs(fx, case, kind, resident_bytes=BIG)
    assert_equal_epochs(got, want, case)
    st = ld.stats
    # an image that the prefetch thread staged again before the batch in flight made it resident is decoded a second time, into scratch
    assert st["host_fallback_batches"] == 0 and st["decoded_images"] - st["scratch_images"] == ld.resident_images > 0
    assert 0 < ld.resident_bytes_used <= BIG
    assert ld._pool_dev.numel() == BIG


@pytest.mark.parametrize("case", ["vqa_plain", "nlvr_plain", "refer_plain"])
def test_second_epoch_is_served_from_the_pool(fx, case):
    """cases whose image draw does not depend on a random negative: the second epoch decodes nothing and every image is a resident hit"""
    from volta_amd.datasets import TaskLoader
    ds = fx.dataset(case)
    ld = TaskLoader(ds, 4 if len(ds) > 4 else 3, prefetch=0, resident_bytes=BIG)
    for _ in ld:
        pass
    first = dict(ld.stats)
    used, images = ld.resident_bytes_used, ld.resident_images
    for _ in ld:
        pass
    assert ld.stats["decoded_images"] == first["decoded_images"] == images
    assert ld.stats["resident_hits"] - first["resident_hits"] == images_staged(fx, case, "sequential")
    assert ld.resident_bytes_used == used and ld.resident_images == images and ld.stats["scratch_images"] == 0


@pytest.mark.parametrize("case", ["vqa_plain", "nlvr_first_over", "retr_flickr_train"])
def test_a_pool_that_holds_about_half_the_images(fx, case):
    _, want = epochs(fx, case, "random")
    full, _ = epochs(fx, case, "random", epochs=1, resident_bytes=BIG)
    half = full.resident_bytes_used // 2
    ld, got = epochs(fx, case, "random", resident_bytes=half)
    assert_equal_epochs(got, want, case)
    assert ld.stats["scratch_images"] > 0 and 0 < ld.resident_bytes_used <= half == ld.resident_bytes
    assert 0 < ld.resident_images < full.resident_images and ld.stats["host_fallback_batches"] == 0


def batch_images(ds):
    """the image ids of every batch of a sequential epoch at the batch size `epochs` uses"""
    bs = 4 if len(ds) > 4 else 3
    return [{iid for i in range(at, min(at + bs, len(ds))) for iid in ds.images(i)} for at in range(0, len(ds), bs)]


def rewritten_store(fx, root, change):
    """the fixture's feature store with the record of one image -- one that a single batch of a sequential epoch uses -- passed through
    `change(record) -> record`; -> (path, image id)"""
    batches = batch_images(fx.dataset("vqa_plain"))
    once = [iid for b in batches for iid in b if sum(iid in other for other in batches) == 1]
    image_id = once[0]
    key = str(image_id)
    rd = fx.reader("vqa_plain")
    recs = {}
    for k in fx.image_keys:
        item = pickle.loads(rd.env.get(k.encode()))
        recs[k.encode()] = pickle.dumps(change(item) if k == key else item)
    recs[b"keys"] = pickle.dumps([k.encode() for k in fx.image_keys])
    path = os.path.join(str(root), "features.lmdb")
    write_lmdb(path, recs)
    return path, image_id


def reader_of(fx, path):
    import types
    from volta_amd.readers import ImageFeaturesH5Reader
    kw = fx.cases["vqa_plain"][1]
    return ImageFeaturesH5Reader(path, types.SimpleNamespace(v_feature_size=F, num_locs=kw["num_locs"], add_global_imgfeat=kw["add_global_imgfeat"]), False)


def test_a_line_break_in_the_text_sends_that_batch_through_the_host_path(fx, tmp_path):
    """The record keeps 3 * k rows, so that its unpadded text has a whole number of 4-character groups and the length arithmetic of the host
    path still gives the row count with one line break inside; both loaders read the same rewritten store."""
    def change(item):
        rows = max(3, item["num_boxes"] // 3 * 3)
        feats = np.frombuffer(base64.b64decode(item["features"]), np.float32).reshape(-1, F)[:rows]
        boxes = np.frombuffer(base64.b64decode(item["boxes"]), np.float32).reshape(-1, 4)[:rows]
        assert feats.shape[0] == rows == boxes.shape[0]
        text = base64.b64encode(feats.tobytes()).decode()
        assert not text.endswith("=")
        return dict(item, num_boxes=rows, boxes=base64.b64encode(boxes.tobytes()).decode(), features=text[:76 * 50] + "\n" + text[76 * 50:])

    from volta_amd.datasets import _ResidentPool
    path, image_id = rewritten_store(fx, tmp_path, change)
    _, want = epochs(fx, "vqa_plain", "sequential", reader=reader_of(fx, path), epochs=1)
    ld, got = epochs(fx, "vqa_plain", "sequential", reader=reader_of(fx, path), epochs=1, resident_bytes=BIG)
    assert_equal_epochs(got, want, "line break")
    assert ld.stats["host_fallback_batches"] == 1
    batches = batch_images(ld.dataset)
    (spoiled,) = [b for b in batches if image_id in b]
    clean = set().union(*[b for b in batches if b is not spoiled])
    assert all(ld._resident.get(iid) is None for iid in spoiled - clean)                  # nothing of that batch entered the pool
    assert set(ld._resident.items) == clean and ld.resident_images == len(clean)
    # the stretches of the failed batch were given back: the pool holds the resident images and nothing else
    assert ld.resident_bytes_used == sum(_ResidentPool.layout(0, ld._resident.get(iid)[3], F)[3] for iid in clean)


def test_a_truncated_record_raises_the_host_paths_error(fx, tmp_path):
    change = lambda item: dict(item, features=item["features"][:len(item["features"]) // 2 // 4 * 4])
    path, _ = rewritten_store(fx, tmp_path, change)
    errors = []
    for kw in (dict(), dict(resident_bytes=BIG)):
        with pytest.raises(ValueError) as e:
            epochs(fx, "vqa_plain", "sequential", reader=reader_of(fx, path), epochs=1, **kw)
        errors.append(str(e.value))
    assert errors[0] == errors[1] and errors[0]


def test_in_memory_and_negative_sizes_are_refused(fx):
    from volta_amd.datasets import TaskLoader
    ds = fx.dataset("vqa_plain")
    with pytest.raises(ValueError):
        TaskLoader(ds, 2, in_memory=True, resident_bytes=1 << 20)
    with pytest.raises(ValueError):
        TaskLoader(ds, 2, resident_bytes=-5)
