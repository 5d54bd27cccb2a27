"""Host side of `TaskLoader(resident_bytes > 0)`: the pool's allocator and dictionary, the text layout against `_b64_rows` on the fixture's
records, `vk_task_texts_pack`, the struct mirrors and the argument errors.  No GPU needed."""
import ctypes as C
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.task_data_fixture import F, Fixture  # noqa: E402


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    return Fixture(tmp_path_factory.mktemp("task_resident"))


def test_pool_allocator_alignment_refusal_and_rollback():
    from volta_amd.datasets import _ResidentPool
    size = lambda n: _ResidentPool.layout(0, n, 8)[3]
    assert size(3) == 3 * 32 + 32 + 48 and _ResidentPool.layout(160, 3, 8) == (160, 160 + 128, 160 + 96, 176)
    pool = _ResidentPool(1000)
    a = pool.reserve(size(3))
    b = pool.reserve(40)                                       # not a multiple of 16: the next offset is rounded up
    c = pool.reserve(size(1))
    assert (a, b, c) == (0, 176, 224) and all(o % 16 == 0 for o in (a, b, c)) and pool.used == 224 + size(1)
    mark = pool.mark()
    assert pool.reserve(1000) is None and pool.used == mark     # refused when full, nothing taken
    d = pool.reserve(size(2))
    assert d == 304 and pool.used > mark
    pool.rollback(mark)
    assert pool.used == mark and pool.reserve(size(2)) == d     # the stretch is handed out again
    assert pool.reserve(1000 - pool.used + 1) is None
    assert len(pool) == 0 and pool.get("x") is None
    pool.commit({"x": (0, 128, 96, 3, 640, 480)})
    assert len(pool) == 1 and pool.get("x")[3] == 3
    with pytest.raises(AssertionError):
        pool.rollback(pool.used + 16)


def _records(fx):
    from volta_amd.readers import ImageFeaturesH5Reader  # noqa: F401
    rd = fx.reader("vqa_plain")
    return {k: pickle.loads(rd.env.get(k.encode())) for k in fx.image_keys}


def test_text_layout_of_the_fixture_records_agrees_with_b64_rows(fx):
    from volta_amd import ops
    from volta_amd.datasets import _b64_nsig, _b64_rows, _text_layout
    recs = _records(fx)
    texts = []
    for r in recs.values():
        texts += [r["features"], r["boxes"]]
    fields, total = _text_layout(texts)
    assert len(fields) == 2 * len(recs) and total % 16 == 0
    end = 0
    jobs = []
    for (t, nsig, at), row_bytes in zip(fields, [4 * F, 16] * len(recs)):
        assert at % 16 == 0 and at >= end and nsig == len(t.rstrip("=")) == _b64_nsig(t.encode())
        assert nsig * 3 // 4 == _b64_rows(t, row_bytes) * row_bytes
        end = at + nsig
        jobs.append((at, 0, nsig, nsig * 3 // 4))
    assert end <= total
    tab, mx = ops.b64_jobs(jobs)                               # the Python-side length check accepts every field of the fixture
    assert tab.shape == (len(jobs), 6) and mx == max(j[2] for j in jobs)
    for r in recs.values():
        assert _b64_rows(r["features"], 4 * F) == _b64_rows(r["boxes"], 16) == r["num_boxes"]


@pytest.mark.parametrize("as_bytes", [False, True])
def test_texts_pack_copies_the_fields_without_padding_to_aligned_offsets(fx, as_bytes):
    from volta_amd import _lib as L
    from volta_amd.datasets import _text_address, _text_layout
    texts = []
    for r in _records(fx).values():
        texts += [r["features"], r["boxes"]]
    texts += ["QUJD", "QUI=", "QQ==", ""]
    if as_bytes:
        texts = [t.encode() for t in texts]
    fields, total = _text_layout(texts)
    arena = np.full(total + 32, 0x7E, np.uint8)
    jobs, alive = (L.TaskText * len(fields))(), []
    for j, (t, nsig, at) in enumerate(fields):
        p, keep = _text_address(t)
        alive.append(keep)
        jobs[j] = L.TaskText(p, nsig, at)
    L.check(L.lib.vk_task_texts_pack(jobs, len(fields), C.c_void_p(arena.ctypes.data), total, 3))
    covered = np.zeros(arena.size, bool)
    for t, nsig, at in fields:
        raw = t if as_bytes else t.encode()
        assert arena[at:at + nsig].tobytes() == raw.rstrip(b"=") and at % 16 == 0
        covered[at:at + nsig] = True
    assert (arena[~covered] == 0x7E).all()
    assert [f[1] for f in fields[-4:]] == [4, 3, 2, 0]
    if not as_bytes:                                           # an ASCII str is read in place: its own buffer, no encode copy
        assert alive[0] is texts[0]
    bad = (L.TaskText * 1)(L.TaskText(jobs[0].src, 64, 8))
    assert L.lib.vk_task_texts_pack(bad, 1, C.c_void_p(arena.ctypes.data), total, 1) != 0 and b"misaligned" in L.lib.vk_last_error()
    bad = (L.TaskText * 1)(L.TaskText(jobs[0].src, 64, total - 16))
    assert L.lib.vk_task_texts_pack(bad, 1, C.c_void_p(arena.ctypes.data), total, 1) != 0


def test_a_non_ascii_str_takes_the_encode_of_the_host_path():
    from volta_amd.datasets import _text_address
    with pytest.raises(UnicodeEncodeError):
        _text_address("QUJDé")


def test_struct_mirrors_match_the_header():
    from volta_amd import _lib as L
    pairs = {"vk_task_pool_args": L.TaskPoolArgs, "vk_b64_job": L.B64Job, "vk_task_text": L.TaskText, "vk_task_batch_args": L.TaskBatchArgs}
    src = '#include <stdio.h>\n#include "volta_hip.h"\nint main(void){' + "".join('printf("%s %%zu\\n", sizeof(%s));' % (n, n) for n in pairs) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = subprocess.check_output([exe]).decode().split()
    for name, size in zip(out[0::2], map(int, out[1::2])):
        assert C.sizeof(pairs[name]) == size, (name, C.sizeof(pairs[name]), size)


def test_argument_errors(fx):
    from volta_amd.datasets import TaskLoader
    ds = fx.dataset("vqa_plain")
    with pytest.raises(ValueError, match="in_memory"):
        TaskLoader(ds, 2, in_memory=True, resident_bytes=1 << 20)
    with pytest.raises(ValueError, match="resident_bytes"):
        TaskLoader(ds, 2, resident_bytes=-1)
    ld = TaskLoader(ds, 2, resident_bytes=1 << 20)
    assert ld.resident_bytes_used == 0 and ld.resident_images == 0
    assert ld.stats == dict(decoded_images=0, resident_hits=0, scratch_images=0, host_fallback_batches=0)
    off = TaskLoader(ds, 2)
    assert off._resident is None and off.resident_bytes_used == 0 and off.resident_images == 0


def test_load_dataset_passes_resident_bytes_through(fx):
    import types
    from volta_amd import task_utils as TU
    config = types.SimpleNamespace(v_feature_size=F, num_locs=5, add_global_imgfeat="first", fusion_method="mul")
    task_cfg = {"TASK1": dict(name="VQA", dataroot=fx.dataroot("VQA"), features_h5path1=fx.store, features_h5path2="", train_annotations_jsonpath="",
                              val_annotations_jsonpath="", train_split="train", val_split="val", max_seq_length=12, max_region_num=16, batch_size=4,
                              type="VL-classifier", process="normal")}
    base = dict(bert_model=fx.vocab_file, do_lower_case=True, in_memory=False, grad_acc_steps=1, local_rank=-1, num_workers=2, drop_last=False,
                batch_size=3, split="", seed=0)
    _, _, _, _, ltr, lva = TU.LoadDataset(types.SimpleNamespace(**base, resident_bytes=1 << 20), config, task_cfg, "1")
    assert ltr.resident_bytes == lva.resident_bytes == 1 << 20 and ltr._resident is not lva._resident
    assert TU.LoadDatasetEval(types.SimpleNamespace(**base, resident_bytes=1 << 21), config, task_cfg, "1")[3].resident_bytes == 1 << 21
    _, _, _, _, ltr, lva = TU.LoadDataset(types.SimpleNamespace(**base), config, task_cfg, "1")            # no such argument: today's loaders
    assert ltr.resident_bytes == 0 and ltr._resident is None and lva._resident is None
    with pytest.raises(ValueError):
        TU.LoadDataset(types.SimpleNamespace(**dict(base, in_memory=True), resident_bytes=1 << 20), config, task_cfg, "1")
