"""`vk_task_batch` (csrc/taskbatch.hip) against its numpy restatement (tests/taskbatch_restate.py, which the CPU tests tie to the reference
fixture), `TaskLoader` against `torch.stack` of the host `__getitem__` results, and fine-tuning steps fed by the loader against the same steps
fed by the fixture's collated tensors.  Equal bits everywhere: the kernel rounds every fp32 operation on its own and adds the rows of the global
feature in the reference's order.  GPU only."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import taskbatch_restate as RS  # noqa: E402
from tests.task_data_fixture import Fixture  # noqa: E402

# |fp32 global row - float64 mean|: the bound of tests/test_task_datasets_cpu.py (2 x the larger of the observed errors, 4.768e-08 both) holds
# for the fixture's features; for the random features below the kernel's row must equal the restatement's bit for bit (same order of additions).


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    return Fixture(tmp_path_factory.mktemp("task_data"))


def _random_case(rng, S, Rcap, F, N, R, B):
    feat = rng.standard_normal((S, Rcap, F)).astype(np.float32)
    n = rng.integers(1, Rcap + 1, S).astype(np.int32)
    n[0] = Rcap
    wh = np.stack([rng.integers(100, 900, S), rng.integers(80, 700, S)], 1).astype(np.int32)
    xy = rng.uniform(0, 0.6, (S, Rcap, 2)) * wh[:, None, :]
    ext = rng.uniform(0.05, 0.4, (S, Rcap, 2)) * wh[:, None, :]
    boxes = np.concatenate([xy, xy + ext], 2).astype(np.float32)
    segs = np.zeros((N, 2, 4), np.int32)
    for o in range(N):
        kind = o % 6
        a, b = int(rng.integers(0, S)), int(rng.integers(0, S))
        if kind == 0:                                   # one image, block longer or shorter than it
            segs[o, 0] = (a, 0, 0, R)
        elif kind == 1:                                 # two images back to back (NLVR2), cut at the block length
            segs[o, 0] = (a, 0, 0, R)
            segs[o, 1] = (b, 0, int(n[a]) + 1, max(R - int(n[a]) - 1, 0))
        elif kind == 2:                                 # the second image over the head of the first (retrieval option 3)
            segs[o, 0] = (a, 0, 0, R)
            segs[o, 1] = (b, 0, 0, R)
        elif kind == 3:                                 # an empty block
            pass
        elif kind == 4:                                 # count == 0 in front of a window into the image
            segs[o, 0] = (a, 0, 0, 0)
            segs[o, 1] = (b, int(rng.integers(0, 4)), int(rng.integers(0, R)), int(rng.integers(1, R + 1)))
        else:                                           # values the kernel must skip, not follow
            segs[o, 0] = (S + 3, 0, 0, R)
            segs[o, 1] = (b, int(n[b]) + 5, 2, R)
    counts = rng.integers(0, R + 1, N).astype(np.int32)
    nnz = rng.integers(0, 5, B)
    csr = np.concatenate([[0], np.cumsum(nnz)]).astype(np.int32)
    labels = np.concatenate([rng.choice(31, k, replace=False) for k in nnz] + [np.zeros(0, np.int64)]).astype(np.int32)
    scores = rng.choice([0.3, 0.6, 0.9, 1.0], int(csr[-1])).astype(np.float32)
    ref_box = np.concatenate([xy[:N % S + 1, 0].repeat(N, 0)[:N], (xy + ext)[:N % S + 1, 0].repeat(N, 0)[:N]], 1).astype(np.float32)
    return feat, boxes, n, wh, segs, counts, (csr, labels, scores, 31), ref_box


@pytest.mark.parametrize("target", ["scatter", "iou"])
@pytest.mark.parametrize("add_global", [None, "first", "last"])
@pytest.mark.parametrize("F,R,num_locs", [(64, 37, 5), (64, 101, 4), (64, 202, 5), (2048, 37, 4), (2048, 101, 5), (2048, 202, 5)])
def test_kernel_equals_the_restatement(F, R, num_locs, add_global, target):
    from volta_amd import ops
    rng = np.random.default_rng(F + R + num_locs)
    S, Rcap, N, B = 5, 45 if F == 2048 else 120, 13, 13
    feat, boxes, n, wh, segs, counts, scatter, ref_box = _random_case(rng, S, Rcap, F, N, R, B)
    kw = dict(scatter=scatter) if target == "scatter" else dict(ref_box=ref_box)
    want = RS.task_batch(feat, boxes, n, wh, segs, counts, R, num_locs, add_global, **kw)
    dev = lambda a: torch.from_numpy(a).cuda()
    pre = dict(features=torch.full((N, R, F), float("nan"), device="cuda"), spatials=torch.full((N, R, num_locs), float("nan"), device="cuda"),
               image_mask=torch.full((N, R), -7, dtype=torch.int64, device="cuda"),
               target=torch.full((B, 31) if target == "scatter" else (N, R, 1), float("nan"), device="cuda"))   # every element must be written
    gkw = dict(scatter=(dev(scatter[0]), dev(scatter[1]), dev(scatter[2]), 31)) if target == "scatter" else dict(ref_box=dev(ref_box))
    got = ops.task_batch(dev(feat), dev(boxes), dev(n), dev(wh), dev(segs), dev(counts), R, num_locs, add_global, out=pre, **gkw)
    torch.cuda.synchronize()
    for name in ("features", "spatials", "image_mask", "target"):
        g = got[name].cpu().numpy()
        assert g.shape == want[name].shape and g.dtype == want[name].dtype, name
        assert not np.isnan(g.astype(np.float64)).any(), name
        assert np.array_equal(g, want[name]), (name, int((g != want[name]).sum()))


def test_kernel_refuses_bad_arguments():
    from volta_amd import _lib as L
    a = L.TaskBatchArgs()
    a.S, a.Rcap, a.F, a.N, a.R, a.num_locs = 1, 4, 6, 1, 4, 5
    assert L.lib.vk_task_batch(a, None) != 0 and b"multiple of 4" in L.lib.vk_last_error()
    a.F, a.num_locs = 8, 3
    assert L.lib.vk_task_batch(a, None) != 0 and b"num_locs" in L.lib.vk_last_error()


CASES = ["vqa_plain", "vqa_first_cut_sep", "vqa_last_cut", "vqa_test", "gqa_last", "gqa_cut", "gqa_test", "nlvr_plain", "nlvr_first_over", "nlvr_last_over",
         "refer_plain", "refer_first_cut", "refer_last_cut_g", "refer_testA", "retr_flickr_train", "retr_coco_val"]


@pytest.mark.parametrize("in_memory", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_loader_equals_the_stacked_host_samples(fx, case, in_memory):
    """batch by batch, the last short batch included, two epochs (the second comes from the pool when in_memory)"""
    from volta_amd.datasets import TaskLoader
    ds = fx.dataset(case)
    host = [ds[i] for i in range(len(ds))]
    ld = TaskLoader(ds, 4 if len(ds) > 4 else 3, in_memory=in_memory, prefetch=1)
    for epoch in range(2):
        at = 0
        for batch in ld:
            b = batch[0].shape[0]
            assert len(batch) == 8 and all(t.is_cuda for t in batch)
            for j in range(8):
                want = torch.stack([host[i][j] for i in range(at, at + b)]) if torch.is_tensor(host[at][j]) else torch.tensor([host[i][j] for i in range(at, at + b)])
                assert batch[j].dtype == want.dtype and batch[j].shape == want.shape, (j, batch[j].dtype, want.dtype, batch[j].shape, want.shape)
                assert torch.equal(batch[j].cpu(), want), (epoch, at, j)
            at += b
        assert at == len(ds)
    assert (ld.pool_bytes_used > 0) == in_memory


def test_three_training_steps_fed_by_the_loader_equal_those_fed_by_the_fixture(fx):
    """A tiny ViLBERT VQA model (the one of tests/test_task_loss_gpu.py with 2048-wide image features), three ForwardModelsTrain + backward
    + AdamW steps: the losses with TaskLoader batches equal, bit for bit, the losses with the reference's recorded samples collated and moved
    to the GPU (same inputs, same engine)."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_engine_gpu import CONFIGS
    from oracle import volta_ref as R
    from volta_amd import task_utils as TU
    from volta_amd.config import BertConfig
    from volta_amd.datasets import TaskLoader
    from volta_amd.modeling import BertForVLTasks
    from volta_amd.optimization import AdamW
    case = "vqa_last_cut"
    ds = fx.dataset(case)
    cd = dict(CONFIGS["vilbert"], clf_hidden_size=1536, v_feature_size=2048, add_global_imgfeat="last")
    task_cfg = {"TASK1": dict(type="VL-classifier", num_labels=ds.num_labels, process="normal", loss="BCEWithLogitLoss")}
    rcfg = R.RefConfig(cd)
    sd = R.make_task_weights(rcfg, task_cfg, ["TASK1"], seed=4, std=0.04)
    crit = TU.LoadLoss(task_cfg, "1")
    dev = torch.device("cuda")

    def run(batches):
        cfg = BertConfig.from_dict(cd)
        model = BertForVLTasks(cfg, task_cfg, ["TASK1"])
        model.load_state_dict(sd, strict=True)
        model.cuda().eval()
        opt = AdamW(model.parameters(), lr=1e-3)
        losses = []
        for batch in batches:
            loss, score = TU.ForwardModelsTrain(cfg, task_cfg, dev, "TASK1", batch, model, crit)
            loss.backward()
            opt.step()
            opt.zero_grad()
            losses.append((float(loss.detach()), float(score)))
        return losses

    fixture_batches = []
    for at in range(0, 6, 2):
        rows = [fx.sample(case, i)[0] for i in range(at, at + 2)]
        fixture_batches.append(tuple(torch.from_numpy(np.stack([r[j] for r in rows])) for j in range(8)))
    want = run(fixture_batches)
    got = run(TaskLoader(ds, 2))
    print("losses:", want, got)
    assert len(got) == 3 and got == want and len(set(w[0] for w in want)) == 3
