"""Retrieval evaluation on the GPU: the resident arrays of `RetrievalDatasetVal.device_arrays` against the reference's recorded
`features_all` / `spatials_all` / `image_mask_all` (bit for bit, the chunked path included), the driver's batch-of-one loader, and
`evaluate_retrieval` against the driver's loop (eval_retrieval.py:168-263: the whole model per caption and image block over that loader,
scores copied to the host, ranks by tests/ranks_restate.py) in all ten metrics, both rank vectors and the top-k lists.  Integer outputs are
compared for equality.  GPU only."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tests.retrieval_eval_fixture import CASES, F, EvalFixture  # noqa: E402
from tests import ranks_restate as RR  # noqa: E402

TASK_CFG = {"TASK8": {"type": "VL-logit"}}


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    return EvalFixture(tmp_path_factory.mktemp("retrieval_eval_gpu"))


def _tiny(zero_shot, seed=4):
    """the reduced-depth ViLBERT of tests/test_retrieval_gpu.py with the feature width of the fixture's store"""
    from test_engine_gpu import CONFIGS
    from oracle import volta_ref as R
    from volta_amd.config import BertConfig
    from volta_amd.modeling import BertForVLPreTraining, BertForVLTasks
    cd = dict(CONFIGS["vilbert"], clf_hidden_size=1536, v_feature_size=F)
    rcfg = R.RefConfig(cd)
    if zero_shot:
        model = BertForVLPreTraining(BertConfig.from_dict(cd))
        model.load_state_dict(R.make_weights(rcfg, seed=seed, std=0.04), strict=True)
    else:
        model = BertForVLTasks(BertConfig.from_dict(cd), TASK_CFG, list(TASK_CFG))
        model.load_state_dict(R.make_task_weights(rcfg, TASK_CFG, list(TASK_CFG), seed=seed, std=0.04), strict=True)
    return model.cuda().eval()


@pytest.mark.parametrize("chunk", [256, 3])
@pytest.mark.parametrize("case", CASES)
def test_device_arrays_equal_the_reference(fx, case, chunk):
    """chunk 3: the six images arrive in two staging chunks"""
    ds = fx.dataset(case, chunk_images=chunk)
    assert ds.chunk_images == chunk
    arr = ds.device_arrays()
    assert ds.device_arrays("cuda") is arr                                        # resident: built once
    (feat, loc, mask), _ = fx.arrays(case)
    for name, want, dt in (("features", feat, torch.float32), ("spatials", loc, torch.float32), ("image_mask", mask, torch.int64)):
        got = arr[name]
        assert got.is_cuda and got.dtype == dt and tuple(got.shape) == want.shape, (name, got.dtype, tuple(got.shape), want.shape)
        assert np.array_equal(got.cpu().numpy(), want), (name, float(np.abs(got.cpu().numpy().astype(np.float64) - want).max()))
    host = ds.host_tables()
    for name, dt in (("input_ids", torch.int64), ("input_mask", torch.int64), ("segment_ids", torch.int64), ("caption_image", torch.int32), ("image_ids", torch.int64)):
        assert arr[name].is_cuda and arr[name].dtype == dt and np.array_equal(arr[name].cpu().numpy(), host[name]), name
    assert np.array_equal(host["caption_image"], fx.z["%s::caption_image" % case])


def test_loader_yields_the_drivers_batches_over_the_resident_arrays(fx):
    from volta_amd import datasets as D
    ds = fx.dataset("coco_last")
    dl = D.RetrievalEvalLoader(ds)
    arr = ds.device_arrays()
    Ni, R, T = 6, 16, 12
    n = 0
    for index, batch in enumerate(dl):
        assert len(batch) == 9 and all(t.is_cuda for t in batch)
        k = Ni if index % 2 == 0 else 0                                           # six images: all of them in [:500], none in [500:]
        assert [tuple(t.shape) for t in batch] == [(1, k, R, F), (1, k, R, 5), (1, k, R), (1, T), (1, T), (1, T), (1, 500), (1,), (1,)]
        assert [t.dtype for t in batch] == [torch.float32, torch.float32, torch.int64, torch.int64, torch.int64, torch.int64, torch.float32, torch.int64, torch.int64]
        for t, name in zip(batch[:3], ("features", "spatials", "image_mask")):
            assert t.untyped_storage().data_ptr() == arr[name].untyped_storage().data_ptr(), name
        want = [fx.z["coco_last::%d::%d" % (index, j)] for j in range(3, 9)]
        for t, w in zip(batch[3:], want):
            assert np.array_equal(t[0].cpu().numpy(), w), index
        n += 1
    assert n == len(dl) == len(ds) == 20


def _driver(model, dl, Nc, Ni, zero_shot):
    """eval_retrieval.py:164-198 over the loader, the whole model per batch -> the float64 score matrix on the host"""
    score_matrix = np.zeros((Nc, Ni))
    for batch in dl:
        features, spatials, image_mask, question, input_mask, segment_ids, target, caption_idx, image_idx = batch
        features, spatials, image_mask = features.squeeze(0), spatials.squeeze(0), image_mask.squeeze(0)
        n = features.size(0)
        if n == 0:                                                                # the empty [500:] half of a small set
            continue
        question, segment_ids, input_mask = question.repeat(n, 1), segment_ids.repeat(n, 1), input_mask.repeat(n, 1)
        lo = int(image_idx.item()) * 500
        with torch.no_grad():
            if zero_shot:
                vil_logit = model(question, features, spatials, segment_ids, input_mask, image_mask)[2]
                score_matrix[int(caption_idx.item()), lo:lo + n] = torch.softmax(vil_logit.float(), dim=1)[:, 0].view(-1).cpu().numpy()
            else:
                vil_logit = model(question, features, spatials, "TASK8", segment_ids, input_mask, image_mask)[0]
                score_matrix[int(caption_idx.item()), lo:lo + n] = vil_logit.float().view(-1).cpu().numpy()
    return score_matrix


@pytest.mark.parametrize("case", ["coco_last", "flickr_plain"])
@pytest.mark.parametrize("zero_shot", [False, True])
def test_evaluate_retrieval_equals_the_driver_loop(fx, zero_shot, case):
    from volta_amd import datasets as D
    from volta_amd.parallel import DistributedDataParallel
    from volta_amd.retrieval import evaluate_retrieval
    model = _tiny(zero_shot)
    ds = fx.dataset(case)
    Nc, Ni = len(ds) // 2, 6
    S = _driver(model, D.RetrievalEvalLoader(ds), Nc, Ni, zero_shot)
    ci = ds.host_tables()["caption_image"]
    want_ir, want_top, want_tr = RR.ranks(S.astype(np.float32), ci, 20)
    if case == "coco_last" and not zero_shot:                                     # wrapped as the driver wraps it: unwrapped here
        wrapped = DistributedDataParallel.__new__(DistributedDataParallel)
        torch.nn.Module.__init__(wrapped)
        wrapped.module = model
        res = evaluate_retrieval(wrapped, ds, task_id="TASK8", pair_chunk=7, topk=20)
    else:
        res = evaluate_retrieval(model, ds, task_id=None if zero_shot else "TASK8", pair_chunk=1000, topk=20)
    assert res.rank_ir.is_cuda and res.rank_tr.is_cuda and res.score_matrix.is_cuda and tuple(res.score_matrix.shape) == (Nc, Ni)
    assert np.array_equal(res.rank_ir.cpu().numpy(), want_ir) and np.array_equal(res.rank_tr.cpu().numpy(), want_tr)
    assert res.results == [[v for v in row if v >= 0] for row in want_top.tolist()] and all(len(r) == Ni for r in res.results)
    assert want_tr[5] == -1 and (want_tr[:5] >= 0).all()                          # the image without a caption is left out of text retrieval
    assert res.image_retrieval == RR.metrics(want_ir) and res.text_retrieval == RR.metrics(want_tr[want_tr >= 0])
    assert set(res.image_retrieval) == set(res.text_retrieval) == {"r1", "r5", "r10", "medr", "meanr"}


def test_evaluate_retrieval_refuses_what_the_scorer_refuses(fx):
    from volta_amd.retrieval import evaluate_retrieval
    model = _tiny(False)
    ds = fx.dataset("coco_last")
    with pytest.raises(ValueError, match="unknown task id"):
        evaluate_retrieval(model, ds, task_id="TASK9")
    with pytest.raises(ValueError, match="pair_chunk must be positive"):
        evaluate_retrieval(model, ds, task_id="TASK8", pair_chunk=0)
    with pytest.raises(ValueError, match="topk"):
        evaluate_retrieval(model, ds, task_id="TASK8", topk=65)
    with pytest.raises(ValueError, match="not from"):
        evaluate_retrieval(torch.nn.Linear(2, 2), ds)


def _train_step(model, arr):
    n = 4
    pred = model(arr["input_ids"][:n], arr["features"][:n], arr["spatials"][:n], "TASK8", arr["segment_ids"][:n], arr["input_mask"][:n], arr["image_mask"][:n])[0]
    loss = (pred.float() * torch.linspace(-1.0, 1.0, pred.numel(), device=pred.device).view_as(pred)).sum()
    return pred, loss


def test_model_state_is_left_alone(fx):
    """`training`, the dropout step counter and a following training step (prediction, loss, every gradient, every updated weight) are what
    they are without the evaluation in between"""
    from volta_amd.optimization import AdamW
    from volta_amd.retrieval import evaluate_retrieval
    a, b = _tiny(False), _tiny(False)
    ds = fx.dataset("coco_last")
    arr = ds.device_arrays()
    for m in (a, b):
        m.train()
        m.set_dropout_seed(77)
    opt_a, opt_b = AdamW(a.parameters(), lr=1e-3), AdamW(b.parameters(), lr=1e-3)
    for step in range(2):
        step_before = a._step
        res = evaluate_retrieval(a, ds, task_id="TASK8", pair_chunk=16)
        assert a.training and a._step == step_before == b._step and len(res.results) == 10
        pa, la = _train_step(a, arr)
        la.backward()
        pb, lb = _train_step(b, arr)
        lb.backward()
        assert torch.equal(pa, pb) and torch.equal(la, lb), step
        for (n, p), q in zip(a.named_parameters(), b.parameters()):
            assert (p.grad is None) == (q.grad is None), n
            assert p.grad is None or torch.equal(p.grad, q.grad), (step, n)
        opt_a.step()
        opt_b.step()
        opt_a.zero_grad()
        opt_b.zero_grad()
        for (n, p), q in zip(a.named_parameters(), b.parameters()):
            assert torch.equal(p, q), (step, n)
