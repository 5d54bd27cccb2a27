"""BertForVLTasks.task_loss behind volta_amd.task_utils against the unfused path (model(...) + the reference's torch arithmetic) on
the same model and batch: the tiny configurations and task table of tests/test_tasks_gpu.py, evaluation mode (no dropout), batches
laid out as the datasets lay them out, padded captions and regions.

Bounds.  Loss: the two paths read the same logits, so the kernel-level bound holds: |fused - float64| <= max(4 x |torch - float64|,
16 fp32 ulp).  Score: exact (at most two samples of a batch score, so the fp32 sum has one rounding whatever the order).  Gradients,
per parameter: rel(G_fused, G_ref) <= max(2 x rel(G_torch, G_ref), 2^-8), G_ref = the unfused backward fed the float64 loss gradient,
G_torch = today's path (torch criterion + autograd): the fused path may be no further from the exact loss gradient than twice what the
present path is, with a floor of one bf16 ulp on the seed.  Measured on an MI355X: fused loss 0.01 - 0.43 ulp from float64 (torch path 0.01 - 0.82); worst rel(G_fused, G_ref) / bound below 0.001
(DESIGN.md section 4).  GPU only."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

PROCESS = {"TASK1": "normal", "TASK9": "normal", "TASK12": "nlvr", "TASK13": "normal", "TASK8": "retrieval"}
LOSS = {"TASK1": "BCEWithLogitLoss", "TASK9": "BCEWithLogitLoss", "TASK12": "BCEWithLogitLoss", "TASK13": "BCEWithLogitLoss", "TASK8": "CrossEntropyLoss"}
T, RN = 20, 36


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def build(tasks, mc_regions=None):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_engine_gpu import CONFIGS
    from test_tasks_gpu import TASK_CFG
    from oracle import volta_ref as R
    from volta_amd.config import BertConfig
    from volta_amd.modeling import BertForVLTasks
    cd = dict(CONFIGS["vilbert"], clf_hidden_size=1536)
    rcfg = R.RefConfig(cd)
    task_cfg = {t: dict(TASK_CFG[t], process=PROCESS[t], loss=LOSS[t]) for t in tasks}
    if mc_regions:
        task_cfg["TASK9"]["type"] = "V-logit-mc"
    sd = R.make_task_weights(rcfg, task_cfg, list(tasks), seed=4, std=0.04)
    cfg = BertConfig.from_dict(cd)
    model = BertForVLTasks(cfg, task_cfg, list(tasks))
    model.load_state_dict(sd, strict=True)
    return model.cuda().eval(), cfg, rcfg, task_cfg


def driver_batch(model, rcfg, task_cfg, task, B, seed, regions=RN):
    """The 8-tuple of the task's dataset (features, spatials, image_mask, question, target, input_mask, segment_ids, question_id), on the
    CPU as a DataLoader hands it over; the targets put a score on the predicted label of at most two samples."""
    from oracle import volta_ref as R
    from volta_amd import task_utils as TU
    typ, process = task_cfg[task]["type"], task_cfg[task]["process"]
    mult = {"nlvr": 2, "retrieval": 4}.get(process, 1)
    sb = R.synthetic_batch(rcfg, B * mult, T, regions, seed=seed, pad=True)
    feats, locs, im = sb["image_feat"], sb["image_loc"], sb["image_mask"]
    q, am, seg = sb["input_ids"], sb["input_mask"], sb["segment_ids"]
    Rv = feats.shape[1]
    if process == "nlvr":                                         # one caption, two images side by side
        feats, locs, im = feats.view(B, 2 * Rv, -1), locs.view(B, 2 * Rv, -1), im.view(B, 2 * Rv)
        q, am, seg = q[:B], am[:B], seg[:B]
    elif process == "retrieval":
        feats, locs, im = feats.view(B, 4, Rv, -1), locs.view(B, 4, Rv, -1), im.view(B, 4, Rv)
        q, am, seg = q.view(B, 4, T), am.view(B, 4, T), seg.view(B, 4, T)
    qid = torch.arange(B) + 7
    g = torch.Generator().manual_seed(seed + 1)
    dummy = {"VL-logit": torch.zeros(B, dtype=torch.int64), "V-logit": torch.zeros(B, Rv, 1)}.get(typ, torch.zeros(B, 1))
    probe = TU._Batch(model.config, task_cfg, torch.device("cuda"), task, (feats, locs, im, q, dummy, am, seg, qid))
    with torch.no_grad():
        pred = model(*probe.model_args(task))[0].float().cpu()
    if typ == "VL-logit":
        top = pred.view(B, 4).argmax(1)
        target = (top + 1) % 4
        target[:2] = top[:2]
    elif typ == "V-logit":
        top = pred.squeeze(2).argmax(1)
        target = torch.rand(B, Rv, 1, generator=g) * 0.45         # IoU below the 0.5 mark ...
        target[0, top[0], 0], target[1, top[1], 0] = 0.8, 0.55    # ... except at two predicted regions
    else:
        C = pred.shape[1]
        top = pred.argmax(1)
        target = torch.zeros(B, C)
        for r in range(B):
            for c in torch.randperm(C, generator=g)[:3].tolist():
                if c != int(top[r]) and (C > 3 or r > 1):
                    target[r, c] = [0.3, 0.6, 0.9, 1.0][int(torch.randint(0, 4, (1,), generator=g))]
        target[0, top[0]], target[1, top[1]] = 0.9, 0.3
        if typ in ("VL-binary-classifier", "VL-tri-classifier"):  # one-hot labels
            target = torch.zeros(B, C)
            target[torch.arange(B), (top + 1) % C] = 1.0
            target[0], target[1] = 0.0, 0.0
            target[0, top[0]], target[1, top[1]] = 1.0, 1.0
    return (feats, locs, im, q, target, am, seg, qid)


def loss64(typ, pred, target, batch_size, num_options):
    """the task's loss in float64 from the fp32 logits, and its gradient with respect to them"""
    t = target.cuda()
    with torch.enable_grad():
        p = pred.detach().double().requires_grad_(True)
        if typ == "VL-logit":
            loss = nn.CrossEntropyLoss()(p.view(batch_size, num_options), t)
        else:
            loss = nn.BCEWithLogitsLoss()(p, t.double())
            if typ in ("VL-classifier", "VL-classifier-GQA", "V-logit"):
                loss = loss * t.size(1)
        (grad,) = torch.autograd.grad(loss, p)
    return float(loss.detach()), grad


def grads(model):
    out = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}
    for p in model.parameters():
        p.grad = None
    return out


@pytest.mark.parametrize("B", [4, 6])
@pytest.mark.parametrize("task", ["TASK1", "TASK12", "TASK13", "TASK9", "TASK8"])
def test_fused_step_matches_the_unfused_path(task, B, monkeypatch):
    from volta_amd import task_utils as TU
    model, cfg, rcfg, task_cfg = build([task])
    typ = task_cfg[task]["type"]
    batch = driver_batch(model, rcfg, task_cfg, task, B, seed=11 + B)
    crit = TU.LoadLoss({"TASK" + task[4:]: task_cfg[task]}, task[4:])
    dev = torch.device("cuda")
    monkeypatch.delenv("VOLTA_TASK_LOSS", raising=False)
    assert TU.fused_kind(model, crit, typ) is not None
    loss_f, score_f = TU.ForwardModelsTrain(cfg, task_cfg, dev, task, batch, model, crit)
    assert loss_f.dim() == 0 and loss_f.dtype == torch.float32 and loss_f.is_cuda and score_f.dim() == 0 and score_f.is_cuda
    loss_f.backward()
    G_fused = grads(model)
    monkeypatch.setenv("VOLTA_TASK_LOSS", "torch")
    loss_t, score_t = TU.ForwardModelsTrain(cfg, task_cfg, dev, task, batch, model, crit)
    loss_t.backward()
    G_torch = grads(model)
    b = TU._Batch(cfg, task_cfg, dev, task, batch)
    pred = model(*b.model_args(task))[0]
    want, g64 = loss64(typ, pred, batch[4], b.batch_size, b.num_options)
    pred.backward(gradient=g64.to(torch.float32).view_as(pred))
    G_ref = grads(model)
    # loss and score
    err_f, err_t = abs(float(loss_f.double()) - want), abs(float(loss_t.double()) - want)
    ulp = float(np.spacing(np.float32(abs(want))))
    print("%s B=%d loss %.9g: fused error %.3g (%.2f ulp), torch error %.3g (%.2f ulp); score %.6g" % (task, B, want, err_f, err_f / ulp, err_t, err_t / ulp, float(score_f)))
    assert err_f <= max(4 * err_t, 16 * ulp), (task, B, float(loss_f), float(loss_t), want)
    # the fused batch score is an fp32 device tensor; for the count-type tasks the unfused path returns a Python double: compare as fp32
    assert np.float32(float(score_f)) == np.float32(float(score_t)) and float(score_f) > 0, (task, B, float(score_f), float(score_t))
    # gradients
    worst, checked = 0.0, 0
    for n, gr in G_ref.items():
        if gr is None or float(gr.norm()) < 1e-12:
            assert G_fused[n] is None or float(G_fused[n].norm()) <= 1e-6, n
            continue
        assert G_fused[n] is not None and G_torch[n] is not None, n
        e_f, e_t = rel(G_fused[n], gr), rel(G_torch[n], gr)
        bound = max(2 * e_t, 2.0 ** -8)
        worst = max(worst, e_f / bound)
        assert e_f <= bound, (task, B, n, e_f, e_t)
        checked += 1
    assert checked > 20
    print("%s B=%d gradients: worst rel(G_fused, G_ref) / bound = %.3f over %d parameters" % (task, B, worst, checked))


def test_accumulation_frozen_layer_and_training_steps(monkeypatch):
    from oracle import volta_ref as R
    from volta_amd import task_utils as TU
    from volta_amd.optimization import AdamW, clip_grad_norm_
    monkeypatch.delenv("VOLTA_TASK_LOSS", raising=False)
    model, cfg, rcfg, task_cfg = build(["TASK1"])
    frozen = [n for n, p in model.named_parameters() if n.startswith("bert.encoder.layer.0.")]
    assert frozen
    for n, p in model.named_parameters():
        if n in frozen:
            p.requires_grad_(False)
    batch = driver_batch(model, rcfg, task_cfg, "TASK1", 4, seed=3)
    crit, dev = TU.LossMap["BCEWithLogitLoss"], torch.device("cuda")
    loss, _ = TU.ForwardModelsTrain(cfg, task_cfg, dev, "TASK1", batch, model, crit)
    loss.backward()
    full = grads(model)
    assert all(full[n] is None for n in frozen), "a frozen layer gets no .grad"
    for _ in range(2):      # two micro-batches of loss / 4: the seed is scaled by a power of two, so its bf16 rounding is the full seed's
        loss, _ = TU.ForwardModelsTrain(cfg, task_cfg, dev, "TASK1", batch, model, crit)
        (loss / 4).backward()
    acc = grads(model)
    worst = 0.0
    for n, g in full.items():
        if g is None or float(g.norm()) < 1e-12:
            continue
        worst = max(worst, rel(acc[n] * 2, g))
    print("accumulated 2 x (loss / 4) against loss / 2: worst relative difference %.3g" % worst)
    assert worst <= 2.0 ** -8, worst
    # three fine-tuning steps in training mode
    model.train()
    model.set_dropout_seed(5)
    opt = AdamW(model.parameters(), lr=1e-3)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    losses = []
    for _ in range(3):
        loss, score = TU.ForwardModelsTrain(cfg, task_cfg, dev, "TASK1", batch, model, crit)
        loss.backward()
        clip_grad_norm_(model.parameters(), 5.0)
        opt.step()
        opt.zero_grad()
        losses.append(float(loss.detach()))
        float(score)
    assert losses[-1] < losses[0], losses
    after = model.state_dict()
    assert not torch.equal(after["clfs_dict.TASK1.logit_fc.3.weight"], before["clfs_dict.TASK1.logit_fc.3.weight"])
    assert all(torch.equal(after[n], before[n]) for n in frozen)


class HostReads:
    """Counts the Python-level device-to-host reads of CUDA tensors."""

    def __init__(self, monkeypatch):
        self.calls = []
        for name in ("tolist", "item", "cpu", "numpy", "__float__", "__int__", "__bool__"):
            orig = getattr(torch.Tensor, name)

            def spy(t, *a, _orig=orig, _name=name, **k):
                if t.is_cuda:
                    self.calls.append(_name)
                return _orig(t, *a, **k)
            monkeypatch.setattr(torch.Tensor, name, spy)


@pytest.mark.parametrize("task", ["TASK1", "TASK9", "TASK8"])
def test_validation_step_reads_the_host_once(task, monkeypatch):
    from volta_amd import task_utils as TU
    model, cfg, rcfg, task_cfg = build([task])
    batch = driver_batch(model, rcfg, task_cfg, task, 6, seed=23)
    crit, dev = TU.LossMap[LOSS[task]], torch.device("cuda")
    monkeypatch.setenv("VOLTA_TASK_LOSS", "torch")
    with torch.no_grad():
        loss_t, score_t, n_t = TU.ForwardModelsVal(cfg, task_cfg, dev, task, batch, model, crit)
    monkeypatch.delenv("VOLTA_TASK_LOSS")
    b = TU._Batch(cfg, task_cfg, dev, task, batch)
    with torch.no_grad():
        want, _ = loss64(task_cfg[task]["type"], model(*b.model_args(task))[0], batch[4], b.batch_size, b.num_options)
        TU.ForwardModelsVal(cfg, task_cfg, dev, task, batch, model, crit)        # plans built, buffers allocated
        reads = HostReads(monkeypatch)
        loss_f, score_f, n_f = TU.ForwardModelsVal(cfg, task_cfg, dev, task, batch, model, crit)
    assert reads.calls == ["tolist"], reads.calls
    assert isinstance(loss_f, float) and isinstance(score_f, float) and n_f == n_t == 6
    ulp = float(np.spacing(np.float32(abs(want))))
    assert abs(loss_f - want) <= max(4 * abs(loss_t - want), 16 * ulp), (loss_f, loss_t, want)
    assert score_f == score_t and score_f > 0


def test_what_the_kernels_do_not_cover_takes_the_torch_path(monkeypatch):
    from volta_amd import task_utils as TU
    monkeypatch.delenv("VOLTA_TASK_LOSS", raising=False)
    dev = torch.device("cuda")
    # a criterion with pos_weight
    model, cfg, rcfg, task_cfg = build(["TASK1"])
    batch = driver_batch(model, rcfg, task_cfg, "TASK1", 4, seed=5)
    crit = nn.BCEWithLogitsLoss(pos_weight=torch.full((3129,), 2.0, device="cuda"))
    assert TU.fused_kind(model, crit, "VL-classifier") is None
    loss, score = TU.ForwardModelsTrain(cfg, task_cfg, dev, "TASK1", batch, model, crit)
    b = TU._Batch(cfg, task_cfg, dev, "TASK1", batch)
    pred = model(*b.model_args("TASK1"))[0]
    want = crit(pred, b.target).mean() * 3129
    assert float(loss.detach()) == float(want.detach())
    assert float(score) == float(TU.compute_score_with_logits(pred, b.target).sum() / 4.0)
    loss.backward()
    assert model.clfs_dict["TASK1"].logit_fc[3].weight.grad is not None
    # V-logit-mc: the region scores behind the first 101, gathered at the four candidate boxes
    model, cfg, rcfg, task_cfg = build(["TASK9"], mc_regions=True)
    B, regions = 4, 107
    feats, locs, im, q, _, am, seg, qid = driver_batch(model, rcfg, dict(task_cfg, TASK9=dict(task_cfg["TASK9"], type="V-logit")), "TASK9", B, seed=9, regions=regions)
    Rv = feats.shape[1]
    g = torch.Generator().manual_seed(1)
    ids = torch.stack([torch.randperm(Rv - 101, generator=g)[:4] for _ in range(B)])
    target = torch.zeros(B, 4, 1)
    target[torch.arange(B), torch.randint(0, 4, (B,), generator=g), 0] = 1.0
    batch = (feats, locs, im, q, target, am, seg, ids, qid)
    crit = TU.LossMap["BCEWithLogitLoss"]
    assert TU.fused_kind(model, crit, "V-logit-mc") is None
    with torch.no_grad():
        loss, score, n = TU.ForwardModelsVal(cfg, task_cfg, dev, "TASK9", batch, model, crit)
        pred = model(q.cuda(), feats.cuda(), locs.cuda(), "TASK9", seg.cuda(), am.cuda(), im.cuda())[0]
    logit = pred[:, 101:].squeeze(2).gather(1, ids.cuda()).unsqueeze(2)
    want = crit(logit, target.cuda()).mean() * 4
    hits = (torch.max(logit, dim=1)[1] == torch.max(target.cuda(), dim=1)[1]).sum()
    assert loss == float(want) and score == float(hits) and n == B


def test_evaluating_model_uses_the_row_argmax(monkeypatch):
    import types
    from volta_amd import task_utils as TU
    monkeypatch.delenv("VOLTA_TASK_LOSS", raising=False)
    model, cfg, rcfg, task_cfg = build(["TASK1"])
    batch = driver_batch(model, rcfg, task_cfg, "TASK1", 4, seed=5)
    loader = types.SimpleNamespace(dataset=types.SimpleNamespace(label2ans=["a%d" % i for i in range(3129)]))
    crit, dev = TU.LossMap["BCEWithLogitLoss"], torch.device("cuda")
    out = TU.EvaluatingModel(cfg, task_cfg, dev, "TASK1", batch, model, loader, crit, [], [])
    monkeypatch.setenv("VOLTA_TASK_LOSS", "torch")
    ref = TU.EvaluatingModel(cfg, task_cfg, dev, "TASK1", batch, model, loader, crit, [], [])
    assert out == ref and len(out[3]) == 4 and out[3][0]["question_id"] == 7 and out[:3] == (0.0, 0.0, 4)
