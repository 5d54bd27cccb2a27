"""volta_amd.task_utils against values recorded from the reference's own ForwardModelsTrain / ForwardModelsVal
(tests/golden/task_loss_reference.npz, written by tools/make_task_loss_golden.py): the `process` reshapes, the torch arithmetic of
the fallback path, which (criterion, task type) pairs select the fused step, and the C ABI of the two new entry points.  No GPU needed."""
import ctypes
import os
import subprocess
import tempfile
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "task_loss_reference.npz"))
CASES = [str(c) for c in Z["cases"]]
RUNS = [(c, m) for c in CASES for m in ("train", "val") if "%s/%s/pred" % (c, m) in Z.files]


class StubModel:
    def __init__(self, pred):
        self.pred, self.seen = pred, None

    def __call__(self, question, features, spatials, task_id, segment_ids, input_mask, image_mask):
        self.seen = (question, features, spatials, segment_ids, input_mask, image_mask)
        return self.pred, None, None, None


def run(case, mode):
    from volta_amd import task_utils as TU
    typ, process, loss_name = (str(x) for x in Z["%s/meta" % case])
    F, LOCS = int(Z["dims"][0]), int(Z["dims"][1])
    config = types.SimpleNamespace(v_feature_size=F, num_locs=LOCS)
    task_cfg = {"TASK1": {"type": typ, "process": process, "loss": loss_name}}
    pre = "%s/%s/" % (case, mode)
    batch = tuple(torch.from_numpy(Z[pre + "b%d" % k]) for k in range(sum(1 for f in Z.files if f.startswith(pre + "b") and f[len(pre) + 1:].isdigit())))
    pred = torch.from_numpy(Z[pre + "pred"]).clone().requires_grad_(True)
    model = StubModel(pred)
    fn = TU.ForwardModelsTrain if mode == "train" else TU.ForwardModelsVal
    res = fn(config, task_cfg, torch.device("cpu"), "TASK1", batch, model, TU.LoadLoss(task_cfg, "1"))
    return pre, model, pred, res


def test_the_golden_file_covers_every_task_type_and_process():
    metas = {tuple(str(x) for x in Z["%s/meta" % c][:2]) for c in CASES}
    assert {m[0] for m in metas} == {"VL-classifier", "VL-classifier-GQA", "VL-binary-classifier", "VL-tri-classifier", "VL-logit", "V-logit", "V-logit-mc"}
    assert {m[1] for m in metas} == {"normal", "expand", "retrieval", "nlvr", "dialog"}
    assert ("dialog", "val") not in RUNS and len(RUNS) == 2 * len(CASES) - 1


@pytest.mark.parametrize("case,mode", RUNS)
def test_process_hands_the_model_the_recorded_tensors(case, mode):
    pre, model, _, _ = run(case, mode)
    for k, got in enumerate(model.seen):
        want = torch.from_numpy(Z[pre + "m%d" % k])
        assert got.dtype == want.dtype and torch.equal(got, want), (case, mode, k, tuple(got.shape), tuple(want.shape))


@pytest.mark.parametrize("case,mode", RUNS)
def test_fallback_arithmetic_returns_the_recorded_loss_and_score(case, mode):
    pre, _, pred, res = run(case, mode)
    want_loss, want_score = float(Z[pre + "loss"]), float(Z[pre + "score"])
    got_loss, got_score = float(res[0].detach() if torch.is_tensor(res[0]) else res[0]), float(res[1])
    assert abs(got_loss - want_loss) <= 1e-6 * abs(want_loss), (case, mode, got_loss, want_loss)
    assert abs(got_score - want_score) <= 1e-6 * abs(want_score), (case, mode, got_score, want_score)
    if mode == "train":
        res[0].backward()
        want = torch.from_numpy(Z[pre + "grad"])
        assert float((pred.grad - want).abs().max()) <= 1e-6 * float(want.abs().max()), (case, mode)
    else:
        assert isinstance(res[0], float) and isinstance(res[1], float) and res[2] == int(Z[pre + "batch_size"])


def test_dialog_is_refused_in_validation():
    from volta_amd import task_utils as TU
    pre = "dialog/train/"
    batch = tuple(torch.from_numpy(Z[pre + "b%d" % k]) for k in range(8))
    task_cfg = {"TASK1": {"type": "VL-logit", "process": "dialog", "loss": "CrossEntropyLoss"}}
    with pytest.raises(NotImplementedError):
        TU.ForwardModelsVal(types.SimpleNamespace(v_feature_size=8, num_locs=5), task_cfg, torch.device("cpu"), "TASK1", batch, StubModel(None), nn.CrossEntropyLoss())


def test_compute_score_with_logits_and_lossmap():
    from volta_amd import task_utils as TU
    logits = torch.tensor([[0.1, 2.0, -1.0], [3.0, 3.0, 0.0]])
    labels = torch.tensor([[0.3, 0.9, 0.0], [0.6, 1.0, 0.0]])
    assert torch.equal(TU.compute_score_with_logits(logits, labels), torch.tensor([[0.0, 0.9, 0.0], [0.6, 0.0, 0.0]]))
    assert type(TU.LossMap["BCEWithLogitLoss"]) is nn.BCEWithLogitsLoss and type(TU.LossMap["CrossEntropyLoss"]) is nn.CrossEntropyLoss
    assert TU.LoadLoss({"TASK7": {"loss": "CrossEntropyLoss"}}, "7") is TU.LossMap["CrossEntropyLoss"]


def test_dispatch_selects_the_fused_step_only_for_the_table(monkeypatch):
    from volta_amd import task_utils as TU
    from volta_amd.config import BertConfig
    from volta_amd.modeling import BertForVLTasks
    monkeypatch.delenv("VOLTA_TASK_LOSS", raising=False)
    cfg = BertConfig.from_dict(dict(vocab_size=50, hidden_size=64, num_attention_heads=1, intermediate_size=64, pooler_size=64, v_feature_size=8,
                                    v_hidden_size=64, v_num_attention_heads=1, v_intermediate_size=64, v_pooler_size=64, clf_hidden_size=64,
                                    max_position_embeddings=16, tt_attn_sublayers=[0], tv_attn_sublayers=[], vt_attn_sublayers=[], vv_attn_sublayers=[0],
                                    t_ff_sublayers=[1], v_ff_sublayers=[1]))
    model = BertForVLTasks(cfg, {"TASK1": {"type": "VL-classifier", "num_labels": 10}}, ["TASK1"])
    bce, ce = nn.BCEWithLogitsLoss(), nn.CrossEntropyLoss()
    want = {"VL-classifier": "bce_scaled", "VL-classifier-GQA": "bce_scaled", "VL-binary-classifier": "bce_mean", "VL-tri-classifier": "bce_mean",
            "V-logit": "bce_regions"}
    for typ, kind in want.items():
        assert TU.fused_kind(model, bce, typ) == kind and TU.fused_kind(model, TU.LossMap["BCEWithLogitLoss"], typ) == kind
        assert TU.fused_kind(model, ce, typ) is None
    assert TU.fused_kind(model, ce, "VL-logit") == "ce_options" and TU.fused_kind(model, bce, "VL-logit") is None
    assert TU.fused_kind(model, bce, "V-logit-mc") is None
    for crit in (nn.BCEWithLogitsLoss(pos_weight=torch.ones(10)), nn.BCEWithLogitsLoss(weight=torch.ones(10)), nn.BCEWithLogitsLoss(reduction="sum"),
                 nn.BCEWithLogitsLoss(reduction="none"), nn.BCELoss()):
        assert TU.fused_kind(model, crit, "VL-classifier") is None
    for crit in (nn.CrossEntropyLoss(label_smoothing=0.1), nn.CrossEntropyLoss(weight=torch.ones(4)), nn.CrossEntropyLoss(reduction="sum"),
                 nn.CrossEntropyLoss(ignore_index=0)):
        assert TU.fused_kind(model, crit, "VL-logit") is None
    assert TU.fused_kind(StubModel(None), bce, "VL-classifier") is None and TU.fused_kind(nn.Linear(2, 2), bce, "VL-classifier") is None
    monkeypatch.setenv("VOLTA_TASK_LOSS", "torch")
    assert TU.fused_kind(model, bce, "VL-classifier") is None


def test_task_loss_abi():
    from volta_amd import _lib as L
    for name in ("vk_task_loss_fwd", "vk_task_loss_bwd", "vk_task_loss_work_bytes"):
        assert hasattr(L.lib, name) and name in L.EXPORTS
    src = '#include <stdio.h>\n#include "volta_hip.h"\nint main(void){printf("%zu %d %d %d %d\\n", sizeof(vk_task_loss_args), VK_TASK_BCE_SCALED, VK_TASK_BCE_MEAN, VK_TASK_BCE_REGIONS, VK_TASK_CE_OPTIONS);return 0;}'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert ctypes.sizeof(L.TaskLossArgs) == out[0]
    assert [L.TASK_BCE_SCALED, L.TASK_BCE_MEAN, L.TASK_BCE_REGIONS, L.TASK_CE_OPTIONS] == out[1:]
    assert L.lib.vk_task_loss_work_bytes(256) >= 256 * 12 and L.lib.vk_task_loss_work_bytes(0) == 0
    # argument checks happen on the host, before any launch
    bad = L.TaskLossArgs(None, None, None, None, None, None, L.TASK_BCE_SCALED, 4, 10, 64)
    assert L.lib.vk_task_loss_fwd(ctypes.byref(bad), None) != 0 and b"missing logits" in L.lib.vk_last_error()
    bad = L.TaskLossArgs(8, 8, None, 8, 8, 8, L.TASK_BCE_SCALED, 4, 10, 60)
    assert L.lib.vk_task_loss_fwd(ctypes.byref(bad), None) != 0 and b"multiple of 64" in L.lib.vk_last_error()
    bad = L.TaskLossArgs(8, 8, None, 8, 8, 8, 7, 4, 10, 64)
    assert L.lib.vk_task_loss_bwd(ctypes.byref(bad), None, None, None) != 0 and b"unknown kind" in L.lib.vk_last_error()
    bad = L.TaskLossArgs(8, 8, None, 8, 8, 8, L.TASK_BCE_MEAN, 4, 100, 64)
    assert L.lib.vk_task_loss_bwd(ctypes.byref(bad), None, None, None) != 0 and b"exceeds ld" in L.lib.vk_last_error()
