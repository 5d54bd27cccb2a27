"""The step functions of the fine-tuning and evaluation drivers (volta/task_utils.py:24-281,429-618) without the reference's imports:
`from volta_amd.task_utils import LoadLoss, ForwardModelsTrain, ForwardModelsVal, EvaluatingModel` in train_task.py:30 / eval_task.py:27.

With a volta_amd BertForVLTasks, a default nn.BCEWithLogitsLoss / nn.CrossEntropyLoss and a task type of the table below, model, loss
and score run as ONE engine step (BertForVLTasks.task_loss: csrc/taskloss.hip reads the logits where the engine left them; loss and score
stay on the device).  Every other combination -- V-logit-mc, a criterion with pos_weight / weight / label smoothing / another reduction,
any other model object -- calls `model(...)` and does the reference's torch arithmetic, so the module replaces the reference's completely.
VOLTA_TASK_LOSS=torch forces that path (the A/B switch of tools/bench_task_step.py).  The dataset loaders (LoadDataset, LoadDatasetEval) are
host code over the feature readers and stay the reference's."""
import os

import torch
import torch.nn as nn

LossMap = {
    "BCEWithLogitLoss": nn.BCEWithLogitsLoss(reduction="mean"),
    "CrossEntropyLoss": nn.CrossEntropyLoss(),
}

# task type -> (criterion class, kind of BertForVLTasks.task_loss)
FUSED_KINDS = {
    "VL-classifier": (nn.BCEWithLogitsLoss, "bce_scaled"),
    "VL-classifier-GQA": (nn.BCEWithLogitsLoss, "bce_scaled"),
    "VL-binary-classifier": (nn.BCEWithLogitsLoss, "bce_mean"),
    "VL-tri-classifier": (nn.BCEWithLogitsLoss, "bce_mean"),
    "V-logit": (nn.BCEWithLogitsLoss, "bce_regions"),
    "VL-logit": (nn.CrossEntropyLoss, "ce_options"),
}


def LoadLoss(task_cfg, task_id):
    return LossMap[task_cfg["TASK" + task_id]["loss"]]


def compute_score_with_logits(logits, labels):
    """labels where the row's arg-max is, zero elsewhere"""
    one_hots = torch.zeros_like(labels)
    one_hots.scatter_(1, torch.max(logits, 1)[1].detach().view(-1, 1), 1)
    return one_hots * labels


def _unwrap(model):
    from .parallel import DistributedDataParallel
    return model.module if isinstance(model, DistributedDataParallel) else model


def _default_criterion(criterion, cls):
    if type(criterion) is not cls or criterion.reduction != "mean" or getattr(criterion, "weight", None) is not None:
        return False
    if cls is nn.BCEWithLogitsLoss:
        return criterion.pos_weight is None
    return criterion.ignore_index == -100 and float(getattr(criterion, "label_smoothing", 0.0)) == 0.0


def fused_kind(model, criterion, task_type):
    """The task_loss kind that serves (model, criterion, task type), or None for the torch path."""
    if os.environ.get("VOLTA_TASK_LOSS", "") == "torch" or task_type not in FUSED_KINDS:
        return None
    from .modeling import BertForVLTasks
    cls, kind = FUSED_KINDS[task_type]
    if not isinstance(_unwrap(model), BertForVLTasks) or not _default_criterion(criterion, cls):
        return None
    return kind


class _Batch:
    """One driver batch, unpacked and reshaped by the task's `process` into what the model takes."""

    def __init__(self, config, task_cfg, device, task_id, batch, dialog=True):
        batch = tuple(t.to(device=device, non_blocking=True) for t in batch)
        self.multi_choice_ids = None
        if task_cfg[task_id]["type"] == "V-logit-mc":
            features, spatials, image_mask, question, target, input_mask, segment_ids, self.multi_choice_ids, question_id = batch
        else:
            features, spatials, image_mask, question, target, input_mask, segment_ids, question_id = batch
        process = task_cfg[task_id]["process"]
        B = features.size(0)
        self.num_options = None
        if process == "dialog":
            if not dialog:
                raise NotImplementedError("dialog process for validation")
            R, rounds, self.num_options = features.size(1), question.size(1), question.size(2)
            target = target.view(-1)
            features = features[:, None, None].expand(B, rounds, self.num_options, R, config.v_feature_size).contiguous().view(-1, R, config.v_feature_size)
            spatials = spatials[:, None, None].expand(B, rounds, self.num_options, R, config.num_locs).contiguous().view(-1, R, config.num_locs)
            image_mask = image_mask[:, None].expand(B, rounds, self.num_options, R).contiguous().view(-1, R)
            question, input_mask, segment_ids = (t.view(-1, t.size(-1)) for t in (question, input_mask, segment_ids))
            B = B * rounds
        elif process == "expand":
            R, self.num_options = features.size(1), question.size(1)
            features = features[:, None].expand(B, self.num_options, R, config.v_feature_size).contiguous().view(-1, R, config.v_feature_size)
            spatials = spatials[:, None].expand(B, self.num_options, R, config.num_locs).contiguous().view(-1, R, config.num_locs)
            image_mask = image_mask[:, None].expand(B, self.num_options, R).contiguous().view(-1, R)
            question, input_mask, segment_ids = (t.view(-1, t.size(2)) for t in (question, input_mask, segment_ids))
        elif process == "retrieval":
            self.num_options = question.size(1)
            features, spatials = (t.view(-1, t.size(2), t.size(3)) for t in (features, spatials))
            image_mask, question, input_mask, segment_ids = (t.view(-1, t.size(2)) for t in (image_mask, question, input_mask, segment_ids))
        elif process == "nlvr":
            self.num_options = question.size(1)
            features, spatials = (t.view(B * 2, t.size(1) // 2, t.size(2)) for t in (features, spatials))
            image_mask = image_mask.view(B * 2, image_mask.size(1) // 2)
            question, input_mask, segment_ids = (t.repeat(1, 2).view(B * 2, t.size(1)) for t in (question, input_mask, segment_ids))
        self.batch_size, self.target, self.question_id = B, target, question_id
        self.model_args = lambda task: (question, features, spatials, task, segment_ids, input_mask, image_mask)

    def fused(self, model, task_id, kind):
        """(float[2] = loss, score sum; int32 arg-max per group) of the fused step, or None when the target does not have the layout the
        kernels read (the torch path then takes it, and raises what torch raises)."""
        t, n_opt = self.target, self.num_options
        if kind == "ce_options":
            if t.dtype != torch.int64 or t.dim() != 1 or not n_opt or t.numel() != self.batch_size:
                return None
        elif t.dtype != torch.float32 or t.dim() != (3 if kind == "bce_regions" else 2):
            return None
        q, f, s, task, seg, im, vm = self.model_args(task_id)
        return _unwrap(model)._task_loss(q, f, s, task, seg, im, vm, t, kind, n_opt)


def _torch_loss_and_score(task_type, criterion, pred, b):
    """The reference's arithmetic behind the model: (loss, score sum or count as it computes it)."""
    target = b.target
    if task_type in ("VL-classifier", "VL-classifier-GQA"):
        return criterion(pred, target).mean() * target.size(1), compute_score_with_logits(pred, target).sum()
    if task_type in ("VL-binary-classifier", "VL-tri-classifier"):
        return criterion(pred, target).mean(), compute_score_with_logits(pred, target).sum()
    if task_type == "VL-logit":
        logit = pred.view(b.batch_size, b.num_options)
        return criterion(logit, target), (torch.max(logit, 1)[1] == target).sum()
    if task_type == "V-logit":
        select_idx = torch.max(pred, dim=1)[1]
        select_target = target.squeeze(2).gather(1, select_idx.view(-1, 1))
        return criterion(pred, target).mean() * target.size(1), torch.sum(select_target > 0.5)
    if task_type == "V-logit-mc":
        logit = pred[:, 101:].squeeze(2).gather(1, b.multi_choice_ids).unsqueeze(2)
        loss = criterion(logit, target).mean() * target.size(1)
        return loss, (torch.max(logit, dim=1)[1] == torch.max(target, dim=1)[1]).sum()
    raise KeyError("task type %r has no loss" % (task_type,))       # the reference fails on the unbound `loss` here


def ForwardModelsTrain(config, task_cfg, device, task_id, batch, model, criterion):
    """-> (loss, batch_score): the differentiable loss and the batch's mean score"""
    task_type = task_cfg[task_id]["type"]
    b = _Batch(config, task_cfg, device, task_id, batch)
    kind = fused_kind(model, criterion, task_type)
    res = b.fused(model, task_id, kind) if kind else None
    if res is not None:
        return res[0][0], res[0][1].detach() / float(b.batch_size)
    pred = model(*b.model_args(task_id))[0]
    loss, score = _torch_loss_and_score(task_type, criterion, pred, b)
    if task_type in ("VL-logit", "V-logit", "V-logit-mc"):
        return loss, float(score) / float(b.batch_size)
    return loss, score / float(b.batch_size)


def ForwardModelsVal(config, task_cfg, device, task_id, batch, model, criterion):
    """-> (loss, batch score sum, batch size) as Python numbers"""
    task_type = task_cfg[task_id]["type"]
    b = _Batch(config, task_cfg, device, task_id, batch, dialog=False)
    kind = fused_kind(model, criterion, task_type)
    res = b.fused(model, task_id, kind) if kind else None
    if res is not None:
        loss, score = res[0].tolist()                 # the one host transfer of the step
        return loss, score, b.batch_size
    pred = model(*b.model_args(task_id))[0]
    loss, score = _torch_loss_and_score(task_type, criterion, pred, b)
    return float(loss.detach()), float(score), b.batch_size


def EvaluatingModel(config, task_cfg, device, task_id, batch, model, dataloader, criterion, results, others):
    """-> (loss, batch score sum, batch size, results, others); appends the task's answer records to `results`"""
    task_type = task_cfg[task_id]["type"]
    b = _Batch(config, task_cfg, device, task_id, batch)
    qid = b.question_id
    if task_type in ("VL-classifier", "VL-classifier-GQA"):
        kind = fused_kind(model, criterion, task_type)
        with torch.no_grad():
            res = b.fused(model, task_id, kind) if kind else None
            answers = (res[1] if res is not None else torch.max(model(*b.model_args(task_id))[0], 1)[1]).tolist()
        label2ans = dataloader.dataset.label2ans
        for i, a in enumerate(answers):
            if task_type == "VL-classifier":
                results.append({"question_id": qid[i].item(), "answer": label2ans[a]})
            else:
                results.append({"questionId": str(qid[i].item()), "prediction": label2ans[a]})
        return 0.0, 0.0, b.batch_size, results, others
    with torch.no_grad():
        pred = model(*b.model_args(task_id))[0]
    loss, score = _torch_loss_and_score(task_type, criterion, pred, b)
    if task_type == "VL-logit":
        probs = torch.softmax(pred.view(b.batch_size, b.num_options), dim=1)
        for i in range(probs.size(0)):
            results.append({"question_id": qid[i].item(), "answer": [p.item() for p in probs[i]]})
    elif task_type == "V-logit":
        select_idx = torch.max(pred, dim=1)[1]
        select_target = b.target.squeeze(2).gather(1, select_idx.view(-1, 1))
        for i in range(select_idx.size(0)):
            results.append({"id": qid[i].item(), "target": select_idx[i].item(), "IOU": select_target[i].item()})
    elif task_type == "V-logit-mc":
        preds = torch.max(pred[:, 101:].squeeze(2).gather(1, b.multi_choice_ids).unsqueeze(2), dim=1)[1]
        for i in range(preds.size(0)):
            results.append({"id": qid[i].item(), "target": preds[i].item()})
    return float(loss.detach()), float(score), b.batch_size, results, others
