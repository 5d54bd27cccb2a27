"""The step functions of the fine-tuning and evaluation drivers (volta/task_utils.py:24-281,429-618) without the reference's imports:
`from volta_amd.task_utils import LoadDataset, LoadLoss, ForwardModelsTrain, ForwardModelsVal` in train_task.py:30,
`from volta_amd.task_utils import LoadDatasetEval, LoadLoss, ForwardModelsTrain, ForwardModelsVal, EvaluatingModel` in eval_task.py:27.

With a volta_amd BertForVLTasks, a default nn.BCEWithLogitsLoss / nn.CrossEntropyLoss and a task type of the table below, model, loss
and score run as ONE engine step (BertForVLTasks.task_loss: csrc/taskloss.hip reads the logits where the engine left them; loss and score
stay on the device).  Every other combination -- V-logit-mc, a criterion with pos_weight / weight / label smoothing / another reduction,
any other model object -- calls `model(...)` and does the reference's torch arithmetic, so the module replaces the reference's completely.
VOLTA_TASK_LOSS=torch forces that path (the A/B switch of tools/bench_task_step.py).

LoadDataset / LoadDatasetEval (volta/task_utils.py:290-426) build the datasets of volta_amd.datasets over this project's readers and hand out
`TaskLoader`s, which assemble the batches on the device (csrc/taskbatch.hip); VQA, GQA, NLVR2, refcoco / refcoco+ / refcocog and (training)
RetrievalCOCO / RetrievalFlickr30k are covered, LoadDatasetEval also serves the retrieval test sets (RetrievalDatasetVal), any other task name raises a KeyError that names the reference class to fall back to."""
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


def _tokenizer(args):
    """`BertTokenizer.from_pretrained(args.bert_model, do_lower_case=...)` for a model that is on disk: a directory holding vocab.txt, or the
    vocabulary file itself.  Nothing is ever downloaded."""
    from .readers import WordPieceTokenizer
    name = str(args.bert_model)
    if "roberta" in name:
        raise ValueError("bert_model=%r: RoBERTa vocabularies are not supported; use the reference's loaders" % name)
    path = os.path.join(name, "vocab.txt") if os.path.isdir(name) else name
    if not os.path.isfile(path):
        raise FileNotFoundError("bert_model=%r is neither a directory with a vocab.txt nor a vocabulary file; volta_amd does not download "
                                "vocabularies -- point --bert_model at a local copy" % name)
    return WordPieceTokenizer(path, do_lower_case=getattr(args, "do_lower_case", True))


def _world(args):
    import torch.distributed as dist
    if args.local_rank == -1:
        return 1, 0
    return dist.get_world_size(), dist.get_rank()


def _threads(args, world):
    """the reference's worker arithmetic (num_workers / world size, task_utils.py:306-309) for the decode threads; None = the loader's default"""
    return int((getattr(args, "num_workers", 0) or 0) / world) or None


def _readers(args, config, cfg):
    from .readers import ImageFeaturesH5Reader
    return tuple(ImageFeaturesH5Reader(cfg[k], config, args.in_memory) if cfg[k] != "" else None for k in ("features_h5path1", "features_h5path2"))


def _dataset(cls_map, args, config, cfg, readers, tokenizer, annotations, split):
    return cls_map[cfg["name"]](task=cfg["name"], dataroot=cfg["dataroot"], annotations_jsonpath=annotations, split=split, image_features_reader=readers[0],
                                gt_image_features_reader=readers[1], tokenizer=tokenizer, bert_model=args.bert_model, padding_index=0,
                                max_seq_length=cfg["max_seq_length"], max_region_num=cfg["max_region_num"], num_locs=config.num_locs,
                                add_global_imgfeat=config.add_global_imgfeat, append_mask_sep=(config.fusion_method == "vl-bert_vqa"))


def LoadDataset(args, config, task_cfg, task_id, split="trainval"):
    """-> (batch_size, task2num_iters, dset_train, dset_val, dl_train, dl_val) with the reference's batch-size arithmetic; the loaders are
    volta_amd.datasets.TaskLoader: RandomSampler semantics without a process group, DistributedSampler semantics with one, sequential for
    validation.  `args.seed` (default 0) seeds the permutations."""
    from . import datasets as D
    tokenizer = _tokenizer(args)
    task = "TASK" + task_id
    cfg = task_cfg[task]
    readers = _readers(args, config, cfg)
    world, rank = _world(args)
    batch_size = cfg["batch_size"] // args.grad_acc_steps
    if args.local_rank != -1:
        batch_size = int(batch_size / world)
    seed = int(getattr(args, "seed", 0) or 0)
    kw = dict(drop_last=args.drop_last, in_memory=args.in_memory, threads=_threads(args, world), resident_bytes=getattr(args, "resident_bytes", 0))
    dset_train, dl_train, task2num_iters = None, None, {}
    if "train" in split:
        dset_train = _dataset(D.DatasetMapTrain, args, config, cfg, readers, tokenizer, cfg["train_annotations_jsonpath"], cfg["train_split"])
        sampler = D.RandomSampler(len(dset_train), seed) if args.local_rank == -1 else D.DistributedSampler(len(dset_train), world, rank, True, seed)
        dl_train = D.TaskLoader(dset_train, batch_size, sampler, **kw)
        task2num_iters = {task: len(dl_train)}
    dset_val, dl_val = None, None
    if "val" in split:
        dset_val = _dataset(D.DatasetMapTrain, args, config, cfg, readers, tokenizer, cfg["val_annotations_jsonpath"], cfg["val_split"])
        dl_val = D.TaskLoader(dset_val, batch_size, None, **kw)
    return batch_size, task2num_iters, dset_train, dset_val, dl_train, dl_val


def LoadDatasetEval(args, config, task_cfg, task_id):
    """-> (batch_size, task2num_iters, dset_val, dl_val): `eval_batch_size` of the task (else args.batch_size), args.split over the task's val_split.
    RetrievalCOCO / RetrievalFlickr30k (datasets.RetrievalEvalMap): a RetrievalDatasetVal, {task: 2 * captions} and a RetrievalEvalLoader, what
    eval_retrieval.py:131 expects; `volta_amd.retrieval.evaluate_retrieval(model, dset_val, ...)` then replaces the driver's loop."""
    from . import datasets as D
    tokenizer = _tokenizer(args)
    task = "TASK" + task_id
    cfg = task_cfg[task]
    readers = _readers(args, config, cfg)
    batch_size = cfg.get("eval_batch_size", args.batch_size)
    world = _world(args)[0]
    if args.local_rank != -1:
        batch_size = int(batch_size / world)
    split = args.split if args.split else cfg["val_split"]
    if cfg["name"] in D.RetrievalEvalMap:
        dset_val = _dataset(D.RetrievalEvalMap, args, config, cfg, readers, tokenizer, cfg["val_annotations_jsonpath"], split)
        dl_val = D.RetrievalEvalLoader(dset_val)
        return batch_size, {task: len(dl_val)}, dset_val, dl_val
    dset_val = _dataset(D.DatasetMapEval, args, config, cfg, readers, tokenizer, cfg["val_annotations_jsonpath"], split)
    dl_val = D.TaskLoader(dset_val, batch_size, None, drop_last=args.drop_last, in_memory=args.in_memory, threads=_threads(args, world),
                          resident_bytes=getattr(args, "resident_bytes", 0))
    return batch_size, {task: len(dl_val)}, dset_val, dl_val


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
