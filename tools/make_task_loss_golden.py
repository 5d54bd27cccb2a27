"""Records tests/golden/task_loss_reference.npz from the reference's own ForwardModelsTrain / ForwardModelsVal (volta/task_utils.py),
loaded by file path and driven on the CPU:

  python tools/make_task_loss_golden.py --reference /path/to/volta-checkout [--out tests/golden/task_loss_reference.npz]

The reference module imports pytorch_transformers and volta.datasets at the top; neither is needed by the two functions, so stub modules
stand in for them, and Tensor.cuda is the identity while they run.  The `model` is a stub that records the tensors it is called with and
returns a given prediction (a leaf tensor, so the loss's gradient with respect to it can be recorded).  Per case (task type, process) and
mode (train, val) the file holds: the raw batch (`b0`..), the tensors the model received (`m0`..`m5`: question, features, spatials,
segment_ids, input_mask, image_mask), the prediction fed back, the loss, the score the function returned and, for train, d loss / d
prediction.  Values only; the tests never import the reference."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

F, LOCS, T, R = 8, 5, 6, 5          # v_feature_size, num_locs, tokens, regions
SOFT = [0.3, 0.6, 0.9, 1.0]

# name -> (task type, process, loss, batch size)
CASES = {
    "vqa": ("VL-classifier", "normal", "BCEWithLogitLoss", 3),
    "gqa": ("VL-classifier-GQA", "normal", "BCEWithLogitLoss", 2),
    "nlvr": ("VL-binary-classifier", "nlvr", "BCEWithLogitLoss", 2),
    "snli": ("VL-tri-classifier", "normal", "BCEWithLogitLoss", 4),
    "retrieval": ("VL-logit", "retrieval", "CrossEntropyLoss", 3),
    "expand": ("VL-logit", "expand", "CrossEntropyLoss", 2),
    "dialog": ("VL-logit", "dialog", "CrossEntropyLoss", 2),
    "refcoco": ("V-logit", "normal", "BCEWithLogitLoss", 3),
    "visual7w": ("V-logit-mc", "normal", "BCEWithLogitLoss", 2),
}
WIDTH = {"vqa": 3129, "gqa": 1533, "nlvr": 2, "snli": 3}


def load_reference(root):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    stub("pytorch_transformers")
    stub("pytorch_transformers.tokenization_bert", BertTokenizer=object)
    stub("pytorch_transformers.tokenization_roberta", RobertaTokenizer=object)
    stub("volta")
    stub("volta.datasets", DatasetMapTrain={}, DatasetMapEval={})
    stub("volta.datasets._image_features_reader", ImageFeaturesH5Reader=object)
    spec = importlib.util.spec_from_file_location("volta_reference_task_utils", os.path.join(root, "volta", "task_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def soft_targets(g, rows, width, pred):
    """A few soft scores per row as the VQA / GQA datasets produce them; row 0 scores at its arg-max, the last row is all zero."""
    t = torch.zeros(rows, width)
    for r in range(rows - 1 if rows > 1 else rows):
        for c in torch.randperm(width, generator=g)[:min(3, width)].tolist():
            t[r, c] = SOFT[int(torch.randint(0, 4, (1,), generator=g))]
    t[0, int(pred[0].argmax())] = 0.9
    return t


def make_case(name, seed):
    """-> (batch tuple, prediction) with the layouts the datasets produce"""
    typ, process, _, B = CASES[name]
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    ids = lambda *s: torch.randint(1, 1000, s, generator=g)
    mask = lambda *s: (torch.rand(*s, generator=g) > 0.2).long()
    qid = torch.arange(B) + 100
    extra = ()
    if process == "retrieval":
        n_opt = 4
        feats, locs, im = rn(B, n_opt, R, F), torch.rand(B, n_opt, R, LOCS, generator=g), mask(B, n_opt, R)
        q, am, seg = ids(B, n_opt, T), mask(B, n_opt, T), torch.zeros(B, n_opt, T, dtype=torch.int64)
        pred, target = rn(B * n_opt, 1) * 3, torch.randint(0, n_opt, (B,), generator=g)
    elif process == "expand":
        n_opt = 4
        feats, locs, im = rn(B, R, F), torch.rand(B, R, LOCS, generator=g), mask(B, R)
        q, am, seg = ids(B, n_opt, T), mask(B, n_opt, T), torch.zeros(B, n_opt, T, dtype=torch.int64)
        pred, target = rn(B * n_opt, 1) * 3, torch.randint(0, n_opt, (B,), generator=g)
    elif process == "dialog":             # the reference's mask expansion needs batch size == number of rounds
        rounds, n_opt = B, 3
        feats, locs, im = rn(B, R, F), torch.rand(B, R, LOCS, generator=g), mask(B, R)
        q, am, seg = ids(B, rounds, n_opt, T), mask(B, rounds, n_opt, T), torch.zeros(B, rounds, n_opt, T, dtype=torch.int64)
        pred, target = rn(B * rounds * n_opt, 1) * 3, torch.randint(0, n_opt, (B, rounds), generator=g)
    elif process == "nlvr":
        feats, locs, im = rn(B, 2 * R, F), torch.rand(B, 2 * R, LOCS, generator=g), mask(B, 2 * R)
        q, am, seg = ids(B, T), mask(B, T), torch.zeros(B, T, dtype=torch.int64)
        pred = rn(B, 2) * 3
        target = torch.zeros(B, 2)
        target[torch.arange(B), torch.randint(0, 2, (B,), generator=g)] = 1.0
    elif typ == "V-logit":
        feats, locs, im = rn(B, R, F), torch.rand(B, R, LOCS, generator=g), mask(B, R)
        q, am, seg = ids(B, T), mask(B, T), torch.zeros(B, T, dtype=torch.int64)
        pred = rn(B, R, 1) * 3 + ((1.0 - im.float()) * -10000.0).unsqueeze(2)
        target = torch.rand(B, R, 1, generator=g)
    elif typ == "V-logit-mc":
        Rm = 101 + R
        feats, locs, im = rn(B, Rm, F), torch.rand(B, Rm, LOCS, generator=g), mask(B, Rm)
        q, am, seg = ids(B, T), mask(B, T), torch.zeros(B, T, dtype=torch.int64)
        pred = rn(B, Rm, 1) * 3
        target = torch.zeros(B, 4, 1)
        target[torch.arange(B), torch.randint(0, 4, (B,), generator=g), 0] = 1.0
        extra = (torch.stack([torch.randperm(R, generator=g)[:4] for _ in range(B)]),)
    else:
        feats, locs, im = rn(B, R, F), torch.rand(B, R, LOCS, generator=g), mask(B, R)
        q, am, seg = ids(B, T), mask(B, T), torch.zeros(B, T, dtype=torch.int64)
        pred = rn(B, WIDTH[name]) * 3
        if typ == "VL-tri-classifier":
            target = torch.zeros(B, 3)
            target[torch.arange(B), torch.randint(0, 3, (B,), generator=g)] = 1.0
        else:
            target = soft_targets(g, B, WIDTH[name], pred)
    return (feats, locs, im, q, target, am, seg) + extra + (qid,), pred


class StubModel:
    def __init__(self, pred):
        self.pred, self.seen = pred, None

    def __call__(self, question, features, spatials, task_id, segment_ids, input_mask, image_mask):
        self.seen = (question, features, spatials, segment_ids, input_mask, image_mask)
        return self.pred, None, None, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "task_loss_reference.npz"))
    args = ap.parse_args()
    ref = load_reference(args.reference)
    config = types.SimpleNamespace(v_feature_size=F, num_locs=LOCS)
    out = {"cases": np.array(sorted(CASES)), "dims": np.array([F, LOCS, T, R])}
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        for i, name in enumerate(sorted(CASES)):
            typ, process, loss_name, _ = CASES[name]
            task_cfg = {"TASK1": {"type": typ, "process": process, "loss": loss_name}}
            criterion = ref.LoadLoss(task_cfg, "1")
            out["%s/meta" % name] = np.array([typ, process, loss_name])
            for mode in ("train", "val"):
                if mode == "val" and process == "dialog":
                    continue                  # the reference raises NotImplementedError there
                batch, pred = make_case(name, 100 + i)
                pred = pred.clone().requires_grad_(True)
                model = StubModel(pred)
                fn = ref.ForwardModelsTrain if mode == "train" else ref.ForwardModelsVal
                res = fn(config, task_cfg, "cpu", "TASK1", batch, model, criterion)
                pre = "%s/%s/" % (name, mode)
                for k, t in enumerate(batch):
                    out[pre + "b%d" % k] = t.numpy()
                for k, t in enumerate(model.seen):
                    out[pre + "m%d" % k] = t.detach().numpy()
                out[pre + "pred"] = pred.detach().numpy()
                out[pre + "loss"] = np.float32(float(res[0].detach()) if torch.is_tensor(res[0]) else res[0])
                out[pre + "score"] = np.float32(float(res[1]))
                if mode == "train":
                    res[0].backward()
                    out[pre + "grad"] = pred.grad.numpy()
                else:
                    out[pre + "batch_size"] = np.int64(res[2])
    finally:
        torch.Tensor.cuda = real_cuda
    np.savez_compressed(args.out, **out)
    print("wrote %s: %d arrays, %d bytes" % (args.out, len(out), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
