"""The fine-tuning datasets of the reference (volta/datasets/*_dataset.py) over this project's readers, and a loader that assembles their batches
on the device.

  VQAClassificationDataset   volta/datasets/vqa_dataset.py        one image, question, soft target [num_labels]
  GQAClassificationDataset   volta/datasets/gqa_dataset.py        as VQA with its own files and splits
  NLVR2Dataset               volta/datasets/nlvr2_dataset.py      two images packed into one block of 2 * max_region_num rows
  ReferExpressionDataset     volta/datasets/refer_expression_dataset.py   one image, IoU target [R, 1] against the referred box
  RetrievalDataset           volta/datasets/retrieval_dataset.py:45-257   four options: true pair, random caption, random image, hard caption
  RetrievalDatasetVal        volta/datasets/retrieval_dataset.py:260-417  the test set: every caption against every image; `device_arrays`
  RetrievalEvalMap / RetrievalEvalLoader                                  its map and the driver's batch-of-one loader over resident arrays
  DatasetMapTrain / Eval     volta/datasets/__init__.py           task name -> class; any other name raises a KeyError naming the reference class
  TaskLoader                 torch's DataLoader + default_collate + `.cuda()` of the drivers, as staging -> one copy -> `vk_task_batch`

Same constructor signature, `len`, `num_labels`, `label2ans` / `ans2label` and annotation file layouts as the reference.  `dataset[i]` returns
the reference's tuple with its dtypes and shapes, computed on the host with numpy: that is the compatibility surface (a torch DataLoader over
it works) and what the CPU tests pin against recorded reference outputs.  `TaskLoader` yields the collated batch on the GPU without building
samples in Python: image records are base64-decoded by one native call per batch into pinned staging (`vk_task_images_stage`), copied once,
and padded / normalised / masked / targeted by `vk_task_batch` (csrc/taskbatch.hip).  `TaskLoader(resident_bytes=N)` keeps the images in a
device-resident pool instead: the text fields are decoded on the device (`vk_b64_decode_device`, csrc/b64.hip) during the first epoch and
`vk_task_batch_pool` reads the pool, so later epochs send only the small integer tables.

Tokenisation happens once in the constructor (one native call with a `WordPieceTokenizer`).  The reference's `cache/*.pkl` of tokenised
entries is neither read nor written: it holds pickled torch tensors tied to another tokenizer object, and tokenising a whole split takes well
under a second here.  No `pytorch_transformers`, `lmdb`, `jsonlines` or `tools.refer` is needed."""
import ctypes as C
import json
import os
import pickle
import queue
import threading

import numpy as np
import torch

from . import _lib as L
from .readers import WordPieceTokenizer, _encoder


def _read_jsonlines(path):
    with open(path, "rb") as f:
        return [json.loads(line) for line in f if line.strip()]


def _load_pickle(path):
    with open(path, "rb") as f:
        return pickle.load(f)


def _special_id(tokenizer, name):
    v = getattr(tokenizer, name + "_token_id", None)
    if v is None:
        v = tokenizer.convert_tokens_to_ids(["[%s]" % name.upper()])[0]
    return int(v)


class _TaskDataset:
    """What the classes share: tokenised text as three int64 tables [entries, T], the reader, the padded block length, and the description of a
    sample for the assembler (`images`, `blocks`)."""

    images_per_sample = 1
    options = 1                     # output blocks per sample (retrieval: 4)
    target_kind = "scatter"         # scatter: soft target [num_labels] | iou: [R, 1] against ref_box(index) | zero: the constant 0
    block_images = 1                # blocks are `block_images * max_region_num` rows long

    def __init__(self, task, dataroot, annotations_jsonpath, split, image_features_reader, gt_image_features_reader, tokenizer, bert_model,
                 padding_index=0, max_seq_length=16, max_region_num=101, num_locs=5, add_global_imgfeat=None, append_mask_sep=False):
        if "roberta" in str(bert_model):
            raise ValueError("RoBERTa vocabularies are not supported by volta_amd.datasets; use the reference's dataset classes")
        self.task, self.split, self.dataroot = task, split, dataroot
        self._max_region_num = max_region_num + int(add_global_imgfeat is not None)
        self._max_seq_length = max_seq_length
        self._image_features_reader = image_features_reader
        self._tokenizer = tokenizer
        self._padding_index = padding_index
        self._num_locs = num_locs
        self._add_global_imgfeat = add_global_imgfeat
        self._append_mask_sep = append_mask_sep

    def __len__(self):
        return len(self.entries)

    @property
    def block_rows(self):
        return self.block_images * self._max_region_num

    def _tokenize(self, texts, append_mask_sep=False):
        """-> tokens, input_mask, segment_ids: int64 [n, T].  ids[: T - 2] between [CLS] and [SEP], padded with `padding_index` (the reference
        pads the mask and the segment ids with the same value)."""
        T, tok, pad = self._max_seq_length, self._tokenizer, self._padding_index
        cls, sep = _special_id(tok, "cls"), _special_id(tok, "sep")
        if isinstance(tok, WordPieceTokenizer):
            ids, counts = tok.encode_batch(list(texts), max(T - 2, 1))
            ids, counts = ids.numpy(), np.minimum(counts.numpy(), T - 2)
            rows = [ids[i, :counts[i]].tolist() for i in range(len(texts))]
        else:
            enc = _encoder(tok)
            rows = [enc(t)[:T - 2] for t in texts]
        n = len(rows)
        tokens, mask, seg = (np.full((n, T), pad, dtype=np.int64) for _ in range(3))
        for i, r in enumerate(rows):
            full = [cls] + list(r) + [sep]
            tokens[i, :len(full)], mask[i, :len(full)], seg[i, :len(full)] = full, 1, 0
        if append_mask_sep:                     # vqa_dataset.py:266-271: the two ids behind the last real token, mask 1, segment 1
            extra = tok.convert_tokens_to_ids(["[MASK]", "[CLS]"])
            t2, m2, s2 = (np.empty((n, T + 2), dtype=np.int64) for _ in range(3))
            for i in range(n):
                p = int(mask[i].sum())
                t2[i] = np.concatenate([tokens[i, :p], extra, tokens[i, p:]])
                m2[i] = np.concatenate([mask[i, :p], [1, 1], mask[i, p:]])
                s2[i] = np.concatenate([seg[i, :p], [1, 1], seg[i, p:]])
            tokens, mask, seg = t2, m2, s2
        return tokens, mask, seg

    def _set_targets(self, answers, num_labels):
        """CSR (label, score) lists of the soft targets; labels of one sample must be distinct (scatter_ with repeated indices has no defined
        winner, and the device kernel assumes none)."""
        csr, labels, scores = [0], [], []
        for a in answers:
            lab = [] if a is None else [int(x) for x in a["labels"]]
            sc = [] if a is None else [float(x) for x in a["scores"]]
            assert len(lab) == len(sc) and len(set(lab)) == len(lab), "labels of one sample must be distinct"
            assert all(0 <= x < num_labels for x in lab), "label outside [0, num_labels)"
            labels += lab
            scores += sc
            csr.append(len(labels))
        self._csr, self._labels, self._scores = np.asarray(csr, np.int32), np.asarray(labels, np.int32), np.asarray(scores, np.float32)

    def _target(self, index):
        t = np.zeros(self.num_labels, dtype=np.float32)
        lo, hi = self._csr[index], self._csr[index + 1]
        t[self._labels[lo:hi]] = self._scores[lo:hi]
        return t

    # ---- the sample as the assembler sees it
    def images(self, index):
        """image ids of sample `index`, in the order `blocks` refers to them"""
        raise NotImplementedError

    def blocks(self, index, nl):
        """nl[k]: logical row count (global row included) of images(index)[k] -> per output block (segments, mask count), a segment being
        (k, src_from, dst_from, count)."""
        raise NotImplementedError

    def sample_id(self, index):
        raise NotImplementedError

    def text_rows(self, index):
        """rows of the token tables, one per option"""
        return [index]

    def _pad_block(self, parts):
        """host counterpart of the assembler for one block: `parts` = (features, boxes) row lists laid one after the other, cut at the block
        length"""
        R = self.block_rows
        F = parts[0][0].shape[1]
        feat, loc = np.zeros((R, F), dtype=np.float32), np.zeros((R, self._num_locs), dtype=np.float32)
        at = 0
        for f, b in parts:
            k = min(f.shape[0], R - at)
            if k <= 0:
                break
            feat[at:at + k], loc[at:at + k] = f[:k], b[:k]
            at += k
        mask = np.zeros(R, dtype=np.int64)
        mask[:at] = 1
        return feat, loc, mask


class VQAClassificationDataset(_TaskDataset):
    """volta/datasets/vqa_dataset.py:36-285, every split rule of `_load_dataset` included."""

    _questions = "v2_OpenEnded_mscoco_%s_questions.json"

    def _pairs(self, name):
        q = sorted(json.load(open(os.path.join(self.dataroot, self._questions % (name + "2014"))))["questions"], key=lambda x: x["question_id"])
        a = sorted(_load_pickle(os.path.join(self.dataroot, "cache", "%s_target.pkl" % name)), key=lambda x: x["question_id"])
        return q, a

    def _load_dataset(self, name):
        if name in ("train", "val"):
            questions, answers = self._pairs(name)
        elif name == "trainval":
            (qt, at), (qv, av) = self._pairs("train"), self._pairs("val")
            questions, answers = qt + qv[:-3000], at + av[:-3000]
        elif name == "minval":
            qv, av = self._pairs("val")
            questions, answers = qv[-3000:], av[-3000:]
        elif name == "test":
            questions = sorted(json.load(open(os.path.join(self.dataroot, self._questions % "test2015")))["questions"], key=lambda x: x["question_id"])
            return [dict(question_id=q["question_id"], image_id=q["image_id"], question=q["question"], answer=None) for q in questions]
        elif name == "mteval":
            questions, answers = self._pairs("train")
            self._pairs("val")                                  # the reference reads (and so requires) the val files too
            keep = set(int(x) for x in np.load(os.path.join(self.dataroot, "cache", "coco_test_ids.npy")))
            both = [(q, a) for q, a in zip(questions, answers) if int(q["image_id"]) in keep]
            questions, answers = [q for q, _ in both], [a for _, a in both]
        else:
            raise AssertionError("data split is not recognized.")
        assert len(questions) == len(answers), "%s (true) vs %s (expected)" % (len(questions), len(answers))
        entries = []
        for q, a in zip(questions, answers):
            if name != "mteval":
                assert q["question_id"] == a["question_id"] and q["image_id"] == a["image_id"], (q["question_id"], a["question_id"])
            entries.append(dict(question_id=q["question_id"], image_id=q["image_id"], question=q["question"],
                                answer=dict(labels=a["labels"], scores=a["scores"])))
        return entries

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.ans2label = _load_pickle(os.path.join(self.dataroot, "trainval_ans2label.pkl"))
        self.label2ans = _load_pickle(os.path.join(self.dataroot, "trainval_label2ans.pkl"))
        self.num_labels = len(self.ans2label)
        self.entries = self._load_dataset(self.split)
        self._text = self._tokenize([e["question"] for e in self.entries], self._uses_mask_sep())
        self._set_targets([e.get("answer") for e in self.entries], self.num_labels)
        self.qid2imgid = {e["question_id"]: e["image_id"] for e in self.entries}

    def _uses_mask_sep(self):
        return bool(self._append_mask_sep)

    def images(self, index):
        return [self.entries[index]["image_id"]]

    def blocks(self, index, nl):
        R = self.block_rows
        return [([(0, 0, 0, R)], min(nl[0], R))]

    def sample_id(self, index):
        return self.entries[index]["question_id"]

    def __getitem__(self, index):
        e = self.entries[index]
        features, _, boxes, _ = self._image_features_reader[e["image_id"]]
        feat, loc, mask = self._pad_block([(features, boxes)])
        tok, im, seg = (torch.from_numpy(t[index]) for t in self._text)
        return (torch.from_numpy(feat), torch.from_numpy(loc), torch.from_numpy(mask), tok, torch.from_numpy(self._target(index)), im, seg,
                e["question_id"])


class GQAClassificationDataset(VQAClassificationDataset):
    """volta/datasets/gqa_dataset.py:39-238.  The reference's GQA class accepts `append_mask_sep` and never applies it; neither does this."""

    def _uses_mask_sep(self):
        return False

    def _load_dataset(self, name):
        if name == "test":
            items = json.load(open(os.path.join(self.dataroot, "testdev_balanced_questions.json"), "rb"))
            return [dict(question_id=int(k), image_id=v["imageId"], question=v["question"], answer=None) for k, v in items.items()]
        if name in ("train", "val", "trainval"):
            items = sorted(_load_pickle(os.path.join(self.dataroot, "%s_target.pkl" % name)), key=lambda x: x["question_id"])
            if name == "trainval":
                items = items[:-3000]
        elif name == "minval":
            items = sorted(_load_pickle(os.path.join(self.dataroot, "trainval_target.pkl")), key=lambda x: x["question_id"])[-3000:]
        else:
            raise AssertionError("data split is not recognized.")
        return [dict(question_id=int(it["question_id"]), image_id=it["image_id"], question=it["question"],
                     answer=dict(labels=it["labels"], scores=it["scores"])) for it in items]


class NLVR2Dataset(_TaskDataset):
    """volta/datasets/nlvr2_dataset.py:37-226: the regions of image 1 follow those of image 0 with no gap, the whole cut at 2 * max_region_num
    rows (the `nlvr` process of the drivers then views the block as two halves)."""

    images_per_sample = 2
    block_images = 2

    def __init__(self, *args, **kw):
        kw.setdefault("max_region_num", 37)
        super().__init__(*args, **kw)
        if self.split not in ("train", "dev", "test"):
            raise AssertionError("data split is not recognized.")
        self.num_labels = 2
        self.entries = []
        for count, ann in enumerate(_read_jsonlines(os.path.join(self.dataroot, "%s.json" % self.split))):
            stem = "-".join(ann["identifier"].split("-")[:-1])
            self.entries.append(dict(question_id=count, image_id_0=stem + "-img0", image_id_1=stem + "-img1", sentence=str(ann["sentence"]),
                                     answer=dict(labels=[0 if str(ann["label"]) == "False" else 1], scores=[1.0])))
        self._text = self._tokenize([e["sentence"] for e in self.entries])
        self._set_targets([e["answer"] for e in self.entries], self.num_labels)

    def images(self, index):
        e = self.entries[index]
        return [e["image_id_0"], e["image_id_1"]]

    def blocks(self, index, nl):
        R = self.block_rows
        return [([(0, 0, 0, R), (1, 0, nl[0], max(R - nl[0], 0))], min(nl[0] + nl[1], R))]

    def sample_id(self, index):
        return self.entries[index]["question_id"]

    def __getitem__(self, index):
        e = self.entries[index]
        f0, _, b0, _ = self._image_features_reader[e["image_id_0"]]
        f1, _, b1, _ = self._image_features_reader[e["image_id_1"]]
        feat, loc, mask = self._pad_block([(f0, b0), (f1, b1)])
        tok, im, seg = (torch.from_numpy(t[index]) for t in self._text)
        return (torch.from_numpy(feat), torch.from_numpy(loc), torch.from_numpy(mask), tok, torch.from_numpy(self._target(index)), im, seg,
                e["question_id"])


class ReferExpressionDataset(_TaskDataset):
    """volta/datasets/refer_expression_dataset.py:65-272.  `refs(unc).p` (`refs(umd).p` for refcocog) and `instances.json` under
    `dataroot/<task>/` are read directly with the split rule of tools/refer/refer.py:144-168; that package (and its plotting imports) is not
    needed.  Target [R, 1]: IoU (+1 pixel convention) of every ORIGINAL pixel box, the global row's whole-image box included, with the
    referred box; returns the image id in the last place."""

    target_kind = "iou"

    def __init__(self, *args, **kw):
        kw.setdefault("max_seq_length", 20)
        kw.setdefault("max_region_num", 60)
        super().__init__(*args, **kw)
        self.num_labels = 1
        base = os.path.join(self.dataroot, self.task)
        refs = _load_pickle(os.path.join(base, "refs(%s).p" % ("umd" if self.task == "refcocog" else "unc")))
        with open(os.path.join(base, "instances.json")) as f:
            anns = {a["id"]: a for a in json.load(f)["annotations"]}
        split = "train" if self.split == "mteval" else self.split
        if split in ("testA", "testB", "testC"):
            keep = [r for r in refs if split[-1] in r["split"]]
        elif split in ("testAB", "testBC", "testAC"):
            keep = [r for r in refs if r["split"] == split]
        elif split == "test":
            keep = [r for r in refs if "test" in r["split"]]
        elif split in ("train", "val"):
            keep = [r for r in refs if r["split"] == split]
        else:
            raise ValueError("No such split [%s]" % split)
        by_id = {r["ref_id"]: r for r in refs}                      # REFER.Refs: the last ref of an id wins
        remove = set()
        if self.split == "mteval":
            remove = set(int(x) for x in np.load(os.path.join(self.dataroot, "cache", "coco_test_ids.npy")))
        self.entries = []
        for r in keep:
            ref = by_id[r["ref_id"]]
            if self.split == "mteval" and int(ref["image_id"]) not in remove:
                continue
            box = anns[ref["ann_id"]]["bbox"]
            for sent, sent_id in zip(ref["sentences"], ref["sent_ids"]):
                self.entries.append(dict(caption=sent["raw"], sent_id=sent_id, image_id=ref["image_id"], refBox=box, ref_id=ref["ref_id"]))
        self._text = self._tokenize([e["caption"] for e in self.entries])
        self._set_targets([None] * len(self.entries), 1)

    def ref_box(self, index):
        x, y, w, h = self.entries[index]["refBox"]
        return np.asarray([x, y, x + w, y + h], dtype=np.float32)

    def images(self, index):
        return [self.entries[index]["image_id"]]

    def blocks(self, index, nl):
        R = self.block_rows
        return [([(0, 0, 0, R)], min(nl[0], R))]

    def sample_id(self, index):
        return self.entries[index]["image_id"]

    def __getitem__(self, index):
        e = self.entries[index]
        features, n, boxes, ori = self._image_features_reader[e["image_id"]]
        feat, loc, mask = self._pad_block([(features, boxes)])
        bx, g, one = np.asarray(ori[:, :4], dtype=np.float32), self.ref_box(index), np.float32(1)
        ga = (g[2] - g[0] + one) * (g[3] - g[1] + one)
        aa = (bx[:, 2] - bx[:, 0] + one) * (bx[:, 3] - bx[:, 1] + one)
        iw = np.minimum(bx[:, 2], g[2]) - np.maximum(bx[:, 0], g[0]) + one
        ih = np.minimum(bx[:, 3], g[3]) - np.maximum(bx[:, 1], g[1]) + one
        iw[iw < 0] = 0
        ih[ih < 0] = 0
        k = min(int(n), self.block_rows)
        target = np.zeros((self.block_rows, 1), dtype=np.float32)
        target[:k, 0] = (iw * ih / (aa + ga - iw * ih))[:k]
        tok, im, seg = (torch.from_numpy(t[index]) for t in self._text)
        return (torch.from_numpy(feat), torch.from_numpy(loc), torch.from_numpy(mask), tok, torch.from_numpy(target), im, seg, e["image_id"])


class RetrievalDataset(_TaskDataset):
    """volta/datasets/retrieval_dataset.py:26-257: four options per sample -- the true pair, a random caption, a random image, and a hard
    (split "train", from `hard_negative.pkl`) or random caption.  As in the reference, option 3 is built in the padded arrays of option 1:
    rows [n3, n1) keep image 1's features and boxes while the mask has n3 ones.  The reference builds that mask from the uncut region count,
    so an image with more regions than the block makes its `torch.stack` fail; here that is a ValueError that says so.

    Random choices come from `self.rng`, a `random.Random(seed)` owned by the dataset.  `negatives`, when given, is called with the sample
    index and returns the three draws (entry index of the random caption, image id of the random image, entry index of the hard / random
    caption) instead: tests inject the reference's recorded draws through it."""

    options = 4
    target_kind = "zero"

    def __init__(self, *args, seed=0, negatives=None, **kw):
        import random
        kw.setdefault("max_seq_length", 20)
        kw.setdefault("max_region_num", 36)
        super().__init__(*args, **kw)
        self.num_labels = 1
        self.rng, self.negatives = random.Random(seed), negatives
        path = args[2] if len(args) > 2 else kw["annotations_jsonpath"]
        self._entries, self.imgid2entry = [], {}
        for ann in _read_jsonlines(path):
            if self.task == "RetrievalCOCO":
                image_id = ann["id"]
            elif self.task == "RetrievalFlickr30k":
                image_id = int(ann["img_path"].split(".")[0])
            else:
                raise ValueError("RetrievalDataset serves RetrievalCOCO and RetrievalFlickr30k, not %r" % self.task)
            self.imgid2entry[image_id] = []
            for sent in ann["sentences"]:
                self.imgid2entry[image_id].append(len(self._entries))
                self._entries.append(dict(caption=sent, image_id=image_id))
        self.entries = self._entries
        self.image_id_list = [*self.imgid2entry]
        if self.split == "train":
            for key, value in _load_pickle(os.path.join(self.dataroot, "hard_negative.pkl")).items():
                setattr(self, key, value)
            self.train_imgId2pool = {image_id: i for i, image_id in enumerate(self.train_image_list)}
        self._text = self._tokenize([e["caption"] for e in self._entries])
        self._set_targets([None] * len(self._entries), 1)
        self._drawn = {}

    def _other_image(self, image_id):
        while True:
            other = self.rng.choice(self.image_id_list)
            if other != image_id:
                return other

    def draw(self, index):
        """(entry of the random caption, random image id, entry of the hard / random caption) of one visit of sample `index`"""
        if self.negatives is not None:
            e2, img3, e4 = self.negatives(index)
            return int(e2), img3, int(e4)
        image_id = self._entries[index]["image_id"]
        e2 = self.rng.choice(self.imgid2entry[self._other_image(image_id)])
        img3 = self._other_image(image_id)
        if self.split == "train":
            pool = self.train_hard_pool[self.train_imgId2pool[image_id]]
            img4 = self.train_image_list[int(pool[self.rng.randrange(1, len(pool))])]
        else:
            img4 = self._other_image(image_id)
        return e2, img3, self.rng.choice(self.imgid2entry[img4])

    def images(self, index):
        """draws this visit's negatives; `blocks` and `text_rows` of the same index then refer to them"""
        d = self._drawn[index] = self.draw(index)
        return [self._entries[index]["image_id"], d[1]]

    def blocks(self, index, nl):
        R = self.block_rows
        if nl[1] > R:
            raise ValueError("retrieval negative image %r has %d rows, more than the %d of a block: the reference's mask of option 3 is built "
                             "from the uncut count and cannot be stacked; raise max_region_num" % (self._drawn[index][1], nl[1], R))
        one = ([(0, 0, 0, R)], min(nl[0], R))
        return [one, one, ([(0, 0, 0, R), (1, 0, 0, R)], nl[1]), one]

    def text_rows(self, index):
        d = self._drawn[index]
        return [index, d[0], index, d[2]]

    def sample_id(self, index):
        return self._entries[index]["image_id"]

    def __getitem__(self, index):
        ids = self.images(index)
        f1, _, b1, _ = self._image_features_reader[ids[0]]
        f3, n3, b3, _ = self._image_features_reader[ids[1]]
        (_, m1), _, (_, m3), _ = self.blocks(index, [f1.shape[0], f3.shape[0]])
        feat1, loc1, mask1 = self._pad_block([(f1, b1)])
        feat3, loc3 = feat1.copy(), loc1.copy()
        feat3[:m3], loc3[:m3] = f3[:m3], b3[:m3]
        mask3 = (np.arange(self.block_rows) < m3).astype(np.int64)
        rows = self.text_rows(index)
        tok, im, seg = (torch.from_numpy(t[rows]) for t in self._text)
        return (torch.from_numpy(np.stack([feat1, feat1, feat3, feat1])), torch.from_numpy(np.stack([loc1, loc1, loc3, loc1])),
                torch.from_numpy(np.stack([mask1, mask1, mask3, mask1])), tok, 0, im, seg, ids[0])


class RetrievalDatasetVal(_TaskDataset):
    """volta/datasets/retrieval_dataset.py:260-417, the retrieval test set: every caption against every image.

    Annotations as `_load_annotationsVal`: the image id is `id` (RetrievalCOCO) or the stem of `img_path` (RetrievalFlickr30k), images in
    first-seen order, one caption entry per sentence.  Tokenisation as :340-375 through `_tokenize`.  `caption_image[c]` is the index of
    caption c's image in the image list; a caption whose image is not in the list is refused here with a ValueError that names it (the
    reference fails in the driver with an IndexError).

    Host surface (the compatibility surface; never used by the fast path): `len` is 2 * captions and `dataset[index]` is the reference's
    9-tuple for caption index // 2 against the image half index % 2 -- (features_all, spatials_all, image_mask_all) of images [:500] or
    [500:], caption, input_mask, segment_ids, target_all float32 [500], caption_idx, image_idx -- from host copies of the image arrays
    built on first use through the reader.  The `[:500]` / `[500:]` halves and the length-500 target are kept as they are: with more than
    1000 images a target past 500 raises the reference's IndexError.

    Device surface: `device_arrays(device)` -> dict of `features` [Ni, R, F] fp32, `spatials` [Ni, R, num_locs] fp32, `image_mask` [Ni, R]
    int64, `input_ids` / `input_mask` / `segment_ids` [Nc, T] int64, `caption_image` [Nc] int32, `image_ids` [Ni] int64, resident on the
    device (the reference keeps a float64 host copy of everything).  The image arrays are assembled by `vk_task_batch` writing into slices
    of the resident arrays, from chunks of at most `chunk_images` images that `ImageStager` decodes into two alternating pinned staging
    sets: same kernel as the other datasets, so the values equal the reference's bit for bit."""

    target_kind = "zero"
    HALF = 500                      # the reference's image block (retrieval_dataset.py:382-392, eval_retrieval.py:184)

    def __init__(self, *args, chunk_images=256, **kw):
        kw.setdefault("max_seq_length", 20)
        kw.setdefault("max_region_num", 36)
        super().__init__(*args, **kw)
        self.num_labels = 1
        self.chunk_images = max(1, min(256, int(chunk_images)))
        path = args[2] if len(args) > 2 else kw["annotations_jsonpath"]
        images, self._caption_entries = {}, []
        for ann in _read_jsonlines(path):
            if self.task == "RetrievalCOCO":
                image_id = ann["id"]
            elif self.task == "RetrievalFlickr30k":
                image_id = int(ann["img_path"].split(".")[0])
            else:
                raise ValueError("RetrievalDatasetVal serves RetrievalCOCO and RetrievalFlickr30k, not %r" % self.task)
            images[image_id] = 1
            for sent in ann["sentences"]:
                self._caption_entries.append(dict(caption=sent, image_id=image_id))
        self._image_entries = [*images]
        self.entries = self._caption_entries
        self.caption_image = self._index_captions(self._image_entries, self._caption_entries)
        self._text = self._tokenize([e["caption"] for e in self._caption_entries])
        self._host, self._device = None, {}

    @staticmethod
    def _index_captions(image_entries, caption_entries):
        """int32 [captions]: the position of each caption's image in `image_entries`"""
        at = {image_id: i for i, image_id in enumerate(image_entries)}
        out = np.empty(len(caption_entries), np.int32)
        for c, e in enumerate(caption_entries):
            if e["image_id"] not in at:
                raise ValueError("caption %d (%r) belongs to image %r, which is not among the %d images of the set" % (c, e["caption"], e["image_id"], len(at)))
            out[c] = at[e["image_id"]]
        return out

    def __len__(self):
        return 2 * len(self._caption_entries)

    def host_tables(self):
        """the small tables `device_arrays` uploads, as numpy"""
        return dict(input_ids=self._text[0], input_mask=self._text[1], segment_ids=self._text[2], caption_image=self.caption_image,
                    image_ids=np.asarray(self._image_entries, np.int64))

    def _host_arrays(self):
        if self._host is None:
            blocks = []
            for image_id in self._image_entries:
                features, _, boxes, _ = self._image_features_reader[image_id]
                blocks.append(self._pad_block([(features, boxes)]))
            F = blocks[0][0].shape[1] if blocks else int(self._image_features_reader.feature_size)
            R = self.block_rows
            self._host = tuple(torch.from_numpy(np.stack([b[k] for b in blocks]) if blocks else np.zeros(shape, dt))
                               for k, (shape, dt) in enumerate((((0, R, F), np.float32), ((0, R, self._num_locs), np.float32), ((0, R), np.int64))))
        return self._host

    def _target_pos(self, caption_idx, half):
        """(position of the caption's image in the image half, or None)"""
        pos = int(self.caption_image[caption_idx]) - half * self.HALF
        if pos < 0 or (half == 0 and pos >= self.HALF):
            return None
        if pos >= self.HALF:        # target_all[i] = 1 with i past the 500 entries (retrieval_dataset.py:399-402)
            raise IndexError("index %d is out of bounds for dimension 0 with size %d" % (pos, self.HALF))
        return pos

    def __getitem__(self, index):
        caption_idx, image_idx = int(index / 2), index % 2
        half = slice(0, self.HALF) if image_idx == 0 else slice(self.HALF, None)
        features, spatials, image_mask = (t[half] for t in self._host_arrays())
        tok, im, seg = (torch.from_numpy(t[caption_idx]) for t in self._text)
        target_all = torch.zeros(self.HALF)
        pos = self._target_pos(caption_idx, image_idx)
        if pos is not None:
            target_all[pos] = 1
        return features, spatials, image_mask, tok, im, seg, target_all, caption_idx, image_idx

    def device_arrays(self, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("RetrievalDatasetVal.device_arrays assembles the image arrays with vk_task_batch on an MI355X; there is no host "
                               "path (index the dataset for that)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._device:
            self._device[device] = self._assemble(device)
        return self._device[device]

    def _chunk_blocks(self, n):
        """n [S]: region counts of a staged chunk -> (segs int32 [S, TASK_MAX_SEGS, 4], mask counts int32 [S]) for `vk_task_batch`: image s
        fills block s from its logical row 0, masked up to min(rows, block length)"""
        S, R = len(n), self.block_rows
        segs = np.zeros((S, L.TASK_MAX_SEGS, 4), np.int32)
        segs[:, 0, 0], segs[:, 0, 3] = np.arange(S), R
        return segs, np.minimum(np.asarray(n, np.int64) + int(self._add_global_imgfeat is not None), R).astype(np.int32)

    def _assemble(self, dev):
        from . import ops
        Ni, R = len(self._image_entries), self.block_rows
        stager = ImageStager(self._image_features_reader, sets=2)
        out = dict(features=torch.empty(Ni, R, stager.F, dtype=torch.float32, device=dev),
                   spatials=torch.empty(Ni, R, self._num_locs, dtype=torch.float32, device=dev),
                   image_mask=torch.empty(Ni, R, dtype=torch.int64, device=dev))
        with torch.cuda.device(dev):
            busy = [None, None]                 # per staging set: the event after which its pinned memory may be rewritten
            for k, i0 in enumerate(range(0, Ni, self.chunk_images)):
                which = k % 2
                if busy[which] is not None:
                    busy[which].synchronize()
                h = stager.stage(self._image_entries[i0:i0 + self.chunk_images], which)
                S = h["S"]
                feat, boxes = (h["stage"][name][:S].to(dev, non_blocking=True) for name in ("feat", "boxes"))
                segs, counts = self._chunk_blocks(h["n"])
                small = torch.from_numpy(np.concatenate([h["n"], h["wh"].reshape(-1), counts, segs.reshape(-1)]).astype(np.int32))
                small = (small.pin_memory() if stager._pin else small).to(dev, non_blocking=True)      # the small tables as one copy
                ops.task_batch(feat, boxes, small[:S], small[S:3 * S].view(S, 2), small[4 * S:].view(S, L.TASK_MAX_SEGS, 4), small[3 * S:4 * S], R,
                               self._num_locs, self._add_global_imgfeat, out={name: t[i0:i0 + S] for name, t in out.items()})
                busy[which] = torch.cuda.Event()
                busy[which].record()
            for name, table in self.host_tables().items():
                out[name] = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
            torch.cuda.current_stream().synchronize()      # the staging sets go away with the stager
        return out


class RetrievalEvalLoader:
    """What the driver's DataLoader(batch_size=1) over a RetrievalDatasetVal yields (eval_retrieval.py:168-170), as device tensors: per index
    the collated 9-tuple with its leading dimension of 1.  The image tensors are views of the dataset's resident arrays (no copy), so the
    unchanged driver loop runs -- slowly, through the whole model; `volta_amd.retrieval.evaluate_retrieval` is the fast path."""

    def __init__(self, dataset, device="cuda"):
        self.dataset, self.device, self.batch_size = dataset, device, 1

    def __len__(self):
        return len(self.dataset)

    def __iter__(self):
        ds = self.dataset
        arr = ds.device_arrays(self.device)
        dev, H = arr["features"].device, ds.HALF
        for index in range(len(ds)):
            c, half = index // 2, index % 2
            lo, hi = (0, H) if half == 0 else (H, None)
            target = torch.zeros(1, H, dtype=torch.float32, device=dev)
            pos = ds._target_pos(c, half)
            if pos is not None:
                target[0, pos] = 1
            yield (arr["features"][lo:hi].unsqueeze(0), arr["spatials"][lo:hi].unsqueeze(0), arr["image_mask"][lo:hi].unsqueeze(0),
                   arr["input_ids"][c:c + 1], arr["input_mask"][c:c + 1], arr["segment_ids"][c:c + 1], target,
                   torch.full((1,), c, dtype=torch.int64, device=dev), torch.full((1,), half, dtype=torch.int64, device=dev))


class _DatasetMap(dict):
    """task name -> dataset class; a task this module does not cover names the reference class to fall back to"""

    _reference = {"GenomeQA": "GenomeQAClassificationDataset", "VCR_Q-A": "VCRDataset", "VCR_QA-R": "VCRDataset", "RetrievalCOCO": "RetrievalDatasetVal",
                  "RetrievalFlickr30k": "RetrievalDatasetVal", "VisualEntailment": "VisualEntailmentDataset", "GuessWhat": "GuessWhatDataset",
                  "Visual7w": "Visual7wPointingDataset", "GuessWhatPointing": "GuessWhatPointingDataset", "FlickrGrounding": "FlickrGroundingDataset"}

    def __missing__(self, name):
        ref = self._reference.get(name)
        raise KeyError("task %r has no dataset in volta_amd.datasets; %s" % (
            name, "use the reference's volta.datasets.%s" % ref if ref else "the reference has none either"))


_COMMON = {"VQA": VQAClassificationDataset, "GQA": GQAClassificationDataset, "NLVR2": NLVR2Dataset, "refcoco": ReferExpressionDataset,
           "refcoco+": ReferExpressionDataset, "refcocog": ReferExpressionDataset}
DatasetMapTrain = _DatasetMap(_COMMON, RetrievalCOCO=RetrievalDataset, RetrievalFlickr30k=RetrievalDataset)
DatasetMapEval = _DatasetMap(_COMMON)      # the datasets TaskLoader batches; retrieval evaluation is not one of them:
RetrievalEvalMap = {"RetrievalCOCO": RetrievalDatasetVal, "RetrievalFlickr30k": RetrievalDatasetVal}    # LoadDatasetEval consults this first


# ------------------------------------------------------------------------------------------------ samplers
class SequentialSampler:
    def __init__(self, n):
        self.n = int(n)

    def __len__(self):
        return self.n

    def __iter__(self):
        return iter(range(self.n))


class RandomSampler:
    """torch's RandomSampler semantics: a fresh permutation per epoch, here from a generator seeded by (seed, epoch) so that a run repeats."""

    def __init__(self, n, seed=0):
        self.n, self.seed, self.epoch = int(n), int(seed), 0

    def __len__(self):
        return self.n

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __iter__(self):
        g = torch.Generator().manual_seed(self.seed + 7919 * self.epoch)
        self.epoch += 1
        return iter(torch.randperm(self.n, generator=g).tolist())


class DistributedSampler:
    """torch's DistributedSampler semantics: the (shuffled) index list padded with its own head to a multiple of the world size, then the
    rank-strided shard; the permutation depends on (seed, epoch) only, so every rank draws the same one.  `set_epoch` as in torch."""

    def __init__(self, n, num_replicas, rank, shuffle=True, seed=0):
        assert 0 <= rank < num_replicas
        self.n, self.world, self.rank, self.shuffle, self.seed, self.epoch = int(n), int(num_replicas), int(rank), shuffle, int(seed), 0
        self.num_samples = -(-self.n // self.world)

    def __len__(self):
        return self.num_samples

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __iter__(self):
        if self.shuffle:
            idx = torch.randperm(self.n, generator=torch.Generator().manual_seed(self.seed + self.epoch)).tolist()
        else:
            idx = list(range(self.n))
        total = self.num_samples * self.world
        while len(idx) < total:
            idx += idx[:total - len(idx)]
        return iter(idx[self.rank:total:self.world])


# ------------------------------------------------------------------------------------------------ record staging
def _b64_rows(text, row_bytes):
    """rows of `row_bytes` that a base64 text decodes to, from its length alone"""
    n = len(text)
    pad = 2 if text[-2:] in ("==", b"==") else 1 if text[-1:] in ("=", b"=") else 0
    nbytes = (n - pad) * 3 // 4 if n % 4 == 0 or pad else n * 3 // 4
    if nbytes % row_bytes:
        raise ValueError("base64 payload of %d bytes is not a whole number of %d-byte rows" % (nbytes, row_bytes))
    return nbytes // row_bytes


class _PinnedPool:
    """Decoded images kept in pinned memory, keyed by image id (`in_memory`): later epochs skip lookup and decode and copy straight from here.
    Memory comes in chunks; the pool stops taking images at `max_bytes`."""

    CHUNK = 64 << 20

    def __init__(self, max_bytes, pin):
        self.max_bytes, self.pin, self.bytes, self.items = int(max_bytes), pin, 0, {}
        self._chunk, self._at = None, 0

    def alloc(self, floats):
        need = floats * 4
        if self._chunk is None or self._at + floats > self._chunk.numel():
            size = max(self.CHUNK, need)
            if self.bytes + size > self.max_bytes:
                size = need
                if self.bytes + size > self.max_bytes:
                    return None
            self._chunk, self._at = torch.empty(size // 4, dtype=torch.float32, pin_memory=self.pin), 0
            self.bytes += size
        out = self._chunk[self._at:self._at + floats]
        self._at += floats
        return out


def _b64_nsig(text):
    """significant characters of a base64 text: its length without up to two trailing '=' (only the last two characters are looked at)"""
    return len(text) - (2 if text[-2:] in ("==", b"==") else 1 if text[-1:] in ("=", b"=") else 0)


def _text_layout(texts):
    """texts: one base64 field after the other -> ([(field, nsig, arena offset)], arena bytes): the fields packed without their padding at
    16-byte aligned offsets, as `vk_task_texts_pack` copies them and `vk_b64_decode_device` reads them"""
    fields, at = [], 0
    for t in texts:
        nsig = _b64_nsig(t)
        fields.append((t, nsig, at))
        at += -(-nsig // 16) * 16
    return fields, at


_as_utf8 = C.pythonapi.PyUnicode_AsUTF8AndSize          # the str's own buffer for an ASCII str (CPython keeps UTF-8 == the compact ASCII data)
_as_utf8.argtypes, _as_utf8.restype = [C.py_object, C.POINTER(C.c_ssize_t)], C.c_void_p


def _text_address(text):
    """(address of the field's bytes, the object that keeps them alive).  A `str` is read in place -- no `encode` copy -- when it is ASCII;
    anything else takes the `encode("ascii")` of the host path, with its exception."""
    if isinstance(text, str):
        size = C.c_ssize_t()
        p = _as_utf8(text, C.byref(size))
        if p and size.value == len(text):
            return p, text
        text = text.encode("ascii")
    else:
        text = bytes(text)
    return C.cast(C.c_char_p(text), C.c_void_p).value, text


class _ResidentPool:
    """Bookkeeping of the device-resident image store of `TaskLoader(resident_bytes > 0)`: a bump allocator over `capacity` bytes of ONE device
    tensor (16-byte aligned offsets, no eviction, no free) and the dictionary image id -> (feat_off, box_off, mean_off, n, w, h).  An image
    occupies one stretch: features [n, F] | global row [F] | boxes [n, 4], fp32.  Offsets are reserved while a batch is put together and
    committed to the dictionary only after its decode came back clean; `rollback(mark)` gives the stretches of a failed batch back.  All
    reservations, commits and rollbacks come from the consumer's thread, one batch after the other; the prefetch thread only reads the
    dictionary, under the lock."""

    ALIGN = 16

    def __init__(self, capacity):
        self.capacity, self.used, self.items, self.lock = int(capacity), 0, {}, threading.Lock()

    @staticmethod
    def layout(at, n, F):
        """(feat_off, box_off, mean_off, bytes) of an image of n regions placed at byte `at`"""
        feat, mean = n * F * 4, F * 4
        return at, at + feat + mean, at + feat, feat + mean + n * 16

    def reserve(self, nbytes):
        """offset of `nbytes` fresh bytes, or None when the pool cannot hold them"""
        at = -(-self.used // self.ALIGN) * self.ALIGN
        if at + nbytes > self.capacity:
            return None
        self.used = at + nbytes
        return at

    def mark(self):
        return self.used

    def rollback(self, mark):
        assert 0 <= mark <= self.used
        self.used = mark

    def get(self, image_id):
        with self.lock:
            return self.items.get(image_id)

    def commit(self, entries):
        with self.lock:
            self.items.update(entries)

    def __len__(self):
        with self.lock:
            return len(self.items)


class ImageStager:
    """The batch form of `ImageFeaturesH5Reader.__getitem__`: for a list of distinct image ids, the records are looked up in the LMDB mapping
    and unpickled in Python, then ONE native call (`vk_task_images_stage`, GIL released, up to `threads` host threads, never more than 16)
    base64-decodes every `features` / `boxes` field straight into its slot of pinned staging arrays feat [S, Rcap, F] / boxes [S, Rcap, 4];
    n [S] and wh [S, 2] (width, height) come with them.  Rows >= n are not initialised and not read by `vk_task_batch`.  `in_memory=True`
    decodes into a pinned pool keyed by image id instead (at most `pool_bytes`; `pool_bytes_used` reports it), so a later call for the same
    id neither looks up nor decodes.  `sets` staging sets rotate (`which`)."""

    def __init__(self, reader, threads=None, in_memory=False, pool_bytes=8 << 30, sets=1, pin_memory=None):
        cpus = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        self.threads = max(1, min(16, int(threads) if threads else cpus))
        self.reader, self.F = reader, int(reader.feature_size)
        self._pin = torch.cuda.is_available() if pin_memory is None else pin_memory
        self._pool = _PinnedPool(pool_bytes, self._pin) if in_memory else None
        self._sets = [None] * max(1, int(sets))

    @property
    def pool_bytes_used(self):
        return self._pool.bytes if self._pool else 0

    def _record(self, image_id):
        """(features text, boxes text, h, w) of one image: the lookup of ImageFeaturesH5Reader.__getitem__ (same exceptions) without its decode"""
        key = str(image_id).encode()
        if key not in self.reader._index:
            raise ValueError("%r is not in list" % key)
        raw = self.reader.env.get(key)
        if raw is None:
            raise KeyError(key)
        item = pickle.loads(raw)
        return item["features"], item["boxes"], int(item["img_h"]), int(item["img_w"])

    def _staging(self, which, S, Rcap):
        s = self._sets[which]
        if s is None or s["feat"].shape[0] < S or s["feat"].shape[1] < Rcap:
            S, Rcap = max(S, s["feat"].shape[0] if s else 0), max(Rcap, s["feat"].shape[1] if s else 0)
            s = self._sets[which] = dict(feat=torch.empty(S, Rcap, self.F, dtype=torch.float32, pin_memory=self._pin),
                                         boxes=torch.empty(S, Rcap, 4, dtype=torch.float32, pin_memory=self._pin))
        return s

    def stage(self, order, which=0):
        """order: distinct image ids -> dict(S, Rcap, n, wh, src = per slot the (features [n, F], boxes [n, 4]) host views, stage = the staging
        set, staged_all = every image sits in the staging set)"""
        S = len(order)
        n, wh = np.zeros(S, np.int32), np.zeros((S, 2), np.int32)
        fresh, texts = [], {}
        for s, iid in enumerate(order):
            hit = self._pool.items.get(iid) if self._pool else None
            if hit is not None:
                n[s], wh[s] = hit[0].shape[0], hit[2]
                continue
            ft, bt, h, w = self._record(iid)
            ft = ft.encode("ascii") if isinstance(ft, str) else bytes(ft)
            bt = bt.encode("ascii") if isinstance(bt, str) else bytes(bt)
            rows = _b64_rows(bt, 16)
            if _b64_rows(ft, 4 * self.F) != rows:
                raise ValueError("image %r: %d feature rows, %d boxes" % (iid, _b64_rows(ft, 4 * self.F), rows))
            n[s], wh[s] = rows, (w, h)
            texts[s] = (ft, bt)
            fresh.append(s)
        Rcap = max(1, int(n.max()) if S else 1)
        stage = self._staging(which, max(S, 1), Rcap)
        src = [None] * S
        jobs = (L.TaskImage * max(len(fresh), 1))()
        for j, s in enumerate(fresh):
            rows = int(n[s])
            f = b = None
            if self._pool is not None:
                mem = self._pool.alloc(rows * (self.F + 4))
                if mem is not None:
                    f, b = mem[:rows * self.F].view(rows, self.F), mem[rows * self.F:].view(rows, 4)
                    self._pool.items[order[s]] = (f, b, (int(wh[s, 0]), int(wh[s, 1])))
            if f is None:
                f, b = stage["feat"][s, :rows], stage["boxes"][s, :rows]
            src[s] = (f, b)
            ft, bt = texts[s]
            jobs[j] = L.TaskImage(C.cast(C.c_char_p(ft), C.c_void_p), len(ft), C.cast(C.c_char_p(bt), C.c_void_p), len(bt),
                                  C.c_void_p(f.data_ptr()), C.c_void_p(b.data_ptr()), rows, self.F)
        if fresh:
            L.check(L.lib.vk_task_images_stage(jobs, len(fresh), self.threads, None))
        for s, iid in enumerate(order):
            if src[s] is None:
                src[s] = self._pool.items[iid][:2]
        return dict(S=S, Rcap=Rcap, n=n, wh=wh, src=src, stage=stage, staged_all=self._pool is None)


class TaskLoader:
    """Batches of a task dataset, assembled on the device.  Iterating yields what `default_collate` of the dataset's per-sample tuples gives
    after the drivers' `.cuda(non_blocking=True)`: (features, spatials, image_mask, question, target, input_mask, segment_ids, question_id),
    same order, shapes and dtypes, so the `_Batch` of volta_amd.task_utils takes it unchanged.

    Mechanics (as ConceptCapLoaderTrain): `prefetch` batches are staged ahead by a background thread -- for the image ids of a batch ONE
    native call decodes every base64 field into pinned staging (ImageStager: up to `threads` host threads, default min(16, cpu count), never
    more, GIL released) -- `prefetch + 2` staging sets rotate, copies and `vk_task_batch` run on the loader's own stream, and the tensors handed
    out are recorded on the consumer's stream.  `in_memory=True` decodes into a pinned pool keyed by image id instead (at most `pool_bytes`,
    `pool_bytes_used` reports it), so later epochs neither look up nor decode.

    `resident_bytes > 0` keeps the images on the device instead: ONE device tensor of that many bytes is the resident pool.  The prefetch
    thread looks up and unpickles only the images that are not resident yet and copies their two base64 text fields into a pinned text arena
    (`vk_task_texts_pack`, no decode on the host); on the loader's stream one H2D copy of that arena, `vk_b64_decode_device` (straight into
    the pool while the image fits, else into a scratch tensor of the staging set), `vk_task_pool_means` for the new images and
    `vk_task_batch_pool` follow.  An image enters the pool's dictionary only after its decode's status words came back clean; a flagged job
    (whitespace in the text, a corrupt record) sends the whole batch through the host path above, with nothing of it kept.  From the second
    epoch on the host contributes the small integer tables and nothing else.  There is no eviction; `resident_bytes_used`,
    `resident_images` and `stats` (decoded_images, resident_hits, scratch_images, host_fallback_batches) report what happened.  Outputs are
    bit for bit those of the default path.  Not combinable with `in_memory`.

    `sampler`: anything iterable over indices with `len` (SequentialSampler / RandomSampler / DistributedSampler above; torch's work too);
    None = sequential."""

    def __init__(self, dataset, batch_size, sampler=None, drop_last=False, device="cuda", prefetch=2, threads=None, in_memory=False,
                 pool_bytes=8 << 30, resident_bytes=0):
        resident_bytes = int(resident_bytes)
        if resident_bytes < 0:
            raise ValueError("resident_bytes = %d: the size of the device-resident image pool in bytes, 0 = none" % resident_bytes)
        if resident_bytes and in_memory:
            raise ValueError("resident_bytes > 0 keeps the images on the device; in_memory=True keeps them in pinned host memory: choose one")
        self.dataset, self.batch_size, self.drop_last, self.device = dataset, int(batch_size), bool(drop_last), device
        self.sampler = sampler if sampler is not None else SequentialSampler(len(dataset))
        self.prefetch = max(0, int(prefetch))
        self.stager = ImageStager(dataset._image_features_reader, threads, in_memory, pool_bytes, sets=self.prefetch + 2)
        self.threads = self.stager.threads
        self._stream = None
        self._text_dev = None
        self.resident_bytes = resident_bytes
        self._resident = _ResidentPool(resident_bytes) if resident_bytes else None
        self._pool_dev = None                # the resident pool: one uint8 device tensor, allocated at first use
        self._arenas = [None] * (self.prefetch + 2)     # pinned text arenas, one per staging set
        self._scratch = [None] * (self.prefetch + 2)    # device scratch for images the pool cannot hold, one per staging set
        self.stats = dict(decoded_images=0, resident_hits=0, scratch_images=0, host_fallback_batches=0)

    def __len__(self):
        n = len(self.sampler)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    @property
    def pool_bytes_used(self):
        return self.stager.pool_bytes_used

    @property
    def resident_bytes_used(self):
        return self._resident.used if self._resident is not None else 0

    @property
    def resident_images(self):
        return len(self._resident) if self._resident is not None else 0

    # ---- host side (prefetch thread)
    def _batch_images(self, indices):
        """per sample its image ids, the text rows of the batch, and the slot of every distinct image id"""
        ds = self.dataset
        per_sample, text_rows = [], []
        for i in indices:                    # a dataset with random negatives draws them in images(); text_rows() refers to that draw
            per_sample.append(ds.images(i))
            text_rows += ds.text_rows(i)
        slot_of = {}
        for ids in per_sample:
            for iid in ids:
                slot_of.setdefault(iid, len(slot_of))
        return per_sample, text_rows, slot_of

    def _stage(self, indices, which):
        """Everything of one batch that the host contributes: decoded images (staging set `which` or the pool) and the small integer tables."""
        per_sample, text_rows, slot_of = self._batch_images(indices)
        h = self.stager.stage(list(slot_of), which)
        return self._tables(h, indices, per_sample, text_rows, slot_of)

    def _stage_resident(self, indices, which):
        """`_stage` of the device-resident path: nothing for an image the pool holds; for the others the record lookup and, in one native call,
        their text fields packed into the pinned text arena of staging set `which`.  Where the images go is decided in `_produce`."""
        per_sample, text_rows, slot_of = self._batch_images(indices)
        order, F = list(slot_of), self.stager.F
        S = len(order)
        n, wh = np.zeros(S, np.int32), np.zeros((S, 2), np.int32)
        known, fresh, texts = {}, [], []
        for s, iid in enumerate(order):
            e = self._resident.get(iid)
            if e is not None:
                n[s], wh[s], known[s] = e[3], (e[4], e[5]), e
                continue
            ft, bt, h, w = self.stager._record(iid)
            rows = _b64_rows(bt, 16)
            if _b64_rows(ft, 4 * F) != rows:
                raise ValueError("image %r: %d feature rows, %d boxes" % (iid, _b64_rows(ft, 4 * F), rows))
            n[s], wh[s] = rows, (w, h)
            fresh.append(s)
            texts += [ft, bt]
        fields, arena_bytes = _text_layout(texts)
        arena = self._arenas[which]
        if arena is None or arena.numel() < arena_bytes:
            arena = self._arenas[which] = torch.empty(max(arena_bytes, 16), dtype=torch.uint8, pin_memory=self.stager._pin)
        jobs, alive = (L.TaskText * max(len(fields), 1))(), []
        for j, (t, nsig, at) in enumerate(fields):
            p, keep = _text_address(t)
            alive.append(keep)
            jobs[j] = L.TaskText(p, nsig, at)
        if fields:
            L.check(L.lib.vk_task_texts_pack(jobs, len(fields), C.c_void_p(arena.data_ptr()), arena.numel(), self.threads))
        h = dict(S=S, n=n, wh=wh, order=order, known=known, fresh=fresh, fields=[(nsig, at) for _, nsig, at in fields], arena=arena,
                 arena_bytes=arena_bytes, which=which, resident=True)
        return self._tables(h, indices, per_sample, text_rows, slot_of)

    def _tables(self, h, indices, per_sample, text_rows, slot_of):
        """the small integer tables of a batch, added to `h` (which holds n and wh of the staged images) and packed into one pinned buffer"""
        ds = self.dataset
        nl = h["n"] + (1 if ds._add_global_imgfeat is not None else 0)
        segs, counts = [], []
        for i, ids in zip(indices, per_sample):
            slots = [slot_of[iid] for iid in ids]
            for seg_list, count in ds.blocks(i, [int(nl[s]) for s in slots]):
                rows = [(slots[k], a, b, c) for k, a, b, c in seg_list]
                assert len(rows) <= L.TASK_MAX_SEGS
                segs.append(rows + [(0, 0, 0, 0)] * (L.TASK_MAX_SEGS - len(rows)))
                counts.append(count)
        idx = np.asarray(indices, np.int64)
        lo, hi = ds._csr[idx], ds._csr[idx + 1]
        take = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)] + [np.zeros(0, np.int64)]).astype(np.int64)
        csr = np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.int32)
        ref_box = np.stack([ds.ref_box(i) for i in indices]) if ds.target_kind == "iou" else np.zeros((0, 4), np.float32)
        h.update(indices=idx, text_rows=np.asarray(text_rows, np.int64), ids=np.asarray([ds.sample_id(i) for i in indices], np.int64),
                 segs=np.asarray(segs, np.int32).reshape(-1, L.TASK_MAX_SEGS, 4), counts=np.asarray(counts, np.int32), csr=csr,
                 labels=ds._labels[take], scores=ds._scores[take], ref_box=ref_box.astype(np.float32))
        # the small tables travel as ONE pinned buffer (int64 tables first, so their views stay 8-byte aligned)
        parts = [(k, np.ascontiguousarray(h[k])) for k in self._TABLES]
        words = [a.view(np.int32).reshape(-1) for _, a in parts]
        packed = torch.empty(max(1, sum(w.size for w in words)), dtype=torch.int32, pin_memory=self.stager._pin)
        layout, at = {}, 0
        for (k, a), w in zip(parts, words):
            packed.numpy()[at:at + w.size] = w
            layout[k] = (at, w.size, a.dtype, a.shape)
            at += w.size
        h["packed"], h["layout"] = packed, layout
        return h

    # ---- device side
    _TABLES = ("text_rows", "ids", "n", "wh", "segs", "counts", "csr", "labels", "scores", "ref_box")
    _TORCH = {np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32}

    def _device_tables(self, h):
        packed = h["packed"].to(self.device, non_blocking=True)

        def table(k):
            at, size, dt, shape = h["layout"][k]
            return packed[at:at + size].view(self._TORCH[np.dtype(dt)]).view(shape)

        return table

    def _target_args(self, table):
        ds = self.dataset
        if ds.target_kind == "scatter":
            return dict(scatter=(table("csr"), table("labels"), table("scores"), ds.num_labels))
        if ds.target_kind == "iou":
            return dict(ref_box=table("ref_box"))
        return {}

    def _assemble_resident(self, h):
        """The device half of the resident path, on the loader's stream: where every image of the batch lives (pool, or this staging set's
        scratch), one H2D copy of the text arena, the decode, the global rows of the new images, the batch.  Leaves in `h` what `_produce`
        needs once the stream has been synchronised: the status words (pinned), the pool mark, the entries to commit."""
        from . import ops
        ds, dev, pool, F = self.dataset, self.device, self._resident, self.stager.F
        S, n, order = h["S"], h["n"], h["order"]
        if self._pool_dev is None:
            self._pool_dev = torch.empty(self.resident_bytes, dtype=torch.uint8, device=dev)
        h["mark"] = pool.mark()
        where, offs = np.zeros(max(S, 1), np.int32), np.zeros((3, max(S, 1)), np.int64)     # offs: feat_off, box_off, mean_off
        for s, e in h["known"].items():
            offs[:, s] = e[:3]
        jobs, entries, scratch_at = ([], []), {}, 0
        for k, s in enumerate(h["fresh"]):
            rows = int(n[s])
            size = _ResidentPool.layout(0, rows, F)[3]
            at = pool.reserve(size) if pool.get(order[s]) is None else None      # staged a second time by an earlier batch: decode into scratch
            w = 0 if at is not None else 1
            if at is None:
                at, scratch_at = scratch_at, scratch_at + size
            fo, bo, mo, _ = _ResidentPool.layout(at, rows, F)
            if w == 0:
                entries[order[s]] = (fo, bo, mo, rows, int(h["wh"][s, 0]), int(h["wh"][s, 1]))
            where[s], offs[:, s] = w, (fo, bo, mo)
            (nsig_f, at_f), (nsig_b, at_b) = h["fields"][2 * k], h["fields"][2 * k + 1]
            jobs[w].extend([(at_f, fo, nsig_f, rows * F * 4), (at_b, bo, nsig_b, rows * 16)])
        h["entries"], h["scratch_images"] = entries, len(jobs[1]) // 2
        scratch = self._scratch[h["which"]]
        if scratch_at and (scratch is None or scratch.numel() < scratch_at):
            scratch = self._scratch[h["which"]] = torch.empty(scratch_at, dtype=torch.uint8, device=dev)
        regions = (self._pool_dev, scratch)
        # the tables of this half travel as one buffer as well: int64 offsets first, then the 24-byte job records, then the int32 lists
        tabs = [ops.b64_jobs(j) for j in jobs]
        parts = [offs.view(np.int32).reshape(-1)] + [t.numpy().reshape(-1) for t, _ in tabs] + [where, np.asarray(h["fresh"], np.int32)]
        small = torch.from_numpy(np.concatenate(parts)).to(dev)
        cuts = np.cumsum([0] + [p.size for p in parts])
        part = lambda i: small[cuts[i]:cuts[i + 1]]
        offs_d = part(0).view(torch.int64).view(3, -1)
        where_d, fresh_d = part(3), part(4)
        statuses = []
        if h["fresh"]:
            text = h["arena"][:max(h["arena_bytes"], 1)].to(dev, non_blocking=True)
            for w in (0, 1):
                if jobs[w]:
                    statuses.append(ops.b64_decode_device(text, regions[w], part(1 + w).view(-1, 6), tabs[w][1]))
        status = torch.cat(statuses) if statuses else torch.zeros(0, dtype=torch.int32, device=dev)
        h["status"] = torch.empty(status.numel(), dtype=torch.int32, pin_memory=self.stager._pin)
        h["status"].copy_(status, non_blocking=True)
        table = self._device_tables(h)
        n_d, wh_d = table("n"), table("wh")
        if S == 0:
            n_d, wh_d = torch.zeros(1, dtype=torch.int32, device=dev), torch.ones(1, 2, dtype=torch.int32, device=dev)
        slots = (regions, where_d, offs_d[0], offs_d[1], offs_d[2], n_d, wh_d, F)
        if ds._add_global_imgfeat is not None and h["fresh"]:
            ops.task_pool_means(*slots, fresh_d)
        out = ops.task_batch_pool(*slots, table("segs"), table("counts"), ds.block_rows, ds._num_locs, ds._add_global_imgfeat, **self._target_args(table))
        return self._finish(h, table, out)

    def _assemble(self, h):
        from . import ops
        ds, dev = self.dataset, self.device
        table = self._device_tables(h)
        S = h["S"]
        if h["staged_all"]:                  # one copy per array, at the staging set's own width (rows >= n are never read)
            feat, boxes = (h["stage"][k][:max(S, 1)].to(dev, non_blocking=True) for k in ("feat", "boxes"))
        else:                                # pooled images: one copy per image, straight from the pinned pool
            Rcap = h["Rcap"]
            feat = torch.empty(max(S, 1), Rcap, self.stager.F, dtype=torch.float32, device=dev)
            boxes = torch.empty(max(S, 1), Rcap, 4, dtype=torch.float32, device=dev)
            for s, (f, b) in enumerate(h["src"]):
                feat[s, :f.shape[0]].copy_(f, non_blocking=True)
                boxes[s, :b.shape[0]].copy_(b, non_blocking=True)
        n, wh = table("n"), table("wh")
        if S == 0:
            n, wh = torch.zeros(1, dtype=torch.int32, device=dev), torch.ones(1, 2, dtype=torch.int32, device=dev)
        out = ops.task_batch(feat, boxes, n, wh, table("segs"), table("counts"), ds.block_rows, ds._num_locs, ds._add_global_imgfeat,
                             **self._target_args(table))
        return self._finish(h, table, out)

    def _finish(self, h, table, out):
        """the assembled image tensors joined with the text rows, the target and the ids: the batch tuple"""
        ds, dev = self.dataset, self.device
        if self._text_dev is None:
            self._text_dev = tuple(torch.from_numpy(t).to(dev) for t in ds._text)
        tok, im, seg = (t.index_select(0, table("text_rows")) for t in self._text_dev)
        B, k = len(h["indices"]), ds.options
        images = (out["features"], out["spatials"], out["image_mask"])
        if k > 1:                            # default_collate of [options, ...] samples: [B, options, ...]
            images = tuple(t.view(B, k, *t.shape[1:]) for t in images)
            tok, im, seg = (t.view(B, k, t.shape[1]) for t in (tok, im, seg))
        target = out["target"] if "target" in out else torch.zeros(B, dtype=torch.int64, device=dev)
        return images + (tok, target, im, seg, table("ids").clone())

    def _produce(self, h):
        on_gpu = torch.cuda.is_available() and str(self.device).startswith("cuda")
        if not on_gpu:
            raise RuntimeError("TaskLoader assembles its batches with vk_task_batch on an MI355X; there is no host path (iterate the dataset "
                               "with a torch DataLoader for that)")
        if self._stream is None:
            self._stream = torch.cuda.Stream()
        with torch.cuda.stream(self._stream):
            batch = self._assemble_resident(h) if h.get("resident") else self._assemble(h)
        self._stream.synchronize()          # the staging set is rewritten prefetch + 2 batches later; the host waits for THIS stream only
        if h.get("resident"):
            batch = self._settle_resident(h, batch)
        user = torch.cuda.current_stream()
        for t in batch:
            t.record_stream(user)
        return batch

    def _settle_resident(self, h, batch):
        """After the synchronisation: a clean decode commits the batch's new images to the pool's dictionary; a flagged job gives their
        stretches back and redoes the whole batch on the host path (same images, same tables), which produces it or raises its own message."""
        if not h["status"].numpy().any():
            self._resident.commit(h["entries"])
            self.stats["decoded_images"] += len(h["fresh"])
            self.stats["resident_hits"] += len(h["known"])
            self.stats["scratch_images"] += h["scratch_images"]
            return batch
        self._resident.rollback(h["mark"])
        self.stats["host_fallback_batches"] += 1
        hs = self.stager.stage(h["order"], h["which"])
        assert np.array_equal(hs["n"], h["n"]) and np.array_equal(hs["wh"], h["wh"])
        h.update(Rcap=hs["Rcap"], src=hs["src"], stage=hs["stage"], staged_all=hs["staged_all"])
        with torch.cuda.stream(self._stream):
            batch = self._assemble(h)
        self._stream.synchronize()
        return batch

    def _index_batches(self):
        cur = []
        for i in self.sampler:
            cur.append(int(i))
            if len(cur) == self.batch_size:
                yield cur
                cur = []
        if cur and not self.drop_last:
            yield cur

    def _staged_batches(self):
        nsets = len(self.stager._sets)
        stage = self._stage_resident if self._resident is not None else self._stage
        if not self.prefetch:
            for k, idx in enumerate(self._index_batches()):
                yield stage(idx, k % nsets)
            return
        q, stop = queue.Queue(maxsize=self.prefetch), threading.Event()

        def put(x):
            while not stop.is_set():
                try:
                    q.put(x, timeout=0.1)
                    return True
                except queue.Full:
                    pass
            return False

        def fill():
            try:
                for k, idx in enumerate(self._index_batches()):
                    if not put(stage(idx, k % nsets)):
                        return
                put(None)
            except BaseException as e:      # handed to the consumer, raised there
                put(e)

        th = threading.Thread(target=fill, daemon=True)
        th.start()
        try:
            while True:
                h = q.get()
                if h is None:
                    return
                if isinstance(h, BaseException):
                    raise h
                yield h
        finally:
            stop.set()
            th.join()

    def __iter__(self):
        for h in self._staged_batches():
            yield self._produce(h)
