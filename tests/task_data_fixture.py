"""Rebuilds the synthetic dataroot of tests/golden/task_data_reference.npz (recorded by tools/make_task_data_golden.py from the reference's own
dataset classes) in a directory: the annotation files byte for byte, the feature store as an LMDB file written by tests/lmdb_writer.py, a
vocab.txt.  Shared by the CPU and GPU tests of volta_amd.datasets."""
import base64
import json
import os
import pickle
import types

import numpy as np

from tests.lmdb_writer import write_lmdb

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "task_data_reference.npz")
SUBDIR = {"VQA": "", "GQA": "gqa", "NLVR2": "nlvr2", "refcoco": "refer", "refcoco+": "refer", "refcocog": "refer", "RetrievalCOCO": "retrieval",
          "RetrievalFlickr30k": "retrieval"}
JSONPATH = {"RetrievalCOCO": "retrieval/coco.jsonline", "RetrievalFlickr30k": "retrieval/flickr.jsonline"}
F = 2048


class WordTokenizer:
    """the stand-in the fixture was recorded with: lower-case words looked up in the vocabulary"""

    def __init__(self, vocab):
        self.vocab = {w: i for i, w in enumerate(vocab)}

    def encode(self, text):
        return [self.vocab.get(w, self.vocab["[UNK]"]) for w in text.lower().split()]

    def convert_tokens_to_ids(self, tokens):
        return [self.vocab.get(t, self.vocab["[UNK]"]) for t in tokens]


class Fixture:
    def __init__(self, root):
        self.z = np.load(GOLD)
        self.root = str(root)
        self.cases = json.loads(str(self.z["cases_json"]))
        self.vocab = json.loads(str(self.z["vocab_json"]))
        self.image_keys = json.loads(str(self.z["image_keys_json"]))
        for name in self.z.files:
            if name.startswith("file::"):
                path = os.path.join(self.root, name[6:])
                os.makedirs(os.path.dirname(path), exist_ok=True)
                with open(path, "wb") as f:
                    f.write(self.z[name].tobytes())
        recs = {}
        for key in self.image_keys:
            h, w = (int(v) for v in self.z["img::%s::hw" % key])
            boxes, feats = self.z["img::%s::boxes" % key], self.z["img::%s::features" % key]
            recs[key.encode()] = pickle.dumps(dict(img_id=key, img_h=h, img_w=w, num_boxes=boxes.shape[0], boxes=base64.b64encode(boxes.tobytes()).decode(),
                                                   features=base64.b64encode(feats.tobytes()).decode()))
        recs[b"keys"] = pickle.dumps([k.encode() for k in self.image_keys])
        self.store = os.path.join(self.root, "features.lmdb")
        write_lmdb(self.store, recs)
        self.vocab_file = os.path.join(self.root, "vocab.txt")
        with open(self.vocab_file, "w") as f:
            f.write("\n".join(self.vocab) + "\n")

    def tokenizer(self, kind="words"):
        from volta_amd.readers import WordPieceTokenizer
        return WordTokenizer(self.vocab) if kind == "words" else WordPieceTokenizer(self.vocab_file)

    def reader(self, case, in_memory=False):
        from volta_amd.readers import ImageFeaturesH5Reader
        kw = self.cases[case][1]
        cfg = types.SimpleNamespace(v_feature_size=F, num_locs=kw["num_locs"], add_global_imgfeat=kw["add_global_imgfeat"])
        return ImageFeaturesH5Reader(self.store, cfg, in_memory)

    def dataroot(self, kind):
        return os.path.join(self.root, SUBDIR[kind])

    def jsonpath(self, kind):
        return os.path.join(self.root, JSONPATH[kind]) if kind in JSONPATH else ""

    def negatives(self, case):
        """the reference's recorded draws of a retrieval case, as the `negatives=` hook of RetrievalDataset takes them"""
        return lambda i: tuple(int(v) for v in self.z["%s::%d::negatives" % (case, i)])

    def dataset(self, case, tokenizer="words", reader=None, **extra):
        from volta_amd import datasets as D
        kind, kw = self.cases[case]
        if kind.startswith("Retrieval") and "negatives" not in extra and "seed" not in extra:
            extra["negatives"] = self.negatives(case)
        return D.DatasetMapTrain[kind](task=kind, dataroot=self.dataroot(kind), annotations_jsonpath=self.jsonpath(kind),
                                       image_features_reader=reader or self.reader(case), gt_image_features_reader=None, tokenizer=self.tokenizer(tokenizer),
                                       bert_model="bert-base-uncased", padding_index=0, **kw, **extra)

    def sample(self, case, i):
        """the reference's tuple of sample i: numpy arrays, and their torch dtype names (None for plain Python values)"""
        vals = [self.z["%s::%d::%d" % (case, i, j)] for j in range(8)]
        dtypes = [str(self.z["%s::%d::%d::dtype" % (case, i, j)]) if "%s::%d::%d::dtype" % (case, i, j) in self.z.files else None for j in range(8)]
        return vals, dtypes

    def length(self, case):
        return int(self.z["%s::len" % case])
