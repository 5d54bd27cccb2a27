"""Rebuilds the synthetic feature store of tests/golden/hard_pool_reference.npz (tools/make_hard_pool_golden.py) in a directory: an LMDB file
written by tests/lmdb_writer.py, Flickr30k- and COCO-style annotation files over the golden image list, a vocab.txt.  Shared by the CPU and
GPU tests of the hard-negative pool."""
import base64
import json
import os
import pickle
import types

import numpy as np

from tests.lmdb_writer import write_lmdb

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hard_pool_reference.npz")
TASKS = {"RetrievalFlickr30k": "flickr.jsonline", "RetrievalCOCO": "coco.jsonline"}
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "a", "photo", "of", "scene", "number"] + [str(i) for i in range(10)]


class WordTokenizer:
    def __init__(self, vocab):
        self.vocab = {w: i for i, w in enumerate(vocab)}

    def encode(self, text):
        return [self.vocab.get(w, self.vocab["[UNK]"]) for w in text.lower().split()]

    def convert_tokens_to_ids(self, tokens):
        return [self.vocab.get(t, self.vocab["[UNK]"]) for t in tokens]


def golden():
    z = np.load(GOLD)
    return {k: z[k] for k in z.files}


class PoolFixture:
    def __init__(self, root):
        self.root, self.z = str(root), golden()
        z = self.z
        self.N, self.F = len(z["image_list"]), z["features"].shape[1]
        self.image_list = [int(v) for v in z["image_list"]]
        ends = np.cumsum(z["num_boxes"])
        self.regions = {iid: z["features"][e - n:e] for iid, e, n in zip(self.image_list, ends, z["num_boxes"])}
        rng = np.random.default_rng(5)
        recs = {}
        for iid in self.image_list:
            f = self.regions[iid]
            n = f.shape[0]
            xy = rng.uniform(0, 200, (n, 2)).astype(np.float32)
            boxes = np.concatenate([xy, xy + rng.uniform(10, 100, (n, 2)).astype(np.float32)], 1)
            recs[str(iid).encode()] = pickle.dumps(dict(img_id=str(iid), img_h=400, img_w=320, num_boxes=n, boxes=base64.b64encode(boxes.tobytes()).decode(),
                                                        features=base64.b64encode(np.ascontiguousarray(f).tobytes()).decode()))
        recs[b"keys"] = pickle.dumps([str(i).encode() for i in self.image_list])
        self.store = os.path.join(self.root, "features.lmdb")
        write_lmdb(self.store, recs)
        for task, name in TASKS.items():
            with open(os.path.join(self.root, name), "w") as f:
                for pos, iid in enumerate(self.image_list):
                    sentences = ["a photo of scene number %s" % " ".join(str(iid)), "scene %s" % " ".join(str(pos))]
                    ann = dict(img_path="%d.jpg" % iid, sentences=sentences) if task == "RetrievalFlickr30k" else dict(id=iid, sentences=sentences)
                    f.write(json.dumps(ann) + "\n")

    def jsonpath(self, task):
        return os.path.join(self.root, TASKS[task])

    def reader(self, add_global_imgfeat="first"):
        from volta_amd.readers import ImageFeaturesH5Reader
        cfg = types.SimpleNamespace(v_feature_size=self.F, num_locs=5, add_global_imgfeat=add_global_imgfeat)
        return ImageFeaturesH5Reader(self.store, cfg, False)
