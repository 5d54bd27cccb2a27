"""Rebuilds the inputs of tests/golden/retrieval_eval_reference.npz (recorded by tools/make_retrieval_eval_golden.py from the reference's
RetrievalDatasetVal) in a directory: both annotation files byte for byte, the feature store as an LMDB file written by tests/lmdb_writer.py, a
vocab.txt.  Shared by the CPU and GPU tests of the retrieval evaluation."""
import base64
import json
import os
import pickle
import types

import numpy as np

from tests.lmdb_writer import write_lmdb
from tests.task_data_fixture import WordTokenizer

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "retrieval_eval_reference.npz")
F = 2048
CASES = ["flickr_plain", "flickr_first_cut", "flickr_last_cut", "coco_last", "coco_none_cut", "coco_first"]


class EvalFixture:
    def __init__(self, root):
        self.z = np.load(GOLD)
        self.root = str(root)
        self.cases = json.loads(str(self.z["cases_json"]))
        self.vocab = json.loads(str(self.z["vocab_json"]))
        self.image_keys = json.loads(str(self.z["image_keys_json"]))
        for name in self.z.files:
            if name.startswith("file::"):
                with open(os.path.join(self.root, name[6:]), "wb") as f:
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

    def jsonpath(self, kind):
        return os.path.join(self.root, "%s_test.jsonline" % ("coco" if kind == "RetrievalCOCO" else "flickr"))

    def reader(self, case):
        from volta_amd.readers import ImageFeaturesH5Reader
        kw = self.cases[case][1]
        return ImageFeaturesH5Reader(self.store, types.SimpleNamespace(v_feature_size=F, num_locs=kw["num_locs"], add_global_imgfeat=kw["add_global_imgfeat"]))

    def dataset(self, case, tokenizer="words", **extra):
        from volta_amd import datasets as D
        kind, kw = self.cases[case]
        return D.RetrievalEvalMap[kind](task=kind, dataroot=self.root, annotations_jsonpath=self.jsonpath(kind), image_features_reader=self.reader(case),
                                        gt_image_features_reader=None, tokenizer=self.tokenizer(tokenizer), bert_model="bert-base-uncased", padding_index=0,
                                        **kw, **extra)

    def arrays(self, case):
        """the reference's features_all, spatials_all, image_mask_all and their torch dtype names"""
        keys = ("features_all", "spatials_all", "image_mask_all")
        return [self.z["%s::%s" % (case, k)] for k in keys], [str(self.z["%s::%s::dtype" % (case, k)]) for k in keys]
