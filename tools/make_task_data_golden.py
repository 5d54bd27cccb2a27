"""Records tests/golden/task_data_reference.npz from the reference's own fine-tuning dataset classes (volta/datasets/vqa_dataset.py,
gqa_dataset.py, nlvr2_dataset.py, refer_expression_dataset.py, retrieval_dataset.py over _image_features_reader.py), loaded by file path and driven on the CPU:

  python tools/make_task_data_golden.py --reference /path/to/volta-checkout [--out tests/golden/task_data_reference.npz]

A tiny synthetic dataroot is written into a temporary directory: 10 images of 3 to 14 regions with 2048 features (values from a small set of
exactly representable numbers, so the compressed file stays small), the annotation files of each dataset in the reference's layout, and a
feature store of pickled records with base64 fields.  Stand-ins replace the modules this environment lacks: `lmdb` (a dict behind the
reference reader; tests rebuild the same records as an LMDB file with tests/lmdb_writer.py), `jsonlines`, `pytorch_transformers`, and the
plotting imports of tools/refer/refer.py (`skimage`, `matplotlib`, its compiled `mask` extension).  The retrieval dataset's random draws
(`random.choice`, `np.random.randint`) are recorded per sample as the three values a `negatives=` hook injects.  The
tokenizer is a whitespace / lower-case stand-in over a recorded vocabulary (texts are plain lower-case words, so BERT's WordPiece over the
same vocabulary gives the same ids).

Recorded: the inputs (image arrays, every annotation file as bytes, the vocabulary, each case's constructor arguments) and every tensor every
`__getitem__` returned, plus per image the float64 mean of its regions and the reference's fp32 global row.  Cases cover add_global_imgfeat in
{None, first, last}, num_locs in {4, 5}, max_region_num above and below the largest image (retrieval: above only -- the reference cannot
stack its option-3 mask otherwise), append_mask_sep, the NLVR2 overflow and the retrieval option-3 carry-over (n3 < n1); the generator
asserts that each of these occurs.  Values only; the tests never import the reference."""
import argparse
import base64
import contextlib
import importlib
import json
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import torch

F = 2048
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "what", "is", "the", "color", "of", "cat", "dog", "left", "right", "both", "images", "show",
         "a", "two", "how", "many", "are", "there", "on", "table", "red", "blue", "in", "one", "image", "and", "other", "sitting", "person"]
QUESTIONS = ["what is the color of the cat", "how many dog are there on the table", "is the cat left of the dog",
             "what is on the table in the image and what color is the other one sitting there right of the person",
             "is there a zebra", "what color is the table"]
SENTENCES = ["both images show a cat", "one image show two dog and the other image show a person sitting on the table left of a red cat",
             "there are two blue table in the left image", "a dog is sitting"]
VQA_IMAGES, NLVR_STEMS, RETRIEVAL_IMAGES = [11, 12, 13, 14, 15, 16], ["dev-1-0", "dev-2-3"], [11, 12, 13, 15]
REGIONS = {"11": 3, "12": 14, "13": 9, "14": 10, "15": 5, "16": 12, "dev-1-0-img0": 4, "dev-1-0-img1": 6, "dev-2-3-img0": 14, "dev-2-3-img1": 13}

# name -> (dataset, constructor arguments)
CASES = {
    "vqa_plain": ("VQA", dict(split="train", max_region_num=16, num_locs=5, add_global_imgfeat=None, append_mask_sep=False, max_seq_length=12)),
    "vqa_first_cut_sep": ("VQA", dict(split="val", max_region_num=8, num_locs=4, add_global_imgfeat="first", append_mask_sep=True, max_seq_length=12)),
    "vqa_last_cut": ("VQA", dict(split="minval", max_region_num=8, num_locs=5, add_global_imgfeat="last", append_mask_sep=False, max_seq_length=8)),
    "vqa_test": ("VQA", dict(split="test", max_region_num=16, num_locs=5, add_global_imgfeat="first", append_mask_sep=False, max_seq_length=12)),
    "gqa_last": ("GQA", dict(split="train", max_region_num=16, num_locs=4, add_global_imgfeat="last", append_mask_sep=True, max_seq_length=12)),
    "gqa_cut": ("GQA", dict(split="val", max_region_num=8, num_locs=5, add_global_imgfeat=None, append_mask_sep=False, max_seq_length=10)),
    "gqa_test": ("GQA", dict(split="test", max_region_num=8, num_locs=5, add_global_imgfeat="first", append_mask_sep=False, max_seq_length=10)),
    "nlvr_plain": ("NLVR2", dict(split="dev", max_region_num=16, num_locs=5, add_global_imgfeat=None, append_mask_sep=False, max_seq_length=12)),
    "nlvr_first_over": ("NLVR2", dict(split="train", max_region_num=6, num_locs=4, add_global_imgfeat="first", append_mask_sep=False, max_seq_length=12)),
    "refer_plain": ("refcoco", dict(split="train", max_region_num=16, num_locs=5, add_global_imgfeat=None, append_mask_sep=False, max_seq_length=10)),
    "refer_first_cut": ("refcoco+", dict(split="val", max_region_num=8, num_locs=4, add_global_imgfeat="first", append_mask_sep=False, max_seq_length=10)),
    "refer_last_cut_g": ("refcocog", dict(split="test", max_region_num=8, num_locs=5, add_global_imgfeat="last", append_mask_sep=False, max_seq_length=12)),
    "refer_testA": ("refcoco", dict(split="testA", max_region_num=16, num_locs=5, add_global_imgfeat="last", append_mask_sep=False, max_seq_length=10)),
    "retr_flickr_train": ("RetrievalFlickr30k", dict(split="train", max_region_num=15, num_locs=5, add_global_imgfeat="first", append_mask_sep=False, max_seq_length=12)),
    "retr_coco_val": ("RetrievalCOCO", dict(split="val", max_region_num=14, num_locs=4, add_global_imgfeat="last", append_mask_sep=False, max_seq_length=10)),
    "nlvr_last_over": ("NLVR2", dict(split="test", max_region_num=9, num_locs=5, add_global_imgfeat="last", append_mask_sep=False, max_seq_length=20)),
}


def make_images(seed=5):
    rng = np.random.default_rng(seed)
    images = {}
    for key, n in REGIONS.items():
        w, h = int(rng.integers(200, 640)), int(rng.integers(150, 480))
        xy = rng.uniform(0, 0.6, (n, 2)) * [w, h]
        wh = rng.uniform(0.1, 0.4, (n, 2)) * [w, h]
        boxes = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        feats = (rng.integers(0, 8, (n, F)) / 4.0).astype(np.float32)
        feats[rng.random((n, F)) < 0.88] = 0.0                           # ReLU-like sparsity, and a smaller file
        images[key] = dict(h=h, w=w, boxes=boxes, features=feats)
    return images


def store_records(images):
    """key -> pickled record, in the layout the reference's convert_*_lmdb.py writers emit"""
    recs = {}
    for key, im in images.items():
        recs[key.encode()] = pickle.dumps(dict(img_id=key, img_h=im["h"], img_w=im["w"], num_boxes=im["boxes"].shape[0],
                                               boxes=base64.b64encode(im["boxes"].tobytes()).decode(),
                                               features=base64.b64encode(im["features"].tobytes()).decode()))
    recs[b"keys"] = pickle.dumps([k.encode() for k in images])
    return recs


def write_dataroot(root):
    """annotation files of the three datasets; returns {relative path: bytes}"""
    rng = np.random.default_rng(9)
    files = {}
    ans = ["yes", "no", "red", "blue", "two", "table", "cat"]
    files["trainval_ans2label.pkl"] = pickle.dumps({a: i for i, a in enumerate(ans)})
    files["trainval_label2ans.pkl"] = pickle.dumps(ans)

    def soft(k):
        labels = sorted(int(x) for x in rng.choice(len(ans), size=k, replace=False))
        return labels, [float(x) for x in rng.choice([0.3, 0.6, 0.9, 1.0], size=k)]

    qid = 100
    for split, year in (("train", "train2014"), ("val", "val2014"), ("test", "test2015")):
        qs, targets = [], []
        for i, q in enumerate(QUESTIONS):
            qid += 7
            img = VQA_IMAGES[(i + len(split)) % len(VQA_IMAGES)]
            qs.append(dict(question_id=qid, image_id=img, question=q))
            labels, scores = soft(i % 4)                                 # 0 labels occurs: the reference stores None then
            targets.append(dict(question_id=qid, image_id=img, labels=labels, scores=scores))
        order = rng.permutation(len(qs))                                 # unsorted on disk: the loaders sort by question id
        files["v2_OpenEnded_mscoco_%s_questions.json" % year] = json.dumps(dict(questions=[qs[j] for j in order])).encode()
        if split != "test":
            files["cache/%s_target.pkl" % split] = pickle.dumps([targets[j] for j in rng.permutation(len(qs))])
    for split in ("train", "val"):
        items = []
        for i, q in enumerate(QUESTIONS[::-1]):
            qid += 3
            labels, scores = soft(1 + i % 2)
            items.append(dict(question_id=qid, image_id=str(VQA_IMAGES[(2 * i + 1) % len(VQA_IMAGES)]), question=q, labels=labels, scores=scores))
        files["gqa/%s_target.pkl" % split] = pickle.dumps(items)
    files["gqa/trainval_ans2label.pkl"], files["gqa/trainval_label2ans.pkl"] = files["trainval_ans2label.pkl"], files["trainval_label2ans.pkl"]
    files["gqa/testdev_balanced_questions.json"] = json.dumps({str(900 + i): dict(imageId=str(VQA_IMAGES[i % 6]), question=q) for i, q in enumerate(QUESTIONS[:4])}).encode()
    for split in ("train", "dev", "test"):
        lines = []
        for i, s in enumerate(SENTENCES):
            stem = NLVR_STEMS[(i + len(split)) % 2]
            lines.append(json.dumps(dict(identifier="%s-%d" % (stem, i), sentence=s, label="True" if (i + len(split)) % 3 else "False")))
        files["nlvr2/%s.json" % split] = ("\n".join(lines) + "\n").encode()
    # referring expressions: refs(unc|umd).p + instances.json under <dataroot>/<task>/, as tools/refer/refer.py reads them
    for task, by in (("refcoco", "unc"), ("refcoco+", "unc"), ("refcocog", "umd")):
        refs, anns = [], []
        splits = ["train", "val", "testA", "testB", "test", "train", "val", "testA"]
        for r in range(8):
            img = VQA_IMAGES[(r + len(task)) % len(VQA_IMAGES)]
            x, y = float(rng.integers(0, 120)) + 0.5 * (r % 2), float(rng.integers(0, 90)) + 0.25
            anns.append(dict(id=500 + r, image_id=img, category_id=1, bbox=[x, y, float(rng.integers(20, 200)) + 0.75, float(rng.integers(20, 150))]))
            sents = [dict(raw=QUESTIONS[(r + k) % len(QUESTIONS)], sent_id=10 * r + k, tokens=[]) for k in range(1 + r % 2)]
            refs.append(dict(ref_id=40 + r, ann_id=500 + r, category_id=1, image_id=img, split=splits[r], sentences=sents, sent_ids=[s_["sent_id"] for s_ in sents]))
        files["refer/%s/refs(%s).p" % (task, by)] = pickle.dumps(refs)
        files["refer/%s/instances.json" % task] = json.dumps(dict(images=[dict(id=i) for i in VQA_IMAGES], annotations=anns, categories=[dict(id=1, name="thing")])).encode()
    # retrieval: jsonlines annotations (COCO: `id`; Flickr30k: `img_path`) and the hard-negative pool of the train split
    for name, key in (("coco", "id"), ("flickr", "img_path")):
        lines = []
        for i, img in enumerate(RETRIEVAL_IMAGES):
            ann = dict(sentences=[SENTENCES[(i + k) % len(SENTENCES)] for k in range(1 + (i == 1))])
            ann[key] = img if key == "id" else "%d.jpg" % img
            lines.append(json.dumps(ann))
        files["retrieval/%s.jsonline" % name] = ("\n".join(lines) + "\n").encode()
    pool = np.stack([rng.permutation(len(RETRIEVAL_IMAGES)) for _ in RETRIEVAL_IMAGES])
    files["retrieval/hard_negative.pkl"] = pickle.dumps(dict(train_hard_pool=pool, train_image_list=list(RETRIEVAL_IMAGES)))
    for rel, data in files.items():
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(data)
    for sub in ("cache", "gqa/cache", "nlvr2/cache", "refer/cache"):                    # the reference writes its token caches here
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    return files


class WordTokenizer:
    """whitespace / lower-case stand-in with the three methods the reference datasets call (pytorch-transformers 1.1 names)"""

    def __init__(self, vocab):
        self.vocab = {w: i for i, w in enumerate(vocab)}

    def encode(self, text):
        return [self.vocab.get(w, self.vocab["[UNK]"]) for w in text.lower().split()]

    def add_special_tokens_single_sentence(self, tokens):
        return [self.vocab["[CLS]"]] + tokens + [self.vocab["[SEP]"]]

    def convert_tokens_to_ids(self, tokens):
        return [self.vocab.get(t, self.vocab["[UNK]"]) for t in tokens]


@contextlib.contextmanager
def reference_datasets(ref_root, store):
    """the reference's volta/datasets directory as a package that does not run its __init__ (which imports every dataset and their
    dependencies), with stand-ins for lmdb, jsonlines and pytorch_transformers"""
    class Txn:
        def __enter__(self): return self
        def __exit__(self, *a): return False
        def get(self, key): return store.get(key)

    class Lines:
        def __init__(self, path): self.f = open(path, "rb")
        def __enter__(self): return self
        def __exit__(self, *a): self.f.close(); return False
        def __iter__(self): return (json.loads(line) for line in self.f if line.strip())

    fake = {"lmdb": types.ModuleType("lmdb"), "jsonlines": types.ModuleType("jsonlines"), "pytorch_transformers": types.ModuleType("pytorch_transformers"),
            "pytorch_transformers.tokenization_bert": types.ModuleType("pytorch_transformers.tokenization_bert"), "refds": types.ModuleType("refds")}
    for name in ("skimage", "skimage.io", "matplotlib", "matplotlib.pyplot", "matplotlib.collections", "matplotlib.patches", "tools", "tools.refer",
                 "tools.refer.external", "tools.refer.external.mask"):
        fake[name] = types.ModuleType(name)
    fake["matplotlib.collections"].PatchCollection = fake["matplotlib.patches"].Polygon = fake["matplotlib.patches"].Rectangle = object
    fake["tools"].__path__ = [os.path.join(ref_root, "tools")]
    fake["tools.refer"].__path__ = [os.path.join(ref_root, "tools", "refer")]
    fake["tools.refer.external"].__path__ = []
    fake["tools.refer.external"].mask = fake["tools.refer.external.mask"]
    fake["skimage"].io = fake["skimage.io"]
    fake["matplotlib"].pyplot = fake["matplotlib.pyplot"]
    fake["lmdb"].open = lambda *a, **k: types.SimpleNamespace(begin=lambda write=False: Txn())
    fake["jsonlines"].open = Lines
    fake["pytorch_transformers.tokenization_bert"].BertTokenizer = object
    fake["refds"].__path__ = [os.path.join(ref_root, "volta", "datasets")]
    saved = {k: sys.modules.get(k) for k in fake}
    sys.modules.update(fake)
    try:
        yield {name: importlib.import_module("refds." + name) for name in ("_image_features_reader", "vqa_dataset", "gqa_dataset", "nlvr2_dataset",
                                                                             "refer_expression_dataset", "retrieval_dataset")}
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        for k in [k for k in sys.modules if k.startswith("refds.") or k.startswith("tools.refer.")]:
            del sys.modules[k]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "task_data_reference.npz"))
    args = ap.parse_args()
    images = make_images()
    store = store_records(images)
    blob = {"vocab_json": np.array(json.dumps(VOCAB)), "cases_json": np.array(json.dumps(CASES)), "image_keys_json": np.array(json.dumps(list(images)))}
    for key, im in images.items():
        blob["img::%s::hw" % key] = np.array([im["h"], im["w"]], np.int64)
        blob["img::%s::boxes" % key], blob["img::%s::features" % key] = im["boxes"], im["features"]
        blob["img::%s::mean64" % key] = im["features"].astype(np.float64).mean(axis=0)
    hit = dict(truncation=0, nlvr_overflow=0, nlvr_first_image_overflow=0, empty_target=0, mask_sep=0, refer_truncation=0, retrieval_carry_over=0,
               retrieval_hard=0)
    with tempfile.TemporaryDirectory() as root, reference_datasets(args.reference, store) as ref:
        files = write_dataroot(root)
        for rel, data in files.items():
            blob["file::" + rel] = np.frombuffer(data, dtype=np.uint8)
        classes = {"VQA": ref["vqa_dataset"].VQAClassificationDataset, "GQA": ref["gqa_dataset"].GQAClassificationDataset, "NLVR2": ref["nlvr2_dataset"].NLVR2Dataset,
                   "refcoco": ref["refer_expression_dataset"].ReferExpressionDataset, "RetrievalCOCO": ref["retrieval_dataset"].RetrievalDataset}
        classes["refcoco+"] = classes["refcocog"] = classes["refcoco"]
        classes["RetrievalFlickr30k"] = classes["RetrievalCOCO"]
        roots = {"VQA": root, "GQA": os.path.join(root, "gqa"), "NLVR2": os.path.join(root, "nlvr2"), "refcoco": os.path.join(root, "refer"),
                 "refcoco+": os.path.join(root, "refer"), "refcocog": os.path.join(root, "refer"), "RetrievalCOCO": os.path.join(root, "retrieval"),
                 "RetrievalFlickr30k": os.path.join(root, "retrieval")}
        jsonpath = {"RetrievalCOCO": os.path.join(root, "retrieval", "coco.jsonline"), "RetrievalFlickr30k": os.path.join(root, "retrieval", "flickr.jsonline")}
        rmod = ref["retrieval_dataset"]
        drawn = []
        real_random, real_randint = rmod.random, np.random.randint

        class Rec:                                                       # records what the retrieval dataset draws
            @staticmethod
            def choice(seq):
                drawn.append(real_random.choice(seq))
                return drawn[-1]

        def randint(*a, **k):
            drawn.append(("pool", int(real_randint(*a, **k))))
            return drawn[-1][1]
        rmod.random = Rec
        real_random.seed(3)
        np.random.seed(3)
        tok = WordTokenizer(VOCAB)
        rd = ref["_image_features_reader"].ImageFeaturesH5Reader("unused", types.SimpleNamespace(v_feature_size=F, num_locs=5, add_global_imgfeat="first"))
        for key in images:
            blob["img::%s::global_ref32" % key] = np.asarray(rd[key][0][0], dtype=np.float32)
        for name, (kind, kw) in CASES.items():
            cfg = types.SimpleNamespace(v_feature_size=F, num_locs=kw["num_locs"], add_global_imgfeat=kw["add_global_imgfeat"])
            reader = ref["_image_features_reader"].ImageFeaturesH5Reader("unused", cfg)
            ds = classes[kind](task=kind, dataroot=roots[kind], annotations_jsonpath=jsonpath.get(kind, ""), image_features_reader=reader, gt_image_features_reader=None,
                               tokenizer=tok, bert_model="bert-base-uncased", padding_index=0, **kw)
            R = kw["max_region_num"] + int(kw["add_global_imgfeat"] is not None)
            blob["%s::len" % name] = np.array(len(ds), np.int64)
            blob["%s::num_labels" % name] = np.array(ds.num_labels, np.int64)
            for i in range(len(ds)):
                del drawn[:]
                np.random.randint = randint
                try:
                    out = ds[i]
                finally:
                    np.random.randint = real_randint
                assert len(out) == 8
                for j, t in enumerate(out):
                    blob["%s::%d::%d" % (name, i, j)] = t.numpy() if torch.is_tensor(t) else np.array(t)
                    if torch.is_tensor(t):
                        blob["%s::%d::%d::dtype" % (name, i, j)] = np.array(str(t.dtype))
                extra = int(kw["add_global_imgfeat"] is not None)
                if kind.startswith("Retrieval"):
                    # drawn: img2 tries.., entry2, img3 tries.., [("pool", k) | img4 tries..], entry4
                    own, r, at = ds._entries[i]["image_id"], list(drawn), 0
                    while r[at] == own:
                        at += 1
                    e2, at = r[at + 1], at + 2
                    while r[at] == own:
                        at += 1
                    img3, at = r[at], at + 1
                    if isinstance(r[at], tuple):
                        hit["retrieval_hard"] += 1
                    else:
                        while r[at] == own:
                            at += 1
                    e4 = r[at + 1]
                    assert at + 2 == len(r), (r, at)
                    blob["%s::%d::negatives" % (name, i)] = np.array([e2, img3, e4], np.int64)
                    hit["retrieval_carry_over"] += REGIONS[str(img3)] < REGIONS[str(own)]
                    continue
                e = ds.entries[i]
                if kind.startswith("refcoco"):
                    hit["refer_truncation"] += REGIONS[str(e["image_id"])] + extra > R
                    continue
                if kind == "NLVR2":
                    n0, n1 = REGIONS[e["image_id_0"]] + extra, REGIONS[e["image_id_1"]] + extra
                    hit["nlvr_overflow"] += n0 + n1 > 2 * R
                    hit["nlvr_first_image_overflow"] += n0 >= 2 * R
                else:
                    hit["truncation"] += REGIONS[str(e["image_id"])] + extra > R
                    hit["mask_sep"] += out[3].numel() == kw["max_seq_length"] + 2
                hit["empty_target"] += float(out[4].abs().sum()) == 0.0
            for cache in ("cache", "gqa/cache", "nlvr2/cache", "refer/cache", "retrieval/annotations/cache"):   # every case tokenises afresh
                if not os.path.isdir(os.path.join(root, cache)):
                    continue
                for fn in os.listdir(os.path.join(root, cache)):
                    if not fn.endswith("_target.pkl"):
                        os.remove(os.path.join(root, cache, fn))
    assert all(v > 0 for v in hit.values()), hit
    np.savez_compressed(args.out, **blob)
    print("wrote %s: %d arrays, %d bytes; cases hit: %s" % (args.out, len(blob), os.path.getsize(args.out), hit))


if __name__ == "__main__":
    main()
