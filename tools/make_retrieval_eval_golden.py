"""Records tests/golden/retrieval_eval_reference.npz from the reference's own RetrievalDatasetVal (volta/datasets/retrieval_dataset.py:260-417
over _image_features_reader.py), loaded by file path and driven on the CPU:

  python tools/make_retrieval_eval_golden.py --reference /path/to/volta-checkout [--out tests/golden/retrieval_eval_reference.npz]

Same pattern and stand-ins as tools/make_task_data_golden.py (its images, feature-store records, word tokenizer and module stand-ins for
`lmdb` / `jsonlines` / `pytorch_transformers` are imported from there).  The annotation files list six images in an order of their own, one
of them twice (first-seen order must hold) and one without a sentence (an image no caption belongs to), with one to three sentences each, in
the COCO (`id`) and the Flickr30k (`img_path`) layout.

Recorded: the inputs (image arrays, both annotation files as bytes, the vocabulary, each case's constructor arguments), per case the
reference's `features_all` / `spatials_all` / `image_mask_all`, `_image_entries`, the image index of every caption, and for every index the
six small members of the 9-tuple; the three image members of the tuple are asserted here to be the `[:500]` / `[500:]` halves of the arrays
and recorded by shape only.  Cases cover both id rules, add_global_imgfeat in {None, first, last}, num_locs in {4, 5}, max_region_num above
and below the largest image, and a caption longer than max_seq_length - 2.  Values only; the tests never import the reference."""
import argparse
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_task_data_golden import F, REGIONS, SENTENCES, VOCAB, WordTokenizer, make_images, reference_datasets, store_records  # noqa: E402

IMAGES = [13, 11, 16, 12, 15, 14]
# (image, sentences) per annotation line: 11 comes twice, 14 has no sentence
LINES = [(13, [0, 1]), (11, [2]), (16, [3, 0, 1]), (12, [1]), (11, [3]), (15, [2, 0]), (14, [])]
CASES = {
    "flickr_plain": ("RetrievalFlickr30k", dict(split="test", max_region_num=16, num_locs=5, add_global_imgfeat=None, append_mask_sep=False, max_seq_length=12)),
    "flickr_first_cut": ("RetrievalFlickr30k", dict(split="test", max_region_num=8, num_locs=4, add_global_imgfeat="first", append_mask_sep=False, max_seq_length=20)),
    "flickr_last_cut": ("RetrievalFlickr30k", dict(split="test", max_region_num=9, num_locs=5, add_global_imgfeat="last", append_mask_sep=False, max_seq_length=10)),
    "coco_last": ("RetrievalCOCO", dict(split="test", max_region_num=15, num_locs=5, add_global_imgfeat="last", append_mask_sep=False, max_seq_length=12)),
    "coco_none_cut": ("RetrievalCOCO", dict(split="test", max_region_num=6, num_locs=4, add_global_imgfeat=None, append_mask_sep=False, max_seq_length=8)),
    "coco_first": ("RetrievalCOCO", dict(split="test", max_region_num=16, num_locs=4, add_global_imgfeat="first", append_mask_sep=False, max_seq_length=24)),
}


def annotation_files():
    files = {}
    for name, key in (("coco", "id"), ("flickr", "img_path")):
        lines = []
        for img, sents in LINES:
            ann = dict(sentences=[SENTENCES[k] for k in sents])
            ann[key] = img if key == "id" else "%d.jpg" % img
            lines.append(json.dumps(ann))
        files["%s_test.jsonline" % name] = ("\n".join(lines) + "\n").encode()
    return files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "retrieval_eval_reference.npz"))
    args = ap.parse_args()
    images = {k: v for k, v in make_images().items() if k in {str(i) for i in IMAGES}}
    store = store_records(images)
    blob = {"vocab_json": np.array(json.dumps(VOCAB)), "cases_json": np.array(json.dumps(CASES)), "image_keys_json": np.array(json.dumps(list(images)))}
    for key, im in images.items():
        blob["img::%s::hw" % key] = np.array([im["h"], im["w"]], np.int64)
        blob["img::%s::boxes" % key], blob["img::%s::features" % key] = im["boxes"], im["features"]
    hit = dict(cut=0, uncut=0, long_caption=0)
    with tempfile.TemporaryDirectory() as root, reference_datasets(args.reference, store) as ref:
        files = annotation_files()
        for rel, data in files.items():
            blob["file::" + rel] = np.frombuffer(data, dtype=np.uint8)
            with open(os.path.join(root, rel), "wb") as f:
                f.write(data)
        tok = WordTokenizer(VOCAB)
        for name, (kind, kw) in CASES.items():
            cfg = types.SimpleNamespace(v_feature_size=F, num_locs=kw["num_locs"], add_global_imgfeat=kw["add_global_imgfeat"])
            reader = ref["_image_features_reader"].ImageFeaturesH5Reader("unused", cfg)
            path = os.path.join(root, "%s_test.jsonline" % ("coco" if kind == "RetrievalCOCO" else "flickr"))
            ds = ref["retrieval_dataset"].RetrievalDatasetVal(task=kind, dataroot=root, annotations_jsonpath=path, image_features_reader=reader,
                                                              gt_image_features_reader=None, tokenizer=tok, bert_model="bert-base-uncased", padding_index=0, **kw)
            R = kw["max_region_num"] + int(kw["add_global_imgfeat"] is not None)
            extra = int(kw["add_global_imgfeat"] is not None)
            hit["cut"] += any(REGIONS[str(i)] + extra > R for i in IMAGES)
            hit["uncut"] += all(REGIONS[str(i)] + extra <= R for i in IMAGES)
            hit["long_caption"] += any(len(e["caption"].split()) > kw["max_seq_length"] - 2 for e in ds._caption_entries)
            assert ds._image_entries == IMAGES, ds._image_entries
            blob["%s::len" % name] = np.array(len(ds), np.int64)
            blob["%s::image_entries" % name] = np.asarray(ds._image_entries, np.int64)
            blob["%s::caption_image" % name] = np.asarray([ds._image_entries.index(e["image_id"]) for e in ds._caption_entries], np.int64)
            for key in ("features_all", "spatials_all", "image_mask_all"):
                t = getattr(ds, key)
                blob["%s::%s" % (name, key)] = t.numpy()
                blob["%s::%s::dtype" % (name, key)] = np.array(str(t.dtype))
            for i in range(len(ds)):
                out = ds[i]
                assert len(out) == 9
                half = slice(0, 500) if i % 2 == 0 else slice(500, None)
                for j, key in enumerate(("features_all", "spatials_all", "image_mask_all")):
                    assert torch.equal(out[j], getattr(ds, key)[half])
                    blob["%s::%d::%d::shape" % (name, i, j)] = np.asarray(out[j].shape, np.int64)
                for j in range(3, 9):
                    t = out[j]
                    blob["%s::%d::%d" % (name, i, j)] = t.numpy() if torch.is_tensor(t) else np.array(t)
                    if torch.is_tensor(t):
                        blob["%s::%d::%d::dtype" % (name, i, j)] = np.array(str(t.dtype))
    assert all(v > 0 for v in hit.values()), hit
    np.savez_compressed(args.out, **blob)
    print("wrote %s: %d arrays, %d bytes; cases hit: %s" % (args.out, len(blob), os.path.getsize(args.out), hit))


if __name__ == "__main__":
    main()
