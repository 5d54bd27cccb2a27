"""A restatement of vk_concap_batch (csrc/concap.hip) in numpy, written from the contract in include/volta_hip.h and the header comment of
concap.hip, plus the case table that tests/test_concap_restate_cpu.py and tests/test_concap_kernels_gpu.py share.  CPU only, numpy only.

The restatement takes the padded arrays of the C ABI, not record lists.  Every fp32 operation is one numpy float32 operation and so rounds
on its own; the decisions on the Philox words are made in Python floats (double), as the reference makes them on `word / 2^32`:
  swap       objective != 2, not visualization, word(3, b, 0) / 2^32 > 0.5 -> caption word(3, b, 1) % n_caps, is_match = 1
  tokens     caption cut to T - 2; slot t - 1: word(0) / 2^32 < 0.15 selects; p = that / 0.15: < 0.8 [MASK], < 0.9 word(1) % V, else kept
  regions    num_boxes clamped to [0, R]; word(2, b, r) / 2^32 < 0.15 selects row r < n, p < 0.9 zeroes its feature row
  co-masking row r < n is masked if a selected row i has IoU(i, r) > 0.4 (+1 pixel convention, fp32 op by op); rows >= n never are
  global     in-order fp32 sum over r = 0 .. R-1 of the written rows, then one fp32 division by max(R - #masked, 1)
  objective 1  a swapped pair loses its token and region labels; a token label 0 becomes -1
  visualization  no swap, no token masking, no region masking
`fault` plants one deviation for the sensitivity checks: "cnt_plus_one" (the divisor off by one) or "region_next_slot" (row r decided by
the word of slot r + 1)."""
import zlib

import numpy as np

from oracle import volta_ref as R

f32 = np.float32
SENT = 0x5A5A5A          # caption-table filler: no vocabulary id, no special id; must never reach an output
ADD_GLOBAL = {None: 0, "first": 1, "last": 2}
THRESHOLD_SEED = 3357760257          # word(stream 2, pair 0, slot 0) == 644245094, the largest word with word / 2^32 < 0.15
THRESHOLD_WORD = 644245094


def iou_matrix(boxes):
    """[n, 4] -> [n, n] fp32, every operation rounded on its own: ((x2 - x1) + 1) * ((y2 - y1) + 1), inter / ((ai + aj) - inter)."""
    b = np.asarray(boxes, f32)
    one = f32(1)
    area = ((b[:, 2] - b[:, 0]) + one) * ((b[:, 3] - b[:, 1]) + one)
    iw = (np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0])) + one
    ih = (np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1])) + one
    inter = np.maximum(iw, f32(0)) * np.maximum(ih, f32(0))
    out = inter / ((area[:, None] + area[None, :]) - inter)
    assert out.dtype == f32
    return out


def inorder_sum(rows):
    """[R, F] fp32 -> [F]: ((0 + row 0) + row 1) + ... in fp32."""
    s = np.zeros(rows.shape[1], f32)
    for r in range(rows.shape[0]):
        s = s + rows[r]
    return s


def region_decisions(boxes_b, n, words_b, Rl, visualization=0):
    """-> sel [R], zero [R], masked [R] (bool) and the global-feature divisor (int)."""
    p = words_b.astype(np.float64) / 2.0 ** 32
    live = np.arange(Rl) < n
    sel = live & (p < 0.15) & (not visualization)
    zero = sel & (p / 0.15 < 0.9)
    masked = np.zeros(Rl, bool)
    if n > 0:
        ov = iou_matrix(boxes_b[:n])
        masked[:n] = (sel[:n, None] & (ov > f32(0.4))).any(0)
    cnt = Rl - int(masked.sum())
    return sel, zero, masked, (1 if cnt == 0 else cnt)


def restate(feat, cls, boxes, num_boxes, img_wh, cap_index, cap_tokens, cap_len, n_caps, seed, T, V, cls_id=101, sep_id=102, mask_id=103,
            add_global=1, objective=0, visualization=0, fault=None):
    feat, cls, boxes, img_wh = (np.asarray(x, f32) for x in (feat, cls, boxes, img_wh))
    B, Rl, F = feat.shape
    C = cls.shape[2]
    Rv, off, g = Rl + (1 if add_global else 0), (1 if add_global == 1 else 0), (0 if add_global == 1 else Rl)
    w_tok, w_rnd = R.concap_words(seed, R.CC_SITE_TOKEN, B, T), R.concap_words(seed, R.CC_SITE_RANDTOK, B, T)
    w_reg, w_cap = R.concap_words(seed, R.CC_SITE_REGION, B, Rl + 1), R.concap_words(seed, R.CC_SITE_CAPTION, B, 2)
    w_reg = w_reg[:, 1:] if fault == "region_next_slot" else w_reg[:, :Rl]
    o = dict(input_ids=np.zeros((B, T), np.int64), input_mask=np.zeros((B, T), np.int64), segment_ids=np.zeros((B, T), np.int64),
             lm_label_ids=np.full((B, T), -1, np.int64), is_match=np.zeros(B, np.int64), image_feat=np.zeros((B, Rv, F), f32),
             image_loc=np.zeros((B, Rv, 5), f32), image_cls=np.zeros((B, Rl, C), f32), image_label=np.full((B, Rl), -1, np.int64),
             image_mask=np.zeros((B, Rv), np.int64))
    for b in range(B):
        n = min(max(int(num_boxes[b]), 0), Rl)
        cap, swapped = int(cap_index[b]), False
        if objective != 2 and not visualization and float(w_cap[b, 0]) / 2.0 ** 32 > 0.5:
            cap, swapped = int(w_cap[b, 1]) % int(n_caps), True
        drop = objective == 1 and swapped
        o["is_match"][b] = int(swapped)
        ln = min(int(cap_len[cap]), T - 2)
        o["input_ids"][b, 0], o["input_ids"][b, ln + 1] = cls_id, sep_id
        o["input_mask"][b, :ln + 2] = 1
        for t in range(1, ln + 1):
            tok = int(cap_tokens[cap, t - 1])
            ident, lab = tok, -1
            prob = float(w_tok[b, t - 1]) / 2.0 ** 32
            if prob < 0.15 and not visualization:
                prob /= 0.15
                if prob < 0.8:
                    ident = mask_id
                elif prob < 0.9:
                    ident = int(w_rnd[b, t - 1]) % int(V)
                lab = tok
            if objective == 1 and (drop or lab == 0):
                lab = -1
            o["input_ids"][b, t], o["lm_label_ids"][b, t] = ident, lab
        sel, zero, _, cnt = region_decisions(boxes[b], n, w_reg[b], Rl, visualization)
        if fault == "cnt_plus_one":
            cnt += 1
        live = np.arange(Rl) < n
        o["image_label"][b] = np.where(sel & (not drop), 1, -1)
        o["image_mask"][b, off:off + Rl] = live
        w, h = img_wh[b, 0], img_wh[b, 1]
        wh = f32(float(w) * float(h))
        bx = boxes[b, :n]
        loc = o["image_loc"][b, off:off + Rl]
        loc[:n, 0], loc[:n, 1], loc[:n, 2], loc[:n, 3] = bx[:, 0] / w, bx[:, 1] / h, bx[:, 2] / w, bx[:, 3] / h
        loc[:n, 4] = ((bx[:, 3] - bx[:, 1]) * (bx[:, 2] - bx[:, 0])) / wh
        rows = np.where((live & ~zero)[:, None], feat[b], f32(0))
        o["image_feat"][b, off:off + Rl] = rows
        o["image_cls"][b] = np.where((np.arange(Rl) < int(num_boxes[b]))[:, None], cls[b], f32(0))
        if add_global:
            o["image_feat"][b, g] = inorder_sum(rows) / f32(cnt)
            o["image_loc"][b, g] = (0, 0, 1, 1, 1)
            o["image_mask"][b, g] = 1
    return o


def restate_inputs(inp, **over):
    """restate() on a dict of make_inputs() / from_records()."""
    kw = {k: inp[k] for k in ("feat", "cls", "boxes", "num_boxes", "img_wh", "cap_index", "cap_tokens", "cap_len", "n_caps", "seed", "T", "V",
                              "cls_id", "sep_id", "mask_id", "add_global", "objective", "visualization")}
    kw.update(over)
    return restate(**kw)


def from_records(recs, caps, Rl, seed, T, V, add_global, objective):
    """The record lists of oracle.make_golden.concap_records as the padded arrays of the C ABI (NaN beyond num_boxes)."""
    B, F, C = len(recs), recs[0]["feat"].shape[1], recs[0]["cls"].shape[1]
    feat, cls, boxes = (np.full((B, Rl, k), np.nan, f32) for k in (F, C, 4))
    for b, r in enumerate(recs):
        n = r["feat"].shape[0]
        feat[b, :n], cls[b, :n], boxes[b, :n] = r["feat"], r["cls"], r["boxes"]
    ld = max(len(c) for c in caps) + 2
    tok = np.full((len(caps), ld), SENT, np.int32)
    for i, c in enumerate(caps):
        tok[i, :len(c)] = c
    return dict(feat=feat, cls=cls, boxes=boxes, num_boxes=np.array([r["feat"].shape[0] for r in recs], np.int32),
                img_wh=np.array([[r["w"], r["h"]] for r in recs], f32), cap_index=np.array([r["caption_index"] for r in recs], np.int32),
                cap_tokens=tok, cap_len=np.array([len(c) for c in caps], np.int32), n_caps=len(caps), seed=seed, T=T, V=V, cls_id=101,
                sep_id=102, mask_id=103, add_global=ADD_GLOBAL[add_global], objective=objective, visualization=0)


# ------------------------------------------------------------------------------------------------ IoU pairs next to the 0.4 decision
def _iou_variants(p, q):
    """p, q [N, 4] fp32 -> the `> 0.4` decision of IoU(p, q) op by op and under each contraction a compiler may choose.  A contraction
    is emulated by doing the fused product-and-add in float64 and rounding once."""
    one, d = f32(1), np.float64
    wp, hp, wq, hq = (p[:, 2] - p[:, 0]) + one, (p[:, 3] - p[:, 1]) + one, (q[:, 2] - q[:, 0]) + one, (q[:, 3] - q[:, 1]) + one
    ap, aq = wp * hp, wq * hq
    iw = np.maximum((np.minimum(p[:, 2], q[:, 2]) - np.maximum(p[:, 0], q[:, 0])) + one, f32(0))
    ih = np.maximum((np.minimum(p[:, 3], q[:, 3]) - np.maximum(p[:, 1], q[:, 1])) + one, f32(0))
    inter = iw * ih
    dens = dict(plain=(ap + aq) - inter,
                area_i=(wp.astype(d) * hp.astype(d) + aq.astype(d)).astype(f32) - inter,         # fma(wi, hi, aj) - inter
                area_j=(wq.astype(d) * hq.astype(d) + ap.astype(d)).astype(f32) - inter,         # fma(wj, hj, ai) - inter
                inter=((ap + aq).astype(d) - iw.astype(d) * ih.astype(d)).astype(f32))           # fma(-iw, ih, ai + aj)
    return {k: (inter / v) > f32(0.4) for k, v in dens.items()}


def iou_flip_pairs(per_kind=2, seed=20, n_cand=200000):
    """Seeded search for non-integer box pairs (p, q) whose fp32 decision IoU(p, q) > 0.4 differs between the op-by-op evaluation and one
    contraction.  -> {kind: [(p, q, plain decision)] * per_kind} for kind in area_i (p's area fused), area_j, inter.  q is p moved by
    (dx, dy) with dx solved in float64 for IoU = 0.4, so the candidates lie within a few ulps of the decision."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(20, 200, n_cand), rng.uniform(20, 200, n_cand)
    W, H = rng.uniform(60, 300, n_cand), rng.uniform(60, 300, n_cand)              # widths with the +1 of the convention
    dy = rng.uniform(0, 0.3, n_cand) * H
    dx = W - 4.0 * W * H / (7.0 * (H - dy))                                          # (W - dx)(H - dy) = 4 W H / 7  <=>  IoU = 0.4
    p = np.stack([x, y, x + W - 1, y + H - 1], 1).astype(f32)
    q = (p.astype(np.float64) + np.stack([dx, dy, dx, dy], 1)).astype(f32)
    v = _iou_variants(p, q)
    out = {}
    for kind in ("area_i", "area_j", "inter"):
        idx = np.nonzero(v[kind] != v["plain"])[0][:per_kind]
        assert len(idx) == per_kind, "no IoU pair found for contraction %s" % kind
        out[kind] = [(p[i], q[i], bool(v["plain"][i])) for i in idx]
    return out


# ------------------------------------------------------------------------------------------------ the case table
class Case:
    def __init__(self, id, B=3, R=5, F=8, C=3, T=6, V=3000, add_global=1, objective=0, visualization=0, seed=None, nb=None, cap_lens=None,
                 n_rows=None, n_caps=None, special=None):
        self.id = id
        self.B, self.R, self.F, self.C, self.T, self.V = B, R, F, C, T, V
        self.add_global, self.objective, self.visualization = add_global, objective, visualization
        self.seed = zlib.crc32(id.encode()) if seed is None else seed
        self.nb, self.cap_lens, self.n_rows, self.n_caps, self.special = nb, cap_lens, n_rows, n_caps, special

    def __repr__(self):
        return self.id


def cases():
    c = []
    for Rl in (1, 127, 128, 129, 255, 256):                                  # the 128-thread region loops and the 256 cap
        c.append(Case("regions_R%d" % Rl, B=3, R=Rl, F=8, C=3, add_global=1 + Rl % 2))
    for F in (1, 255, 256, 257, 513):                                        # feature column blocks
        c.append(Case("feat_F%d" % F, B=3, R=5, F=F, C=3, add_global=1 + F % 2))
    for C in (1, 33):
        c.append(Case("cls_C%d" % C, B=3, R=5, F=8, C=C))
    c.append(Case("cls_grid_loops", B=8, R=256, F=8, C=513, add_global=0))     # B R C = 1050624 > 4096 * 256
    c.append(Case("text_T3", B=4, R=5, T=3))
    for obj in (0, 2):
        c.append(Case("text_lengths_obj%d" % obj, B=5, R=5, T=14, objective=obj, cap_lens=[0, 1, 12, 13, 40]))
    c.append(Case("text_token0_obj1", B=16, R=5, T=14, objective=1, special="token0"))
    for ag in (0, 1, 2):
        c.append(Case("box_counts_ag%d" % ag, B=6, R=8, F=8, C=3, add_global=ag, nb=[0, 1, 7, 8, 13, -2]))
    for obj in (0, 1, 2):
        c.append(Case("objective%d" % obj, B=24, R=10, F=16, C=5, T=14, objective=obj))
    for obj in (0, 1):
        c.append(Case("visualization_obj%d" % obj, B=8, R=10, F=16, C=5, T=14, objective=obj, visualization=1))
    c.append(Case("n_caps_below_rows", B=16, R=5, T=14, n_rows=12, n_caps=4))
    c.append(Case("divisor_floor", B=4, R=4, F=8, C=3, special="coincident"))
    c.append(Case("iou_near_0p4", B=64, R=6, F=8, C=3, add_global=1, objective=2, special="iou"))
    c.append(Case("threshold_word", B=1, R=4, F=8, C=3, objective=2, seed=THRESHOLD_SEED))
    return c


def _planted_rows(case):
    """For the IoU case: the pairs b in which exactly one of rows 0 and 1 is selected -> [(b, selected row)]."""
    p = R.concap_words(case.seed, R.CC_SITE_REGION, case.B, case.R).astype(np.float64) / 2.0 ** 32
    s = p[:, :2] < 0.15
    return [(b, int(s[b, 1])) for b in range(case.B) if s[b, 0] != s[b, 1]]


def iou_plan(case):
    """[(b, row of the selected box, kind, p, q, plain decision)]: six searched pairs (two for each contraction), then integer-pixel pairs
    whose IoU is exactly 0.4 (40 / 100: not co-masked under the strict >) and the next pixel above it (4100 / 9900)."""
    flips = iou_flip_pairs()
    plant = [(k,) + t for k in ("area_i", "area_j", "inter") for t in flips[k]]
    for k in ("a", "b"):                # the same integer pairs with either box in the selected row
        pq = [np.array([30, 40, 36, 49], f32), np.array([33, 40, 39, 49], f32), np.array([30, 40, 99, 139], f32), np.array([59, 40, 128, 139], f32)]
        pq = pq if k == "a" else [pq[1], pq[0], pq[3], pq[2]]
        plant.append(("exact_0p4_" + k, pq[0], pq[1], False))
        plant.append(("above_0p4_" + k, pq[2], pq[3], True))
    rows = _planted_rows(case)
    assert len(rows) >= len(plant), "IoU case: %d pairs with exactly one of rows 0, 1 selected, %d needed" % (len(rows), len(plant))
    # p goes to the selected row i, q to the other row r: the kernel evaluates IoU(box i, box r), so area_i is the selected row's area
    return [(b, s, kind, p, q, dec) for (b, s), (kind, p, q, dec) in zip(rows, plant)]


def make_inputs(case):
    """The padded arrays of one case.  Rows >= num_boxes of feat / cls / boxes hold NaN; the caption table holds SENT beyond cap_len and in
    the rows [n_caps, n_rows), whose cap_len is the full row so that a caption drawn there would show."""
    c = case
    rng = np.random.default_rng(zlib.crc32(c.id.encode()) ^ 0x9E3779B9)
    B, Rl = c.B, c.R
    nb = np.array(c.nb, np.int32) if c.nb is not None else rng.integers(max(1, Rl - 3), Rl + 1, B).astype(np.int32)
    if c.nb is None:
        nb[0] = Rl
    if c.special in ("coincident", "iou") or c.id == "threshold_word":
        nb[:] = Rl
    img_wh = np.stack([rng.integers(300, 800, B), rng.integers(300, 800, B)], 1).astype(f32)
    feat = rng.standard_normal((B, Rl, c.F), dtype=f32)
    cls = rng.random((B, Rl, c.C), dtype=f32)
    cls = (cls / cls.sum(2, keepdims=True)).astype(f32)
    xy = rng.uniform(0, 0.6, (B, Rl, 2)) * img_wh[:, None, :]
    wh = rng.uniform(0.1, 0.4, (B, Rl, 2)) * img_wh[:, None, :]
    boxes = np.concatenate([xy, xy + wh], 2).astype(f32)
    if Rl > 3:
        boxes[:, 1] = boxes[:, 0] + rng.uniform(-4, 4, (B, 4)).astype(f32)       # a heavily overlapping pair (IoU > 0.4)
    if c.special == "coincident":
        boxes[:] = boxes[:, :1]
    if c.special == "iou":
        img_wh[:] = (2000, 1500)
        for r in range(2, Rl):          # the other rows: disjoint from the planted ones (all inside x < 700) and from each other
            boxes[:, r] = np.array([1000.25 + 150 * (r - 2), 100.5, 1080.75 + 150 * (r - 2), 190.125], f32) + rng.uniform(0, 9, (B, 4)).astype(f32)
        for b, s, _, p, q, _ in iou_plan(c):
            boxes[b, s], boxes[b, 1 - s] = p, q
    for b in range(B):
        n = min(max(int(nb[b]), 0), Rl)
        feat[b, n:], cls[b, n:], boxes[b, n:] = np.nan, np.nan, np.nan
    n_rows = c.n_rows if c.n_rows is not None else B + 3
    n_caps = c.n_caps if c.n_caps is not None else n_rows
    lens = list(c.cap_lens) if c.cap_lens is not None else [int(x) for x in rng.integers(0, 17, n_rows)]
    lens = (lens + [int(x) for x in rng.integers(0, 17, n_rows)])[:n_rows]
    ld = max(lens) + 2
    tok = np.full((n_rows, ld), SENT, np.int32)
    cap_len = np.zeros(n_rows, np.int32)
    for i in range(n_caps):
        t = rng.integers(1000, c.V, lens[i])
        if c.special == "token0":
            t[rng.random(lens[i]) < 0.5] = 0
        tok[i, :lens[i]], cap_len[i] = t, lens[i]
    cap_len[n_caps:] = ld
    cap_index = (np.arange(B) % n_caps).astype(np.int32)
    return dict(case=c, feat=feat, cls=cls, boxes=boxes, num_boxes=nb, img_wh=img_wh, cap_index=cap_index, cap_tokens=tok, cap_len=cap_len,
                n_caps=n_caps, seed=c.seed, T=c.T, V=c.V, cls_id=101, sep_id=102, mask_id=103, add_global=c.add_global, objective=c.objective,
                visualization=c.visualization)


_CACHE = {}


def reference(case):
    """(inputs, restatement) of a case, computed once per process and shared by the tests; neither is modified by them."""
    if case.id not in _CACHE:
        inp = make_inputs(case)
        _CACHE[case.id] = (inp, restate_inputs(inp))
    return _CACHE[case.id]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == f32 else a


FLOAT_KEYS = ("image_feat", "image_loc", "image_cls")
INT_KEYS = ("input_ids", "input_mask", "segment_ids", "lm_label_ids", "is_match", "image_label", "image_mask")


def same_bits(x, y):
    """Every output of two result dicts equal: integers exactly, floats by their bit patterns.  -> list of the keys that differ."""
    return [k for k in INT_KEYS + FLOAT_KEYS if x[k].shape != y[k].shape or not np.array_equal(bits(x[k]), bits(y[k]))]
