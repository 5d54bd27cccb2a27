"""numpy restatement of `vk_task_batch` (csrc/taskbatch.hip), operation by operation in fp32, kept beside the tests the way radam_restate.py is:
the CPU tests check the segment lists the datasets emit against the reference fixture through it, the GPU tests check the kernel against it."""
import numpy as np

F32 = np.float32


def logical_rows(feat, boxes, n, w, h, add_global, num_locs):
    """(features [nl, F], spatials [nl, num_locs], pixel boxes [nl, 4]) of one staged image: the regions with the global row first / last."""
    n = int(n)
    x, bx = feat[:n].astype(F32), boxes[:n].astype(F32)
    fw, fh = F32(w), F32(h)
    loc = np.zeros((n, num_locs), dtype=F32)
    loc[:, 0], loc[:, 1], loc[:, 2], loc[:, 3] = bx[:, 0] / fw, bx[:, 1] / fh, bx[:, 2] / fw, bx[:, 3] / fh
    if num_locs == 5:
        loc[:, 4] = (bx[:, 3] - bx[:, 1]) * (bx[:, 2] - bx[:, 0]) / (fw * fh)
    if add_global is None:
        return x, loc, bx
    acc = np.zeros(feat.shape[1], dtype=F32)
    for i in range(n):                                   # rows in order, fp32: ((x0 + x1) + x2) + ...
        acc = x[i].copy() if i == 0 else acc + x[i]
    with np.errstate(invalid="ignore", divide="ignore"):
        g = (acc / F32(n))[None]
    gl = np.array([[0, 0, 1, 1, 1][:num_locs]], dtype=F32)
    gb = np.array([[0, 0, w, h]], dtype=F32)
    first = add_global == "first"
    cat = (lambda a, b: np.concatenate([a, b])) if first else (lambda a, b: np.concatenate([b, a]))
    return cat(g, x), cat(gl, loc), cat(gb, bx)


def iou_rows(bx, ref):
    one = F32(1)
    ga = (ref[2] - ref[0] + one) * (ref[3] - ref[1] + one)
    aa = (bx[:, 2] - bx[:, 0] + one) * (bx[:, 3] - bx[:, 1] + one)
    iw = np.minimum(bx[:, 2], ref[2]) - np.maximum(bx[:, 0], ref[0]) + one
    ih = np.minimum(bx[:, 3], ref[3]) - np.maximum(bx[:, 1], ref[1]) + one
    iw[iw < 0] = 0
    ih[ih < 0] = 0
    inter = iw * ih
    return (inter / (aa + ga - inter)).astype(F32)


def task_batch(feat, boxes, n, wh, segs, mask_count, R, num_locs, add_global, scatter=None, ref_box=None):
    S, Rcap, F = feat.shape
    N = segs.shape[0]
    features, spatials = np.zeros((N, R, F), dtype=F32), np.zeros((N, R, num_locs), dtype=F32)
    image_mask = (np.arange(R)[None, :] < np.asarray(mask_count).reshape(N, 1)).astype(np.int64)
    out = dict(features=features, spatials=spatials, image_mask=image_mask)
    iou = np.zeros((N, R, 1), dtype=F32) if ref_box is not None else None
    rows = {}
    for o in range(N):
        for k in range(segs.shape[1]):                   # in order: the later segment overwrites the earlier one
            s, src, dst, cnt = (int(v) for v in segs[o, k])
            if cnt <= 0 or s < 0 or s >= S or src < 0:
                continue
            if s not in rows:
                rows[s] = logical_rows(feat[s], boxes[s], min(max(int(n[s]), 0), Rcap), int(wh[s, 0]), int(wh[s, 1]), add_global, num_locs)
            x, loc, bx = rows[s]
            lo = max(dst, 0)
            hi = min(dst + cnt, R, dst + x.shape[0] - src)
            if hi <= lo:
                continue
            q = slice(src + lo - dst, src + hi - dst)
            features[o, lo:hi], spatials[o, lo:hi] = x[q], loc[q]
            if iou is not None:
                iou[o, lo:hi, 0] = iou_rows(bx[q], np.asarray(ref_box[o], dtype=F32))
    if iou is not None:
        out["target"] = iou
    if scatter is not None:
        csr, labels, scores, num_labels = scatter
        t = np.zeros((len(csr) - 1, num_labels), dtype=F32)
        for b in range(len(csr) - 1):
            for p in range(int(csr[b]), int(csr[b + 1])):
                t[b, int(labels[p])] = scores[p]
        out["target"] = t
    return out
