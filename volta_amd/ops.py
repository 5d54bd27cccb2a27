"""Thin tensor-level wrappers over the C ABI (one call = one kernel launch on the current stream).
Used by the parity tests and by the plan builder; they validate shapes on the host because a wrong
shape in a hand-written kernel is a GPU fault, not an exception."""
import ctypes as C

import torch

from . import _lib as L
from . import _lib as L_
from ._lib import check, ptr, stream_ptr


def _bf16(t):
    assert t.dtype == torch.bfloat16 and t.is_cuda, "bf16 cuda tensor expected"
    return t


def gemm_problem(A, B, Cout, layout, M, N, K, bias=None, R=None, C2=None, bias_grad=None, dyn=None, n_store=0,
                 lda=None, ldb=None, ldc=None, ldr=None):
    """Builds one vk_gemm_problem after checking that every operand really covers what the kernel reads."""
    lda = lda if lda is not None else A.stride(-2)
    ldb = ldb if ldb is not None else B.stride(-2)
    ldc = ldc if ldc is not None else Cout.stride(-2)
    a_rows, a_cols = (K, M) if layout == L.TN else (M, K)
    b_rows, b_cols = (N, K) if layout == L.NT else (K, N)
    for name, t, rows, cols, ld in (("A", A, a_rows, a_cols, lda), ("B", B, b_rows, b_cols, ldb)):
        _bf16(t)
        need = (rows - 1) * ld + cols if rows > 0 else 0
        have = t.numel() - 0 if t.is_contiguous() else t.untyped_storage().nbytes() // 2 - t.storage_offset()
        assert need <= have, "%s operand too small: need %d elements, have %d" % (name, need, have)
    ncols = max(N, n_store)
    need_c = (M - 1) * ldc + ncols if M > 0 else 0
    have_c = Cout.untyped_storage().nbytes() // Cout.element_size() - Cout.storage_offset()
    assert need_c <= have_c, "C too small: need %d have %d" % (need_c, have_c)
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() >= N
    if R is not None:
        _bf16(R)
        ldr = ldr if ldr is not None else R.stride(-2)
        assert ldr % 2 == 0 and ldr >= N, "ldr must be even and >= N"
        assert (M - 1) * ldr + min((N + 1) & ~1, ldr) <= R.untyped_storage().nbytes() // 2 - R.storage_offset()      # rows end on an even count (gemm_epilogue)
    if bias_grad is not None:
        assert bias_grad.dtype == torch.float32 and bias_grad.numel() >= M
    if dyn is not None:
        assert dyn.dtype == torch.int32
    return L.GemmProblem(ptr(A), ptr(B), ptr(Cout), ptr(C2), ptr(bias), ptr(R), ptr(bias_grad), ptr(dyn),
                         M, N, K, lda, ldb, ldc, ldr or 0, n_store)


def split_geometry(N):
    """Tile geometry a split accumulation runs on: 256 x 192 tiles when they cover N without a ragged last column tile and 256-wide ones
    would not (N = 768: 4 x 192), 256 x 256 otherwise."""
    return 259 if (N % 192 == 0 and N % 256 != 0) else 258


def split_workspace(layout, M, N, nparts, geometry, device):
    """(ws uint8 tensor, cnt int32 tensor) of one split accumulation; cnt starts (and is left by every launch) at zero."""
    tiles = C.c_int(0)
    nbytes = L.lib.vk_gemm_split_workspace_bytes(layout, M, N, nparts, geometry, C.byref(tiles))
    assert nbytes > 0, "split accumulation: nparts >= 2 and geometry 258 / 259"
    return torch.empty(nbytes, dtype=torch.uint8, device=device), torch.zeros(tiles.value, dtype=torch.int32, device=device)


def split_parts(problem, layout, slices, ws, cnt):
    """K-slices of ONE product as the problems of a split accumulation.  `problem`: the whole product (gemm_problem); `slices`: list of
    (A view, B view, K) -- operand pointers and contraction length of each part (a part may come from other tensors altogether: the
    weight gradient of a parameter shared by two modalities sums row chunks of both)."""
    out = []
    for i, (A, B, K) in enumerate(slices):
        q = L.GemmProblem.from_buffer_copy(problem)
        q.A, q.B, q.K = ptr(A), ptr(B), K
        q.ws, q.cnt, q.part, q.nparts = ptr(ws), ptr(cnt), i, len(slices)
        out.append(q)
    return out


def k_slices(A, B, layout, K, nparts, lda=None, ldb=None):
    """Even K-slices (multiples of 64 elements / rows) of the operands of one product, for split_parts()."""
    step = -(-K // nparts)
    step = -(-step // 64) * 64
    out, k0 = [], 0
    while k0 < K:
        kc = min(step, K - k0)
        a = A[k0:] if layout == L.TN else A[:, k0:]
        b = B[:, k0:] if layout == L.NT else B[k0:]
        out.append((a, b, kc))
        k0 += step
    return out


default_geometry = 0      # what gemm_grouped() passes when the caller names none (the parity tests sweep it; 0 = the library's heuristic)


def gemm_grouped(layout, epilogue, problems, geometry=None):
    """geometry: tile code of vk_gemm_grouped_ex (128 / 258 / 259 / 260, | L.GEMM_PERSISTENT / L.GEMM_ONE_TILE_PER_WG), 0 = heuristic."""
    arr = (L.GemmProblem * len(problems))(*problems)
    check(L.lib.vk_gemm_grouped_ex(layout, epilogue, arr, len(problems), default_geometry if geometry is None else geometry, stream_ptr()))


def gemm_chain(layout, epi_p, producers, epi_c, consumers):
    """vk_gemm_chain: producers (256 x 256 tiles, `sig`) and the consumers of their outputs (256 x 192 tiles, `dep`) in one persistent launch."""
    ap, ac = (L.GemmProblem * len(producers))(*producers), (L.GemmProblem * len(consumers))(*consumers)
    check(L.lib.vk_gemm_chain(layout, epi_p, ap, len(producers), epi_c, ac, len(consumers), stream_ptr()))


def cast_f32_bf16(src, dst):
    assert src.dtype == torch.float32 and dst.dtype == torch.bfloat16 and src.numel() == dst.numel()
    check(L.lib.vk_cast_f32_bf16(ptr(src), ptr(dst), src.numel(), stream_ptr()))


def set_seed(seed_t, value):
    assert seed_t.dtype == torch.int64 and seed_t.is_cuda
    check(L.lib.vk_set_seed(ptr(seed_t), C.c_uint64(value & 0xFFFFFFFFFFFFFFFF), stream_ptr()))


def _segs(drop, segs):
    """segs: None -> identity rows on drop.site; else [(site, div, mul, off), (site, div, mul, off)]."""
    arr = (L.DropRows * 2)()
    if segs is None:
        site = drop.site if drop is not None else 0
        segs = [(site, 0, 0, 0), (site + 1, 0, 0, 0)]
    for i, sg in enumerate(segs):
        arr[i] = L.DropRows(*sg)
    return arr


def ln_fwd(d, x, gamma, beta, y, z, mean, rstd, M, H, drop=None, split_row=None, post=0, out_scale=1.0, addvec=None,
           dyn=None, segs=None):
    for t in (d, y):
        _bf16(t)
        assert t.numel() >= M * H
    assert gamma.dtype == torch.float32 and gamma.numel() == H and beta.numel() == H
    assert mean.numel() >= M and rstd.numel() >= M and mean.dtype == torch.float32
    drop = drop or L.dropout_cfg(None, 0, 0.0)
    a = L.LnArgs(ptr(d), ptr(x), ptr(addvec), ptr(gamma), ptr(beta), ptr(y), ptr(z), ptr(mean), ptr(rstd), ptr(dyn), M, H,
                 split_row if split_row is not None else M, post, out_scale, drop, _segs(drop, segs))
    check(L.lib.vk_ln_fwd(C.byref(a), stream_ptr()))


def ln_bwd(dy, z, mean, rstd, gamma, dz, dd, partial, dgamma, dbeta, M, H, drop=None, split_row=None, post=0,
           out_scale=1.0, dyn=None, segs=None):
    check(L.lib.vk_ln_bwd(C.byref(ln_bwd_args(dy, z, mean, rstd, gamma, dz, dd, partial, dgamma, dbeta, M, H, drop, split_row, post, out_scale,
                                              dyn, segs)), stream_ptr()))


def ln_bwd_args(dy, z, mean, rstd, gamma, dz, dd, partial, dgamma, dbeta, M, H, drop=None, split_row=None, post=0,
                out_scale=1.0, dyn=None, segs=None):
    """vk_ln_bwd_args.  partial None: gamma and beta are frozen -- the launch without column sums, dgamma / dbeta ignored (may be None);
    dz / dd None: that output is not stored."""
    for t in (dy, z) + ((dz,) if dz is not None else ()):
        _bf16(t)
        assert t.numel() >= M * H
    if partial is not None:
        assert partial.numel() >= L.lib.vk_ln_bwd_partial_rows(M) * 2 * H and partial.dtype == torch.float32
        assert dgamma.numel() == H and dbeta.numel() == H
    drop = drop or L.dropout_cfg(None, 0, 0.0)
    return L.LnBwdArgs(ptr(dy), ptr(z), ptr(mean), ptr(rstd), ptr(gamma), ptr(dz), ptr(dd), ptr(partial), ptr(dgamma),
                       ptr(dbeta), ptr(dyn), M, H, split_row if split_row is not None else M, post, out_scale, 0, drop,
                       _segs(drop, segs))


def ln_bwd_pair(a, b):
    """Two vk_ln_bwd_args jobs of equal H in one launch (two, when only one of them has parameter gradients)."""
    check(L.lib.vk_ln_bwd_pair(C.byref(a), C.byref(b), stream_ptr()))


def attn_args(qkv, L, masks, ctx, lse, B, nh, gate, drops=None, H=None, dh=64):
    """qkv[m]: [B*L[m], 3H] fused projection output (Q | K | V column blocks); ctx[m]: [B*L[m], H]; H = nh * dh."""
    a = L_.AttnArgs()
    H = H or nh * dh
    assert H == nh * dh
    for m in range(2):
        used_q = gate[m][0] or gate[m][1]
        used_k = gate[0][m] or gate[1][m]
        if not (used_q or used_k):
            continue
        t = _bf16(qkv[m])
        assert t.shape == (B * L[m], 3 * H) and t.is_contiguous()
        es = 2
        a.q[m] = t.data_ptr()
        a.k[m] = t.data_ptr() + H * es
        a.v[m] = t.data_ptr() + 2 * H * es
        a.ld[m] = 3 * H
        a.L[m] = L[m]
        if used_k:
            assert masks[m].dtype == torch.float32 and masks[m].shape == (B, L[m]) and masks[m].is_contiguous()
            a.mask[m] = masks[m].data_ptr()
        if used_q:
            assert _bf16(ctx[m]).shape == (B * L[m], H) and lse[m].numel() == B * nh * L[m] and lse[m].dtype == torch.float32
            a.ctx[m] = ctx[m].data_ptr()
            a.ldo[m] = H
            a.lse[m] = lse[m].data_ptr()
    a.B, a.nh, a.scale, a.dh = B, nh, 1.0 / (dh ** 0.5), dh
    for i in range(2):
        for j in range(2):
            a.gate[i][j] = int(bool(gate[i][j]))
            a.drop[i][j] = drops[i][j] if drops is not None else L_.dropout_cfg(None, 0, 0.0)
    a._refs = (qkv, masks, ctx, lse)      # the struct only holds raw pointers: keep the tensors alive
    return a


def attn_fwd(a):
    check(L_.lib.vk_gated_attn_fwd(C.byref(a), stream_ptr()))


def attn_bwd(a, dctx, dqkv, L, B, gate, H):
    b = L_.AttnBwdArgs()
    for m in range(2):
        if gate[m][0] or gate[m][1]:
            assert _bf16(dctx[m]).shape == (B * L[m], H)
            b.dctx[m] = dctx[m].data_ptr()
        if gate[m][0] or gate[m][1] or gate[0][m] or gate[1][m]:
            t = _bf16(dqkv[m])
            assert t.shape == (B * L[m], 3 * H) and t.is_contiguous()
            b.dq[m] = t.data_ptr()
            b.dk[m] = t.data_ptr() + H * 2
            b.dv[m] = t.data_ptr() + 2 * H * 2
            b.ldg[m] = 3 * H
    check(L_.lib.vk_gated_attn_bwd(C.byref(a), C.byref(b), stream_ptr()))


GLOBAL_CODE = {None: 0, "first": 1, "last": 2}


def task_batch(feat, boxes, n, wh, segs, mask_count, R, num_locs, add_global, scatter=None, ref_box=None, out=None, mean=None):
    """vk_task_batch: staged images (feat [S, Rcap, F] fp32, boxes [S, Rcap, 4] fp32 pixels, n [S] int32, wh [S, 2] int32) and per output
    block a segment list (segs [N, 2, 4] int32 = slot, src_from, dst_from, count) and a mask count (mask_count [N] int32) -> dict of
    `features` [N, R, F], `spatials` [N, R, num_locs], `image_mask` [N, R] int64 and -- `scatter=(csr [B + 1] int32, labels int32, scores fp32,
    num_labels)` -- `target` [B, num_labels], or -- `ref_box` [N, 4] fp32 pixels -- `target` [N, R, 1].  `out`: a dict of preallocated
    outputs to write into (every element is written)."""
    dev = feat.device
    S, Rcap, F = feat.shape
    N = segs.shape[0]
    for t, dt, shape in ((feat, torch.float32, (S, Rcap, F)), (boxes, torch.float32, (S, Rcap, 4)), (n, torch.int32, (S,)), (wh, torch.int32, (S, 2)),
                         (segs, torch.int32, (N, L.TASK_MAX_SEGS, 4)), (mask_count, torch.int32, (N,))):
        assert t.is_cuda and t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous(), (t.dtype, tuple(t.shape), shape)
    assert F % 4 == 0 and num_locs in (4, 5) and R > 0 and add_global in GLOBAL_CODE
    assert scatter is None or ref_box is None
    out = dict(out) if out else {}

    def buf(name, shape, dt):
        t = out.get(name)
        if t is None:
            t = out[name] = torch.empty(shape, dtype=dt, device=dev)
        assert t.is_cuda and t.dtype == dt and tuple(t.shape) == tuple(shape) and t.is_contiguous(), name
        return t

    features, spatials, image_mask = buf("features", (N, R, F), torch.float32), buf("spatials", (N, R, num_locs), torch.float32), buf("image_mask", (N, R), torch.int64)
    a = L.TaskBatchArgs(ptr(feat), ptr(boxes), ptr(n), ptr(wh), None, ptr(segs), ptr(mask_count), ptr(features), ptr(spatials), ptr(image_mask))
    a.S, a.Rcap, a.F, a.N, a.R, a.num_locs, a.add_global = S, Rcap, F, N, R, num_locs, GLOBAL_CODE[add_global]
    if add_global is not None:
        if mean is None:
            mean = torch.empty(S, F, dtype=torch.float32, device=dev)
        assert mean.is_cuda and mean.dtype == torch.float32 and mean.numel() >= S * F and mean.is_contiguous()
        a.mean = ptr(mean)
    if scatter is not None:
        csr, labels, scores, num_labels = scatter
        B = csr.numel() - 1
        assert csr.dtype == torch.int32 and labels.dtype == torch.int32 and scores.dtype == torch.float32 and csr.is_cuda and labels.is_cuda and scores.is_cuda
        assert B >= 0 and labels.numel() == scores.numel() and num_labels > 0
        target = buf("target", (B, num_labels), torch.float32)
        a.target, a.csr, a.labels, a.scores, a.B, a.num_labels, a.target_kind = ptr(target), ptr(csr), ptr(labels), ptr(scores), B, num_labels, L.TASK_TARGET_SCATTER
    elif ref_box is not None:
        assert ref_box.is_cuda and ref_box.dtype == torch.float32 and tuple(ref_box.shape) == (N, 4) and ref_box.is_contiguous()
        target = buf("target", (N, R, 1), torch.float32)
        a.target, a.ref_box, a.target_kind = ptr(target), ptr(ref_box), L.TASK_TARGET_IOU
    check(L.lib.vk_task_batch(C.byref(a), stream_ptr()))
    a._refs = (feat, boxes, n, wh, segs, mask_count, mean, scatter, ref_box)
    return out


def _pool_args(regions, where, feat_off, box_off, mean_off, n, wh, F, add_global):
    """the slot half of vk_task_pool_args: regions = (pool, scratch) uint8 device tensors (None = empty), per-slot tables on the device"""
    S = n.shape[0]
    for t, dt, shape in ((where, torch.int32, (S,)), (feat_off, torch.int64, (S,)), (box_off, torch.int64, (S,)), (n, torch.int32, (S,)), (wh, torch.int32, (S, 2))):
        assert t.is_cuda and t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous(), (t.dtype, tuple(t.shape), shape)
    assert len(regions) == 2 and F % 4 == 0 and F > 0 and add_global in GLOBAL_CODE
    a = L.TaskPoolArgs()
    for w, r in enumerate(regions):
        if r is not None and r.numel():
            assert r.is_cuda and r.dtype == torch.uint8 and r.is_contiguous() and r.data_ptr() % 16 == 0
            a.base[w], a.bytes[w] = r.data_ptr(), r.numel()
    a.where, a.feat_off, a.box_off, a.n, a.wh = ptr(where), ptr(feat_off), ptr(box_off), ptr(n), ptr(wh)
    if mean_off is not None:
        assert mean_off.is_cuda and mean_off.dtype == torch.int64 and tuple(mean_off.shape) == (S,) and mean_off.is_contiguous()
        a.mean_off = ptr(mean_off)
    a.S, a.F, a.R, a.num_locs, a.add_global = S, F, 1, 4, GLOBAL_CODE[add_global]
    a._refs = (regions, where, feat_off, box_off, mean_off, n, wh)
    return a


def task_pool_means(regions, where, feat_off, box_off, mean_off, n, wh, F, slots):
    """vk_task_pool_means: the global row (rows added in order in fp32, one division by n) of the slots the int32 device list `slots` names,
    written at their mean_off of region where[s].  Arguments as `task_batch_pool`."""
    assert mean_off is not None and slots.is_cuda and slots.dtype == torch.int32 and slots.dim() == 1 and slots.is_contiguous()
    a = _pool_args(regions, where, feat_off, box_off, mean_off, n, wh, F, "first")
    check(L.lib.vk_task_pool_means(C.byref(a), ptr(slots), slots.numel(), stream_ptr()))


def task_batch_pool(regions, where, feat_off, box_off, mean_off, n, wh, F, segs, mask_count, R, num_locs, add_global, scatter=None, ref_box=None,
                    out=None):
    """vk_task_batch_pool: `task_batch` over images kept in two byte regions.  regions = (pool, scratch) uint8 device tensors (either may be
    None); slot s holds features [n[s], F] at byte feat_off[s], boxes [n[s], 4] at box_off[s] and its global row [F] at mean_off[s] (needed
    when add_global is not None; written by `task_pool_means`) of region where[s] (int32 0 | 1; the offsets are int64 tensors).  Everything
    else, and the returned dict, as `task_batch`.  The slot tables are checked on the device: a slot that fails contributes no row."""
    dev = n.device
    N = segs.shape[0]
    for t, dt, shape in ((segs, torch.int32, (N, L.TASK_MAX_SEGS, 4)), (mask_count, torch.int32, (N,))):
        assert t.is_cuda and t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous(), (t.dtype, tuple(t.shape), shape)
    assert num_locs in (4, 5) and R > 0 and (add_global is None or mean_off is not None)
    assert scatter is None or ref_box is None
    a = _pool_args(regions, where, feat_off, box_off, mean_off, n, wh, F, add_global)
    out = dict(out) if out else {}

    def buf(name, shape, dt):
        t = out.get(name)
        if t is None:
            t = out[name] = torch.empty(shape, dtype=dt, device=dev)
        assert t.is_cuda and t.dtype == dt and tuple(t.shape) == tuple(shape) and t.is_contiguous(), name
        return t

    features, spatials, image_mask = buf("features", (N, R, F), torch.float32), buf("spatials", (N, R, num_locs), torch.float32), buf("image_mask", (N, R), torch.int64)
    a.segs, a.mask_count, a.features, a.spatials, a.image_mask = ptr(segs), ptr(mask_count), ptr(features), ptr(spatials), ptr(image_mask)
    a.N, a.R, a.num_locs = N, R, num_locs
    if scatter is not None:
        csr, labels, scores, num_labels = scatter
        B = csr.numel() - 1
        assert csr.dtype == torch.int32 and labels.dtype == torch.int32 and scores.dtype == torch.float32 and csr.is_cuda and labels.is_cuda and scores.is_cuda
        assert B >= 0 and labels.numel() == scores.numel() and num_labels > 0
        target = buf("target", (B, num_labels), torch.float32)
        a.target, a.csr, a.labels, a.scores, a.B, a.num_labels, a.target_kind = ptr(target), ptr(csr), ptr(labels), ptr(scores), B, num_labels, L.TASK_TARGET_SCATTER
    elif ref_box is not None:
        assert ref_box.is_cuda and ref_box.dtype == torch.float32 and tuple(ref_box.shape) == (N, 4) and ref_box.is_contiguous()
        target = buf("target", (N, R, 1), torch.float32)
        a.target, a.ref_box, a.target_kind = ptr(target), ptr(ref_box), L.TASK_TARGET_IOU
    check(L.lib.vk_task_batch_pool(C.byref(a), stream_ptr()))
    return out


def b64_jobs(fields):
    """fields: (text_off, dst_off, nsig, want_bytes) per job -> (the vk_b64_job table as an int32 host tensor [njobs, 6], max nsig).  Checks
    from the lengths what the device would refuse: want_bytes a multiple of 4 and nsig * 3 // 4, 16-byte aligned offsets."""
    import numpy as np
    tab = np.zeros(len(fields), np.dtype([("text_off", "<u8"), ("dst_off", "<u8"), ("nsig", "<u4"), ("want_bytes", "<u4")]))
    for j, (text_off, dst_off, nsig, want) in enumerate(fields):
        if want % 4 or want != nsig * 3 // 4 or nsig >= 1 << 31:
            raise ValueError("base64 job %d: %d characters do not decode to %d bytes of fp32" % (j, nsig, want))
        if text_off % 16 or dst_off % 16:
            raise ValueError("base64 job %d: offsets %d / %d are not 16-byte aligned" % (j, text_off, dst_off))
        tab[j] = (text_off, dst_off, nsig, want)
    return torch.from_numpy(tab.view(np.int32).reshape(len(fields), 6)), int(tab["nsig"].max()) if len(fields) else 0


def b64_decode_device(text, dst, jobs, max_nsig, status=None):
    """vk_b64_decode_device: `text` (uint8 device tensor, the packed text fields) decoded into `dst` (uint8 device tensor, or any contiguous
    device tensor taken as bytes) as the job table says (`jobs`: int32 device tensor [njobs, 6] from `b64_jobs`).  Returns the status words as
    an int32 device tensor [njobs] (view them as uint32 on the host): 0 decoded, 1 + offset of the first offending byte, 0xFFFFFFFE for a job
    the device's table check refused."""
    assert text.is_cuda and text.dtype == torch.uint8 and text.is_contiguous() and dst.is_cuda and dst.is_contiguous()
    assert jobs.is_cuda and jobs.dtype == torch.int32 and jobs.dim() == 2 and jobs.shape[1] == 6 and jobs.is_contiguous()
    njobs = jobs.shape[0]
    if status is None:
        status = torch.empty(njobs, dtype=torch.int32, device=jobs.device)
    assert status.is_cuda and status.dtype == torch.int32 and status.numel() >= njobs and status.is_contiguous()
    check(L.lib.vk_b64_decode_device(ptr(text), text.numel(), ptr(dst), dst.numel() * dst.element_size(), ptr(jobs), njobs, int(max_nsig), ptr(status),
                                     stream_ptr()))
    return status[:njobs]


def _ranks_csr(caption_image, Ni):
    """the captions of each image as a CSR over the captions with a valid image (sort + counts; nothing here reads a value on the host)
    -> image_ptr int32 [Ni + 1], image_captions int32 [Nc]"""
    dev = caption_image.device
    ci = caption_image.long()
    bucket = torch.where((ci >= 0) & (ci < Ni), ci, torch.full_like(ci, Ni))
    image_captions = torch.sort(bucket, stable=True)[1].int()
    counts = torch.zeros(Ni + 1, dtype=torch.int64, device=dev).index_add_(0, bucket, torch.ones_like(bucket))
    image_ptr = torch.zeros(Ni + 1, dtype=torch.int32, device=dev)
    image_ptr[1:] = torch.cumsum(counts[:Ni], 0)
    return image_ptr, image_captions


def retrieval_ranks(S, caption_image, topk=20):
    """vk_retrieval_ranks (csrc/ranks.hip): S fp32 [Nc, Ni] on the GPU (rows `S.stride(0) >= Ni` apart: a column slice of a wider tensor is
    taken as it is), caption_image int32 [Nc] = the index of each caption's image -> (rank_ir int32 [Nc], topk_ir int32 [Nc, topk],
    rank_tr int32 [Ni]), all on the device, no host synchronisation.

    One total order defines all three: element (score s, index j) has the key sortable(s) << 32 | (0xFFFFFFFF - j), where sortable maps
    fp32 to uint32 monotonically, -0.0 and +0.0 alike and every NaN lowest; a larger key ranks earlier.  That is the position in
    np.argsort(-s, kind="stable") (NaN last).  rank_ir[c]: images ranked before caption c's own in row c, -1 when caption_image[c] is outside
    [0, Ni); topk_ir[c]: the first `topk` (0..64) images of row c, -1 past Ni; rank_tr[i]: the best position, in column i, of a caption of
    image i, -1 when it has none.  The reference driver calls np.argsort(-s) without `kind`, which is not stable: its rank is only defined
    where the target's score is untied in its row / column, and on those inputs the two agree."""
    assert S.is_cuda and S.dtype == torch.float32 and S.dim() == 2 and S.shape[0] > 0 and S.shape[1] > 0, "S: a non-empty fp32 [Nc, Ni] cuda tensor"
    Nc, Ni = S.shape
    assert S.stride(1) == 1 or Ni == 1, "the scores of a row must be adjacent"
    ld = S.stride(0) if Nc > 1 else max(S.stride(0), Ni)
    have = S.untyped_storage().nbytes() // 4 - S.storage_offset()
    assert ld >= Ni and (Nc - 1) * ld + Ni <= have, "S does not cover %d rows of %d scores %d apart" % (Nc, Ni, ld)
    assert caption_image.is_cuda and caption_image.dtype == torch.int32 and tuple(caption_image.shape) == (Nc,) and caption_image.is_contiguous()
    K, dev = int(topk), S.device
    image_ptr, image_captions = _ranks_csr(caption_image, Ni)
    rank_ir, rank_tr = torch.empty(Nc, dtype=torch.int32, device=dev), torch.empty(Ni, dtype=torch.int32, device=dev)
    topk_ir = torch.empty(Nc, max(K, 0), dtype=torch.int32, device=dev)
    work = torch.empty(2, Nc, dtype=torch.int32, device=dev)
    a = L.RetrievalRanksArgs(ptr(S), ptr(caption_image), ptr(image_ptr), ptr(image_captions), ptr(rank_ir), ptr(topk_ir) if K > 0 else None, ptr(rank_tr),
                             ptr(work[0]), ptr(work[1]), ld, Nc, Ni, K, 0)
    check(L.lib.vk_retrieval_ranks(C.byref(a), stream_ptr()))
    return rank_ir, topk_ir, rank_tr


class RanksShard:
    """What `retrieval_ranks_shard` leaves for the rest of the sharded sequence.  rank_ir int32 [Nc], topk_ir int32 [Nc, K] and target_key
    int32 [Nc] (the bits of the kernel's uint32 words) are global-sized: written at the shard's rows [row0, row0 + nrows), zero elsewhere, so
    the element-wise integer SUM over all shards is the whole array.  image_ptr / image_captions: the global CSR."""

    def __init__(self, S, ld, row0, nrows, Nc, Ni, K, rank_ir, topk_ir, target_key, image_ptr, image_captions):
        self.S, self.ld, self.row0, self.nrows, self.Nc, self.Ni, self.K = S, ld, row0, nrows, Nc, Ni, K
        self.rank_ir, self.topk_ir, self.target_key, self.image_ptr, self.image_captions = rank_ir, topk_ir, target_key, image_ptr, image_captions

    def args(self, **kw):
        a = L.RetrievalRanksShardArgs(S=ptr(self.S) if self.nrows else None, image_ptr=ptr(self.image_ptr), image_captions=ptr(self.image_captions),
                                      ld=self.ld, Nc=self.Nc, Ni=self.Ni, K=self.K, row0=self.row0, nrows=self.nrows)
        for k, v in kw.items():
            setattr(a, k, v)
        return a


def retrieval_ranks_shard(S_local, row0, Nc, caption_image, topk=20):
    """vk_retrieval_ranks_shard_rows (csrc/ranks.hip): the row pass of `retrieval_ranks` for the shard that owns the captions
    [row0, row0 + nrows) of Nc.  S_local fp32 [nrows, Ni] on the GPU (rows `stride(0) >= Ni` apart; nrows may be 0), caption_image int32 [Nc]
    = the GLOBAL table -> a `RanksShard`.  One launch (none for an empty shard) after the CSR build, no host synchronisation.

    The sequence, with `+` an integer sum over the shards (an all_reduce, or a plain add when one device holds several):
        sh = retrieval_ranks_shard(S_local, row0, Nc, caption_image, topk)
        count = retrieval_ranks_shard_counts(sh, + sh.target_key)
        rank_tr = retrieval_ranks_finish(+ count, sh.image_ptr, Ni);   rank_ir = + sh.rank_ir;   topk_ir = + sh.topk_ir
    gives the three outputs of `retrieval_ranks` on the whole matrix, bit for bit."""
    assert S_local.is_cuda and S_local.dtype == torch.float32 and S_local.dim() == 2 and S_local.shape[1] > 0, "S_local: an fp32 [nrows, Ni] cuda tensor"
    nrows, Ni = S_local.shape
    row0, Nc, K, dev = int(row0), int(Nc), int(topk), S_local.device
    assert Nc > 0 and 0 <= row0 and row0 + nrows <= Nc, "rows [%d, %d) are not inside the %d captions" % (row0, row0 + nrows, Nc)
    ld = Ni
    if nrows:
        assert S_local.stride(1) == 1 or Ni == 1, "the scores of a row must be adjacent"
        ld = S_local.stride(0) if nrows > 1 else max(S_local.stride(0), Ni)
        have = S_local.untyped_storage().nbytes() // 4 - S_local.storage_offset()
        assert ld >= Ni and (nrows - 1) * ld + Ni <= have, "S_local does not cover %d rows of %d scores %d apart" % (nrows, Ni, ld)
    assert caption_image.is_cuda and caption_image.dtype == torch.int32 and tuple(caption_image.shape) == (Nc,) and caption_image.is_contiguous()
    image_ptr, image_captions = _ranks_csr(caption_image, Ni)
    rank_ir, target_key = torch.zeros(Nc, dtype=torch.int32, device=dev), torch.zeros(Nc, dtype=torch.int32, device=dev)
    topk_ir = torch.zeros(Nc, max(K, 0), dtype=torch.int32, device=dev)
    sh = RanksShard(S_local, ld, row0, nrows, Nc, Ni, K, rank_ir, topk_ir, target_key, image_ptr, image_captions)
    a = sh.args(caption_image=ptr(caption_image), rank_ir=ptr(rank_ir), topk_ir=ptr(topk_ir) if K > 0 else None, target_key=ptr(target_key))
    check(L.lib.vk_retrieval_ranks_shard_rows(C.byref(a), stream_ptr()))
    return sh


def retrieval_ranks_shard_counts(shard, target_key_all, out=None):
    """vk_retrieval_ranks_shard_cols: the shard's part of the column counts.  target_key_all int32 [Nc]: the sum of every shard's
    `target_key` -> count int32 [Nc] (one word per CSR entry); the sum of all shards' counts is the unsharded count array.  `out`: a count
    array to ADD to instead of a fresh one (VK_RANKS_ACCUMULATE: several local blocks on one device).  One memset (without `out`) and one
    launch (none for an empty shard), no host synchronisation."""
    sh = shard
    assert isinstance(sh, RanksShard), "shard: what retrieval_ranks_shard returned"
    for t, what in ((target_key_all, "target_key_all"), (out, "out")):
        assert t is None or (t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == (sh.Nc,) and t.is_contiguous() and t.device == sh.S.device), \
            "%s: a contiguous int32 [%d] tensor on the shard's device" % (what, sh.Nc)
    assert target_key_all is not None, "target_key_all: a contiguous int32 [%d] tensor on the shard's device" % sh.Nc
    count = out if out is not None else torch.empty(sh.Nc, dtype=torch.int32, device=sh.S.device)
    a = sh.args(target_key=ptr(target_key_all), count=ptr(count), flags=L.RANKS_ACCUMULATE if out is not None else 0)
    check(L.lib.vk_retrieval_ranks_shard_cols(C.byref(a), stream_ptr()))
    return count


def retrieval_ranks_finish(count_sum, image_ptr, Ni):
    """vk_retrieval_ranks_finish: count_sum int32 [Nc] = the sum of all shards' counts, image_ptr int32 [Ni + 1] -> rank_tr int32 [Ni], per
    image the minimum over its CSR entries, -1 without one.  One launch, no host synchronisation."""
    Ni = int(Ni)
    assert count_sum.is_cuda and count_sum.dtype == torch.int32 and count_sum.dim() == 1 and count_sum.numel() > 0 and count_sum.is_contiguous(), "count_sum: a contiguous int32 [Nc] cuda tensor"
    assert image_ptr.dtype == torch.int32 and tuple(image_ptr.shape) == (Ni + 1,) and image_ptr.is_contiguous() and image_ptr.device == count_sum.device, "image_ptr: int32 [Ni + 1] beside count_sum"
    rank_tr = torch.empty(Ni, dtype=torch.int32, device=count_sum.device)
    a = L.RetrievalRanksShardArgs(image_ptr=ptr(image_ptr), count=ptr(count_sum), rank_tr=ptr(rank_tr), Nc=count_sum.numel(), Ni=Ni)
    check(L.lib.vk_retrieval_ranks_finish(C.byref(a), stream_ptr()))
    return rank_tr


def image_means(feat, n):
    """vk_image_means (csrc/knn.hip): feat fp32 [S, Rcap, F] and n int32 [S] on the GPU, as `ImageStager.stage()` leaves them (rows >= n[s]
    are not read) -> mean fp32 [S, F] = np.sum(feat[s, :n[s]], 0) / n[s] bit for bit (rows added in order in fp32, then one division)."""
    assert feat.dtype == torch.float32 and feat.dim() == 3 and feat.is_contiguous() and feat.shape[1] > 0 and feat.shape[2] > 0, "feat: a contiguous fp32 [S, Rcap, F] tensor"
    S, Rcap, F = feat.shape
    assert n.dtype == torch.int32 and tuple(n.shape) == (S,) and n.is_contiguous(), "n: a contiguous int32 [S] tensor"
    assert feat.is_cuda and n.is_cuda, "feat and n must be cuda tensors"
    mean = torch.empty(S, F, dtype=torch.float32, device=feat.device)
    a = L.ImageMeansArgs(ptr(feat), ptr(n), ptr(mean), S, Rcap, F, 0)
    check(L.lib.vk_image_means(C.byref(a), stream_ptr()))
    return mean


def knn_default_shortlist(k):
    """the screen's shortlist for k neighbours: k plus a margin of 28 % (128 for k = 100), at most VK_KNN_MAX_SHORTLIST"""
    return min(L.KNN_MAX_SHORTLIST, max(k, -(-k * 32 // 25)))


def knn_pool(X, k, shortlist=None, return_stats=False, screen_only=False):
    """vk_knn_pool (csrc/knn.hip): X fp32 [N, D] on the GPU, contiguous and finite -> int32 [N, k], row i = the first k indices j under the
    total order (d2(i, j), j) with d2 the float64 squared Euclidean distance; j = i is a candidate like any other (it comes first unless an
    equal vector has a lower index).  Exact for every finite input: an fp32-MFMA screen keeps `shortlist` candidates per
    row (default knn_default_shortlist(k), cut to N), float64 orders and certifies them, uncertified rows are recomputed in float64.
    `return_stats=True` also returns dict(certified=..., fallback=...), the row counts of the two paths (one host read).  `screen_only`
    runs the screen alone (timing): the returned tensor is then not written."""
    assert X.dtype == torch.float32, "X: fp32 expected, got %s" % X.dtype
    assert X.dim() == 2 and X.shape[0] > 0 and X.shape[1] > 0, "X: a non-empty [N, D] matrix expected, got shape %s" % (tuple(X.shape),)
    assert X.is_contiguous(), "X must be contiguous"
    N, D = X.shape
    k = int(k)
    if k < 1:
        raise ValueError("k = %d: at least one neighbour" % k)
    if k > N:
        raise ValueError("k = %d neighbours of N = %d vectors: k must be less than or equal to the number of vectors" % (k, N))
    if k > L.KNN_MAX_SHORTLIST:
        raise ValueError("k = %d exceeds the shortlist limit of %d" % (k, L.KNN_MAX_SHORTLIST))
    M = knn_default_shortlist(k) if shortlist is None else int(shortlist)
    if shortlist is not None and not k <= M <= L.KNN_MAX_SHORTLIST:
        raise ValueError("shortlist = %d: expected k = %d <= shortlist <= %d" % (M, k, L.KNN_MAX_SHORTLIST))
    M = min(M, N)
    assert X.is_cuda, "X must be a cuda tensor"
    if not bool(torch.isfinite(X).all()):
        raise ValueError("X holds non-finite values")
    nbytes = L.lib.vk_knn_pool_work_bytes(N, D, k, M)
    if nbytes < 0:
        raise L.VoltaHipError(L.lib.vk_last_error().decode())
    dev = X.device
    work = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    work = work[(-work.data_ptr()) % 256:]
    out = torch.empty(N, k, dtype=torch.int32, device=dev)
    stats = torch.empty(2, dtype=torch.int32, device=dev)
    a = L.KnnPoolArgs(ptr(X), ptr(out), ptr(work), ptr(stats), nbytes, N, D, k, M, L.KNN_SCREEN_ONLY if screen_only else 0, 0)
    check(L.lib.vk_knn_pool(C.byref(a), stream_ptr()))
    work.record_stream(torch.cuda.current_stream())
    if return_stats:
        c, f = stats.tolist()
        return out, dict(certified=c, fallback=f)
    return out


# ---------------------------------------------------------------------------------------------- LoRA (csrc/lora.hip)
def _extent(t):
    """Elements from the tensor's first one to the end of its storage."""
    return t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()


def _lora_common(X, A, B, T, Y, M, what, cap=1024, y="a [M, N] column range"):
    r, K = A.shape
    N = B.shape[0]
    assert r in (4, 8, 16, 32) and tuple(B.shape) == (N, r), "A [r, K] and B [N, r] with r in 4, 8, 16, 32"
    assert K % 64 == 0 and N % 64 == 0 and K <= cap and N <= cap, "K and N: multiples of 64, at most %d" % cap
    for t in (X, A, B, T, Y):
        _bf16(t)
        assert t.data_ptr() % 16 == 0, "16-byte alignment required"
    assert A.is_contiguous() and B.is_contiguous() and T.is_contiguous(), "A, B and T are dense"
    ldx, ldy = X.stride(0), Y.stride(0)
    assert X.stride(1) == 1 and Y.stride(1) == 1 and ldx % 8 == 0 and ldy % 8 == 0 and ldx >= K and ldy >= N
    assert X.shape[1] == K and Y.shape[1] == N, "%s: X [M, K] and %s" % (what, y)
    assert M <= X.shape[0] and M <= Y.shape[0] and (M == 0 or ((M - 1) * ldx + K <= _extent(X) and (M - 1) * ldy + N <= _extent(Y)))
    assert T.numel() >= M * r
    return r, K, N, ldx, ldy


def _lora_work(work_bytes, arr, n, work, device="cuda"):
    """The workspace of a backward call: `work`, or a new buffer, of at least what `work_bytes` asks for these problems."""
    need = getattr(L.lib, work_bytes)(arr, n)
    assert need > 0, work_bytes + " refused the problems"
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=device)
    assert work.numel() * work.element_size() >= need and work.data_ptr() % 16 == 0
    return work


def _lora_run(fn, cls, problems, drops=None, work_bytes=None, work=None):
    """One vk_lora_* call: the problem array, a _drop call's dropout array, a backward call's workspace (which it returns)."""
    n = len(problems)
    arr = (cls * n)(*problems)
    args = [arr] if drops is None else [arr, _drop_array(problems, drops)]
    if work_bytes is not None:
        work = _lora_work(work_bytes, arr, n, work)
        check(getattr(L.lib, fn)(*args, n, ptr(work), stream_ptr()))
    else:
        check(getattr(L.lib, fn)(*args, n, stream_ptr()))
    return work


def lora_problem(X, A, B, T, Y, scale, M=None, dyn=None):
    """One vk_lora_problem: Y [M, N] is a column range (a view) of the qkv buffer; T [M, r] receives bf16(X A^T)."""
    M = X.shape[0] if M is None else M
    r, K, N, ldx, ldy = _lora_common(X, A, B, T, Y, M, "lora_problem")
    return L.LoraProblem(ptr(X), ptr(A), ptr(B), ptr(T), ptr(Y), ptr(dyn), M, K, N, r, ldx, ldy, float(scale), 0)


def lora_bwd_problem(X, A, B, T, dY, dT, dX, dA, dB, scale, M=None, accumulate=False, dyn=None):
    """One vk_lora_bwd_problem; dX None: the input gradient is not live."""
    M = X.shape[0] if M is None else M
    r, K, N, ldx, ldy = _lora_common(X, A, B, T, dY, M, "lora_bwd_problem")
    _bf16(dT)
    assert dT.is_contiguous() and dT.numel() >= M * r and dT.data_ptr() % 16 == 0
    for g, shape in ((dA, (r, K)), (dB, (N, r))):
        assert g.dtype == torch.float32 and g.is_cuda and g.is_contiguous() and tuple(g.shape) == shape and g.data_ptr() % 16 == 0
    lddx = 0
    if dX is not None:
        _bf16(dX)
        lddx = dX.stride(0)
        assert dX.stride(1) == 1 and dX.shape[1] == K and lddx % 8 == 0 and lddx >= K and dX.data_ptr() % 16 == 0
        assert M <= dX.shape[0] and (M == 0 or (M - 1) * lddx + K <= _extent(dX))
    return L.LoraBwdProblem(ptr(X), ptr(A), ptr(B), ptr(T), ptr(dY), ptr(dT), ptr(dX), ptr(dA), ptr(dB), ptr(dyn), M, K, N, r, ldx, ldy, lddx,
                            int(bool(accumulate)), float(scale), 0)


def lora_fwd(problems):
    _lora_run("vk_lora_fwd", L.LoraProblem, problems)


def lora_bwd_work(problems, device):
    return _lora_work("vk_lora_bwd_work_bytes", (L.LoraBwdProblem * len(problems))(*problems), len(problems), None, device)


def lora_bwd(problems, work=None):
    return _lora_run("vk_lora_bwd", L.LoraBwdProblem, problems, work_bytes="vk_lora_bwd_work_bytes", work=work)


# ---- adapters on a whole projection (vk_lora_proj_*): K and N up to 4096, the GELU in the forward, a saved gelu' in the input gradient
def _lora_side(t, M, cols, what):
    """A bf16 [M, cols] operand beside X or Y (G, R, dX) -> its leading dimension."""
    _bf16(t)
    ld = t.stride(0)
    assert t.stride(1) == 1 and t.shape[1] == cols and ld % 8 == 0 and ld >= cols and t.data_ptr() % 16 == 0, what
    assert M <= t.shape[0] and (M == 0 or (M - 1) * ld + cols <= _extent(t)), what
    return ld


def lora_proj_problem(X, A, B, T, Y, scale, G=None, M=None, dyn=None):
    """One vk_lora_proj_problem.  G None: Y += s (X A^T) B^T; G [M, N]: Y = gelu(Y + ...), G = gelu'(Y + ...)."""
    M = X.shape[0] if M is None else M
    r, K, N, ldx, ldy = _lora_common(X, A, B, T, Y, M, "lora_proj_problem", 4096, "Y [M, N]")
    ldg = 0 if G is None else _lora_side(G, M, N, "G")
    return L.LoraProjProblem(ptr(X), ptr(A), ptr(B), ptr(T), ptr(Y), ptr(G), ptr(dyn), M, K, N, r, ldx, ldy, ldg, float(scale), int(G is not None))


def lora_proj_bwd_problem(X, A, B, T, dY, dT, dX, dA, dB, scale, R=None, M=None, accumulate=False, dyn=None):
    """One vk_lora_proj_bwd_problem; dX None: the input gradient is not live; dA and dB None: a frozen adapter; R: the gelu' buffer of the
    GEMM that produced X, multiplied into the adapter's share of dX."""
    M = X.shape[0] if M is None else M
    r, K, N, ldx, ldy = _lora_common(X, A, B, T, dY, M, "lora_proj_bwd_problem", 4096, "Y [M, N]")
    _bf16(dT)
    assert dT.is_contiguous() and dT.numel() >= M * r and dT.data_ptr() % 16 == 0
    assert (dA is None) == (dB is None), "dA and dB: both or neither"
    if dA is not None:
        for g, shape in ((dA, (r, K)), (dB, (N, r))):
            assert g.dtype == torch.float32 and g.is_cuda and g.is_contiguous() and tuple(g.shape) == shape and g.data_ptr() % 16 == 0
    lddx = 0 if dX is None else _lora_side(dX, M, K, "dX")
    ldr = 0 if R is None else _lora_side(R, M, K, "R")
    return L.LoraProjBwdProblem(ptr(X), ptr(A), ptr(B), ptr(T), ptr(dY), ptr(dT), ptr(dX), ptr(dA), ptr(dB), ptr(R), ptr(dyn), M, K, N, r, ldx, ldy,
                                lddx, ldr, int(bool(accumulate)), float(scale))


def lora_proj_fwd(problems):
    _lora_run("vk_lora_proj_fwd", L.LoraProjProblem, problems)


def lora_proj_bwd(problems, work=None):
    return _lora_run("vk_lora_proj_bwd", L.LoraProjBwdProblem, problems, work_bytes="vk_lora_proj_bwd_work_bytes", work=work)


# ---- LoRA dropout (vk_lora_*_drop): the calls above with one dropout entry per problem, a keep mask on the adapter's input
def lora_drop(seed, site, p):
    """The vk_dropout of one problem: `seed` a device int64 [1] tensor (None with p = 0), `site` the problem's own site, p the rate."""
    return L.dropout_cfg(ptr(seed), int(site), float(p))


def _drop_array(problems, drops):
    assert len(drops) == len(problems), "one dropout entry per problem"
    return (L.Dropout * len(drops))(*drops)


def lora_fwd_drop(problems, drops):
    _lora_run("vk_lora_fwd_drop", L.LoraProblem, problems, drops)


def lora_bwd_drop(problems, drops, work=None):
    return _lora_run("vk_lora_bwd_drop", L.LoraBwdProblem, problems, drops, "vk_lora_bwd_work_bytes", work)


def lora_proj_fwd_drop(problems, drops):
    _lora_run("vk_lora_proj_fwd_drop", L.LoraProjProblem, problems, drops)


def lora_proj_bwd_drop(problems, drops, work=None):
    return _lora_run("vk_lora_proj_bwd_drop", L.LoraProjBwdProblem, problems, drops, "vk_lora_proj_bwd_work_bytes", work)
