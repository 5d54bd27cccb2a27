"""Image-caption retrieval scoring (the reference's eval_retrieval.py:161-222) with the modality-only layers run once per input.

The driver scores every caption against every image by calling the whole model on [caption repeated 500 times, 500 images] pairs.  In a
two-stream model the sub-layers in front of the first cross-attention depend on one modality only, and so does a per-modality embedding:
`split_plan` finds them, `RetrievalScorer.encode_captions` / `encode_images` run them once per caption / image, and `score_matrix` /
`score_pairs` run only the mixing suffix per pair, on inputs that one vk_pair_gather launch per pair chunk copies out of the prefix outputs
(csrc/pairs.hip).  Every launch of these plans is a launch of the model's own forward at another batch size: eval semantics, bf16
activations, no dropout, no backward.

Precision: `projection_dtype="fp8"` runs the Q|K|V and feed-forward projections of every scored sub-layer on the e4m3 MFMA path
(csrc/fp8.hip), whatever the model's own `set_projection_dtype` switch says; a pair's logit is then bit for bit what the driver's loop gets
from the model after `set_projection_dtype("fp8")` -- the fp8 model's scores and ranks, not the bf16 model's.  "bf16" asks for the bf16
projections explicitly; None is bf16 too, but refuses a model whose own switch was left on fp8.  Where a prefix ends in a sub-layer, the
e4m3 copy its last LayerNorm wrote (and the copy's row scales) is kept in the handle and gathered per pair, so that the suffix's first
projection reads the bits the whole model reads there (`engine.pair_segments`, engine/builder.py).

    scorer = RetrievalScorer(model, task_id="TASK8", pair_chunk=1000)
    caps = scorer.encode_captions(input_ids, segment_ids, input_mask)      # [Nc, T] each, on the GPU
    imgs = scorer.encode_images(features, spatials, image_mask)            # [Ni, R, 2048], [Ni, R, num_locs], [Ni, R]
    S = scorer.score_matrix(caps, imgs)                                    # fp32 [Nc, Ni] on the device, no host synchronisation
    s = scorer.score_pairs(caps, imgs, cap_idx, img_idx)                   # fp32 [P] for an explicit pair list (re-ranking)

Scores: a BertForVLTasks with a VL-logit task gives its raw logit (eval_retrieval.py:191-195); a BertForVLPreTraining (zero-shot) gives
softmax(seq_relationship_score)[:, 0] (eval_retrieval.py:181-185).  The scorer leaves the model's state alone: `training`, the dropout step
counter, the model's last forward and its engines; it reads the current weights (the bf16 copies are refreshed as the model's forward
refreshes them).  Handles hold prefix outputs computed with the weights of the time they were encoded.

`evaluate_retrieval(model, dset_val, task_id)` is the whole of eval_retrieval.py:161-263 on top of it: the device arrays of a
`volta_amd.datasets.RetrievalDatasetVal`, the score matrix, `ops.retrieval_ranks` (csrc/ranks.hip: ranks and top-k by counting keys, no sort)
and one transfer of the integer ranks; the recall / rank numbers are the driver's own float64 arithmetic on that copy.  With `group=` the
captions are sharded over the ranks of a process group and the ranks' parts are merged exactly (`ops.retrieval_ranks_shard` and its two
companions, four integer all_reduce calls).
"""
import ctypes as C

import numpy as np
import torch

from .modules import sublayer_schedule


def _first_mixing(config):
    """Number of the first sub-layer in which a stream attends to the other one (len(schedule) when none does)."""
    sched = sublayer_schedule(config)
    mix = set(config.tv_attn_sublayers) | set(config.vt_attn_sublayers)
    return min(mix) if mix else len(sched)


def split_plan(config):
    """(sub-layers that run per caption, sub-layers that run per image, whether each embedding is per modality).

    The first sub-layer in tv_attn_sublayers | vt_attn_sublayers ends both prefixes: before it, an attention sub-layer in
    tt_attn_sublayers and a feed-forward sub-layer in t_ff_sublayers transform the text stream from text alone, vv_attn_sublayers and
    v_ff_sublayers the vision stream from vision alone.  VisualBERT's and VL-BERT's embeddings mix the modalities (one LayerNorm over
    [text | vision], VL-BERT's text tokens carry a region's feature), so those models have no per-modality stage at all."""
    if config.image_embeddings not in ("vilbert", "lxmert", "uniter"):
        return [], [], False
    first = _first_mixing(config)
    text, vision = [], []
    for n, typ in sublayer_schedule(config):
        if n >= first:
            break
        if n in (config.tt_attn_sublayers if typ == "attn" else config.t_ff_sublayers):
            text.append(n)
        if n in (config.vv_attn_sublayers if typ == "attn" else config.v_ff_sublayers):
            vision.append(n)
    return text, vision, True


class Items:
    """Encoded captions (side 0) or images (side 1): the per-item inputs of the pair suffix, by the names of its `pair_inputs`."""

    def __init__(self, scorer, side, n, length, tensors):
        self.scorer, self.side, self.n, self.length, self.tensors = scorer, side, n, length, tensors

    def __len__(self):
        return self.n


def pair_gather_segments(config, projection_dtype=None):
    """[(name, side 0 caption | 1 image)]: what one vk_pair_gather launch copies per pair for this config and precision (host only)."""
    from .engine import pair_segments
    if projection_dtype not in (None, "bf16", "fp8"):
        raise ValueError("projection_dtype %r: None | 'bf16' | 'fp8'" % (projection_dtype,))
    return pair_segments(split_plan(config), projection_dtype == "fp8")


class RetrievalScorer:
    def __init__(self, model, task_id=None, pair_chunk=1000, projection_dtype=None):
        from .modeling import BertForVLPreTraining, BertForVLTasks
        if isinstance(model, BertForVLTasks):
            if task_id not in model.task_cfg or task_id not in model.clfs_dict:
                raise ValueError("unknown task id %r" % (task_id,))
            if model.task_cfg[task_id]["type"] != "VL-logit":
                raise ValueError("task %r is of type %r; retrieval scores a VL-logit task (eval_retrieval.py:191)" % (task_id, model.task_cfg[task_id]["type"]))
            self.task = (task_id, model.task_cfg[task_id])
        elif isinstance(model, BertForVLPreTraining):
            if task_id is not None:
                raise ValueError("the zero-shot scorer (BertForVLPreTraining) takes no task id")
            self.task = None
        else:
            raise ValueError("scores come from a BertForVLTasks with a VL-logit task or a BertForVLPreTraining, not from %s" % type(model).__name__)
        cfg = model.config
        if cfg.fusion_method not in ("mul", "sum", "text"):
            raise ValueError("fusion method %r has no ITM head (encoders.py:744-747, 1192-1193)" % cfg.fusion_method)
        if projection_dtype not in (None, "bf16", "fp8"):
            raise ValueError("projection_dtype %r: None | 'bf16' | 'fp8'" % (projection_dtype,))
        self.projection_dtype = projection_dtype
        self._refuse_model_switch(model)
        self.fp8 = projection_dtype == "fp8"
        if self.fp8:
            from .engine import wide_geometry
            wide = wide_geometry(cfg)
            if wide is not None:
                raise NotImplementedError("projection_dtype='fp8': the e4m3 projection path covers the single-width (ctrl_*) geometry, not %s" % wide)
        if int(pair_chunk) < 1:
            raise ValueError("pair_chunk must be positive, got %r" % (pair_chunk,))
        self.device = next(model.parameters()).device
        if self.device.type != "cuda":
            raise ValueError("the model is not on the GPU (model.cuda())")
        self.model, self.cfg, self.pair_chunk = model, cfg, int(pair_chunk)
        self.split = split_plan(cfg)
        # VL-BERT's text position ids depend on the batch: past the SHORTEST caption of the batch every text position is shifted by the
        # region count (vk_vlbert_positions, the reference's expanded-view quirk, volta/embeddings.py).  The driver's batches hold one
        # caption, so the scorer's pair chunks do as well, and a pair's score is the one the driver computes.
        self.one_caption_per_chunk = cfg.image_embeddings == "vl-bert"
        self._arena, self._engines = None, {}

    # ------------------------------------------------------------------ plumbing
    def _refuse_model_switch(self, model):
        """Without an explicit projection_dtype the scorer is bf16 and will not guess for a model whose own switch says fp8."""
        if self.projection_dtype is None and model.__dict__.get("_fp8", False):
            raise NotImplementedError("the retrieval scorer runs the bf16 projections unless told otherwise and the model's switch is on fp8: "
                                      "pass projection_dtype='fp8' or 'bf16', or set_projection_dtype('bf16') first")

    def _prepare(self):
        """The model's arena with current bf16 (and, for an fp8 scorer, e4m3) weights; the scorer's plans are rebuilt when the arena was."""
        self._refuse_model_switch(self.model)
        arena = self.model.materialize()
        if arena is not self._arena:
            self._arena, self._engines = arena, {}
        arena.sync_optimizer()           # a pipelined optimizer step still in flight: every plan here reads all of the weights
        arena.refresh_shadow()
        if self.fp8:
            arena.refresh_fp8()          # no launch unless the weights changed (weights_epoch) or a plan registered new sites
        return arena

    def _engine(self, part, B, T, Rv):
        from .engine import StepEngine
        key = (part, B, T, Rv)
        eng = self._engines.get(key)
        if eng is None:
            eng = StepEngine(self.cfg, self._arena, B, T, Rv, False, heads="score", task=self.task if part == "pair" else None, part=part, split=self.split,
                             projection_dtype="fp8" if self.fp8 else "bf16")
            self._engines[key] = eng
            if self.fp8:
                self._arena.refresh_fp8()        # building the plan registered its weights' e4m3 sites: quantise them before its first run
        return eng

    def _run_prefix(self, part, tensors, n, length, H, tag):
        """The prefix plan of `part` over n items in chunks: x_<tag> bf16 [n * length, H] and, where the plan's last LayerNorm wrote an e4m3
        copy (fp8 scorer, prefix ending in a sub-layer), x8_<tag> uint8 [n * length, round_up(H, 128)] and its row scales xs_<tag> fp32."""
        self._prepare()
        x = torch.empty(n * length, H, dtype=torch.bfloat16, device=self.device)
        x8 = xs = None
        for i0 in range(0, n, self.pair_chunk):
            nb = min(self.pair_chunk, n - i0)
            eng = self._engine(part, nb, length, 1) if part == "text" else self._engine(part, nb, 1, length)
            eng.bind_inputs({k: v[i0:i0 + nb] for k, v in tensors.items()})
            eng.fwd.run()
            r0, r1 = i0 * length, (i0 + nb) * length
            x[r0:r1].copy_(eng.score_out)
            if eng.score_x8 is not None:
                q, sc = eng.score_x8
                if x8 is None:
                    x8 = torch.empty(n * length, q.shape[1], dtype=torch.uint8, device=self.device)
                    xs = torch.empty(n * length, dtype=torch.float32, device=self.device)
                x8[r0:r1].copy_(q)
                xs[r0:r1].copy_(sc)
        out = {"x_" + tag: x}
        if x8 is not None:
            out["x8_" + tag], out["xs_" + tag] = x8, xs
        return out

    def _tensor(self, x, dtype, shape, what):
        if not isinstance(x, torch.Tensor):
            raise ValueError("%s must be a tensor" % what)
        if x.device != self.device:
            raise ValueError("%s is on %s, the model on %s" % (what, x.device, self.device))
        if tuple(x.shape) != tuple(shape):
            raise ValueError("%s has shape %s, expected %s" % (what, tuple(x.shape), tuple(shape)))
        return x.to(dtype).contiguous()

    # ------------------------------------------------------------------ prefixes
    def encode_captions(self, input_ids, segment_ids=None, input_mask=None):
        if not isinstance(input_ids, torch.Tensor) or input_ids.dim() != 2 or input_ids.shape[0] < 1 or input_ids.shape[1] < 1:
            raise ValueError("input_ids must be a non-empty [Nc, T] tensor")
        Nc, T = input_ids.shape
        ids = self._tensor(input_ids, torch.int64, (Nc, T), "input_ids")
        tt = self._tensor(segment_ids, torch.int64, (Nc, T), "segment_ids") if segment_ids is not None else torch.zeros_like(ids)
        mask = self._tensor(input_mask, torch.int64, (Nc, T), "input_mask") if input_mask is not None else torch.ones_like(ids)
        tensors = dict(input_ids=ids, token_type_ids=tt, attention_mask=mask)
        if self.split[2]:
            tensors.update(self._run_prefix("text", dict(tensors), Nc, T, self.cfg.hidden_size, "t"))
        return Items(self, 0, Nc, T, tensors)

    def encode_images(self, features, spatials, image_mask=None):
        if not isinstance(features, torch.Tensor) or features.dim() != 3 or features.shape[0] < 1 or features.shape[1] < 1:
            raise ValueError("features must be a non-empty [Ni, R, v_feature_size] tensor")
        Ni, Rv = features.shape[:2]
        feat = self._tensor(features, torch.float32, (Ni, Rv, self.cfg.v_feature_size), "features")
        loc = self._tensor(spatials, torch.float32, (Ni, Rv, self.cfg.num_locs), "spatials")
        mask = self._tensor(image_mask, torch.int64, (Ni, Rv), "image_mask") if image_mask is not None else torch.ones(Ni, Rv, dtype=torch.int64, device=self.device)
        tensors = dict(image_feat=feat, image_loc=loc, image_attention_mask=mask)
        if self.split[2]:
            tensors.update(self._run_prefix("image", dict(tensors), Ni, Rv, self.cfg.v_hidden_size, "v"))
        return Items(self, 1, Ni, Rv, tensors)

    # ------------------------------------------------------------------ pairs
    def _check_items(self, caps, imgs):
        if not (isinstance(caps, Items) and caps.side == 0 and caps.scorer is self):
            raise ValueError("caps must come from this scorer's encode_captions")
        if not (isinstance(imgs, Items) and imgs.side == 1 and imgs.scorer is self):
            raise ValueError("imgs must come from this scorer's encode_images")
        if caps.length + imgs.length > 512:
            raise ValueError("%d text + %d region rows: more than 512 keys per query row" % (caps.length, imgs.length))

    def _gather_pairs(self, caps, imgs, npairs, cross=None, idx=None):
        """The vk_pair_gather launch of one pair chunk into the inputs of its plan, which is returned."""
        eng = self._engine("pair", npairs, caps.length, imgs.length)
        a = eng.pair_args
        for k, (name, _, side) in enumerate(eng.pair_inputs):
            a.src[k] = (caps if side == 0 else imgs).tensors[name].data_ptr()
        a.n_items[0], a.n_items[1] = caps.n, imgs.n
        if cross is not None:
            a.cap_idx = a.img_idx = None
            a.c0, a.nc, a.i0, a.ni = cross
        else:
            a.cap_idx, a.img_idx = idx[0].data_ptr(), idx[1].data_ptr()
            a.c0 = a.nc = a.i0 = a.ni = 0
        from . import _lib as L
        L.check(L.lib.vk_pair_gather(C.byref(a), L.stream_ptr()))
        return eng

    def _run_pairs(self, caps, imgs, npairs, cross=None, idx=None):
        """One pair chunk: gather, then the suffix list.  -> fp32 logits [npairs, classes] (a view of the plan's output buffer)."""
        eng = self._gather_pairs(caps, imgs, npairs, cross, idx)
        eng.fwd.run()
        return eng.score_out[:npairs, :eng.score_classes]

    def _matrix_blocks(self, Nc, Ni):
        """score_matrix's pair chunks as cross products (first caption, captions, first image, images)."""
        P = self.pair_chunk
        if Ni >= P or self.one_caption_per_chunk:
            return [(c, 1, i0, min(P, Ni - i0)) for c in range(Nc) for i0 in range(0, Ni, P)]
        per = P // Ni
        return [(c0, min(per, Nc - c0), 0, Ni) for c0 in range(0, Nc, per)]

    def _scores(self, logits):
        """fp32 scores of [n, classes] logits: the VL-logit itself, or the zero-shot match probability softmax(itm)[:, 0]."""
        return logits[:, 0] if self.task is not None else torch.softmax(logits, dim=1)[:, 0]

    def score_matrix(self, caps, imgs, return_logits=False):
        """fp32 [Nc, Ni] scores of every caption against every image, left on the device (no host synchronisation).  Pair chunks of at most
        pair_chunk pairs: one caption against image blocks of pair_chunk, or as many whole captions as fit against all images (one caption
        per chunk for VL-BERT, whose text positions depend on the batch's shortest caption).
        return_logits: also the raw logits, fp32 [Nc, Ni, classes] (1 for VL-logit, the two ITM logits for zero-shot)."""
        self._check_items(caps, imgs)
        self._prepare()
        Nc, Ni = caps.n, imgs.n
        C_ = 1 if self.task is not None else 2
        S = torch.empty(Nc, Ni, dtype=torch.float32, device=self.device)
        Lg = torch.empty(Nc, Ni, C_, dtype=torch.float32, device=self.device) if return_logits else None
        with torch.no_grad():
            for c0, nc, i0, ni in self._matrix_blocks(Nc, Ni):
                lg = self._run_pairs(caps, imgs, nc * ni, cross=(c0, nc, i0, ni))
                S[c0:c0 + nc, i0:i0 + ni].copy_(self._scores(lg).view(nc, ni))
                if Lg is not None:
                    Lg[c0:c0 + nc, i0:i0 + ni].copy_(lg.view(nc, ni, C_))
        return (S, Lg) if return_logits else S

    def score_pairs(self, caps, imgs, cap_idx, img_idx, return_logits=False):
        """fp32 [P] scores of the pairs (cap_idx[p], img_idx[p]) (integer tensors of one length on the model's device; re-ranking).  The
        indices are range-checked on the host (one synchronisation)."""
        self._check_items(caps, imgs)
        ci = self._tensor(cap_idx, torch.int64, tuple(cap_idx.shape), "cap_idx") if isinstance(cap_idx, torch.Tensor) else None
        ii = self._tensor(img_idx, torch.int64, tuple(img_idx.shape), "img_idx") if isinstance(img_idx, torch.Tensor) else None
        if ci is None or ii is None or ci.dim() != 1 or ci.shape != ii.shape:
            raise ValueError("cap_idx and img_idx must be 1-D integer tensors of one length")
        n = ci.numel()
        if n and not (0 <= int(ci.min()) and int(ci.max()) < caps.n and 0 <= int(ii.min()) and int(ii.max()) < imgs.n):
            raise ValueError("pair indices out of range (%d captions, %d images)" % (caps.n, imgs.n))
        self._prepare()
        C_ = 1 if self.task is not None else 2
        s = torch.empty(n, dtype=torch.float32, device=self.device)
        Lg = torch.empty(n, C_, dtype=torch.float32, device=self.device) if return_logits else None
        if self.one_caption_per_chunk:        # chunks of one caption each: the pairs grouped by caption (their order kept within a group)
            order = torch.sort(ci, stable=True)[1]
            counts = torch.bincount(ci, minlength=caps.n).tolist()
            groups, start = [], 0
            for cnt in counts:
                groups += [(start + q, min(self.pair_chunk, cnt - q)) for q in range(0, cnt, self.pair_chunk)]
                start += cnt
            ci, ii = ci[order], ii[order]
        else:
            order = None
            groups = [(p0, min(self.pair_chunk, n - p0)) for p0 in range(0, n, self.pair_chunk)]
        with torch.no_grad():
            for p0, m in groups:
                lg = self._run_pairs(caps, imgs, m, idx=(ci[p0:p0 + m], ii[p0:p0 + m]))
                s[p0:p0 + m].copy_(self._scores(lg))
                if Lg is not None:
                    Lg[p0:p0 + m].copy_(lg)
            if order is not None:            # back to the caller's order
                s = torch.empty_like(s).index_copy_(0, order, s)
                Lg = torch.empty_like(Lg).index_copy_(0, order, Lg) if Lg is not None else None
        return (s, Lg) if return_logits else s


def rank_metrics(ranks):
    """eval_retrieval.py:225-230 / 258-263 on a vector of 0-based ranks, in float64 numpy as the driver computes them."""
    r = np.asarray(ranks, dtype=np.float64)
    return dict(r1=100.0 * np.sum(r < 1) / len(r), r5=100.0 * np.sum(r < 5) / len(r), r10=100.0 * np.sum(r < 10) / len(r),
                medr=np.floor(np.median(r) + 1), meanr=np.mean(r) + 1)


class RetrievalResult:
    """image_retrieval / text_retrieval: dicts of r1, r5, r10, medr, meanr; results: per caption the top-k image indices (what the driver
    dumps into *_result.json); rank_ir [Nc], rank_tr [Ni] int32 and score_matrix fp32 stay on the device.  score_matrix holds the rows
    caption_range = (first caption, one past the last) of the [Nc, Ni] matrix: all of them, (0, Nc), unless the evaluation was sharded."""

    def __init__(self, image_retrieval, text_retrieval, results, rank_ir, rank_tr, score_matrix, caption_range=None):
        self.image_retrieval, self.text_retrieval, self.results = image_retrieval, text_retrieval, results
        self.rank_ir, self.rank_tr, self.score_matrix = rank_ir, rank_tr, score_matrix
        self.caption_range = (0, int(rank_ir.numel())) if caption_range is None else caption_range


def _process_group(group):
    """(torch.distributed, the group or None for the default one) of evaluate_retrieval's `group` argument"""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        raise ValueError("evaluate_retrieval: group=%r was given, but torch.distributed is not initialised (init_process_group first)" % (group,))
    if group is True:
        return dist, None
    if group is False or not isinstance(group, dist.ProcessGroup):
        raise ValueError("evaluate_retrieval: group must be None, True (the default process group) or a torch.distributed group, not %r" % (group,))
    return dist, group


def _all_reduce_sum(dist, pg, t):
    """in-place integer sum of `t` over the group; staged through the host when the backend does not reduce device tensors"""
    if t.numel() == 0:                               # the same on every rank: nobody enters the collective
        return t
    if "nccl" in str(dist.get_backend(pg)):
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=pg)
    else:
        h = t.cpu()
        dist.all_reduce(h, op=dist.ReduceOp.SUM, group=pg)
        t.copy_(h)
    return t


def _ranks_sharded(scorer, arr, K, dist, pg, phase_hook):
    """The score block of this rank's captions and the exact merge of all ranks' parts ("Sharded over ranks"):
    -> rank_ir, topk_ir, rank_tr (the same on every rank), S_local, (row0, row1)"""
    from . import ops
    mark = phase_hook if phase_hook is not None else (lambda name: None)
    rank, W = dist.get_rank(pg), dist.get_world_size(pg)
    Nc = int(arr["input_ids"].shape[0])
    row0, row1 = rank * Nc // W, (rank + 1) * Nc // W
    caps = scorer.encode_captions(arr["input_ids"][row0:row1], arr["segment_ids"][row0:row1], arr["input_mask"][row0:row1]) if row1 > row0 else None
    imgs = scorer.encode_images(arr["features"], arr["spatials"], arr["image_mask"])
    mark("encode")
    if caps is not None:
        S = scorer.score_matrix(caps, imgs)
    else:                                            # more ranks than captions: this one scores nothing and still takes part in the sums
        S = torch.empty(0, imgs.n, dtype=torch.float32, device=scorer.device)
    mark("score")
    sh = ops.retrieval_ranks_shard(S, row0, Nc, arr["caption_image"], K)
    target_key = _all_reduce_sum(dist, pg, sh.target_key)
    count = _all_reduce_sum(dist, pg, ops.retrieval_ranks_shard_counts(sh, target_key))
    rank_tr = ops.retrieval_ranks_finish(count, sh.image_ptr, imgs.n)
    rank_ir, topk_ir = _all_reduce_sum(dist, pg, sh.rank_ir), _all_reduce_sum(dist, pg, sh.topk_ir)
    mark("ranks")
    return rank_ir, topk_ir, rank_tr, S, (row0, row1)


def evaluate_retrieval(model, dset_val, task_id=None, pair_chunk=1000, topk=20, group=None, phase_hook=None, projection_dtype=None):
    """eval_retrieval.py:161-263 for a `RetrievalDatasetVal`: image retrieval (per caption, the rank of its image) and text retrieval (per
    image, the best rank of one of its captions) as recall@1/5/10, median and mean rank, plus the top-`topk` images per caption.

    `model`: a BertForVLTasks with the VL-logit task `task_id`, or a BertForVLPreTraining with task_id None (zero-shot), bare or wrapped in
    volta_amd.parallel.DistributedDataParallel; what RetrievalScorer refuses is refused here with its messages, and the model's state is
    left alone as the scorer leaves it.  Any number of captions and images (COCO's 5k test set is the same call).

    `projection_dtype`: None | "bf16" | "fp8", handed to the scorer.  Under "fp8" the scores, ranks and recalls are those of the model
    with its projections on the e4m3 path (the driver's numbers after `set_projection_dtype("fp8")`), not the bf16 model's.

    `group`: None scores everything on this device, also inside an initialised process group.  True (the default process group) or a
    torch.distributed group shards the captions: every rank of the group must make the same call; rank r of W encodes all images and the
    captions [r * Nc // W, (r + 1) * Nc // W) (none when W > Nc), fills that block of the matrix, and four all_reduce(SUM) calls over small
    integer arrays merge the ranks' parts exactly (csrc/ranks.hip, the shard calls).  Every rank returns the same metrics, `results`,
    `rank_ir` and `rank_tr` -- the bits of the unsharded call on the same scores; `score_matrix` is the rank's own block, the rows
    `caption_range`.  A group of one rank takes this path too.  `phase_hook(name)`, sharded path only, is called when "encode", "score" and
    "ranks" (kernels and exchange) have been issued: a timer's hook synchronises the device itself (tools/eval_retrieval_sharded.py).

    Ties: ranks follow np.argsort(-s, kind="stable") with NaN last (ops.retrieval_ranks).  The driver's np.argsort(-s) is not stable, so
    its rank is only defined where the target's score is untied; there the two agree.  Images without a caption are left out of the
    text-retrieval statistics (the driver's `min(ranks)` fails on them)."""
    from . import ops
    from .parallel import DistributedDataParallel
    dist, pg = _process_group(group) if group is not None else (None, None)
    if isinstance(model, DistributedDataParallel):
        model = model.module
    scorer = RetrievalScorer(model, task_id, pair_chunk=pair_chunk, projection_dtype=projection_dtype)
    if not 0 <= int(topk) <= 64:
        raise ValueError("topk must be in 0..64, got %r" % (topk,))
    arr = dset_val.device_arrays(scorer.device)
    if dist is None:
        caps = scorer.encode_captions(arr["input_ids"], arr["segment_ids"], arr["input_mask"])
        imgs = scorer.encode_images(arr["features"], arr["spatials"], arr["image_mask"])
        S = scorer.score_matrix(caps, imgs)
        rank_ir, topk_ir, rank_tr = ops.retrieval_ranks(S, arr["caption_image"], int(topk))
        caption_range = None
    else:
        rank_ir, topk_ir, rank_tr, S, caption_range = _ranks_sharded(scorer, arr, int(topk), dist, pg, phase_hook)
    Nc, Ni, K = rank_ir.numel(), rank_tr.numel(), int(topk)
    host = torch.cat([rank_ir, rank_tr, topk_ir.reshape(-1)]).cpu().numpy()          # the one transfer
    ir, tr, top = host[:Nc], host[Nc:Nc + Ni], host[Nc + Ni:].reshape(Nc, K)
    results = [[int(v) for v in row if v >= 0] for row in top]
    return RetrievalResult(rank_metrics(ir), rank_metrics(tr[tr >= 0]), results, rank_ir, rank_tr, S, caption_range)


# ------------------------------------------------------------------------------------------------ the hard-negative pool of the training set
def train_image_list(annotations_jsonpath, task):
    """The image id of every annotation line, in file order: `int(img_path.split(".")[0])` for RetrievalFlickr30k (scripts/generate_pool.py:35-39),
    `id` for RetrievalCOCO (the rule of `RetrievalDataset`)."""
    from .datasets import _read_jsonlines
    if task not in ("RetrievalFlickr30k", "RetrievalCOCO"):
        raise ValueError("task: RetrievalFlickr30k or RetrievalCOCO expected, not %r" % (task,))
    anns = _read_jsonlines(annotations_jsonpath)
    return [int(ann["img_path"].split(".")[0]) if task == "RetrievalFlickr30k" else ann["id"] for ann in anns]


def image_mean_features(features_reader, image_list, chunk=256, device="cuda"):
    """fp32 [len(image_list), F] on the device: per image the mean of its region features, `np.sum(features, 0) / num_boxes` bit for bit --
    row 0 of what an `ImageFeaturesH5Reader` with a leading global feature returns.  `chunk` images are decoded by one `ImageStager.stage`
    call, copied once and reduced by `ops.image_means`."""
    from . import ops
    from .datasets import ImageStager
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk = %d: at least one image per chunk" % chunk)
    stager = ImageStager(features_reader, sets=1)
    means = torch.empty(len(image_list), stager.F, dtype=torch.float32, device=device)
    for i0 in range(0, len(image_list), chunk):
        ids = image_list[i0:i0 + chunk]
        order = list(dict.fromkeys(ids))                                 # the stager takes distinct ids
        h = stager.stage(order)
        if int(h["n"].min()) < 1:
            raise ValueError("image %r has no region" % (order[int(h["n"].argmin())],))
        S = h["S"]
        if h["staged_all"]:
            feat = h["stage"]["feat"][:S].to(device)
        else:
            feat = torch.zeros(S, h["Rcap"], stager.F, dtype=torch.float32)
            for s, (f, _) in enumerate(h["src"]):
                feat[s, :f.shape[0]] = f
            feat = feat.to(device)
        m = ops.image_means(feat.contiguous(), torch.from_numpy(h["n"]).to(device))
        if len(order) != len(ids):
            slot = {iid: s for s, iid in enumerate(order)}
            m = m[torch.as_tensor([slot[iid] for iid in ids], device=device)]
        means[i0:i0 + len(ids)] = m
    return means


def generate_hard_pool(features_reader, annotations_jsonpath, task, k=100, out=None, chunk=256):
    """`hard_negative.pkl` of `RetrievalDataset(split="train")`, the product of the reference's scripts/generate_pool.py: per training image
    (one per annotation line) the k nearest training images under the Euclidean distance, in float64, between mean region features.

    Returns dict(train_hard_pool=float64 ndarray [N, k] of positions in train_image_list, train_image_list=list of int) -- dtype and layout
    of what the script pickles.  Row i is ordered by (distance, position): the image itself is a candidate like any other, as in the script's
    `BallTree.query`, and comes first unless an image with the same mean feature has a lower position.  The search is exact (`ops.knn_pool`).
    `out`: a path to pickle the result to, or True for `<directory of the annotations>/hard_negative.pkl`; None writes nothing."""
    from . import ops
    import os
    import pickle
    k = int(k)
    if k < 1:
        raise ValueError("k = %d: at least one neighbour" % k)
    image_list = train_image_list(annotations_jsonpath, task)
    if k > len(image_list):
        raise ValueError("k = %d neighbours of %d training images: k must be less than or equal to the number of images" % (k, len(image_list)))
    if out is not None and out is not True and not isinstance(out, (str, bytes, os.PathLike)):
        raise ValueError("out: a path, True or None expected, not %r" % (out,))
    means = image_mean_features(features_reader, image_list, chunk)
    pool = ops.knn_pool(means, k).cpu().numpy().astype(np.float64)
    result = dict(train_hard_pool=pool, train_image_list=image_list)
    if out is not None:
        path = os.path.join(os.path.dirname(os.path.abspath(annotations_jsonpath)), "hard_negative.pkl") if out is True else out
        with open(path, "wb") as f:
            pickle.dump(result, f)
    return result
