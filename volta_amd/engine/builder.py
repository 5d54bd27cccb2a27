"""StepEngine: the buffers and the forward / backward command lists of one shape, built once and replayed every step."""
import ctypes as C
import os
import re

import torch

from .. import _lib as L
from .._lib import check, ptr
from ..modules import sublayer_schedule
from .arena import CHUNK
from .embeddings import EmbeddingBuilders
from .heads import HeadBuilders
from .plan import (EV_DECODER_WGRAD, EV_IMAGE_EMB_BWD, EV_IMAGE_EMB_FWD, EV_WGRAD_RING, NODROP, Plan, _addr, _mk_segs, _round_up, op, side_begin, side_end, wait_side)
from .sublayers import SublayerBuilders


def frozen_blocks(arena, heads="pretrain"):
    """The blocks a backward list is pruned by: [[arena names]].  A block's gradient ops are dropped when every parameter of it is frozen
    and stay as they are otherwise.  One block each: the weight and bias of a Linear (one TN problem writes both); the six Q|K|V tensors
    of an attention sub-layer and modality (one [3 Ha, Hm] product); `lora_A` and `lora_B` of one projection (one LoRA problem writes
    both); gamma and beta of a LayerNorm; everything under one embedding
    prefix (one backward; VisualBERT, VL-BERT and UNITER embed both modalities under one prefix).  The tied LM decoder of the pre-training
    heads writes the word table's gradient and the decoder bias in one product: there (word table, decoder bias) is a block too, and
    the word table's gradient is left alone only when both blocks it belongs to are frozen."""
    blocks = {}
    if heads == "pretrain":
        blocks["decoder"] = ["bert.embeddings.word_embeddings.weight"]
    for name in arena.params:
        m = re.match(r"bert\.(v_)?embeddings\.", name)
        if m:
            key = m.group(0)
        elif heads == "pretrain" and name == "cls.predictions.bias":
            key = "decoder"
        else:
            key = re.sub(r"\.attention_self\.(v_)?(query|key|value)\.(weight|bias)$", r".attention_self.\1qkv", name)
            if key == name:
                key = re.sub(r"\.lora_[AB]$", ".lora", name)          # the adapter of one projection: a block apart from the base Q|K|V
            if key == name:
                key = name.rsplit(".", 1)[0]
        blocks.setdefault(key, []).append(name)
    return list(blocks.values())


def canonical_frozen(arena, frozen, heads="pretrain"):
    """The pruning decision behind a pattern of frozen parameters: the names of the blocks that are frozen as a whole.  Two patterns with
    the same result build the same plan, so this, not the pattern, is what a plan is keyed by; with only `query` frozen it is empty."""
    frozen = set(frozen)
    if not frozen:
        return frozenset()
    return frozenset(n for blk in frozen_blocks(arena, heads) if all(x in frozen for x in blk) for n in blk)


class Stream:
    """Per-modality geometry: 0 = text, 1 = vision."""

    def __init__(self, L_, B, H):
        self.L, self.M, self.H = L_, B * L_, H


def wide_geometry(cfg):
    """None for the single-width geometry of the ctrl_* configs (both streams one hidden size, 64-wide heads, no per-sub-layer widths), else
    a description of what differs (config/vilbert_base.json: 768 text, 1024 vision, sub-layer widths of their own).  The e4m3 projection
    path covers the single-width geometry only."""
    H, Hv = cfg.hidden_size, cfg.v_hidden_size
    what = []
    if H != Hv:
        what.append("stream widths %d text / %d vision" % (H, Hv))
    per = [k for k in ("sublayer2attn_hidden_size", "sublayer2num_attention_heads", "sublayer2intermediate_size", "sublayer2v_attn_hidden_size",
                       "sublayer2v_num_attention_heads", "sublayer2v_intermediate_size") if getattr(cfg, k)]
    if per:
        what.append("per-sub-layer widths (%s)" % ", ".join(per))
    if H // cfg.num_attention_heads != 64 or Hv // cfg.v_num_attention_heads != 64:
        what.append("head sizes %d text / %d vision, not 64" % (H // cfg.num_attention_heads, Hv // cfg.v_num_attention_heads))
    return "; ".join(what) if what else None


def pair_segments(split, fp8=False):
    """[(name, side 0 caption | 1 image)]: the gather segments of a score pair plan, in the order of its `pair_inputs` -- what one
    vk_pair_gather launch copies per pair out of the encoded handles.  split = retrieval.split_plan(cfg).  On the e4m3 path a modality whose
    prefix ends in a sub-layer also hands over the e4m3 copy its last LayerNorm wrote and that copy's row scales (x8_*, xs_*): the pair plan's
    first projection must read those bits, as the whole-model plan does, not a re-quantisation of the bf16 rows.  A modality whose prefix
    is its embedding alone hands over nothing more; the pair plan quantises its gathered bf16 rows itself.  At most VK_PAIR_MAX_SEGS."""
    text_subs, vision_subs, per_modality = split
    if per_modality:
        segs = [("x_t", 0), ("x_v", 1)]
    else:
        segs = [("input_ids", 0), ("token_type_ids", 0), ("image_feat", 1), ("image_loc", 1)]
    segs += [("attention_mask", 0), ("image_attention_mask", 1)]
    if fp8 and per_modality:
        if text_subs:
            segs += [("x8_t", 0), ("xs_t", 0)]
        if vision_subs:
            segs += [("x8_v", 1), ("xs_v", 1)]
    assert len(segs) <= L.PAIR_MAX_SEGS
    return segs


class StepEngine(EmbeddingBuilders, SublayerBuilders, HeadBuilders):
    """Buffers + forward / backward command lists of one (B, T, Rv, train) shape.  The builders of the embeddings, sub-layers and heads are
    its base classes; this class holds the helpers they share, the two lists' assembly and what runs a built plan."""

    H8_MUL = 8.0           # static scale of the fp8 copy of the GELU output: |h| <= 56 representable, 2^-9 absolute resolution near 0

    LORA_SITE_BASE = 1 << 20      # first LoRA dropout site (lora_drops): the model's own sites count up from 0 and stay far below it

    def __init__(self, cfg, arena, B, T, Rv, train, heads="pretrain", fp8=False, task=None, task_dropout=0.1, attn_maps=False, part=None, split=None,
                 projection_dtype=None, frozen=None, lora_dropout=0.0):
        """fp8: the forward Q|K|V, FFN-up and FFN-down projections of every sub-layer run on the e4m3 MFMA path (csrc/fp8.hip); inputs are
        quantised per row right before the GEMM, weights per output channel whenever they change; the backward stays bf16.
        heads: "pretrain" = the three pre-training heads and losses (BertForVLPreTraining); "tasks" = poolers only, the
        sequence and pooled outputs leave the engine and their gradients enter it (BertForVLTasks); "backbone" = the "tasks" plan without a
        task, its backward seeded from outside: d(loss)/d(every returned state) enters through `bind_grads` (BertModel on its own);
        "score" = one forward-only list of the retrieval scorer (volta_amd/retrieval.py), eval semantics, no backward: `part` "text" (text
        embedding + the text-only sub-layers, B captions), "image" (image embedding + the vision-only sub-layers, B images) or "pair" (the
        mixing suffix on B pairs whose inputs vk_pair_gather wrote into `pair_inputs`, poolers, fusion and the scoring head: `task`'s
        VL-logit classifier, or cls.bi_seq_relationship when task is None); `split` = retrieval.split_plan(cfg).
        projection_dtype: score plans only, None | "bf16" | "fp8" -- the scorer's own precision switch (the `fp8` argument belongs to the
        training plans and stays refused here).  "fp8" builds the same e4m3 launches as `fp8` does for a whole-model plan; a prefix plan then
        exposes the e4m3 copy its last LayerNorm wrote as `score_x8`, and the pair plan starts from gathered copies (`pair_segments`).
        frozen: arena names of parameters that take no gradient (requires_grad False).  The backward list keeps an op only if its output
        reaches the gradient of a trainable parameter ("Frozen parameters"); the forward list, the buffers and, with
        nothing frozen, both lists are what they are without the argument.  A block is pruned as a whole or not at all (`frozen_blocks`),
        so any pattern may be passed: `canonical_frozen` maps it to the one the plan depends on.  Score plans have no backward and ignore it.
        lora_dropout: the rate of the dropout on every LoRA adapter's input (volta_amd/lora.py).  A training plan with a rate > 0 runs
        the adapters on the vk_lora_*_drop entry points; an eval plan, a score plan and a rate of 0 build what they build without it."""
        self.cfg, self.arena, self.B, self.T, self.Rv, self.train = cfg, arena, B, T, Rv, train
        self.heads = heads
        self.part, self.split = part, split
        self.fwd_only = heads == "score"   # the builders return before their backward part
        self.frozen = frozenset() if self.fwd_only else canonical_frozen(arena, frozen or (), heads)
        self.pruned = set()                # arena names whose gradient no op of the backward list writes: they read zero (modeling clears them once)
        self.live = [True, True]           # builder state: a trainable parameter lies upstream of the current x[m], so its dX is needed
        self.wgrad_recorded = set()        # sub-layers (index k) whose weight-gradient side block exists, i.e. whose ring event is recorded
        self.only = None                   # score prefixes: the one stream (0 text, 1 vision) whose problems a sub-layer emits
        if self.fwd_only and (train or fp8 or attn_maps or part not in ("text", "image", "pair") or split is None):
            raise ValueError("a score plan is an eval-mode forward of part text | image | pair with a split plan; its precision is projection_dtype, not fp8")
        if projection_dtype not in (None, "bf16", "fp8") or (projection_dtype is not None and not self.fwd_only):
            raise ValueError("projection_dtype %r: None | 'bf16' | 'fp8', for heads='score' plans only" % (projection_dtype,))
        self.task = task              # heads == "tasks": (task id, its task_cfg entry) -- the classifier built behind the poolers
        self.attn_maps = bool(attn_maps)      # keep every attention sub-layer's probabilities (config.visualization, encoders.py:342-358): generic attention kernels
        self.attn_map_info = []
        self.task_dropout = float(task_dropout)      # BertForVLTasks(dropout_prob=...): nn.Dropout on the fused pooled vector / region states (encoders.py:1118-1122)
        self.fp8 = bool(fp8) or projection_dtype == "fp8"
        self.dev = dev = arena.device
        H, Hv = cfg.hidden_size, cfg.v_hidden_size
        # Widths: the two streams may differ (config/vilbert_base.json: 768 text, 1024 vision) and an attention sub-layer may project to a
        # width of its own (sublayer2attn_hidden_size); every width is a multiple of 64, LayerNorm widths at most 1024.  Head sizes: 64 on
        # the MFMA attention kernels, 32 / 96 / 128 on the generic ones.
        if H % 64 or Hv % 64 or H > 1024 or Hv > 1024:
            raise NotImplementedError("hidden sizes must be multiples of 64, at most 1024 (got %d / %d)" % (H, Hv))
        self.wide = wide_geometry(cfg) is not None
        if self.wide and self.fp8:
            raise NotImplementedError("the fp8 projection path covers the single-width (ctrl_*) geometry")
        if self.wide and cfg.image_embeddings != "vilbert":
            raise NotImplementedError("different stream widths are built for the ViLBERT embeddings (config/vilbert_base.json)")
        if cfg.hidden_act != "gelu" or cfg.v_hidden_act != "gelu":
            raise NotImplementedError("engine supports gelu activations (every reference config)")
        if cfg.fusion_method not in ("mul", "sum", "text", "vl-bert_vqa", "none"):
            raise ValueError("Invalid fusion method: %s" % cfg.fusion_method)
        self.unused_params = set()    # parameters no launch of this plan reads: their .grad stays None, as under the reference's autograd
        # rows beyond the MFMA attention tiles (64 text tokens, 128 regions: VCR's 80-token captions, 200 / 256 / 306 regions of the
        # grounding tasks, config_tasks/all_tasks.yml) run on the generic attention kernels: up to 512 keys per query row
        if T + Rv > 512:
            raise NotImplementedError("more than 512 keys per query row (%d text + %d vision rows)" % (T, Rv))
        self.H, self.I, self.nh = H, cfg.intermediate_size, cfg.num_attention_heads
        self.st = [Stream(T, B, H), Stream(Rv, B, Hv)]
        self.R = Rv - (1 if cfg.add_global_imgfeat is not None else 0)
        self.bufs = {}
        self.keep = []
        self.fwd, self.bwd = Plan(), Plan()
        self.site = 0
        if not 0.0 <= float(lora_dropout) < 1.0:
            raise ValueError("lora_dropout %r: 0 <= p < 1" % (lora_dropout,))
        self.lora_p = float(lora_dropout) if train and not self.fwd_only else 0.0
        self.lora_site = 0            # LoRA dropout sites handed out so far (lora_drops)
        self.seed = torch.zeros(1, dtype=torch.int64, device=dev)
        self.inputs = {}              # name -> list of (struct, field) patched every step
        self.taps = {}
        self.grad_seeds = {}          # heads == "backbone": output name -> vk_grad_seed_args whose source bind_grads() patches every backward
        self.losses = None            # heads == "pretrain": float[3] = lm, img, nsp, written by the forward list
        self.nce_site = None          # dropout site of the nce_2048 negatives, where that visual target is configured
        self.task_loss_bufs = None    # (work, out, amax) of vk_task_loss_fwd for this plan's logits (modeling._task_loss_args)
        # builder state
        self._aside = ""              # suffix of the temporaries of ops being built for a side-stream block (tmp)
        self._split_cur = {}          # stream tag -> [bytes, counters] handed out to the split accumulations of the launch being built
        self._n_ln_partial = 0
        self._deferred_ln = []        # LayerNorm backward arguments whose dgamma / dbeta reduction the next _wgrad() places
        self._slab_cursor = 0
        self._fwd_segments = {}       # fwd_segments() by optimizer range bounds
        self._build()

    # ---------------------------------------------------------------- helpers
    def buf(self, name, shape, dtype=torch.bfloat16, zero=False):
        assert name not in self.bufs, name
        t = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self.dev)
        self.bufs[name] = t
        return t

    def tmp(self, name, shape, dtype=torch.bfloat16, shared=False):
        """Backward temporaries are shared by all sub-layers (launches on one stream are ordered).  Ops that are being built for a
        side-stream block run NEXT to main-stream launches: they get temporaries of their own (`_aside`)."""
        name += "" if shared else self._aside
        if name not in self.bufs:
            self.bufs[name] = torch.empty(shape, dtype=dtype, device=self.dev)
        t = self.bufs[name]
        assert tuple(t.shape) == tuple(shape) and t.dtype == dtype, (name, t.shape, shape)
        return t

    def drop(self, p):
        site = self.site
        self.site += 1
        return L.dropout_cfg(self.seed.data_ptr(), site, p if self.train else 0.0)

    def lora_drops(self, keys):
        """{key: the dropout of one LoRA problem (one adapter on one stream)} for the problems of a sub-layer, or {} when the plan has no
        LoRA dropout.  LoRA sites come from a counter of their own, LORA_SITE_BASE + 0, 1, ..., in the order the forward list meets the
        problems: sub-layer by sub-layer, within a sub-layer stream by stream, within a stream target by target -- a rebuilt plan hands
        out the same sites.  `self.site` is not advanced, so the model's own sites (and masks) are those of the model without adapters.
        The backward problem of an adapter takes the entry of its forward problem: it replays the same stream."""
        if not self.lora_p:
            return {}
        out = {}
        for key in keys:
            out[key] = L.dropout_cfg(self.seed.data_ptr(), self.LORA_SITE_BASE + self.lora_site, self.lora_p)
            self.lora_site += 1
        return out

    def k(self, obj):
        self.keep.append(obj)
        return obj

    def patch(self, name, struct, field, index=None):
        self.inputs.setdefault(name, []).append((struct, field, index))

    def W(self, name):
        return self.arena.view(name, "shadow")

    # ---- frozen parameters: `fz` asks; `prune` asks and notes that the caller leaves the block's gradient ops out
    def fz(self, *names):
        return bool(self.frozen) and all(n in self.frozen for n in names)

    def prune(self, *names):
        if self.fz(*names):
            self.pruned.update(names)
            return True
        return False

    def fz_linear(self, stem, prune=False):
        """stem = "... .dense.": the weight and bias of one Linear, one block."""
        return (self.prune if prune else self.fz)(stem + "weight", stem + "bias")

    def prefix_names(self, prefix):
        return [n for n in self.arena.params if n.startswith(prefix)]

    def Pm(self, name):
        return self.arena.view(name, "master")

    def G(self, name):
        return self.arena.view(name, "grad")

    def gemm(self, plan_ops, layout, epi, probs, geometry=0):
        """geometry: tile code of vk_gemm_grouped_ex carried in the op's i0 above the layout (0 = the library's heuristic)"""
        arr = self.k((L.GemmProblem * len(probs))(*probs))
        self.put(plan_ops, L.OP_GEMM, arr, i0=layout | (geometry << 8), i1=epi, i2=len(probs))

    def gemm_kept(self, plan_ops, layout, epi, probs, keep):
        """`probs` in one launch, without those whose `keep` flag is False (frozen parameters: nothing reads their output).  The launch
        keeps the tile geometry the library picks for the whole group, so what the remaining problems compute does not depend, to the bit, on
        what else is frozen.  All kept: the launch of `gemm`."""
        kept = [q for q, k in zip(probs, keep) if k]
        if len(kept) == len(probs):
            return self.gemm(plan_ops, layout, epi, probs)
        if kept:
            arr = (L.GemmProblem * len(probs))(*probs)
            self.gemm(plan_ops, layout, epi, kept, geometry=L.lib.vk_gemm_geometry(layout, epi, arr, len(probs)))

    def prob(self, A, B, Cout, M, N, K, lda, ldb, ldc, bias=None, R=None, ldr=0, C2=None, bias_grad=None, dyn=None, n_store=0):
        return L.GemmProblem(_addr(A), _addr(B), _addr(Cout), _addr(C2), _addr(bias), _addr(R), _addr(bias_grad), _addr(dyn),
                             M, N, K, lda, ldb, ldc, ldr, n_store)

    # ---- split accumulations (include/volta_hip.h, vk_gemm_problem::ws): K-slices of one product in one launch, summed by the last arriver
    # bytes of partial-tile workspace per stream (launches on one stream are ordered: they share it).  Sized by the first request -- the only user
    # is the image projection's weight gradient, one product per launch: nparts x tiles x 320 KiB = 84 MB for [1024 x 2048] at B = 256 --
    # instead of a fixed 768 MiB per cached engine; VK_SPLIT_WS_MB overrides
    SPLIT_WS_MIN = 32 << 20

    def _split_alloc(self, tag, layout, M, N, nparts, geometry):
        """(ws address, cnt address) for one split accumulation of the launch being built on stream `tag` ("main" / "side")."""
        tiles = C.c_int(0)
        nbytes = L.lib.vk_gemm_split_workspace_bytes(layout, M, N, nparts, geometry, C.byref(tiles))
        assert nbytes > 0 and tiles.value > 0, (layout, M, N, nparts, geometry)
        if "split_ws_" + tag not in self.bufs:          # the arenas belong to a stream, not to a block of ops: no `_aside` suffix
            mb = os.environ.get("VK_SPLIT_WS_MB")
            cap = (int(mb) << 20) if mb else max(self.SPLIT_WS_MIN, _round_up(int(nbytes * 1.25), 1 << 20))
            self.bufs["split_ws_" + tag] = torch.empty(cap, dtype=torch.uint8, device=self.dev)
        ws = self.bufs["split_ws_" + tag]
        if "split_cnt_" + tag not in self.bufs:
            self.bufs["split_cnt_" + tag] = torch.zeros(1 << 16, dtype=torch.int32, device=self.dev)      # zero once: every launch leaves them zero
        cnt = self.bufs["split_cnt_" + tag]
        cur = self._split_cur.setdefault(tag, [0, 0])
        if cur[0] + nbytes > ws.numel() or cur[1] + tiles.value > cnt.numel():
            raise RuntimeError("split-accumulation workspace too small (%d + %d of %d bytes): set VK_SPLIT_WS_MB" % (cur[0], nbytes, ws.numel()))
        out = (ws.data_ptr() + cur[0], cnt.data_ptr() + 4 * cur[1])
        cur[0] += _round_up(nbytes, 256)
        cur[1] += tiles.value
        return out

    def soft_error(self):
        """Always 0.  bench.py reads it into the `handoff_errors` field of its result line: the count of row-block hand-offs and
        weight-gradient gates that gave up waiting.  No plan this engine builds contains a hand-off or a gate, so there is no error word to read."""
        return 0

    @staticmethod
    def split_geometry(widths):
        """One tile geometry for a launch whose outputs are `widths` columns wide: 256 x 192 tiles when they cover every width without a
        ragged column tile and 256-wide ones would not (N = 768), 256 x 256 otherwise."""
        return 259 if all(n % 192 == 0 for n in widths) and any(n % 256 for n in widths) else 258

    def prob_parts(self, tag, geometry, layout, slices, Cout, M, N, ldc, **kw):
        """The problems of ONE product cut into len(slices) parts; slices: [(A address, B address, K, lda, ldb)]."""
        if len(slices) == 1:
            A, B, K, lda, ldb = slices[0]
            return [self.prob(A, B, Cout, M, N, K, lda, ldb, ldc, **kw)]
        ws, cnt = self._split_alloc(tag, layout, M, N, len(slices), geometry)
        out = []
        for i, (A, B, K, lda, ldb) in enumerate(slices):
            q = self.prob(A, B, Cout, M, N, K, lda, ldb, ldc, **kw)
            q.ws, q.cnt, q.part, q.nparts = ws, cnt, i, len(slices)
            out.append(q)
        return out

    def gemm_fp8(self, plan_ops, epi, specs):
        """specs: [(A bf16 [M, K] or (A8, scale_a) already quantised, master weight view [N, K], C, bias, C2)] -- one fp8 launch for all of
        them, preceded by the row quantisation of every bf16 A."""
        probs = []
        for idx, spec in enumerate(specs):
            A, Wm, Cout, bias, C2 = spec[:5]
            c8 = spec[5] if len(spec) > 5 else None            # (h8 uint8 [M, N], multiplier): e4m3 copy of the GELU output
            w8, ws = self.arena.fp8_weight(Wm)
            N, K = Wm.shape
            if isinstance(A, tuple):
                a8, sa = A
                M = a8.shape[0]
            else:
                M = A.shape[0]
                a8 = self.tmp("fp8_a%d_%d_%d" % (idx, M, K), (M, _round_up(K, 128)), torch.uint8)      # consumed by the launch that follows: shared by all sub-layers
                if K % 128:
                    a8[:, K:].zero_()               # the K padding is multiplied into the product: it must be zero, not stale bytes
                sa = self.tmp("fp8_sa%d_%d_%d" % (idx, M, K), (M,), torch.float32)
                self.emit(plan_ops, L.FN_QUANT_ROWS, p=(A, a8, sa, None), n=(M, K, A.stride(0), a8.stride(0), 0))
            probs.append(L.GemmFp8Problem(L.GemmProblem(_addr(a8), _addr(w8), _addr(Cout), _addr(C2), _addr(bias), None, None, None,
                                                        M, N, K, a8.stride(0), w8.stride(0), Cout.stride(0), 0, 0), _addr(sa), _addr(ws),
                                          _addr(c8[0]) if c8 else None, c8[1] if c8 else 0.0, c8[0].stride(0) if c8 else 0))
        arr = self.k((L.GemmFp8Problem * len(probs))(*probs))
        self.put(plan_ops, L.OP_GEMM_FP8, arr, i1=epi, i2=len(probs))

    def generic(self, fn, p=(), n=(), f=(), drop=None):
        g = L.GenericArgs()
        g.fn = fn
        for i, x in enumerate(p):
            g.p[i] = _addr(x)
        for i, x in enumerate(n):
            g.n[i] = int(x)
        for i, x in enumerate(f):
            g.f[i] = float(x)
        g.drop = drop or NODROP
        return self.k(g)

    # ---- emitters: append one op to the list `ops`
    def put(self, ops, kind, *abc, **i012):
        ops.append(op(kind, *abc, **i012))

    def emit(self, ops, fn, **kw):
        """A generic op; returns its arguments (for `patch`)."""
        g = self.generic(fn, **kw)
        self.put(ops, L.OP_GENERIC, g)
        return g

    def zero(self, ops, t):
        self.emit(ops, L.FN_MEMSET, p=(t,), n=(t.numel() * t.element_size(), 0))

    def ln_fwd(self, ops, *args, **kw):
        self.put(ops, L.OP_LN_FWD, self.ln_args(*args, **kw))

    def ln_bwd(self, ops, *args, **kw):
        self.put(ops, L.OP_LN_BWD, self.ln_bwd_args(*args, **kw))

    def ln_args(self, d, x, gname, bname, y, z, mean, rstd, M, drop, post=0, out_scale=1.0, addvec=None, dyn=None, segs=None, fp8_out=None, H=None):
        """fp8_out = (q uint8 [M, ld8], scale fp32 [M]): the kernel also leaves a row-quantised e4m3 copy of y (the next projection's A operand)."""
        a = L.LnArgs(_addr(d), _addr(x), _addr(addvec), _addr(self.Pm(gname)), _addr(self.Pm(bname)), _addr(y), _addr(z), _addr(mean),
                     _addr(rstd), _addr(dyn), M, H or self.H, M, post, out_scale, drop, _mk_segs(drop, segs))
        if fp8_out is not None:
            a.y8, a.y8_scale, a.ld8 = _addr(fp8_out[0]), _addr(fp8_out[1]), fp8_out[0].stride(0)
        return self.k(a)

    def fp8_hidden(self, m):
        """Per-modality e4m3 copy of the current hidden state, written by the LayerNorm that produces it and read by the next
        sub-layer's first projection (one buffer per modality: consumed before the next LayerNorm of that modality runs)."""
        M, H = self.st[m].M, self.H
        q = self.tmp("fp8_x%d" % m, (M, _round_up(H, 128)), torch.uint8)
        if H % 128:
            q.zero_()
        return q, self.tmp("fp8_xs%d" % m, (M,), torch.float32)

    def ln_bwd_args(self, dy, z, mean, rstd, gname, bname, dz, dd, M, drop, post=0, out_scale=1.0, dyn=None, segs=None, accumulate=0, defer=False, own_partial=False,
                    H=None):
        """`defer`: the dgamma / dbeta column reduction is left to an OP_LN_FINALIZE that the next _wgrad() places in its
        side-stream block; the partial records then need a buffer of their own.  `own_partial`: this launch runs inside a side-stream
        block, next to main-stream LayerNorm backwards -- it cannot share their scratch records either."""
        H = H or self.H
        Hmax = max(self.st[0].H, self.st[1].H)
        if self.prune(gname, bname):      # frozen gamma and beta: the launch without column sums -- no records, nothing to reduce later
            return self.k(L.LnBwdArgs(_addr(dy), _addr(z), _addr(mean), _addr(rstd), _addr(self.Pm(gname)), _addr(dz), _addr(dd), None, None, None,
                                      _addr(dyn), M, H, M, post, out_scale, 0, drop, _mk_segs(drop, segs)))
        if defer or own_partial or self._aside:
            self._n_ln_partial += 1
            partial = self.buf("ln_partial_%d" % self._n_ln_partial, (L.lib.vk_ln_bwd_partial_rows(M) * 2 * H,), torch.float32)
            accumulate |= 2 if defer else 0
        else:
            partial = self.tmp("ln_partial", (L.lib.vk_ln_bwd_partial_rows(max(self.st[0].M, self.st[1].M)) * 2 * Hmax,), torch.float32)
        a = L.LnBwdArgs(_addr(dy), _addr(z), _addr(mean), _addr(rstd), _addr(self.Pm(gname)), _addr(dz), _addr(dd), _addr(partial),
                        _addr(self.G(gname)), _addr(self.G(bname)), _addr(dyn), M, H, M, post, out_scale, accumulate, drop,
                        _mk_segs(drop, segs))
        a = self.k(a)
        if defer:
            self._deferred_ln.append(a)
        return a

    def _begin(self):
        """Builder state of a list under construction, and the mask buffers every list starts from."""
        self.x = [None, None]        # current hidden state buffers
        self.x8 = [None, None]       # fp8 path: (e4m3 copy, row scales) of x[m] when its producer wrote one
        self.level = [0, 0]          # number of sub-layers that transformed x[m] so far (ping-pong parity of dX)
        self.bwd_pro = []            # zero-fills of gradient tensors that are accumulated with atomics
        self.masks = [self.buf("mask_t", (self.B, self.T), torch.float32), self.buf("mask_v", (self.B, self.Rv), torch.float32)]

    def _mask_prep(self, m, src=None):
        """Additive attention mask of stream m from the 0/1 mask `src`, or from the per-step input, patched (no static staging copy)."""
        g = self.emit(self.fwd.ops, L.FN_MASK_PREP, p=(src, self.masks[m]), n=(self.B * self.st[m].L,))
        if src is None:
            self.patch(("attention_mask", "image_attention_mask")[m], g, "p", 0)

    def _build(self):
        if self.fwd_only:
            return self._build_score()
        cfg, f = self.cfg, self.fwd.ops
        self._begin()
        self._mask_prep(0)
        self._mask_prep(1)
        kind = cfg.image_embeddings
        bwd_stages = []
        nemb = 1 if kind in ("visualbert", "vl-bert") else 2
        self.stage_prefix = [["bert.embeddings.", "bert.v_embeddings."]] * nemb + [["bert.encoder.layer.%d." % n] for n, _ in sublayer_schedule(cfg)]
        # ViLBERT's first sub-layers are text-only (ctrl_vilbert_base: 0-11): the image embedding does not depend on them, nor they on it.
        # Its forward runs on the executor's side stream next to them (joined before the first sub-layer that touches the vision
        # stream), its backward likewise as soon as that sub-layer's backward has produced the vision gradient -- instead of at the very
        # end of the list, after the text-only sub-layers, whose launches (240 tiles or fewer) leave CUs idle.
        sched = list(sublayer_schedule(cfg))
        uses_v = lambda n, typ: (n in cfg.tv_attn_sublayers or n in cfg.vt_attn_sublayers or n in cfg.vv_attn_sublayers) if typ == "attn" else n in cfg.v_ff_sublayers
        k_vis = next((k for k, (n, typ) in enumerate(sched) if uses_v(n, typ)), len(sched))
        emb_image_aside = kind in ("vilbert", "lxmert") and 0 < k_vis < len(sched)
        emb_image_bwd = None
        if kind in ("vilbert", "lxmert"):
            bwd_stages.append(self._emb_text("bert.embeddings."))
            i0 = len(f)
            self._aside = "_aside" if emb_image_aside else ""           # its backward runs in a side-stream block: own temporaries and LayerNorm scratch
            img_bwd = (self._emb_image_vilbert if kind == "vilbert" else self._emb_image_lxmert)("bert.v_embeddings.")
            self._aside = ""
            if emb_image_aside:
                f.insert(i0, side_begin())
                f.append(side_end(EV_IMAGE_EMB_FWD))
                emb_image_bwd = [side_begin()] + img_bwd + [side_end(EV_IMAGE_EMB_BWD)] if img_bwd else []      # a frozen embedding: no block
                bwd_stages.append([])
            else:
                bwd_stages.append(img_bwd)
        elif kind == "uniter":
            bwd_stages.append(self._emb_text("bert.embeddings."))
            bwd_stages.append(self._emb_image_uniter("bert.embeddings."))
        elif kind == "visualbert":
            bwd_stages.append(self._emb_visualbert("bert.embeddings."))
        elif kind == "vl-bert":
            bwd_stages.append(self._emb_vlbert("bert.embeddings."))
        else:
            raise NotImplementedError("image_embeddings=%r" % kind)
        self.taps["emb_t"], self.taps["emb_v"] = self.x[0], self.x[1]
        self.n_sub = len(list(sublayer_schedule(cfg)))
        self.fwd_sub_start = []       # forward op index at which sub-layer k begins (the optimizer overlap cuts the list there)
        self.sublayer_ids = [n for n, _ in sched]       # taps "t<n>" / "v<n>": both streams' states after sub-layer n, forward order
        backbone = self.heads == "backbone"
        v_level0 = []                 # backbone, vision embedding aside: seeds of vision states no sub-layer has transformed yet
        sub_ops, n_head, sub_tail = [], [], []      # per sub-layer: its backward ops, how many seed ops lead them, what follows them in its stage
        for k, (n, typ) in enumerate(sched):
            self.sub_k = k
            self.fwd_sub_start.append(len(self.fwd.ops))
            if emb_image_aside and k == k_vis:
                f.append(wait_side(EV_IMAGE_EMB_FWD))       # the vision stream enters here: its embedding must be complete
            ops = self._attn_sublayer(n) if typ == "attn" else self._ffn_sublayer(n)
            sub_ops.append(ops)
            n_head.append(0)
            if backbone and k + 1 < self.n_sub:
                # d(loss)/d(state after sub-layer n), output_all_encoded_layers: added into the stream's current dX buffer at the head of the
                # sub-layer's backward stage, before anything reads it (the final states are the seeds of the heads' backward).  A stream the
                # sub-layer does not transform keeps its buffer, so the add lands where the next reader looks either way -- except for a
                # vision embedding that runs aside: its backward reads dX[1] from the side stream behind sub-layer k_vis, so the seeds of
                # the untransformed vision states go in front of that fork instead
                head = []
                for m, tag in ((0, "t"), (1, "v")):
                    if not self.live[m]:          # no trainable parameter upstream of this state: its gradient is carried no further
                        continue
                    self._seed_op(v_level0 if (m == 1 and emb_image_aside and self.level[1] == 0) else head,
                                  "%s%d" % (tag, n), self._dx(m, self.level[m] % 2), self.B, self.st[m].L, self.st[m].H, accumulate=1)
                ops[0:0] = head
                n_head[k] = len(head)
            sub_tail.append((v_level0 + emb_image_bwd) if (emb_image_aside and k == k_vis) else [])      # d(loss)/d(vision embedding) is final after this sub-layer's backward
            self.taps["t%d" % n], self.taps["v%d" % n] = self.x[0], self.x[1]
        # sub-layer k's backward first waits for the weight-gradient block of sub-layer k + 2, the previous user of its set of temporaries
        # (plan.py) -- where that block exists: a sub-layer whose blocks are all frozen has none and records no event
        for k, ops in enumerate(sub_ops):
            if k + 2 < self.n_sub and (k + 2) in self.wgrad_recorded:
                ops.insert(n_head[k], wait_side((k + 2) % EV_WGRAD_RING))
            bwd_stages.append(ops + sub_tail[k])
        self.fwd_heads_start = len(self.fwd.ops)
        head_bwd = self._heads() if self.heads == "pretrain" else self._heads_tasks()
        # backward list: zero-fills, heads, then stages in reverse; bwd_marks[s] = op index at which backward
        # stage s is complete (stage 0 = heads), param_ready_stage[name] = stage after which its gradient is final
        self.bwd.ops = list(self.bwd_pro) + list(head_bwd)
        if self.frozen:
            # A wait whose event the pruned list no longer records goes with the block that recorded it.  EV_DECODER_WGRAD is recorded by the
            # pre-training heads only: the text tables of the other plans wait for it in the unpruned list as well, and go on doing so.
            recorded = set() if self.heads == "pretrain" else {EV_DECODER_WGRAD}
            for ops in [self.bwd.ops] + bwd_stages[::-1]:
                kept = []
                for o in ops:
                    if o[0] == L.OP_SIDE_END:
                        recorded.add(o[1])
                    if o[0] != L.OP_WAIT_SIDE or o[1] in recorded:
                        kept.append(o)
                ops[:] = kept
        self.bwd_marks = [len(self.bwd.ops)]
        for ops in reversed(bwd_stages):
            self.bwd.ops += ops
            self.bwd_marks.append(len(self.bwd.ops))
        self.put(self.bwd.ops, L.OP_JOIN)
        prefixes = [["bert.t_pooler.", "bert.v_pooler.", "cls.", "clfs_dict."]] + [pf for pf in reversed(self.stage_prefix)]
        self.param_ready_stage = {}
        for name in self.arena.params:
            self.param_ready_stage[name] = max(i for i, pf in enumerate(prefixes) if any(name.startswith(q) for q in pf))
        self.fwd.freeze()
        self.bwd.freeze()

    def _build_score(self):
        """heads == "score" (volta_amd/retrieval.py): the existing builders, forward part only.  A prefix list runs one stream at B items;
        the pair list starts from per-pair buffers (`pair_inputs`: [(input name, tensor, side 0 caption | 1 image)], filled by one
        vk_pair_gather launch ahead of the list) and ends in `score_out`, fp32 logits [B, 64]."""
        cfg, B, T, Rv = self.cfg, self.B, self.T, self.Rv
        text_subs, vision_subs, per_modality = self.split
        kinds = dict(sublayer_schedule(cfg))
        self._begin()
        kind = cfg.image_embeddings

        def sublayers(ns):
            for n in ns:
                self._attn_sublayer(n) if kinds[n] == "attn" else self._ffn_sublayer(n)

        if self.part in ("text", "image"):
            m = 0 if self.part == "text" else 1
            subs = text_subs if m == 0 else vision_subs
            if not per_modality:
                raise ValueError("image_embeddings=%r mixes the modalities in its embedding: there is no per-modality prefix" % kind)
            if subs:
                self._mask_prep(m)
            if m == 0:
                self._emb_text("bert.embeddings.")
            elif kind == "uniter":
                self._emb_image_uniter("bert.embeddings.")
            else:
                (self._emb_image_vilbert if kind == "vilbert" else self._emb_image_lxmert)("bert.v_embeddings.")
            self.only = m
            sublayers(subs)
            self.only = None
            self.score_out = self.x[m]
            self.score_x8 = self.x8[m]     # e4m3 path, prefix ending in a sub-layer: (copy, row scales) its LayerNorm wrote; else None
        else:
            i64, f32 = torch.int64, torch.float32
            raw = [self.buf("pair_mask_t", (B, T), i64), self.buf("pair_mask_v", (B, Rv), i64)]
            u8, Hp = torch.uint8, _round_up(self.H, 128)
            make = {"x_t": lambda: self.buf("pair_x_t", (B * T, self.st[0].H)), "x_v": lambda: self.buf("pair_x_v", (B * Rv, self.st[1].H)),
                    "input_ids": lambda: self.buf("pair_ids", (B, T), i64), "token_type_ids": lambda: self.buf("pair_type_ids", (B, T), i64),
                    "image_feat": lambda: self.buf("pair_feat", (B, Rv, cfg.v_feature_size), f32),
                    "image_loc": lambda: self.buf("pair_loc", (B, Rv, cfg.num_locs), f32),
                    "attention_mask": lambda: raw[0], "image_attention_mask": lambda: raw[1],
                    "x8_t": lambda: self.buf("pair_x8_t", (B * T, Hp), u8), "xs_t": lambda: self.buf("pair_xs_t", (B * T,), f32),
                    "x8_v": lambda: self.buf("pair_x8_v", (B * Rv, Hp), u8), "xs_v": lambda: self.buf("pair_xs_v", (B * Rv,), f32)}
            self.pair_inputs = [(name, make[name](), side) for name, side in pair_segments(self.split, self.fp8)]
            ins = {name: t for name, t, _ in self.pair_inputs}
            a = self.pair_args = self.k(L.PairGatherArgs())
            for k, (_, t, side) in enumerate(self.pair_inputs):
                a.dst[k], a.bytes[k], a.side[k] = t.data_ptr(), t.numel() * t.element_size() // B, side
            a.nseg, a.npairs = len(self.pair_inputs), B
            self._mask_prep(0, raw[0])
            self._mask_prep(1, raw[1])
            if per_modality:
                self.x = [ins["x_t"], ins["x_v"]]
                # the hand-over: the gathered copy of the prefix LayerNorm's e4m3 output, or None (the first projection quantises x itself)
                self.x8 = [(ins["x8_" + c], ins["xs_" + c]) if "x8_" + c in ins else None for c in "tv"]
            elif kind == "visualbert":
                self._emb_visualbert("bert.embeddings.")
            else:
                self._emb_vlbert("bert.embeddings.")
            prefix = set(text_subs) | set(vision_subs)
            sublayers([n for n in kinds if n not in prefix])
            self._heads_score()
            self.bind_inputs({name: t for name, t, _ in self.pair_inputs})
        self.fwd.freeze()
        self.bwd.freeze()

    # -- gradient buffers of the hidden states.  dX[m] ping-pongs between two buffers: the k-th sub-layer (in
    # forward order) that transforms x[m] reads d(loss)/d(its output) from buffer k%2 and writes the gradient of
    # its input to buffer (k-1)%2; the embeddings read buffer 0, the heads fill buffer (final k)%2.
    def _dx(self, m, parity):
        return self.tmp("dx%d_%d" % (m, parity), (self.st[m].M, self.st[m].H), shared=True)      # the hidden-state gradients are shared by definition

    def _dx_step(self, m):
        self.level[m] += 1
        k = self.level[m]
        return self._dx(m, k % 2), self._dx(m, (k - 1) % 2)

    def _seed_op(self, ops, name, dst, B, L_, H, y=None, accumulate=0):
        """Appends to `ops` a vk_grad_seed launch into the bf16 gradient buffer dst [B * L_, H] from the fp32 gradient of output `name` (patched by bind_grads)."""
        a = self.k(L.GradSeedArgs(None, 0, 0, _addr(dst), _addr(y), B, L_, H, 0, dst.stride(0), y.stride(0) if y is not None else 0, accumulate, 0))
        assert name not in self.grad_seeds, name
        self.grad_seeds[name] = a
        self.emit(ops, L.FN_GRAD_SEED, p=(a,))

    def bind_grads(self, grads):
        """heads == "backbone": point the seed launches at this backward's gradients {output name: fp32 tensor or None}.  A gradient whose
        layout the kernel cannot read (stride along H other than 1, unaligned) is copied contiguous once; None zero-fills a final state /
        pooled seed and skips an intermediate one.  Returns the tensors the launches read (keep them alive until the backward is issued)."""
        keep = []
        for name, a in self.grad_seeds.items():
            g = grads.get(name)
            if g is None:
                a.src, a.stride_b, a.stride_l = None, 0, 0
                continue
            g3 = g if g.dim() == 3 else g.unsqueeze(1)
            if not (g3.dtype == torch.float32 and g3.device == self.dev and g3.stride(2) == 1 and g3.stride(0) % 4 == 0 and g3.stride(1) % 4 == 0
                    and g3.data_ptr() % 16 == 0):
                g3 = g3.to(device=self.dev, dtype=torch.float32).contiguous()
            assert tuple(g3.shape) == (a.B, a.L, a.H), (name, tuple(g.shape), (a.B, a.L, a.H))
            keep.append(g3)
            a.src, a.stride_b, a.stride_l = g3.data_ptr(), g3.stride(0), g3.stride(1)
        return keep

    def _slab(self, n):
        """fp32 workspace for split-K partials; one arena reused by every sub-layer (launches are stream-ordered)."""
        cap = 48 * 3072 * 768
        ws = self.tmp("wgrad_slabs", (cap,), torch.float32)
        cur = _round_up(self._slab_cursor, 4)
        assert cur + n <= cap, "wgrad slab workspace too small"
        self._slab_cursor = cur + n
        return ws[cur:cur + n]

    # ---------------------------------------------------------------- run
    def attention_maps(self):
        """(all_attention_mask_t, all_attention_mask_v) of BertEncoder.forward (volta/encoders.py:858-886) under config.visualization: per
        attention sub-layer and modality {"intra_attn", "inter_attn", "queries", "keys"} -- probabilities [B, heads, Lq, Lk] after dropout,
        query / key layers [B, heads, L, head size] (encoders.py:342-356); None where the modality takes no part.  Launches of a sub-layer
        whose streams differ in head geometry are listed one after the other."""
        out = ([], [])
        for info in self.attn_map_info:
            nh, dh = info["nh"], info["dh"]
            for m in range(2):
                if m not in info["qkv"]:
                    out[m].append({"intra_attn": None, "inter_attn": None, "queries": None, "keys": None})
                    continue
                qkv, Ha = info["qkv"][m], info["Ha"][m]
                Lm = self.st[m].L
                heads = lambda t: t.view(self.B, Lm, nh, dh).transpose(1, 2).float()
                p = info["probs"]
                out[m].append({"intra_attn": p[(m, m)].clone() if (m, m) in p else None,
                               "inter_attn": p[(m, 1 - m)].clone() if (m, 1 - m) in p else None,
                               "queries": heads(qkv[:, :Ha]), "keys": heads(qkv[:, Ha:2 * Ha])})
        return out

    def fwd_segments(self, bounds):
        """Cut the forward list for an optimizer that is still updating the arena in `bounds` = [chunk index where range r ends] (ranges in
        arena order = forward order): [(ranges that must be complete, op start, op end)].  The embeddings need what lies before the first
        encoder sub-layer, sub-layer n its own slots, the heads (poolers, cls.*, the tied decoder) everything."""
        arena = self.arena
        key = tuple(bounds)
        cache = self._fwd_segments
        if key in cache:
            return cache[key]

        def need(prefixes):          # number of leading ranges covering every parameter with one of these prefixes
            hi = max((arena.offset[nm] + int(torch.tensor(arena.shape[nm]).prod()) for nm in arena.params if nm.startswith(tuple(prefixes))), default=0)
            hi_chunk = -(-hi // CHUNK)
            return next((i + 1 for i, b in enumerate(bounds) if b >= hi_chunk), len(bounds))

        nemb = len(self.stage_prefix) - len(self.fwd_sub_start)
        cuts = [(need(self.stage_prefix[0] if nemb else ["bert.embeddings."]), 0)]
        for k, start in enumerate(self.fwd_sub_start):
            cuts.append((need(self.stage_prefix[nemb + k]), start))
        cuts.append((len(bounds), self.fwd_heads_start))
        segs, cur_need = [], 0
        for i, (nd, start) in enumerate(cuts):
            end = cuts[i + 1][1] if i + 1 < len(cuts) else len(self.fwd.ops)
            nd = max(nd, cur_need)                       # waits are cumulative
            if segs and nd == cur_need:
                segs[-1] = (nd, segs[-1][1], end)        # nothing new to wait for: extend the previous segment
            else:
                segs.append((nd, start, end))
            cur_need = nd
        cache[key] = segs
        return segs

    def run_forward(self):
        """The forward list; when a pipelined optimizer (AdamW(overlap_with_forward=True)) is still walking the arena on its own stream,
        every segment first waits for the ranges whose weights it reads."""
        pend = self.arena.opt_pending
        if not pend:
            self.fwd.run()
            return
        bounds, events = pend
        cur = torch.cuda.current_stream()
        waited = 0
        for nd, start, end in self.fwd_segments(bounds):
            for i in range(waited, nd):
                cur.wait_event(events[i])
            waited = max(waited, nd)
            self.fwd.run(start, end)
        self.arena.opt_pending = None

    def bind_inputs(self, tensors):
        """Patch the per-step input pointers into the few ops that read user tensors."""
        for name, sites in self.inputs.items():
            t = tensors[name]
            addr = t.data_ptr()
            for struct, field, index in sites:
                if index is None:
                    setattr(struct, field, addr)
                else:
                    getattr(struct, field)[index] = addr

    def prepare_step(self, seed):
        if self.train or self.nce_site is not None:      # nce_2048 draws its negatives in eval mode too
            check(L.lib.vk_set_seed(ptr(self.seed), C.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), L.stream_ptr()))
