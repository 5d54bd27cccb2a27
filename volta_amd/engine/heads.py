"""The head builders: the pre-training heads and losses, the task / backbone heads, and the scoring head of the retrieval pair plan."""
import torch

from .. import _lib as L
from .plan import EV_DECODER_WGRAD, EV_HEAD_REGIONS, EV_HEAD_REGIONS_BWD, NODROP, _addr, _mk_segs, _round_up, side_begin, side_end, wait_side

VIS_TARGET_WIDTH = {"0": 1601, "1": 2048, "2": 2048, "3": 1600, "4": 400, "5": 2048, "6": 1601}      # volta/losses.py:129-137
FUSE = {"mul": L.FUSE_MUL, "sum": L.FUSE_SUM, "text": L.FUSE_TEXT, "vl-bert_vqa": L.FUSE_TEXT}         # fusion method -> vk_pool_fuse code (VQA: the text pooler alone)


class HeadBuilders:
    """Base class of StepEngine.  `_heads` / `_heads_tasks` return the backward ops that fill the current dX buffers; `_heads_score` is forward only."""

    def _poolers(self):
        """ReLU(dense(first row)) of the text stream and, unless the fusion reads the text alone, of the vision stream, in one launch -> (pt, pv)."""
        cfg, B, H, Hv, P = self.cfg, self.B, self.H, self.st[1].H, self.cfg.pooler_size
        x_t, x_v = self.x
        pt, pv = self.buf("pooled_t", (B, P)), None
        pools = [self.prob(x_t, self.W("bert.t_pooler.dense.weight"), pt, B, P, H, self.T * H, H, P, bias=self.Pm("bert.t_pooler.dense.bias"))]
        if cfg.fusion_method != "text":
            pv = self.buf("pooled_v", (B, P))
            pools.append(self.prob(x_v, self.W("bert.v_pooler.dense.weight"), pv, B, P, Hv, self.Rv * Hv, Hv, P, bias=self.Pm("bert.v_pooler.dense.bias")))
        self.gemm(self.fwd.ops, L.NT, L.EPI_RELU, pools)
        return pt, pv

    def _pooler_bwd(self, b, wg, m, dy, dxh):
        """Stream m's pooler from dy [B, P] back: added into rows b * L of dxh[m] (every sample's first token); weight gradient listed in `wg`.
        Frozen parameters: the dgrad only where the stream's dX is needed, the weight gradient only for a trainable pooler."""
        B, P, Lm, Hm, pre = self.B, self.cfg.pooler_size, self.st[m].L, self.st[m].H, ("bert.t_pooler.dense.", "bert.v_pooler.dense.")[m]
        if self.live[m]:
            self.gemm(b, L.NN, L.EPI_ADDR, [self.prob(dy, self.W(pre + "weight"), dxh[m], B, Hm, P, P, Hm, Lm * Hm, R=dxh[m], ldr=Lm * Hm)])
        if not self.fz_linear(pre, prune=True):
            self.gemm(wg, L.TN, L.EPI_F32, [self.prob(dy, self.x[m], self.G(pre + "weight"), P, Hm, B, P, Lm * Hm, Hm, bias_grad=self.G(pre + "bias"))])

    def _pool_grad_needed(self, m):
        """Does anything read the gradient at stream m's pooled vector: its pooler's weights, or the stream below it?"""
        return self.live[m] or not self.fz_linear(("bert.t_pooler.dense.", "bert.v_pooler.dense.")[m])

    def _transform_fwd(self, tag, c, x, rows, count, M, Hm, ln=True):
        """cls.*.transform on the labelled rows of x: gather -> dense + GELU -> LayerNorm (where `ln`).  -> (transformed rows, state for _transform_bwd)."""
        f, w = self.fwd.ops, c + "transform."
        hx, h, gp = (self.buf(tag + nm, (M, Hm)) for nm in ("_hx", "_ht", "_gp"))
        self.emit(f, L.FN_GATHER, p=(x, rows, count, hx), n=(Hm, M))
        self.gemm(f, L.NT, L.EPI_GELU, [self.prob(hx, self.W(w + "dense.weight"), h, M, Hm, Hm, Hm, Hm, Hm, bias=self.Pm(w + "dense.bias"), C2=gp, dyn=count)])
        hn, mean, rstd = h, None, None
        if ln:
            hn, mean, rstd = self.buf(tag + "_hn", (M, Hm)), self.buf(tag + "_mean", (M,), torch.float32), self.buf(tag + "_rstd", (M,), torch.float32)
            self.ln_fwd(f, h, None, w + "LayerNorm.weight", w + "LayerNorm.bias", hn, None, mean, rstd, M, NODROP, dyn=count, H=Hm)
        return hn, (w, hx, h, gp, mean, rstd, rows, count, M, Hm)

    def _transform_bwd(self, b, wg, tmp, state, dhn, dx, own_partial=False):
        """From dhn (temporary `tmp`_d1) back into the labelled rows of dx (scatter-add); the dense layer's weight gradient is listed in `wg`."""
        w, hx, h, gp, mean, rstd, rows, count, M, Hm = state
        # frozen parameters: `dx` None = the stream's dX is not needed; every step below runs only if something trainable reads its output
        dense_on = not self.fz_linear(w + "dense.", prune=True)
        need_du = dx is not None or dense_on
        dh = dhn
        if mean is not None:
            dh = self.tmp(tmp + "_d2", (M, Hm))
            if need_du or not self.fz(w + "LayerNorm.weight", w + "LayerNorm.bias"):
                self.ln_bwd(b, dhn, h, mean, rstd, w + "LayerNorm.weight", w + "LayerNorm.bias", dh if need_du else None, None, M, NODROP, dyn=count,
                            own_partial=own_partial, H=Hm)
            else:
                self.prune(w + "LayerNorm.weight", w + "LayerNorm.bias")
        if not need_du:
            return
        du = self.tmp(tmp + "_d3", (M, Hm))
        self.emit(b, L.FN_MUL, p=(dh, gp, du, count), n=(M * Hm, Hm))
        dhx = self.tmp(tmp + ("_d2" if mean is None else "_d1"), (M, Hm))
        if dx is not None:
            self.gemm(b, L.NN, L.EPI_BF16, [self.prob(du, self.W(w + "dense.weight"), dhx, M, Hm, Hm, Hm, Hm, Hm, dyn=count)])
        if dense_on:
            self.gemm(wg, L.TN, L.EPI_F32, [self.prob(du, hx, self.G(w + "dense.weight"), Hm, Hm, M, Hm, Hm, Hm, bias_grad=self.G(w + "dense.bias"), dyn=count)])
        if dx is not None:
            self.emit(b, L.FN_SCATTER_ADD, p=(dhx, rows, count, dx), n=(Hm, M))

    def _heads(self):
        cfg, B, H, T, Rv, R = self.cfg, self.B, self.H, self.T, self.Rv, self.R
        Hv = self.st[1].H                               # the vision stream's width (config/vilbert_base.json: 1024 against 768)
        f = self.fwd.ops
        st_t = self.st[0]
        fm = cfg.fusion_method
        has_itm = fm in ("mul", "sum", "text")         # encoders.py:744-747: no ITM head for "none" / "vl-bert_vqa"
        P = cfg.pooler_size if has_itm else 0
        if has_itm and ((fm != "text" and P != cfg.v_pooler_size) or P % 64):
            raise NotImplementedError("pooler sizes must match and be multiples of 64")
        if fm == "vl-bert_vqa":                        # the VQA text pooler exists but feeds nothing in pre-training (its .grad stays None)
            self.unused_params |= {"bert.t_pooler.dense.weight", "bert.t_pooler.dense.bias"}
        V, Vp = cfg.vocab_size, _round_up(cfg.vocab_size, 64)
        targets = [(ix, float(w)) for ix, w in cfg.visual_target_weights.items() if w > 0]
        if not targets:
            raise NotImplementedError("no visual target with a positive weight")
        if {ix for ix, _ in targets} & {"1", "2", "5"} and cfg.add_global_imgfeat is not None:
            raise NotImplementedError("the feature-regression targets compare [B, R, 2048] predictions with the [B, R+1, 2048] input "
                                      "when a global feature is added (losses.py:28,41,108 fail on the shapes)")
        x_t, x_v = self.x
        self.sums = self.buf("loss_sums", (4,), torch.float32)
        self.losses = self.buf("losses", (3,), torch.float32)
        self.gout = self.buf("gout", (3,), torch.float32)
        self.zero(f, self.sums)
        # ---- ITM: poolers, fusion, classifier
        pt = pv = None
        if has_itm:
            pt, pv = self._poolers()
        elif fm == "vl-bert_vqa":
            pt = self._vqa_text_pooler(f, x_t)[0]               # BertModel's fourth output; nothing in the pre-training loss reads it
        # ---- masked LM on labelled rows
        n_t, n_v = self.buf("n_t", (1,), torch.int32), self.buf("n_v", (1,), torch.int32)
        rows_t, pos_t = self.buf("rows_t", (st_t.M,), torch.int32), self.buf("pos_t", (st_t.M,), torch.int32)
        self.patch("masked_lm_labels", self.emit(f, L.FN_SELECT, p=(None, rows_t, pos_t, n_t), n=(st_t.M, 0, T, T, 0)), "p", 0)
        c = "cls.predictions."
        hn_t, lm_tr = self._transform_fwd("lm", c, x_t, rows_t, n_t, st_t.M, H)
        logits_t = self.buf("lm_logits", (st_t.M, Vp), torch.float32)
        wword = "bert.embeddings.word_embeddings.weight"
        self.gemm(f, L.NT, L.EPI_F32, [self.prob(hn_t, self.W(wword), logits_t, st_t.M, V, H, H, H, Vp, bias=self.Pm(c + "bias"), dyn=n_t, n_store=Vp)])
        lse_t = self.buf("lm_lse", (st_t.M,), torch.float32)
        xa = self.k(L.XentArgs(_addr(logits_t), None, _addr(pos_t), _addr(n_t), _addr(lse_t), _addr(self.sums[0:1]), V, Vp, st_t.M))
        self.patch("masked_lm_labels", xa, "labels")
        self.put(f, L.OP_XENT_FWD, xa)
        # ---- masked regions (kl_1601) on labelled rows: an independent chain of small launches -> side stream, joined before the loss finalisation
        f.append(side_begin())
        Mr = B * R
        rows_v, pos_v = self.buf("rows_v", (Mr,), torch.int32), self.buf("pos_v", (Mr,), torch.int32)
        off = 1 if cfg.add_global_imgfeat == "first" else 0
        self.patch("image_label", self.emit(f, L.FN_SELECT, p=(None, rows_v, pos_v, n_v), n=(Mr, 1, R, Rv, off)), "p", 0)
        ci = "cls.imagePredictions."
        hn_v, img_tr = self._transform_fwd("img", ci, x_v, rows_v, n_v, Mr, Hv, ln=cfg.image_head_ln)
        # one decoder + loss per configured visual target (encoders.py:718-737,1079-1087; losses.py); all of them add their WEIGHTED row
        # losses to sums[1], the image loss is sums[1] / max(#masked regions, 1)
        vis = []                                                # (ix, Cn, Cp, forward-args struct, is_kl)
        for ix, w in targets:
            Cn = VIS_TARGET_WIDTH[ix]
            Cp = _round_up(Cn, 64)
            tag = "img" if ix == "0" else "img%s" % ix
            logits_v = self.buf(tag + "_logits", (Mr, Cp), torch.float32)
            wdec = ci + "decoder_dict.%s." % ix
            self.gemm(f, L.NT, L.EPI_F32, [self.prob(hn_v, self.W(wdec + "weight"), logits_v, Mr, Cn, Hv, Hv, Hv, Cp, bias=self.Pm(wdec + "bias"), dyn=n_v, n_store=Cp)])
            lse_v = self.buf(tag + "_lse", (Mr,), torch.float32)
            if ix == "0":
                tsum_v = self.buf("img_tsum", (Mr,), torch.float32)
                la = self.k(L.KlArgs(_addr(logits_v), None, _addr(pos_v), _addr(n_v), _addr(lse_v), _addr(tsum_v), _addr(self.sums[1:2]), w, Cn, Cp, Mr))
                self.patch("image_cls", la, "target")
                self.put(f, L.OP_KL_FWD, la)
            else:
                kind = {"1": L.VIS_MSE, "2": L.VIS_NCE, "3": L.VIS_XENT, "4": L.VIS_XENT, "5": L.VIS_HUBER, "6": L.VIS_XENT}[ix]
                la = L.VisLossArgs(_addr(logits_v), None, None, None, _addr(pos_v), _addr(n_v), None, _addr(lse_v), None, _addr(self.sums[1:2]), w, Cn, Cp, Mr, kind, 0)
                self.k(la)
                if kind in (L.VIS_MSE, L.VIS_HUBER, L.VIS_NCE):
                    self.patch("image_feat", la, "target")
                if kind == L.VIS_XENT:
                    self.patch("attr_labels" if ix == "4" else "obj_labels", la, "labels")
                    if ix in ("3", "4"):
                        self.patch("attr_confs" if ix == "4" else "obj_confs", la, "conf")
                if kind == L.VIS_NCE:
                    nneg = L.NCE_ACROSS + L.NCE_INSIDE
                    neg = self.buf("img_nce_neg", (B * R * nneg,), torch.int32)
                    aux = self.buf("img_nce_scores", (Mr, L.NCE_MAX_SAMPLES), torch.float32)
                    la.neg_index, la.aux, la.n_neg = _addr(neg), _addr(aux), nneg
                    self.nce_site = self.site                    # the negatives' counter-based stream (drawn in eval mode too, as the reference does)
                    self.site += 1
                    rng = L.rng_cfg(self.seed.data_ptr(), self.nce_site)
                    self.emit(f, L.FN_NCE_NEG, p=(neg,), n=(B, R), drop=rng)
                self.emit(f, L.FN_VIS_LOSS_FWD, p=(la,))
            vis.append((ix, Cn, Cp, la, tag))
        f.append(side_end(EV_HEAD_REGIONS))
        # ---- ITM head (its dropout site is the last one of the forward pass)
        fuse = FUSE.get(fm)
        pdrop = self.drop(0.1)                                   # the reference's nn.Dropout(0.1) sits in every variant of the heads
        if has_itm:
            pooled = self.buf("pooled", (B, P))
            self.emit(f, L.FN_POOL_FWD, p=(pt, pv, pooled), n=(B, P, 0, fuse), drop=pdrop)
            itm = self.buf("itm_logits", (B, 64), torch.float32)
            self.gemm(f, L.NT, L.EPI_F32, [self.prob(pooled, self.W("cls.bi_seq_relationship.weight"), itm, B, 2, P, P, P, 64, bias=self.Pm("cls.bi_seq_relationship.bias"), n_store=64)])
            lse_i = self.buf("itm_lse", (B,), torch.float32)
            xi = self.k(L.XentArgs(_addr(itm), None, None, None, _addr(lse_i), _addr(self.sums[2:3]), 2, 64, B))
            self.patch("next_sentence_label", xi, "labels")
            self.put(f, L.OP_XENT_FWD, xi)
        f.append(wait_side(EV_HEAD_REGIONS))
        self.emit(f, L.FN_LOSS_FINAL, p=(self.sums, n_t, n_v, self.losses), n=(B,), f=(1.0,))
        self.taps.update(seq_t=x_t, seq_v=x_v, pooled_t=pt, pooled_v=pv)

        # ================= backward of the heads: produces dX[0], dX[1].  Three independent chains of small launches, each with temporaries of
        # its own: the masked-LM and ITM chains stay on the caller's stream, the region chain (with its weight gradients) runs on the side
        # stream next to them, and every weight gradient of the two main chains follows in a second side block (events: plan.py).
        # Frozen parameters: a chain runs as far down as something trainable reads it -- its own parameters, or the
        # stream below the heads (`self.live`); a weight gradient only for a trainable block.
        b, wg = [], []
        dxh = [self._dx(m, self.level[m] % 2) for m in range(2)]
        live = list(self.live)
        for m in range(2):
            if live[m]:
                self.zero(b, dxh[m])
        tr_on = lambda c: not self.fz(*self.prefix_names(c + "transform."))
        # ---- region chain (side stream)
        dec_on = [not self.fz_linear(ci + "decoder_dict.%s." % ix, prune=True) for ix, _, _, _, _ in vis]
        need_dhn_v = live[1] or tr_on(ci)
        rb = []
        dhn_v = self.tmp("head_v_d1", (Mr, Hv))
        for j, (ix, Cn, Cp, la, tag) in enumerate(vis):
            dlog_v = self.buf(tag + "_dlogits", (Mr, Cp))
            if not (need_dhn_v or dec_on[j]):
                continue
            if ix == "0":
                self.put(rb, L.OP_KL_BWD, la, dlog_v, self.gout[1:2], i0=Cp)
            else:
                self.emit(rb, L.FN_VIS_LOSS_BWD, p=(la, dlog_v, self.gout[1:2]), n=(Cp,))
            wdec = ci + "decoder_dict.%s." % ix
            if not need_dhn_v:
                pass
            elif j == 0:
                self.gemm(rb, L.NN, L.EPI_BF16, [self.prob(dlog_v, self.W(wdec + "weight"), dhn_v, Mr, Hv, Cn, Cp, Hv, Hv, dyn=n_v)])
            else:                                               # the decoders share the transformed hidden state: their input gradients add up
                self.gemm(rb, L.NN, L.EPI_ADDR, [self.prob(dlog_v, self.W(wdec + "weight"), dhn_v, Mr, Hv, Cn, Cp, Hv, Hv, dyn=n_v, R=dhn_v, ldr=Hv)])
            if dec_on[j]:
                self.gemm(rb, L.TN, L.EPI_F32, [self.prob(dlog_v, hn_v, self.G(wdec + "weight"), Cn, Hv, Mr, Cp, Hv, Hv, bias_grad=self.G(wdec + "bias"), dyn=n_v)])
        if need_dhn_v:
            self._transform_bwd(rb, rb, "head_v", img_tr, dhn_v, dxh[1] if live[1] else None, own_partial=True)
        else:
            self.prune(*self.prefix_names(ci + "transform."))
        if rb:
            b += [side_begin()] + rb + [side_end(EV_HEAD_REGIONS_BWD)]
        # ---- masked-LM chain
        dec_t_on = not self.prune(wword, c + "bias")
        if dec_t_on:
            self.pruned.discard(wword)           # frozen with its embedding, but still written here with the trainable decoder bias
        need_dhn_t = live[0] or tr_on(c)
        dlog_t = self.buf("lm_dlogits", (st_t.M, Vp))
        if need_dhn_t or dec_t_on:
            self.put(b, L.OP_XENT_BWD, xa, dlog_t, self.gout[0:1], i0=Vp)
        dhn_t = self.tmp("head_d1", (st_t.M, H))
        # d(hidden) = dlogits[n_t, V] . E[V, H]: few rows, very long contraction -> split K over the vocabulary into
        # chunks written as fp32 slabs by one grouped launch, then summed (and rounded to bf16) in one pass
        nsplit = max(1, min(16, V // 1920))
        if not need_dhn_t:
            pass
        elif nsplit == 1:
            self.gemm(b, L.NN, L.EPI_BF16, [self.prob(dlog_t, self.W(wword), dhn_t, st_t.M, H, V, Vp, H, H, dyn=n_t)])
        else:
            kc = _round_up(-(-V // nsplit), 64)
            stride = st_t.M * H
            slabs = self.buf("lm_dgrad_slabs", (nsplit * stride,), torch.float32)
            probs, k0, wv = [], 0, self.W(wword)
            while k0 < V:
                kk = min(kc, V - k0)
                i = len(probs)
                probs.append(self.prob(dlog_t[:, k0:], wv[k0:], slabs[i * stride:], st_t.M, H, kk, Vp, H, H, dyn=n_t))
                k0 += kc
            self.gemm(b, L.NN, L.EPI_F32, probs)
            self.emit(b, L.FN_SUM_SLABS_BF16, p=(dhn_t, slabs, n_t), n=(stride, len(probs), stride, H))
        if dec_t_on:
            self.gemm(wg, L.TN, L.EPI_F32, [self.prob(dlog_t, hn_t, self.G(wword), V, H, st_t.M, Vp, H, H, bias_grad=self.G(c + "bias"), dyn=n_t)])
        elif not self.fz(*self.prefix_names("bert.embeddings.")):
            # the text tables' backward adds to the word table's gradient, which the decoder's weight gradient no longer initialises
            self.zero(self.bwd_pro, self.G(wword))
            self.pruned.discard(wword)
        if need_dhn_t:
            self._transform_bwd(b, wg, "head", lm_tr, dhn_t, dxh[0] if live[0] else None)
        else:
            self.prune(*self.prefix_names(c + "transform."))
        # ---- ITM chain
        if has_itm:
            wi = "cls.bi_seq_relationship."
            itm_on = not self.fz_linear(wi, prune=True)
            need_pool = [self._pool_grad_needed(0), pv is not None and self._pool_grad_needed(1)]
            dlog_i = self.buf("itm_dlogits", (B, 64))
            if itm_on or any(need_pool):
                self.put(b, L.OP_XENT_BWD, xi, dlog_i, self.gout[2:3], i0=64)
            dpooled = self.buf("d_pooled", (B, P))
            if any(need_pool):
                self.gemm(b, L.NN, L.EPI_BF16, [self.prob(dlog_i, self.W(wi + "weight"), dpooled, B, P, 2, 64, P, P)])
            if itm_on:
                self.gemm(wg, L.TN, L.EPI_F32, [self.prob(dlog_i, pooled, self.G(wi + "weight"), 2, P, B, 64, P, P, bias_grad=self.G(wi + "bias"))])
            dyt = self.buf("d_pool_t", (B, P))
            dyv = self.buf("d_pool_v", (B, P)) if pv is not None else None
            if any(need_pool):
                self.emit(b, L.FN_POOL_BWD, p=(dpooled, pt, pv, dyt, dyv), n=(B, P, P, fuse), drop=pdrop)
            for m, dy_ in ((0, dyt), (1, dyv)):          # rows b * L: disjoint from the labelled rows the region chain scatters into
                if dy_ is not None and need_pool[m]:
                    self._pooler_bwd(b, wg, m, dy_, dxh)
                elif dy_ is not None:
                    self.fz_linear(("bert.t_pooler.dense.", "bert.v_pooler.dense.")[m], prune=True)
        # ---- the main chains' weight gradients, off the critical path
        if wg:
            b.append(side_begin())
            b += wg
            b.append(side_end(EV_DECODER_WGRAD))
        b.append(wait_side(EV_HEAD_REGIONS_BWD))            # dX[1] is complete
        return b

    def _vqa_text_pooler(self, f, x_t):
        """VLBertTextPooler (volta/encoders.py:610-623): ReLU(dense(hidden state of the token two places before the caption's end)).
        -> (pooled [B, P], gathered rows [B, H], row index [B], count)."""
        cfg, B, H, T = self.cfg, self.B, self.H, self.T
        P = cfg.pooler_size
        if P % 64:
            raise NotImplementedError("pooler size must be a multiple of 64")
        rows, cnt = self.buf("vqa_rows", (B,), torch.int32), self.buf("vqa_cnt", (1,), torch.int32)
        self.patch("input_ids", self.emit(f, L.FN_TEXT_END_ROWS, p=(None, rows, cnt), n=(B, T)), "p", 0)
        xg = self.buf("vqa_x", (B, H))
        self.emit(f, L.FN_GATHER, p=(x_t, rows, cnt, xg), n=(H, B))
        pt = self.buf("pooled_t", (B, P))
        self.gemm(f, L.NT, L.EPI_RELU, [self.prob(xg, self.W("bert.t_pooler.dense.weight"), pt, B, P, H, H, H, P, bias=self.Pm("bert.t_pooler.dense.bias"))])
        return pt, xg, rows, cnt

    def _heads_tasks(self):
        """BertForVLTasks behind the encoder (volta/encoders.py:1117-1206): poolers (:1004-1011; none / text-only / VLBertTextPooler by fusion
        method, :936-947), the fusion + dropout of the pooled vectors (:1184-1195) and the task's classifier (:1128-1149: SimpleClassifier =
        Linear -> GELU -> LayerNorm -> Linear (:787-814), plain Linear heads, the one- and two-layer region-logit heads on dropout(seq_v)),
        forward and backward.  The prediction leaves the engine as fp32 logits (`self.pred`, leading dimension padded to 64); the backward is
        seeded by d(loss)/d(logits), which the host writes (bf16) into `self.d_pred`.  Without a task (BertModel.forward / encode()) only the
        poolers are built."""
        cfg, B, H, Rv = self.cfg, self.B, self.H, self.Rv
        f = self.fwd.ops
        fm = cfg.fusion_method
        P = cfg.pooler_size
        if fm != "none" and ((fm in ("mul", "sum") and P != cfg.v_pooler_size) or P % 64):
            raise NotImplementedError("pooler sizes must match and be multiples of 64")
        x_t, x_v = self.x
        st_v = self.st[1]
        Hv = st_v.H
        pt = pv = vqa = None
        if fm == "vl-bert_vqa":
            pt, xg, vqa_rows, vqa_cnt = vqa = self._vqa_text_pooler(f, x_t)
        elif fm != "none":
            pt, pv = self._poolers()
        self.taps.update(seq_t=x_t, seq_v=x_v, pooled_t=pt, pooled_v=pv)
        # The word-embedding gradient is accumulated with atomics by the embedding backward; in the pre-training model the LM
        # decoder's weight gradient (same tied tensor) is what initialises it, here nothing else writes it: zero it per step.
        for nm in self.arena.params:
            if nm.endswith("embeddings.word_embeddings.weight") and not self.fz(*self.prefix_names(nm[:-len("word_embeddings.weight")])):
                self.zero(self.bwd_pro, self.G(nm))
        # Frozen parameters: a step of the backward runs only if something trainable reads its output -- the
        # parameters of the step before it, or the stream below the heads (`self.live`); a weight gradient only for a trainable block.
        b = []
        dxh = [self._dx(m, self.level[m] % 2) for m in range(2)]
        live = list(self.live)
        backbone = self.heads == "backbone"
        for m in range(2):
            if not live[m]:
                continue
            if backbone:                                   # d(loss)/d(seq_t), d(loss)/d(seq_v) from outside, written before the poolers add theirs
                self._seed_op(b, ("seq_t", "seq_v")[m], dxh[m], B, self.st[m].L, self.st[m].H)
            else:                                          # the sequence outputs feed nothing but the task head
                self.zero(b, dxh[m])
        self.pred = self.d_pred = None
        heads_of_other_tasks = [nm for nm in self.arena.params if nm.startswith("clfs_dict.")]
        dpool = [None, None]                               # gradients at the poolers' pre-activation outputs
        if backbone:
            if self.task is not None:
                raise ValueError("the backbone plan has no task head")
            for m, (py, nm) in enumerate(((pt, "pooled_t"), (pv, "pooled_v"))):
                if py is not None:                         # ReLU poolers: d pre-activation = d pooled * (pooled > 0)
                    dpool[m] = self.buf("d_" + nm, (B, P))
                    if self._pool_grad_needed(m):
                        self._seed_op(b, nm, dpool[m], B, 1, P, y=py)
        elif self.task is not None:
            task_id, tcfg = self.task
            typ = tcfg["type"]
            pre = "clfs_dict.%s." % task_id
            heads_of_other_tasks = [nm for nm in heads_of_other_tasks if not nm.startswith(pre)]

            def linear_out(x, rows, K, wname, C):
                """logits = x W^T + b as fp32 [rows, 64 k]; returns (logits, dlogits bf16)."""
                Cp = _round_up(C, 64)
                out = self.buf("task_logits", (rows, Cp), torch.float32)
                self.gemm(f, L.NT, L.EPI_F32, [self.prob(x, self.W(wname + "weight"), out, rows, C, K, K, K, Cp, bias=self.Pm(wname + "bias"), n_store=Cp)])
                return out, self.buf("task_dlogits", (rows, Cp), zero=True), Cp

            def linear_bwd(dlog, Cp, x, rows, K, wname, C, dx, need_dx=True):
                if need_dx:
                    self.gemm(b, L.NN, L.EPI_BF16, [self.prob(dlog, self.W(wname + "weight"), dx, rows, K, C, Cp, K, K)])
                if not self.fz_linear(wname, prune=True):
                    self.gemm(b, L.TN, L.EPI_F32, [self.prob(dlog, x, self.G(wname + "weight"), C, K, rows, Cp, K, K, bias_grad=self.G(wname + "bias"))])

            if typ.startswith("V-logit"):
                Mv = st_v.M
                d0 = self.drop(self.task_dropout)            # BertForVLTasks.dropout on the region states (:1198)
                xd = self.buf("task_xd", (Mv, Hv))
                self.emit(f, L.FN_ADD_DROPOUT, p=(x_v, None, xd), n=(Mv, Hv, 0), f=(1.0,), drop=d0)
                if tcfg.get("num_clf_layers", 1) == 2:       # Linear -> GELU -> Dropout -> Linear (:1138-1144)
                    h, gp = self.buf("task_h", (Mv, Hv)), self.buf("task_gp", (Mv, Hv))
                    self.gemm(f, L.NT, L.EPI_GELU, [self.prob(xd, self.W(pre + "0.weight"), h, Mv, Hv, Hv, Hv, Hv, Hv, bias=self.Pm(pre + "0.bias"), C2=gp)])
                    d1 = self.drop(cfg.v_attention_probs_dropout_prob)
                    hd = self.buf("task_hd", (Mv, Hv))
                    self.emit(f, L.FN_ADD_DROPOUT, p=(h, None, hd), n=(Mv, Hv, 0), f=(1.0,), drop=d1)
                    self.pred, self.d_pred, Cp = linear_out(hd, Mv, Hv, pre + "3.", 1)
                    dhd, dh, du = self.buf("task_dhd", (Mv, Hv)), self.buf("task_dh", (Mv, Hv)), self.buf("task_du", (Mv, Hv))
                    need_du = live[1] or not self.fz_linear(pre + "0.")
                    linear_bwd(self.d_pred, Cp, hd, Mv, Hv, pre + "3.", 1, dhd, need_du)
                    if need_du:
                        self.emit(b, L.FN_ADD_DROPOUT, p=(dhd, None, dh), n=(Mv, Hv, 1), f=(1.0,), drop=d1)
                        self.emit(b, L.FN_MUL, p=(dh, gp, du, None), n=(Mv * Hv, Hv))
                    dxd = self.buf("task_dxd", (Mv, Hv))
                    if need_du:
                        linear_bwd(du, Hv, xd, Mv, Hv, pre + "0.", Hv, dxd, live[1])
                    else:
                        self.fz_linear(pre + "0.", prune=True)
                else:
                    self.pred, self.d_pred, Cp = linear_out(xd, Mv, Hv, pre, 1)
                    dxd = self.buf("task_dxd", (Mv, Hv))
                    linear_bwd(self.d_pred, Cp, xd, Mv, Hv, pre, 1, dxd, live[1])
                if live[1]:
                    self.emit(b, L.FN_ADD_DROPOUT, p=(dxd, None, dxh[1]), n=(Mv, Hv, 1), f=(1.0,), drop=d0)
                self.pred_shape = (B, Rv, 1)
            else:
                if fm == "none":
                    raise ValueError("task type %r needs a pooled output; fusion method 'none' has none (encoders.py:1192-1193)" % typ)
                fuse = FUSE[fm]
                d0 = self.drop(self.task_dropout)            # BertForVLTasks.dropout on the fused pooled vector (:1184-1191)
                pooled = self.buf("pooled", (B, P))
                self.emit(f, L.FN_POOL_FWD, p=(pt, pv, pooled), n=(B, P, 0, fuse), drop=d0)
                rows, K0 = (B // 2, 2 * P) if typ == "VL-binary-classifier" else (B, P)      # NLVR2 pairs: view(-1, 2 P) (:1202)
                if typ == "VL-binary-classifier" and B % 2:
                    raise ValueError("VL-binary-classifier pools pairs of samples: the batch size must be even")
                dpooled = self.buf("d_pooled", (B, P))
                need_p = self._pool_grad_needed(0) or (pv is not None and self._pool_grad_needed(1))
                if typ in ("VL-classifier", "VL-classifier-GQA", "VL-binary-classifier"):
                    C = 2 if typ == "VL-binary-classifier" else int(tcfg["num_labels"])
                    Hc = cfg.clf_hidden_size
                    if Hc % 64 or Hc > 2048:
                        raise NotImplementedError("clf_hidden_size must be a multiple of 64, <= 2048")
                    hc, gpc = self.buf("task_h", (rows, Hc)), self.buf("task_gp", (rows, Hc))
                    w0, lnn, w3 = pre + "logit_fc.0.", pre + "logit_fc.2.", pre + "logit_fc.3."
                    self.gemm(f, L.NT, L.EPI_GELU, [self.prob(pooled, self.W(w0 + "weight"), hc, rows, Hc, K0, K0, K0, Hc, bias=self.Pm(w0 + "bias"), C2=gpc)])
                    hn = self.buf("task_hn", (rows, Hc))
                    mean, rstd = self.buf("task_mean", (rows,), torch.float32), self.buf("task_rstd", (rows,), torch.float32)
                    self.ln_fwd(f, hc, None, lnn + "weight", lnn + "bias", hn, None, mean, rstd, rows, NODROP, H=Hc)
                    self.pred, self.d_pred, Cp = linear_out(hn, rows, Hc, w3, C)
                    dhn, dhc, du = self.buf("task_dhn", (rows, Hc)), self.buf("task_dhc", (rows, Hc)), self.buf("task_du", (rows, Hc))
                    need_du = need_p or not self.fz_linear(w0)
                    ln_off = self.prune(lnn + "weight", lnn + "bias")
                    linear_bwd(self.d_pred, Cp, hn, rows, Hc, w3, C, dhn, need_du or not ln_off)
                    part = self.buf("task_ln_partial", (L.lib.vk_ln_bwd_partial_rows(rows) * 2 * Hc,), torch.float32)
                    if need_du or not ln_off:
                        lb = L.LnBwdArgs(_addr(dhn), _addr(hc), _addr(mean), _addr(rstd), _addr(self.Pm(lnn + "weight")), _addr(dhc) if need_du else None, None,
                                         None if ln_off else _addr(part), None if ln_off else _addr(self.G(lnn + "weight")),
                                         None if ln_off else _addr(self.G(lnn + "bias")), None, rows, Hc, rows, 0, 1.0, 0, NODROP, _mk_segs(NODROP, None))
                        self.put(b, L.OP_LN_BWD, self.k(lb))
                    if need_du:
                        self.emit(b, L.FN_MUL, p=(dhc, gpc, du, None), n=(rows * Hc, Hc))
                        linear_bwd(du, Hc, pooled, rows, K0, w0, Hc, dpooled, need_p)
                    else:
                        self.fz_linear(w0, prune=True)
                else:                                         # VL-tri-classifier (3 classes), VL-logit (1 score): one Linear (:1134-1137)
                    C = 3 if typ == "VL-tri-classifier" else 1
                    self.pred, self.d_pred, Cp = linear_out(pooled, rows, K0, pre, C)
                    linear_bwd(self.d_pred, Cp, pooled, rows, K0, pre, C, dpooled, need_p)
                self.pred_shape = (rows, C)
                dpool[0] = self.buf("d_pool_t", (B, P))
                dpool[1] = self.buf("d_pool_v", (B, P)) if pv is not None else None
                if need_p:
                    self.emit(b, L.FN_POOL_BWD, p=(dpooled, pt, pv, dpool[0], dpool[1]), n=(B, P, P, fuse), drop=d0)
        self.unused_params |= set(heads_of_other_tasks)      # the classifiers of the other tasks (and, for region-logit tasks, the poolers) get no gradient
        for m, (pre_p, py) in enumerate((("bert.t_pooler.dense.", pt), ("bert.v_pooler.dense.", pv))):
            if py is None:
                continue
            if dpool[m] is None:
                self.unused_params |= {pre_p + "weight", pre_p + "bias"}
                continue
            if not self._pool_grad_needed(m):
                self.fz_linear(pre_p, prune=True)
            elif vqa is not None:                          # the pooled token differs per caption: gathered rows in, scatter-add out
                dxg = self.buf("vqa_dx", (B, H))
                if live[0]:
                    self.gemm(b, L.NN, L.EPI_BF16, [self.prob(dpool[m], self.W(pre_p + "weight"), dxg, B, H, P, P, H, H)])
                    self.emit(b, L.FN_SCATTER_ADD, p=(dxg, vqa_rows, vqa_cnt, dxh[0]), n=(H, B))
                if not self.fz_linear(pre_p, prune=True):
                    self.gemm(b, L.TN, L.EPI_F32, [self.prob(dpool[m], xg, self.G(pre_p + "weight"), P, H, B, P, H, H, bias_grad=self.G(pre_p + "bias"))])
            else:
                self._pooler_bwd(b, b, m, dpool[m], dxh)
        return b

    def _heads_score(self):
        """Poolers, fusion and the scoring head of the pair list, as the task plan computes them in eval mode (_heads_tasks: VL-logit's
        Linear(P, 1) on the fused pooled vector) or, for task None, as BertForVLPreTraining._scores computes seq_relationship_score: the fp32
        product (sum) of the two bf16 pooled vectors rounded to bf16 -- what vk_pool_fuse_fwd computes without dropout -- then Linear(P, 2)."""
        cfg, B, f = self.cfg, self.B, self.fwd.ops
        fm, P = cfg.fusion_method, cfg.pooler_size
        if fm not in ("mul", "sum", "text"):
            raise ValueError("fusion method %r has no ITM head to score with" % fm)
        if (fm != "text" and P != cfg.v_pooler_size) or P % 64:
            raise NotImplementedError("pooler sizes must match and be multiples of 64")
        pt, pv = self._poolers()
        pooled = self.buf("pooled", (B, P))
        self.emit(f, L.FN_POOL_FWD, p=(pt, pv, pooled), n=(B, P, 0, FUSE[fm]))
        if self.task is not None:
            task_id, tcfg = self.task
            if tcfg["type"] != "VL-logit":
                raise ValueError("task type %r does not score a pair (VL-logit does)" % tcfg["type"])
            wname, C = "clfs_dict.%s." % task_id, 1
        else:
            wname, C = "cls.bi_seq_relationship.", 2
        self.score_out = self.buf("score_logits", (B, 64), torch.float32)
        self.score_classes = C
        self.gemm(f, L.NT, L.EPI_F32, [self.prob(pooled, self.W(wname + "weight"), self.score_out, B, C, P, P, P, 64, bias=self.Pm(wname + "bias"), n_store=64)])
