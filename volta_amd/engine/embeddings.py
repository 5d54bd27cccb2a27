"""The embedding builders: text tables, the image embeddings of ViLBERT / LXMERT / UNITER, and the mixed embeddings of VisualBERT and VL-BERT."""
import torch

from .. import _lib as L
from .plan import EV_DECODER_WGRAD, NODROP, _addr, _round_up, wait_side


class EmbeddingBuilders:
    """Base class of StepEngine.  Every builder appends its forward ops to `self.fwd.ops`, sets `self.x` and returns its backward ops."""

    def _emb_frozen(self, pre, streams):
        """Every parameter under the embedding prefix `pre` is frozen: the embedding takes no backward ("Frozen
        parameters"), and no trainable parameter lies upstream of the `streams` it starts.  An embedding with a trainable parameter runs
        its whole backward."""
        off = self.prune(*self.prefix_names(pre))
        for m in streams:
            self.live[m] = not off
        return off

    def embed_ws(self, eb, tag):
        """Workspace of one embedding backward (vk_embed_sum_bwd: the fixed-order partial sums of its table rows), set into its arguments."""
        n = L.lib.vk_embed_bwd_workspace_bytes(eb.M, eb.H, eb.V, eb.P, int(bool(eb.pos_ids) and bool(eb.dpos)))
        eb.work = _addr(self.tmp("embed_ws_" + tag, (max(n, 1),), torch.uint8))

    def _text_tables_fwd(self, pre, z, pos_ids=None, add=None):
        """z = word[input_ids] + position[pos_ids or 0..T) + type[token_type_ids] (+ the rows of `add`)."""
        cfg, st = self.cfg, self.st[0]
        ea = self.k(L.EmbedArgs(None, None, _addr(pos_ids), _addr(self.Pm(pre + "word_embeddings.weight")), _addr(self.Pm(pre + "position_embeddings.weight")),
                                _addr(self.Pm(pre + "token_type_embeddings.weight")), _addr(add), _addr(z), st.M, st.L, self.H,
                                cfg.vocab_size, cfg.max_position_embeddings, cfg.type_vocab_size))
        self.patch("input_ids", ea, "ids")
        self.patch("token_type_ids", ea, "type_ids")
        self.put(self.fwd.ops, L.OP_EMBED_FWD, ea)

    def _text_tables_bwd(self, b, pre, dz, tag, pos_ids=None):
        """dz scattered into the three tables' gradients; the caller zero-fills the position and type tables (the word table: EV_DECODER_WGRAD)."""
        cfg, st = self.cfg, self.st[0]
        eb = self.k(L.EmbedBwdArgs(_addr(dz), None, None, _addr(pos_ids), _addr(self.G(pre + "word_embeddings.weight")),
                                   _addr(self.G(pre + "position_embeddings.weight")), _addr(self.G(pre + "token_type_embeddings.weight")),
                                   st.M, st.L, self.H, cfg.type_vocab_size, cfg.vocab_size, cfg.max_position_embeddings))
        self.embed_ws(eb, tag)
        self.patch("input_ids", eb, "ids")
        self.patch("token_type_ids", eb, "type_ids")
        b.append(wait_side(EV_DECODER_WGRAD))
        self.put(b, L.OP_EMBED_BWD, eb)

    def _emb_text(self, pre):
        cfg, st, H = self.cfg, self.st[0], self.H
        z, y = self.buf("emb_t_z", (st.M, H)), self.buf("emb_t_y", (st.M, H))
        mean, rstd = self.buf("emb_t_mean", (st.M,), torch.float32), self.buf("emb_t_rstd", (st.M,), torch.float32)
        self._text_tables_fwd(pre, z)
        dr = self.drop(cfg.hidden_dropout_prob)
        self.ln_fwd(self.fwd.ops, z, None, pre + "LayerNorm.weight", pre + "LayerNorm.bias", y, None, mean, rstd, st.M, dr, post=1)
        self.x[0] = y
        if self.fwd_only or self._emb_frozen(pre, (0,)):
            return []
        b = []
        dz = self.tmp("dz0", (st.M, H))
        self.ln_bwd(b, self._dx(0, 0), z, mean, rstd, pre + "LayerNorm.weight", pre + "LayerNorm.bias", dz, None, st.M, dr, post=1)
        self.zero(self.bwd_pro, self.G(pre + "position_embeddings.weight"))
        self.zero(self.bwd_pro, self.G(pre + "token_type_embeddings.weight"))
        self._text_tables_bwd(b, pre, dz, "pre")
        return b

    def _img_proj(self, pre, wname, tag):
        """feat (fp32) -> bf16 -> [Mv, Hv] = feat W^T + b ; returns (proj, feat_bf16)."""
        cfg, st, H = self.cfg, self.st[1], self.st[1].H
        f = self.fwd.ops
        F_ = cfg.v_feature_size
        if F_ % 64:
            raise NotImplementedError("v_feature_size must be a multiple of 64")
        featb = self.buf(tag + "_feat_bf16", (st.M, F_))
        self.patch("image_feat", self.emit(f, L.FN_CAST, p=(None, featb), n=(st.M * F_,)), "p", 0)
        proj = self.buf(tag + "_proj", (st.M, H))
        self.gemm(f, L.NT, L.EPI_BF16, [self.prob(featb, self.W(pre + wname + ".weight"), proj, st.M, H, F_, F_, F_, H, bias=self.Pm(pre + wname + ".bias"))])
        return proj, featb

    def _loc_proj(self, pre, tag):
        cfg, st, H = self.cfg, self.st[1], self.st[1].H
        out = self.buf(tag + "_locproj", (st.M, H))
        g = self.emit(self.fwd.ops, L.FN_LOC_FWD, p=(None, self.Pm(pre + "image_location_embeddings.weight"), self.Pm(pre + "image_location_embeddings.bias"), out),
                      n=(st.M, H, cfg.num_locs))
        self.patch("image_loc", g, "p", 0)
        return out

    def _img_proj_bwd(self, b, pre, wname, dz, featb):
        st, H, F_ = self.st[1], self.st[1].H, self.cfg.v_feature_size
        # [H x F] output (24 tiles of 256 x 256) over B * Rv rows: row chunks as parts of one split accumulation fill the chip (146 -> 87 us, profiles/r03_ops_per_launch.txt)
        nparts = max(1, min(8, st.M // 1024))
        step = _round_up(-(-st.M // nparts), 64)
        tag = "side" if self._aside else "main"
        geo = self.split_geometry([F_])
        slices = [(_addr(dz[r0:]), _addr(featb[r0:]), min(step, st.M - r0), H, F_) for r0 in range(0, st.M, step)]
        probs = self.prob_parts(tag, geo, L.TN, slices, self.G(pre + wname + ".weight"), H, F_, F_, bias_grad=self.G(pre + wname + ".bias"))
        self.gemm(b, L.TN, L.EPI_F32, probs, geometry=geo if len(probs) > 1 else 0)
        self._split_cur[tag] = [0, 0]          # the launch is complete: the next one starts at the head of the stream's workspace

    def _loc_proj_bwd(self, b, pre, dz):
        st, H = self.st[1], self.st[1].H
        part = self.tmp("loc_partial", (L.lib.vk_rows32(st.M) * 9 * H,), torch.float32)
        g = self.emit(b, L.FN_LOC_BWD, p=(dz, None, part, self.G(pre + "image_location_embeddings.weight"), self.G(pre + "image_location_embeddings.bias")),
                      n=(st.M, H, self.cfg.num_locs))
        self.patch("image_loc", g, "p", 1)

    def _emb_image_vilbert(self, pre):
        cfg, st, H = self.cfg, self.st[1], self.st[1].H
        proj, featb = self._img_proj(pre, "image_embeddings", "emb_v")
        loc = self._loc_proj(pre, "emb_v")
        y = self.buf("emb_v_y", (st.M, H))
        mean, rstd = self.buf("emb_v_mean", (st.M,), torch.float32), self.buf("emb_v_rstd", (st.M,), torch.float32)
        dr = self.drop(cfg.v_hidden_dropout_prob)
        self.ln_fwd(self.fwd.ops, proj, loc, pre + "LayerNorm.weight", pre + "LayerNorm.bias", y, proj, mean, rstd, st.M, dr, post=1, H=H)
        self.x[1] = y
        if self.fwd_only or self._emb_frozen(pre, (1,)):
            return []
        b = []
        dz = self.tmp("dz1", (st.M, H))
        self.ln_bwd(b, self._dx(1, 0), proj, mean, rstd, pre + "LayerNorm.weight", pre + "LayerNorm.bias", dz, None, st.M, dr, post=1, H=H)
        self._img_proj_bwd(b, pre, "image_embeddings", dz, featb)
        self._loc_proj_bwd(b, pre, dz)
        return b

    def _img_loc_norms_fwd(self, pre, img_ln, loc_ln):
        """LayerNorm(image projection), LayerNorm(location projection): LXMERT averages the pair, UNITER adds it up under a third LayerNorm.
        -> (normalised image rows, normalised location rows, state for _img_loc_norms_bwd)."""
        st, H = self.st[1], self.H
        f = self.fwd.ops
        proj, featb = self._img_proj(pre, "image_embeddings", "emb_v")
        loc = self._loc_proj(pre, "emb_v")
        a_n, b_n = self.buf("emb_v_imgn", (st.M, H)), self.buf("emb_v_locn", (st.M, H))
        st_a = [self.buf("emb_v_%s" % s, (st.M,), torch.float32) for s in ("mean_a", "rstd_a", "mean_b", "rstd_b")]
        self.ln_fwd(f, proj, None, pre + img_ln + ".weight", pre + img_ln + ".bias", a_n, None, st_a[0], st_a[1], st.M, NODROP)
        self.ln_fwd(f, loc, None, pre + loc_ln + ".weight", pre + loc_ln + ".bias", b_n, None, st_a[2], st_a[3], st.M, NODROP)
        return a_n, b_n, (img_ln, loc_ln, proj, loc, featb, st_a)

    def _img_loc_norms_bwd(self, b, pre, g, state):
        """`g` = the gradient at both LayerNorms' outputs."""
        img_ln, loc_ln, proj, loc, featb, st_a = state
        st, H = self.st[1], self.H
        dza, dzb = self.tmp("dd1", (st.M, H)), self.tmp("dctx1", (st.M, H))
        self.ln_bwd(b, g, proj, st_a[0], st_a[1], pre + img_ln + ".weight", pre + img_ln + ".bias", dza, None, st.M, NODROP)
        self.ln_bwd(b, g, loc, st_a[2], st_a[3], pre + loc_ln + ".weight", pre + loc_ln + ".bias", dzb, None, st.M, NODROP)
        self._img_proj_bwd(b, pre, "image_embeddings", dza, featb)
        self._loc_proj_bwd(b, pre, dzb)

    def _emb_image_lxmert(self, pre):
        cfg, st, H = self.cfg, self.st[1], self.H
        a_n, b_n, norms = self._img_loc_norms_fwd(pre, "ImgLayerNorm", "LocLayerNorm")
        y = self.buf("emb_v_y", (st.M, H))
        dr = self.drop(cfg.v_hidden_dropout_prob)
        self.emit(self.fwd.ops, L.FN_ADD_DROPOUT, p=(a_n, b_n, y), n=(st.M, H, 0), f=(0.5,), drop=dr)
        self.x[1] = y
        if self.fwd_only or self._emb_frozen(pre, (1,)):
            return []
        b = []
        g = self.tmp("dz1", (st.M, H))
        self.emit(b, L.FN_ADD_DROPOUT, p=(self._dx(1, 0), None, g), n=(st.M, H, 1), f=(0.5,), drop=dr)
        self._img_loc_norms_bwd(b, pre, g, norms)
        return b

    def _emb_image_uniter(self, pre):
        cfg, st, H = self.cfg, self.st[1], self.H
        a_n, b_n, norms = self._img_loc_norms_fwd(pre, "image_layer_norm", "image_location_layer_norm")
        mean, rstd = self.buf("emb_v_mean", (st.M,), torch.float32), self.buf("emb_v_rstd", (st.M,), torch.float32)
        y, z = self.buf("emb_v_y", (st.M, H)), self.buf("emb_v_z", (st.M, H))
        dr = self.drop(cfg.hidden_dropout_prob)
        type1 = self.Pm(pre + "token_type_embeddings.weight")[1]
        self.ln_fwd(self.fwd.ops, a_n, b_n, pre + "v_LayerNorm.weight", pre + "v_LayerNorm.bias", y, z, mean, rstd, st.M, dr, post=1, addvec=type1)
        self.x[1] = y
        if self.fwd_only or self._emb_frozen(pre, (1,)):          # one prefix with the text tables: frozen together or not at all
            return []
        b = []
        dz = self.tmp("dz1", (st.M, H))
        self.ln_bwd(b, self._dx(1, 0), z, mean, rstd, pre + "v_LayerNorm.weight", pre + "v_LayerNorm.bias", dz, None, st.M, dr, post=1)
        # the broadcast token-type row 1 receives the column sum of dz (the text side zeroed / filled its table first)
        part = self.tmp("colsum_partial", (L.lib.vk_rows32(st.M) * H,), torch.float32)
        self.emit(b, L.FN_COLSUM, p=(dz, part, self.G(pre + "token_type_embeddings.weight")[1]), n=(st.M, H, 1))
        self._img_loc_norms_bwd(b, pre, dz, norms)
        return b

    def _concat_ln_fwd(self, pre, xt, xv, stats, zv=None, addvec=None):
        """ONE LayerNorm over the per-sample concatenation [text | vision]: two row kernels sharing gamma / beta; the single dropout site sees rows
        b * (T + Rv) + t and b * (T + Rv) + T + r.  stats = [text mean, text rstd, vision mean, vision rstd].  Sets self.x; -> state for _concat_ln_bwd."""
        st_t, st_v = self.st
        T, Rv = st_t.L, st_v.L
        f = self.fwd.ops
        yt, yv = self.buf("emb_t_y", (st_t.M, self.H)), self.buf("emb_v_y", (st_v.M, self.H))
        dr = self.drop(self.cfg.hidden_dropout_prob)
        seg_t = [(dr.site, T, T + Rv, 0), (dr.site, 0, 0, 0)]
        seg_v = [(dr.site, Rv, T + Rv, T), (dr.site, 0, 0, 0)]
        gn, bn = pre + "LayerNorm.weight", pre + "LayerNorm.bias"
        self.ln_fwd(f, xt, None, gn, bn, yt, None, stats[0], stats[1], st_t.M, dr, post=1, segs=seg_t)
        self.ln_fwd(f, xv, None, gn, bn, yv, zv, stats[2], stats[3], st_v.M, dr, post=1, addvec=addvec, segs=seg_v)
        self.x = [yt, yv]
        return gn, bn, dr, seg_t, seg_v, stats

    def _concat_ln_bwd(self, b, state, zt, zv):
        """zt, zv: the LayerNorm's inputs as the forward left them.  -> (dzt, dzv)."""
        gn, bn, dr, seg_t, seg_v, stats = state
        st_t, st_v = self.st
        dzt, dzv = self.tmp("dz0", (st_t.M, self.H)), self.tmp("dz1", (st_v.M, self.H))
        self.ln_bwd(b, self._dx(0, 0), zt, stats[0], stats[1], gn, bn, dzt, None, st_t.M, dr, post=1, segs=seg_t)
        self.ln_bwd(b, self._dx(1, 0), zv, stats[2], stats[3], gn, bn, dzv, None, st_v.M, dr, post=1, segs=seg_v, accumulate=1)
        return dzt, dzv

    def _emb_visualbert(self, pre):
        """embeddings.py:389-392: text tables | projected features + (visual position 0 + visual type 1), under one LayerNorm."""
        H = self.H
        st_t, st_v = self.st
        f = self.fwd.ops
        zt = self.buf("emb_t_z", (st_t.M, H))
        self._text_tables_fwd(pre, zt)
        proj, featb = self._img_proj(pre, "projection", "emb_v")
        # addvec = position_embeddings_visual[0] + token_type_embeddings_visual[1], rebuilt every step by one list op: the two rows are
        # two "slabs" of the fp32 master arena, a fixed distance apart
        vec = self.buf("emb_v_addvec", (H,), torch.float32)
        rows = sorted((self.Pm(pre + "position_embeddings_visual.weight")[0], self.Pm(pre + "token_type_embeddings_visual.weight")[1]), key=lambda r: r.data_ptr())
        gap = rows[1].data_ptr() - rows[0].data_ptr()
        if gap % 16:
            raise NotImplementedError("hidden size must be a multiple of 4")
        self.emit(f, L.FN_SUM_SLABS, p=(vec, rows[0]), n=(gap // 4, 2, H))
        zv = self.buf("emb_v_z", (st_v.M, H))
        stats = [self.buf("emb_%s" % s, (m,), torch.float32) for s, m in (("t_mean", st_t.M), ("t_rstd", st_t.M), ("v_mean", st_v.M), ("v_rstd", st_v.M))]
        ln = self._concat_ln_fwd(pre, zt, proj, stats, zv=zv, addvec=vec)
        if self.fwd_only or self._emb_frozen(pre, (0, 1)):
            return []
        b = []
        dzt, dzv = self._concat_ln_bwd(b, ln, zt, zv)
        for nm in ("position_embeddings.weight", "token_type_embeddings.weight", "position_embeddings_visual.weight", "token_type_embeddings_visual.weight"):
            self.zero(self.bwd_pro, self.G(pre + nm))
        part = self.tmp("colsum_partial", (L.lib.vk_rows32(st_v.M) * H,), torch.float32)
        self.emit(b, L.FN_COLSUM, p=(dzv, part, self.G(pre + "position_embeddings_visual.weight")[0]), n=(st_v.M, H, 0))
        self.emit(b, L.FN_COLSUM, p=(dzv, part, self.G(pre + "token_type_embeddings_visual.weight")[1]), n=(st_v.M, H, 0))
        self._img_proj_bwd(b, pre, "projection", dzv, featb)
        self._text_tables_bwd(b, pre, dzt, "vl")
        return b

    def _emb_vlbert(self, pre):
        """VL-BERT embeddings (volta/embeddings.py:240-301): box geometry sin/cos + appearance -> dropout -> Linear(2F -> H)
        -> ReLU = final; vision token = LN_obj(final) + (object / END) embedding + position + type 2; text token =
        word + LN_text(final of the LAST region of the sample) + position + type; ONE LayerNorm over [text | vision].
        Position ids follow the reference, including its expanded-view quirk (see prepare_step)."""
        cfg, H, B = self.cfg, self.H, self.B
        st_t, st_v = self.st
        T, K = st_t.L, st_v.L
        F_, dim = cfg.v_feature_size, cfg.v_coordinate_embeddings_dim
        W = 8 * dim + F_
        if W != 2 * F_ or W % 64 or cfg.v_hidden_size != cfg.hidden_size:
            raise NotImplementedError("VL-BERT embedding geometry outside the reference configs (8*dim must equal v_feature_size)")
        mvrc = cfg.visual_target_weights.get("6", 0) > 0      # masked regions get a word of their own (embeddings.py:191,262-263)
        nword = 3 if mvrc else 2
        f, dev = self.fwd.ops, self.dev
        i64 = dict(dtype=torch.int64, device=dev)
        # ---- static index tensors and per-step position ids (filled in prepare_step)
        is_last = torch.zeros(B, K, **i64)
        is_last[:, -1] = 1
        self.bufs["vl_is_last"] = is_last = is_last.view(-1).contiguous()
        self.bufs["vl_twos"] = twos = torch.full((st_v.M,), 2, **i64)
        self.bufs["vl_tpos"] = tpos = torch.zeros(st_t.M, **i64)
        self.bufs["vl_opos"] = opos = torch.zeros(st_v.M, **i64)
        self.bufs["vl_last_rows"] = last_rows = (torch.arange(B, device=dev, dtype=torch.int32) * K + (K - 1)).contiguous()
        self.bufs["vl_row2b"] = row2b = (torch.arange(st_t.M, device=dev, dtype=torch.int32) // T).contiguous()
        self.bufs["vl_cntB"] = cntB = torch.tensor([B], device=dev, dtype=torch.int32)
        self.bufs["vl_cntMt"] = cntMt = torch.tensor([st_t.M], device=dev, dtype=torch.int32)
        vtab = self.buf("vl_vtab", (nword, H), torch.float32)       # rows: object word, END word (last region), masked-region word
        dvtab = self.buf("vl_dvtab", (nword, H), torch.float32)
        # ---- forward: position ids from this step's input_ids, and the (object | END | masked) word table from the parameters
        self.patch("input_ids", self.emit(f, L.FN_VLBERT_POSITIONS, p=(None, tpos, opos), n=(B, T, K)), "p", 0)
        for r, nm in enumerate(("object_linguistic_embeddings", "end_embedding", "object_mask_word_embedding")[:nword]):
            self.emit(f, L.FN_COPY, p=(vtab[r], self.Pm(pre + nm + ".weight")[0]), n=(H * 4,))
        x4 = self.buf("vl_x4096", (st_v.M, W))
        zflag = self.buf("vl_zero_flag", (st_v.M,), torch.int32)
        dr0 = self.drop(cfg.v_attention_probs_dropout_prob)
        g = self.emit(f, L.FN_VLBERT_PREP, p=(None, None, self.Pm(pre + "object_mask_visual_embedding.weight"), x4, zflag), n=(st_v.M, F_, dim, cfg.num_locs), drop=dr0)
        self.patch("image_loc", g, "p", 0)
        self.patch("image_feat", g, "p", 1)
        word_ids = is_last
        if mvrc:
            word_ids = self.buf("vl_word_ids", (st_v.M,), torch.int64)
            self.emit(f, L.FN_VLBERT_OBJ_IDS, p=(zflag, word_ids), n=(st_v.M, K))
        final = self.buf("vl_final", (st_v.M, H))
        wds = pre + "obj_downsample.1"
        self.gemm(f, L.NT, L.EPI_RELU, [self.prob(x4, self.W(wds + ".weight"), final, st_v.M, H, W, W, W, H, bias=self.Pm(wds + ".bias"))])
        obj_vis = self.buf("vl_obj_vis", (st_v.M, H))
        so = [self.buf("vl_%s" % n_, (m,), torch.float32) for n_, m in (("mean_o", st_v.M), ("rstd_o", st_v.M), ("mean_x", B), ("rstd_x", B),
                                                                       ("mean_t", st_t.M), ("rstd_t", st_t.M), ("mean_v", st_v.M), ("rstd_v", st_v.M))]
        self.ln_fwd(f, final, None, pre + "visual_ln_object.weight", pre + "visual_ln_object.bias", obj_vis, None, so[0], so[1], st_v.M, NODROP)
        vz = self.buf("emb_v_z", (st_v.M, H))
        ptab, ttab = pre + "position_embeddings.weight", pre + "token_type_embeddings.weight"
        ev = self.k(L.EmbedArgs(_addr(word_ids), _addr(twos), _addr(opos), _addr(vtab), _addr(self.Pm(ptab)), _addr(self.Pm(ttab)), _addr(obj_vis), _addr(vz),
                                st_v.M, K, H, nword, cfg.max_position_embeddings, cfg.type_vocab_size))
        self.put(f, L.OP_EMBED_FWD, ev)
        flast = self.buf("vl_final_last", (B, H))
        self.emit(f, L.FN_GATHER, p=(final, last_rows, cntB, flast), n=(H, B))
        tv = self.buf("vl_tv", (B, H))
        self.ln_fwd(f, flast, None, pre + "visual_ln_text.weight", pre + "visual_ln_text.bias", tv, None, so[2], so[3], B, NODROP)
        tvx = self.buf("vl_tv_exp", (st_t.M, H))
        self.emit(f, L.FN_GATHER, p=(tv, row2b, cntMt, tvx), n=(H, st_t.M))
        tz = self.buf("emb_t_z", (st_t.M, H))
        self._text_tables_fwd(pre, tz, pos_ids=tpos, add=tvx)
        ln = self._concat_ln_fwd(pre, tz, vz, so[4:])
        if self.fwd_only or self._emb_frozen(pre, (0, 1)):
            return []
        # ---- backward
        b = []
        dzt, dzv = self._concat_ln_bwd(b, ln, tz, vz)
        self.zero(self.bwd_pro, self.G(ptab))
        self.zero(self.bwd_pro, self.G(ttab))
        # text tokens: word / position / type tables, and the per-sample visual vector
        self._text_tables_bwd(b, pre, dzt, "txt", pos_ids=tpos)
        dtv = self.buf("vl_dtv", (B, H))
        self.emit(b, L.FN_ROWGROUP_SUM, p=(dzt, dtv), n=(B, T, H))
        dflast = self.buf("vl_dfinal_last", (B, H))
        self.ln_bwd(b, dtv, flast, so[2], so[3], pre + "visual_ln_text.weight", pre + "visual_ln_text.bias", dflast, None, B, NODROP)
        # vision tokens: (object | END) embedding, position, type 2, then LN_obj
        self.zero(b, dvtab)
        evb = self.k(L.EmbedBwdArgs(_addr(dzv), _addr(word_ids), _addr(twos), _addr(opos), _addr(dvtab), _addr(self.G(ptab)), _addr(self.G(ttab)),
                                    st_v.M, K, H, cfg.type_vocab_size, nword, cfg.max_position_embeddings))
        self.embed_ws(evb, "vis")
        self.put(b, L.OP_EMBED_BWD, evb)
        self.emit(b, L.FN_COPY, p=(self.G(pre + "object_linguistic_embeddings.weight"), dvtab[0]), n=(H * 4,))
        self.emit(b, L.FN_COPY, p=(self.G(pre + "end_embedding.weight"), dvtab[1]), n=(H * 4,))
        if mvrc:
            self.emit(b, L.FN_COPY, p=(self.G(pre + "object_mask_word_embedding.weight"), dvtab[2]), n=(H * 4,))
        dfinal = self.tmp("dd1", (st_v.M, H))
        self.ln_bwd(b, dzv, final, so[0], so[1], pre + "visual_ln_object.weight", pre + "visual_ln_object.bias", dfinal, None, st_v.M, NODROP)
        self.emit(b, L.FN_SCATTER_ADD, p=(dflast, last_rows, cntB, dfinal), n=(H, B))
        dpre = self.tmp("dctx1", (st_v.M, H))
        self.emit(b, L.FN_RELU_BWD, p=(dfinal, final, dpre), n=(st_v.M * H,))
        self.gemm(b, L.TN, L.EPI_F32, [self.prob(dpre, x4, self.G(wds + ".weight"), H, W, st_v.M, H, W, W, bias_grad=self.G(wds + ".bias"))])
        dx4 = self.buf("vl_dx4096", (st_v.M, W))
        self.gemm(b, L.NN, L.EPI_BF16, [self.prob(dpre, self.W(wds + ".weight"), dx4, st_v.M, W, H, H, W, W)])
        part = self.tmp("vl_mask_partial", (L.lib.vk_rows32(st_v.M) * F_,), torch.float32)
        self.emit(b, L.FN_VLBERT_MASKGRAD, p=(dx4, zflag, part, self.G(pre + "object_mask_visual_embedding.weight")), n=(st_v.M, F_, W, 8 * dim), drop=dr0)
        return b
