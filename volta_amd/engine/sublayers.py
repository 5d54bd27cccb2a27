"""The encoder's builders: attention and feed-forward sub-layers, their shared residual-LayerNorm tail, and the weight-gradient block."""
import ctypes as C
import math

import torch

from .. import _lib as L
from .plan import EV_WGRAD_RING, NODROP, _addr, _round_up, side_begin, side_end


class SublayerBuilders:
    """Base class of StepEngine.  A builder appends its forward ops to `self.fwd.ops`, advances `self.x` / `self.x8` and returns its backward ops."""

    def _names(self, n, typ):
        """Parameter names per modality for sub-layer n (shared sub-layers: the text names for both)."""
        cfg = self.cfg
        p = "bert.encoder.layer.%d." % n
        shared = n in cfg.shared_sublayers
        out = []
        for m in range(2):
            v = "v_" if (m == 1 and not shared) else ""
            if typ == "attn":
                out.append(dict(q=p + "attention_self.%squery" % v, k=p + "attention_self.%skey" % v, v=p + "attention_self.%svalue" % v,
                                o=p + "attention_output.%sdense" % v, ln=p + "attention_output.%sLayerNorm" % v))
            else:
                out.append(dict(up=p + "intermediate.%sdense" % v, down=p + "output.%sdense" % v, ln=p + "output.%sLayerNorm" % v))
        return out, shared

    def _attn_sublayer(self, n):
        cfg, B = self.cfg, self.B
        f = self.fwd.ops
        gate = [[int(n in cfg.tt_attn_sublayers), int(n in cfg.tv_attn_sublayers)], [int(n in cfg.vt_attn_sublayers), int(n in cfg.vv_attn_sublayers)]]
        if self.only is not None:          # a score prefix: this stream's self-attention only (before the split no block crosses the streams)
            gate = [[g if i == j == self.only else 0 for j, g in enumerate(row)] for i, row in enumerate(gate)]
        act = [bool(gate[0][0] or gate[0][1]), bool(gate[1][0] or gate[1][1])]
        names, shared = self._names(n, "attn")
        ms = [m for m in range(2) if act[m]]
        tag = "L%d_" % n
        x_in = list(self.x)
        x8_in = list(self.x8)
        # widths: Hm = the stream's hidden size, Ha = the sub-layer's attention width for that stream, nhm heads of dh (encoders.py:164-206)
        Hm = [self.st[0].H, self.st[1].H]
        Ha = [cfg.sublayer2attn_hidden_size.get(str(n), cfg.hidden_size), cfg.sublayer2v_attn_hidden_size.get(str(n), cfg.v_hidden_size)]
        nhm = [cfg.sublayer2num_attention_heads.get(str(n), cfg.num_attention_heads), cfg.sublayer2v_num_attention_heads.get(str(n), cfg.v_num_attention_heads)]
        dh = [Ha[m] // nhm[m] for m in range(2)]
        for m in ms:
            if Ha[m] % nhm[m] or dh[m] not in (32, 64, 96, 128) or Ha[m] % 64:
                raise NotImplementedError("attention width %d with %d heads (head sizes 32, 64, 96, 128; widths multiples of 64)" % (Ha[m], nhm[m]))
        cross = gate[0][1] or gate[1][0]
        if shared and len(ms) == 2 and (Hm[0] != Hm[1] or Ha[0] != Ha[1]):
            raise ValueError("a shared attention sub-layer needs equal widths in both streams")
        if cross and (dh[0] != dh[1] or nhm[0] != nhm[1]):
            raise ValueError("cross-modal attention needs the same head count and size in both streams (sub-layer %d: %d x %d vs %d x %d)"
                             % (n, nhm[0], dh[0], nhm[1], dh[1]))
        qkv = {m: self.buf(tag + "qkv%d" % m, (self.st[m].M, 3 * Ha[m])) for m in ms}
        ctx = {m: self.buf(tag + "ctx%d" % m, (self.st[m].M, Ha[m])) for m in ms}
        lse = {m: self.buf(tag + "lse%d" % m, (B * nhm[m] * self.st[m].L,), torch.float32) for m in ms}
        d = {m: self.buf(tag + "z%d" % m, (self.st[m].M, Hm[m])) for m in ms}

        qkv_names = lambda m, part: [names[m][c] + part for c in "qkv"]                 # adjacent in the arena: one [3 Ha, Hm] block
        wqkv = lambda m, which: self.arena.span(qkv_names(m, ".weight"), which, (3 * Ha[m], Hm[m]))
        bqkv = lambda m, which: self.arena.span(qkv_names(m, ".bias"), which, (3 * Ha[m],))
        # LoRA adapters (volta_amd/lora.py): [(stream, column block 0 q | 1 k | 2 v, holder name)]; a shared sub-layer lists its one adapter per stream
        lora = [(m, c, names[m]["qkv"[c]]) for m in ms for c in range(3) if names[m]["qkv"[c]] + ".lora_A" in self.arena.params]
        # the output projection's adapter (target "attn_out"): [(stream, holder name)], one whole-projection LoRA problem per stream
        lora_o = [(m, names[m]["o"]) for m in ms if names[m]["o"] + ".lora_A" in self.arena.params]
        if (lora or lora_o) and self.fp8:
            raise NotImplementedError("attention sub-layer %d has LoRA adapters: the fp8 (e4m3) projection path does not run them; "
                                      "merge_lora() first or use the bf16 projections" % n)
        if self.fp8:
            self.gemm_fp8(f, L.EPI_BF16, [(x8_in[m] or x_in[m], wqkv(m, "master"), qkv[m], bqkv(m, "master"), None) for m in ms])
        else:
            self.gemm(f, L.NT, L.EPI_BF16, [self.prob(x_in[m], wqkv(m, "shadow"), qkv[m], self.st[m].M, 3 * Ha[m], Hm[m], Hm[m], Hm[m], 3 * Ha[m], bias=bqkv(m, "master")) for m in ms])
        # LoRA dropout: a site per problem (adapter x stream), handed out stream by stream, within a stream q, k, v, o; empty without a rate
        have = {(m, c) for m, c, _ in lora} | {(m, "o") for m, _ in lora_o}
        ld = self.lora_drops([(m, c) for m in ms for c in (0, 1, 2, "o") if (m, c) in have])
        lora_T = self._lora_fwd(f, tag, lora, x_in, qkv, Hm, Ha, ld) if lora else {}
        # dropout sites in the reference's call order: tt, tv, then vv, vt (encoders.py:294-295, 309-310)
        pdrop = (cfg.attention_probs_dropout_prob, cfg.v_attention_probs_dropout_prob)
        drops = {(i, j): self.drop(pdrop[i]) for i, j in ((0, 0), (0, 1), (1, 1), (1, 0)) if gate[i][j]}
        # one launch covers every gate block when the active streams share head count and size (every ctrl_* config, and the co-attention
        # sub-layers of vilbert_base); two self-attentions with different heads (vilbert_base: 12 x 64 text, 8 x 128 vision) are two launches
        if len(ms) == 2 and not cross and (nhm[0], dh[0]) != (nhm[1], dh[1]):
            launches = [[[gate[0][0], 0], [0, 0]], [[0, 0], [0, gate[1][1]]]]
        else:
            launches = [gate]
        attn = []
        for gl in launches:
            mq = [m for m in range(2) if gl[m][0] or gl[m][1] or gl[0][m] or gl[1][m]]
            aa = L.AttnArgs()
            for m in mq:
                base = qkv[m].data_ptr()
                aa.q[m], aa.k[m], aa.v[m] = base, base + 2 * Ha[m], base + 4 * Ha[m]
                aa.ld[m], aa.L[m] = 3 * Ha[m], self.st[m].L
                aa.mask[m] = self.masks[m].data_ptr()
                aa.ctx[m], aa.ldo[m], aa.lse[m] = ctx[m].data_ptr(), Ha[m], lse[m].data_ptr()
            m0 = mq[0]
            aa.B, aa.nh, aa.scale, aa.dh = B, nhm[m0], 1.0 / math.sqrt(float(dh[m0])), dh[m0]
            for i in range(2):
                for j in range(2):
                    aa.gate[i][j] = gl[i][j]
                    aa.drop[i][j] = drops.get((i, j), NODROP) if gl[i][j] else NODROP
            if self.attn_maps:
                pb = {}
                for i in range(2):
                    for j in range(2):
                        if gl[i][j]:
                            pb[(i, j)] = self.buf(tag + "probs%d%d" % (i, j), (B, nhm[m0], self.st[i].L, self.st[j].L), torch.float32)
                            aa.probs[i][j] = pb[(i, j)].data_ptr()
                self.attn_map_info.append(dict(n=n, probs=pb, qkv={m: qkv[m] for m in mq}, Ha={m: Ha[m] for m in mq}, nh=nhm[m0], dh=dh[m0]))
            self.k(aa)
            # rows the generic kernels cannot hold in LDS fail HERE, when the plan is built, not at the first backward launch (their backward
            # keeps two row images of both modalities: ~491 keys at head size 64, ~258 at 128, less than the forward's 512)
            for bwd_pass in (0, 1):
                need = L.lib.vk_gated_attn_lds_bytes(C.byref(aa), bwd_pass)
                if need > 160 * 1024:
                    raise NotImplementedError("attention sub-layer %d: %d + %d rows at head size %d need %d bytes of LDS in the %s pass (160 KiB per workgroup)"
                                              % (n, self.st[0].L, self.st[1].L, dh[m0], need, "backward" if bwd_pass else "forward"))
            self.put(f, L.OP_ATTN_FWD, aa)
            attn.append((aa, mq, gl))
        self.gemm(f, L.NT, L.EPI_BF16, [self.prob(ctx[m], self.W(names[m]["o"] + ".weight"), d[m], self.st[m].M, Hm[m], Ha[m], Ha[m], Ha[m], Hm[m], bias=self.Pm(names[m]["o"] + ".bias")) for m in ms])
        if lora_o:       # behind the output projection, in front of the tail: d += s (ctx A^T) B^T
            To = self._lora_proj_fwd(f, tag, "o", [(m, stem, ctx[m], d[m], None) for m, stem in lora_o], {m: ld[(m, "o")] for m, _ in lora_o if ld})
        tail = self._tail_fwd(tag, ms, names, d, x_in, Hm)
        if self.fwd_only:
            return []
        # ------------- backward
        # Frozen parameters: the attention launch serves both streams, so the sub-layer's backward runs for all of its
        # streams or for none -- none when no stream has a trainable parameter in the sub-layer or upstream of its input.  Per stream, the
        # input gradient (the last dgrad and the LayerNorm's dz) is computed only where a trainable parameter lies upstream of that input.
        live_in = list(self.live)
        qkv_all = lambda m: qkv_names(m, ".weight") + qkv_names(m, ".bias")
        ln_of = lambda m: (names[m]["ln"] + ".weight", names[m]["ln"] + ".bias")
        o_of = lambda m: (names[m]["o"] + ".weight", names[m]["o"] + ".bias")
        lora_of = lambda m: [stem + leaf for mm, _, stem in lora if mm == m for leaf in (".lora_A", ".lora_B")]      # each adapter is a block of its own
        lora_on = lambda m: any(not self.fz(stem + ".lora_A", stem + ".lora_B") for mm, _, stem in lora if mm == m)
        lora_o_of = lambda m: [stem + leaf for mm, stem in lora_o if mm == m for leaf in (".lora_A", ".lora_B")]
        lora_o_on = lambda m: any(not self.fz(stem + ".lora_A", stem + ".lora_B") for mm, stem in lora_o if mm == m)      # a trainable parameter of the sub-layer; dqkv is not its business
        if not any(live_in[m] or lora_on(m) or lora_o_on(m) or not self.fz(*qkv_all(m), *o_of(m), *ln_of(m)) for m in ms):
            for m in ms:
                self._dx_step(m)               # the ping-pong parity of dX counts every sub-layer
                self.prune(*qkv_all(m), *o_of(m), *ln_of(m), *lora_of(m), *lora_o_of(m))
            return []
        for m in ms:
            self.live[m] = True
        b = []
        need_dqkv = any(live_in[m] or lora_on(m) or not self.fz(*qkv_all(m)) for m in ms)      # else nothing reads past dd: o's weight gradient and the LayerNorm's are all
        dz, dd, dxn = self._tail_bwd(b, tail, shared, need_dz=live_in)
        dctx, dqkv, par = {}, {}, self.sub_k % 2
        for m in ms:
            wtag = "" if Ha[m] == Hm[m] == self.H else "_%d" % Ha[m]      # temporaries are shared by name: other widths get their own
            dctx[m] = self.tmp("dctx%d%s" % (m, wtag), (self.st[m].M, Ha[m]))
            dqkv[m] = self.tmp("dqkv%d_%d%s" % (m, par, wtag), (self.st[m].M, 3 * Ha[m]))
        if need_dqkv:
            self.gemm(b, L.NN, L.EPI_BF16, [self.prob(dd[m], self.W(names[m]["o"] + ".weight"), dctx[m], self.st[m].M, Ha[m], Hm[m], Hm[m], Ha[m], Ha[m]) for m in ms])
        if lora_o:       # directly behind the dd W_o dgrad: the attention backward reads the dctx this op adds to; without dqkv only dA and dB
            self._lora_proj_bwd(b, [(m, stem, ctx[m], To[m], dd[m], dctx[m] if need_dqkv else None, None) for m, stem in lora_o],
                                {m: ld[(m, "o")] for m, _ in lora_o if ld})
        if need_dqkv:
            for m in ms:
                if not (gate[0][m] or gate[1][m]):       # K/V of this modality unused: their gradient is zero
                    self.zero(b, dqkv[m])
            for aa, mq, gl in attn:
                ab = L.AttnBwdArgs()
                for m in mq:
                    ab.dctx[m] = dctx[m].data_ptr()
                    base = dqkv[m].data_ptr()
                    ab.dq[m], ab.dk[m], ab.dv[m], ab.ldg[m] = base, base + 2 * Ha[m], base + 4 * Ha[m], 3 * Ha[m]
                self.k(ab)
                self.put(b, L.OP_ATTN_BWD, aa, ab)
        # all weight gradients of the sub-layer in ONE grouped launch (more workgroups per CU), listed in front of the Q|K|V
        # dgrad: they need dqkv, not its product, and start beside that GEMM instead of beside the next sub-layer's LayerNorm backward
        self._wgrad(b, ms, shared, [lambda m: (dd[m], ctx[m], self.G(names[m]["o"] + ".weight"), self.G(names[m]["o"] + ".bias"), Hm[m], Ha[m], Hm[m], Ha[m]),
                                    lambda m: (dqkv[m], x_in[m], wqkv(m, "grad"), bqkv(m, "grad"), 3 * Ha[m], Hm[m], 3 * Ha[m], Hm[m])],
                    [o_of, qkv_all])
        self.gemm_kept(b, L.NN, L.EPI_ADDR, [self.prob(dqkv[m], wqkv(m, "shadow"), dxn[m], self.st[m].M, Hm[m], 3 * Ha[m], 3 * Ha[m], Hm[m], Hm[m], R=dz[m], ldr=Hm[m]) for m in ms],
                       [live_in[m] for m in ms])
        if lora:         # behind the last dgrad: dqkv, x_in and T are still live, dxn[m] holds the base projection's input gradient
            self._lora_bwd(b, lora, lora_T, x_in, dqkv, dxn, live_in, Hm, Ha, ld)
        return b

    def _lora_fwd(self, f, tag, lora, x_in, qkv, Hm, Ha, drops):
        """One LoRA forward op behind the Q|K|V launch: qkv columns += s (x A^T) B^T for every adapter of the active streams.  -> T per adapter
        (kept for the backward; one shared buffer per shape in a forward-only plan).  drops: {(stream, column block): the problem's LoRA
        dropout}, or empty -- then the op is the one a model without LoRA dropout builds."""
        s = self.arena.lora_scale
        assert s is not None, "the arena holds LoRA adapters but no scale: build it from a model that add_lora() prepared"
        probs, T = [], {}
        for m, c, stem in lora:
            A, Bw = self.W(stem + ".lora_A"), self.W(stem + ".lora_B")
            r, M = A.shape[0], self.st[m].M
            assert tuple(A.shape) == (r, Hm[m]) and tuple(Bw.shape) == (Ha[m], r), (stem, tuple(A.shape), tuple(Bw.shape))
            T[(m, c)] = self.tmp("loraT%d%d_%d_%d" % (m, c, M, r), (M, r)) if self.fwd_only else self.buf(tag + "loraT%d%d" % (m, c), (M, r))
            probs.append(L.LoraProblem(_addr(x_in[m]), _addr(A), _addr(Bw), _addr(T[(m, c)]), qkv[m].data_ptr() + 2 * c * Ha[m], None,
                                       M, Hm[m], Ha[m], r, Hm[m], 3 * Ha[m], s, 0))
        assert len(probs) <= L.LORA_MAX_PROBLEMS
        arr = self.k((L.LoraProblem * len(probs))(*probs))
        if drops:
            self.emit(f, L.FN_LORA_FWD_DROP, p=(arr, None, self.k((L.Dropout * len(probs))(*[drops[(m, c)] for m, c, _ in lora]))), n=(len(probs),))
        else:
            self.emit(f, L.FN_LORA_FWD, p=(arr,), n=(len(probs),))
        return T

    def _lora_bwd(self, b, lora, T, x_in, dqkv, dxn, live_in, Hm, Ha, drops):
        """One LoRA backward op: dA, dB of every trainable adapter (a frozen one is pruned, its range reads zero) and, where the input
        gradient is live, every adapter's share of dxn -- a frozen adapter's too: the gradient passes through it.  An adapter shared by both
        streams takes the text rows first, then the vision rows (`accumulate`), like a shared weight in _wgrad.  drops: what _lora_fwd took --
        each problem replays the mask of its forward problem."""
        s = self.arena.lora_scale
        probs, written, dr = [], set(), []
        for m, c, stem in lora:
            off = self.prune(stem + ".lora_A", stem + ".lora_B")
            if off and not live_in[m]:
                continue
            A, Bw = self.W(stem + ".lora_A"), self.W(stem + ".lora_B")
            r, M = A.shape[0], self.st[m].M
            dT = self.tmp("loradT%d%d_%d_%d" % (m, c, M, r), (M, r))
            gA, gB = (None, None) if off else (self.G(stem + ".lora_A"), self.G(stem + ".lora_B"))
            probs.append(L.LoraBwdProblem(_addr(x_in[m]), _addr(A), _addr(Bw), _addr(T[(m, c)]), dqkv[m].data_ptr() + 2 * c * Ha[m], _addr(dT),
                                          _addr(dxn[m]) if live_in[m] else None, _addr(gA), _addr(gB), None,
                                          M, Hm[m], Ha[m], r, Hm[m], 3 * Ha[m], Hm[m], int(stem in written), s, 0))
            if drops:
                dr.append(drops[(m, c)])
            if not off:
                written.add(stem)
        if not probs:
            return
        arr = self.k((L.LoraBwdProblem * len(probs))(*probs))
        nbytes = L.lib.vk_lora_bwd_work_bytes(arr, len(probs))
        assert nbytes > 0, "vk_lora_bwd_work_bytes refused the problems"
        work = self.tmp("lora_work_%d" % nbytes, (nbytes,), torch.uint8)
        if drops:
            self.emit(b, L.FN_LORA_BWD_DROP, p=(arr, work, self.k((L.Dropout * len(dr))(*dr))), n=(len(probs),))
        else:
            self.emit(b, L.FN_LORA_BWD, p=(arr, work), n=(len(probs),))

    def _lora_proj_fwd(self, f, tag, which, items, drops):
        """One whole-projection LoRA forward op (vk_lora_proj_fwd).  items: [(stream, holder name, X [M, K], Y [M, N], G or None)]; G None:
        Y += s (X A^T) B^T; G: Y = gelu(Y + ...), G = gelu'(Y + ...).  -> T per stream (kept for the backward; one shared buffer per
        shape in a forward-only plan).  drops: {stream: the problem's LoRA dropout}, or empty: the op without a mask."""
        s = self.arena.lora_scale
        assert s is not None, "the arena holds LoRA adapters but no scale: build it from a model that add_lora() prepared"
        probs, T = [], {}
        for m, stem, X, Y, G in items:
            A, Bw = self.W(stem + ".lora_A"), self.W(stem + ".lora_B")
            r, M, K, N = A.shape[0], self.st[m].M, X.shape[1], Y.shape[1]
            assert tuple(A.shape) == (r, K) and tuple(Bw.shape) == (N, r) and X.shape[0] == Y.shape[0] == M, (stem, tuple(A.shape), tuple(Bw.shape))
            T[m] = self.tmp("loraT%s%d_%d_%d" % (which, m, M, r), (M, r)) if self.fwd_only else self.buf(tag + "loraT%s%d" % (which, m), (M, r))
            probs.append(L.LoraProjProblem(_addr(X), _addr(A), _addr(Bw), _addr(T[m]), _addr(Y), _addr(G), None, M, K, N, r, X.stride(0), Y.stride(0),
                                           G.stride(0) if G is not None else 0, s, int(G is not None)))
        arr = self.k((L.LoraProjProblem * len(probs))(*probs))
        if drops:
            self.emit(f, L.FN_LORA_PROJ_FWD_DROP, p=(arr, None, self.k((L.Dropout * len(probs))(*[drops[it[0]] for it in items]))), n=(len(probs),))
        else:
            self.emit(f, L.FN_LORA_PROJ_FWD, p=(arr,), n=(len(probs),))
        return T

    def _lora_proj_bwd(self, b, items, drops):
        """One whole-projection LoRA backward op (vk_lora_proj_bwd).  items: [(stream, holder name, X, T, dY, dX or None, R or None)]: dA, dB
        of every trainable adapter (a frozen one is pruned, its range reads zero) and, where dX is given, the adapter's share of the input
        gradient, times R -- a frozen adapter's too: the gradient passes through it.  An adapter shared by both streams takes the text rows
        first, then the vision rows (`accumulate`).  drops: what _lora_proj_fwd took for these adapters."""
        s = self.arena.lora_scale
        probs, written, dr = [], set(), []
        for m, stem, X, T, dY, dX, R in items:
            off = self.prune(stem + ".lora_A", stem + ".lora_B")
            if off and dX is None:
                continue
            A, Bw = self.W(stem + ".lora_A"), self.W(stem + ".lora_B")
            r, M, K, N = A.shape[0], self.st[m].M, X.shape[1], dY.shape[1]
            dT = self.tmp("loradTp%d_%d_%d" % (m, M, r), (M, r))
            gA, gB = (None, None) if off else (self.G(stem + ".lora_A"), self.G(stem + ".lora_B"))
            probs.append(L.LoraProjBwdProblem(_addr(X), _addr(A), _addr(Bw), _addr(T), _addr(dY), _addr(dT), _addr(dX), _addr(gA), _addr(gB), _addr(R), None,
                                              M, K, N, r, X.stride(0), dY.stride(0), dX.stride(0) if dX is not None else 0,
                                              R.stride(0) if R is not None else 0, int(stem in written), s))
            if drops:
                dr.append(drops[m])
            if not off:
                written.add(stem)
        if not probs:
            return
        arr = self.k((L.LoraProjBwdProblem * len(probs))(*probs))
        nbytes = L.lib.vk_lora_proj_bwd_work_bytes(arr, len(probs))
        assert nbytes > 0, "vk_lora_proj_bwd_work_bytes refused the problems"
        work = self.tmp("lora_work_%d" % nbytes, (nbytes,), torch.uint8)
        if drops:
            self.emit(b, L.FN_LORA_PROJ_BWD_DROP, p=(arr, work, self.k((L.Dropout * len(dr))(*dr))), n=(len(probs),))
        else:
            self.emit(b, L.FN_LORA_PROJ_BWD, p=(arr, work), n=(len(probs),))

    def _tail_fwd(self, tag, ms, names, d, x_in, Hm):
        """The tail both kinds of sub-layer end in: y = LayerNorm(dropout(d) + x_in) per active stream, d = the output projection's result (the
        LayerNorm leaves its pre-normalisation input there for the backward).  -> state for _tail_bwd."""
        lnf, state = [], {}
        for m in ms:
            M, ln = self.st[m].M, names[m]["ln"]
            y, mean, rstd = self.buf(tag + "y%d" % m, (M, Hm[m])), self.buf(tag + "mean%d" % m, (M,), torch.float32), self.buf(tag + "rstd%d" % m, (M,), torch.float32)
            drop = self.drop(self.cfg.hidden_dropout_prob if m == 0 else self.cfg.v_hidden_dropout_prob)
            self.x8[m] = self.fp8_hidden(m) if self.fp8 else None
            lnf.append(self.ln_args(d[m], x_in[m], ln + ".weight", ln + ".bias", y, d[m], mean, rstd, M, drop, fp8_out=self.x8[m], H=Hm[m]))
            self.x[m], state[m] = y, (ln, d[m], mean, rstd, drop, Hm[m])
        self._ln_pair(self.fwd.ops, L.OP_LN_FWD, lnf)          # both streams in one launch when their widths agree
        return state

    def _tail_bwd(self, b, state, shared, need_dz=(True, True), skip=()):
        """-> (dz, dd, dxn) per stream: gradients at the residual input and at d, and the buffer the last dgrad writes; dgamma / dbeta: _wgrad.
        need_dz[m] False: nothing reads stream m's input gradient (frozen parameters), the kernel does not store dz.  Streams in `skip`
        take no backward here at all."""
        dz, dd, dxn, lnb, par = {}, {}, {}, [], self.sub_k % 2
        for i, (m, (ln, d, mean, rstd, drop, Hm)) in enumerate(state.items()):
            M = self.st[m].M
            dxi, dxn[m] = self._dx_step(m)
            if m in skip:
                continue
            dz[m] = self.tmp("dz%d_%d" % (m, par), (M, Hm))
            dd[m] = self.tmp("dd%d_%d" % (m, par), (M, Hm)) if self.train else dz[m]
            lnb.append(self.ln_bwd_args(dxi, d, mean, rstd, ln + ".weight", ln + ".bias", dz[m] if (need_dz[m] or not self.train) else None,
                                        dd[m] if self.train else None, M, drop, accumulate=1 if (shared and i > 0) else 0, defer=True, H=Hm))
        self._ln_pair(b, L.OP_LN_BWD, lnb)
        return dz, dd, dxn

    def _ln_pair(self, ops, kind, jobs):
        """One LayerNorm launch for both streams when their widths agree (the kernels share the launch between two jobs of equal width),
        one launch per stream otherwise."""
        if len(jobs) == 2 and jobs[0].H == jobs[1].H:
            self.put(ops, kind, jobs[0], jobs[1])
        else:
            for j in jobs:
                self.put(ops, kind, j)

    def _ffn_sublayer(self, n):
        cfg = self.cfg
        f = self.fwd.ops
        # per-stream widths: hidden Hm, intermediate Im (config/vilbert_base.json: 768 / 3072 text, 1024 / 1024 vision; encoders.py:459-460,514-515)
        Hm = [self.st[0].H, self.st[1].H]
        Im = [cfg.sublayer2intermediate_size.get(str(n), cfg.intermediate_size), cfg.sublayer2v_intermediate_size.get(str(n), cfg.v_intermediate_size)]
        for m in range(2):
            if Im[m] % 64:
                raise NotImplementedError("intermediate sizes must be multiples of 64")
        act = [n in cfg.t_ff_sublayers and self.only in (None, 0), n in cfg.v_ff_sublayers and self.only in (None, 1)]
        names, shared = self._names(n, "ff")
        ms = [m for m in range(2) if act[m]]
        tag = "L%d_" % n
        x_in = list(self.x)
        x8_in = list(self.x8)
        if shared and len(ms) == 2 and (Hm[0] != Hm[1] or Im[0] != Im[1]):
            raise ValueError("a shared feed-forward sub-layer needs equal widths in both streams")
        h = {m: self.buf(tag + "h%d" % m, (self.st[m].M, Im[m])) for m in ms}
        gp = {m: self.buf(tag + "gp%d" % m, (self.st[m].M, Im[m])) for m in ms}
        d = {m: self.buf(tag + "z%d" % m, (self.st[m].M, Hm[m])) for m in ms}
        # adapters on the two projections (targets "ffn_up", "ffn_down"): {stream: holder name}
        lora_up = {m: names[m]["up"] for m in ms if names[m]["up"] + ".lora_A" in self.arena.params}
        lora_dn = {m: names[m]["down"] for m in ms if names[m]["down"] + ".lora_A" in self.arena.params}
        if (lora_up or lora_dn) and self.fp8:
            raise NotImplementedError("feed-forward sub-layer %d has LoRA adapters: the fp8 (e4m3) projection path does not run them; "
                                      "merge_lora() first or use the bf16 projections" % n)
        # LoRA dropout: a site per problem, handed out stream by stream, within a stream up, then down; empty without a rate
        ld = self.lora_drops([(m, which) for m in ms for which, have in (("up", lora_up), ("dn", lora_dn)) if m in have])
        ld_of = lambda which, have: {m: ld[(m, which)] for m in have if ld}
        if self.fp8:
            # the GELU output also leaves the epilogue as e4m3 with one static scale (the FFN-down projection's A operand), de-quantised
            # there through scale_a = 1 / multiplier
            up, specs = [], []
            for m in ms:
                Mm = self.st[m].M
                h8 = self.tmp("fp8_h%d_%d" % (m, Mm), (Mm, Im[m]), torch.uint8)
                if "fp8_hscale_%d" % Mm not in self.bufs:
                    self.bufs["fp8_hscale_%d" % Mm] = torch.full((Mm,), 1.0 / self.H8_MUL, dtype=torch.float32, device=self.dev)
                up.append((x8_in[m] or x_in[m], self.Pm(names[m]["up"] + ".weight"), h[m], self.Pm(names[m]["up"] + ".bias"), gp[m], (h8, self.H8_MUL)))
                specs.append(((h8, self.bufs["fp8_hscale_%d" % Mm]), self.Pm(names[m]["down"] + ".weight"), d[m], self.Pm(names[m]["down"] + ".bias"), None))
            self.gemm_fp8(f, L.EPI_GELU, up)
            self.gemm_fp8(f, L.EPI_BF16, specs)
        else:
            up = [self.prob(x_in[m], self.W(names[m]["up"] + ".weight"), h[m], self.st[m].M, Im[m], Hm[m], Hm[m], Hm[m], Im[m], bias=self.Pm(names[m]["up"] + ".bias"), C2=gp[m]) for m in ms]
            down = [self.prob(h[m], self.W(names[m]["down"] + ".weight"), d[m], self.st[m].M, Hm[m], Im[m], Im[m], Im[m], Hm[m], bias=self.Pm(names[m]["down"] + ".bias")) for m in ms]
            if not lora_up:
                self.gemm(f, L.NT, L.EPI_GELU, up)
            else:
                # A stream with an FFN-up adapter: its term belongs inside the GELU, and the GELU epilogue never stores the pre-activation.
                # That stream's product leaves a plain launch as bf16(u) in h[m]; the adapter's op adds its term and applies the GELU there,
                # writing h[m] and gp[m].  A stream without one keeps the GELU epilogue, in a launch of its own.
                rest = [q for m, q in zip(ms, up) if m not in lora_up]
                if rest:
                    self.gemm(f, L.NT, L.EPI_GELU, rest)
                self.gemm(f, L.NT, L.EPI_BF16, [self.prob(x_in[m], self.W(names[m]["up"] + ".weight"), h[m], self.st[m].M, Im[m], Hm[m], Hm[m], Hm[m], Im[m],
                                                          bias=self.Pm(names[m]["up"] + ".bias")) for m in ms if m in lora_up])
                Tup = self._lora_proj_fwd(f, tag, "up", [(m, lora_up[m], x_in[m], h[m], gp[m]) for m in ms if m in lora_up], ld_of("up", lora_up))
            self.gemm(f, L.NT, L.EPI_BF16, down)
            if lora_dn:
                Tdn = self._lora_proj_fwd(f, tag, "dn", [(m, lora_dn[m], h[m], d[m], None) for m in ms if m in lora_dn], ld_of("dn", lora_dn))
        tail = self._tail_fwd(tag, ms, names, d, x_in, Hm)
        if self.fwd_only:
            return []
        # Frozen parameters: a feed-forward sub-layer's streams do not meet, so each one takes its backward only if it
        # has a trainable parameter here or upstream of its input, its first dgrad only if something reads du, its last one only if
        # something reads the input gradient.
        live_in = list(self.live)
        of = lambda m, *keys: [names[m][k] + s for k in keys for s in (".weight", ".bias")]
        leaves = lambda stem: (stem + ".lora_A", stem + ".lora_B")
        ad_on = lambda which, m: m in which and not self.fz(*leaves(which[m]))
        ad_of = lambda m: [x for which in (lora_up, lora_dn) if m in which for x in leaves(which[m])]
        # a stream stays in the backward while one of its adapters is trainable
        dead = [m for m in ms if not live_in[m] and not ad_on(lora_up, m) and not ad_on(lora_dn, m) and self.prune(*of(m, "up", "down", "ln"), *ad_of(m))]
        for m in ms:
            self.live[m] = m not in dead
        b = []
        dz, dd, dxn = self._tail_bwd(b, tail, shared, need_dz=live_in, skip=dead)
        ma = [m for m in ms if m not in dead]
        if not ma:
            return b
        du, par = {}, self.sub_k % 2
        for m in ma:
            wtag = "" if Im[m] == self.I else "_%d" % Im[m]               # temporaries are shared by name: other widths get their own
            du[m] = self.tmp("du%d_%d%s" % (m, par, wtag), (self.st[m].M, Im[m]))
        d1 = [self.prob(dd.get(m), self.W(names[m]["down"] + ".weight"), du.get(m), self.st[m].M, Im[m], Hm[m], Hm[m], Im[m], Im[m], R=gp[m], ldr=Im[m]) for m in ms]
        d2 = [self.prob(du.get(m), self.W(names[m]["up"] + ".weight"), dxn[m], self.st[m].M, Hm[m], Im[m], Im[m], Hm[m], Hm[m], R=dz.get(m), ldr=Hm[m]) for m in ms]
        keep_d1 = {m: m in ma and (live_in[m] or not self.fz(*of(m, "up")) or ad_on(lora_up, m)) for m in ms}
        self.gemm_kept(b, L.NN, L.EPI_MULR, d1, [keep_d1[m] for m in ms])
        if lora_dn:      # directly behind d1, in front of the weight-gradient side block and d2: both read the du this op adds to, through gelu'
            self._lora_proj_bwd(b, [(m, lora_dn[m], h[m], Tdn[m], dd[m], du[m] if keep_d1[m] else None, gp[m]) for m in ma if m in lora_dn], ld_of("dn", lora_dn))
        # The weight gradients need dd, h, du and x_in: everything but the LAST dgrad's output.  Their side-stream block is listed in front of that
        # dgrad, so that it starts beside a GEMM (two MFMA-bound launches share the chip without loss) instead of beside the LayerNorm backward
        # that follows, which it used to keep waiting for CUs (profiles/r03_experiments.md: 17.00 / 16.94 -> 16.52 / 16.54 ms per step).
        self._wgrad(b, ms, shared, [lambda m: (dd.get(m), h[m], self.G(names[m]["down"] + ".weight"), self.G(names[m]["down"] + ".bias"), Hm[m], Im[m], Hm[m], Im[m]),
                                    lambda m: (du.get(m), x_in[m], self.G(names[m]["up"] + ".weight"), self.G(names[m]["up"] + ".bias"), Im[m], Hm[m], Im[m], Hm[m])],
                    [lambda m: of(m, "down"), lambda m: of(m, "up")], dead=dead)
        self.gemm_kept(b, L.NN, L.EPI_ADDR, d2, [m in ma and live_in[m] for m in ms])
        if lora_up:      # behind the last dgrad: du is the gradient at the pre-activation, dxn[m] holds the base projection's input gradient
            for m in ma:
                if m in lora_up and not keep_d1[m]:      # no du: the adapter is frozen and nothing upstream is trainable
                    assert self.prune(*leaves(lora_up[m]))
            self._lora_proj_bwd(b, [(m, lora_up[m], x_in[m], Tup[m], du[m], dxn[m] if live_in[m] else None, None) for m in ma if m in lora_up and keep_d1[m]],
                                ld_of("up", lora_up))
        return b

    def _wgrad(self, b, ms, shared, specs, blocks=None, dead=()):
        """dW[Mo, No] = dY^T X (+ bias grad) for every spec and modality in ONE grouped TN launch.  The outputs are
        small (<= 3072 x 768) and the contraction (B*L rows) long, so every problem is split along K into chunks of
        ~5120 rows: each chunk is an ordinary problem writing its own fp32 slab (weights | bias), and one reduction
        pass sums the slabs into the gradient arena (plain stores: float atomics would cost 4x the slab traffic).
        This turns 36-144 long tiles into >= 256 balanced ones that take the 256x256 geometry.  Weights shared by
        both modalities simply sum the slabs of both.
        blocks[i](m): the parameter names spec i writes for modality m.  A problem whose block is frozen leaves the launch, with its slabs
        and reductions (streams in `dead` have only such problems); the K-chunking and the tile geometry stay those of the whole group, so
        that a trainable weight's summation order, and so its bits, do not depend on what else is frozen."""
        jobs = []            # (dst weight grad, dst bias grad, Mo, No, [(dY, X, rows, lda, ldb), ...], block frozen)
        for i, spec in enumerate(specs):
            per_w = {}
            for m in ms:
                dY, X, gW, gB, Mo, No, lda, ldb = spec(m)
                key = gW.data_ptr()
                off = blocks is not None and self.prune(*blocks[i](m))
                assert off or m not in dead
                per_w.setdefault(key, (gW, gB, Mo, No, [], off))[4].append((dY, X, self.st[m].M, lda, ldb))
            jobs += list(per_w.values())
        # K-chunk length: ~5120 rows, halved (down to ~1280) while the whole group still yields fewer than 130 tiles of 256 x 256 (half the
        # CUs) -- the attention sub-layers' group ([768, 768] and [2304, 768] outputs) is 108 tiles of 150 K-steps at 5120, i.e. 42 % of the
        # CUs busy for 127 us; more, shorter chunks fill the chip, but every halving doubles the slab traffic: past half the chip it costs more
        # than the idle CUs (a threshold of 200 cut the text-only groups into 288 tiles of 40 K-steps: +0.08 ms per step)
        chunk_rows = 5120.0
        tiles = lambda cr: sum(-(-Mo // 256) * -(-No // 256) * sum(max(1, int(round(rows / cr))) for _, _, rows, _, _ in srcs) for _, _, Mo, No, srcs, _ in jobs)
        while chunk_rows > 1280 and tiles(chunk_rows) < 130:     # (round 3 sweep, profiles/r03_experiments.md: 130 = half the CUs; 200 cut the text-only groups once more, +0.08 ms)
            chunk_rows /= 2
        probs, keep, reduces = [], [], []
        for gW, gB, Mo, No, srcs, off in jobs:
            chunks = []
            for dY, X, rows, lda, ldb in srcs:
                ns = max(1, int(round(rows / chunk_rows)))
                step = -(-rows // ns)
                step = -(-step // 64) * 64
                r0 = 0
                while r0 < rows:
                    chunks.append((None if off else dY[r0:], None if off else X[r0:], min(step, rows - r0), lda, ldb))
                    r0 += step
            keep += [not off] * len(chunks)
            if off:                  # listed for the group's geometry only
                probs += [self.prob(None, None, None, Mo, No, rows, lda, ldb, No) for _, _, rows, lda, ldb in chunks]
                continue
            if len(chunks) == 1:
                dY, X, rows, lda, ldb = chunks[0]
                probs.append(self.prob(dY, X, gW, Mo, No, rows, lda, ldb, No, bias_grad=gB))
                continue
            stride = _round_up(Mo * No + Mo, 4)
            slab = self._slab(len(chunks) * stride)
            for i, (dY, X, rows, lda, ldb) in enumerate(chunks):
                base = slab[i * stride:]
                probs.append(self.prob(dY, X, base, Mo, No, rows, lda, ldb, No, bias_grad=base[Mo * No:]))
            reduces.append((gW, slab, stride, len(chunks), Mo * No))
            reduces.append((gB, slab[Mo * No:], stride, len(chunks), Mo))
        assert len(probs) <= 32, "too many wgrad problems in one group"
        if not any(keep) and not self._deferred_ln:      # every block of the sub-layer is frozen: no side block, and no event for anyone to wait for
            self._slab_cursor = 0
            return
        self.wgrad_recorded.add(self.sub_k)
        b.append(side_begin())
        self.gemm_kept(b, L.TN, L.EPI_F32, probs, keep)
        # every slab sum and every deferred LayerNorm dgamma / dbeta reduction of the sub-layer in ONE launch (vk_side_tail)
        jobs = [L.TailJob(_addr(dst), None, _addr(src), None, stride, n, 0, ns, 0, 0) for dst, src, stride, ns, n in reduces]
        by_dst = {}
        for a in self._deferred_ln:          # LayerNorm parameter gradients of this sub-layer; a LayerNorm shared by both
            by_dst.setdefault(a.dgamma, []).append(a)         # modalities has two sets of partial records: ONE job sums both (no ordering between jobs)
        for group in by_dst.values():
            assert len(group) <= 2 and not (group[0].accumulate & 1) and all(g.accumulate & 1 for g in group[1:]), "unexpected LayerNorm sharing"
            a, b2 = group[0], (group[1] if len(group) > 1 else None)
            jobs.append(L.TailJob(a.dgamma, a.dbeta, a.partial, b2.partial if b2 else None, L.lib.vk_ln_bwd_partial_rows(b2.M) if b2 else 0, a.H, 1,
                                  L.lib.vk_ln_bwd_partial_rows(a.M), 0, 0))
        self._deferred_ln = []
        for i in range(0, len(jobs), L.TAIL_MAX_JOBS):
            chunk = jobs[i:i + L.TAIL_MAX_JOBS]
            arr = self.k((L.TailJob * len(chunk))(*chunk))
            self.emit(b, L.FN_SIDE_TAIL, p=(arr,), n=(len(chunk),))
        b.append(side_end(self.sub_k % EV_WGRAD_RING))
        self._slab_cursor = 0
