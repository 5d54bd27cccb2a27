"""LoRA dropout end to end on the engine (volta_amd/lora.py `dropout`), tiny configs and shape of tests/test_lora_gpu.py,
lora_B randomised as there.

1  Eval mode: a model with dropout = 0.1 gives the taps (bit for bit) and losses of the model with dropout = 0.
2  Train mode: the base model's taps in front of the first adapted projection keep the bits of the dropout = 0 run (the base sites did not
   move); the same seed twice gives the same taps and adapter gradients, bit for bit; another seed gives others.
3  Wiring, from what the step leaves in eng.bufs / eng.taps for the lowest attention sub-layer (its backward LoRA op is the last one, so
   its temporaries survive): the stored T against the restated T (tests/lora_drop_restate.py) from the sub-layer's input rows, lora_A's
   bf16 shadow and the keep mask of (the step's seed, the site the plan reports, p), within bound_bf16; lora_A.grad against the restated dA
   from the surviving dT and the same mask, within the fp32 bound; lora_B.grad as test 1 of tests/test_lora_gpu.py checks it.  A shared
   adapter (uniter: two sources, a site per stream) and separate streams (vilbert); with targets ffn_up / ffn_down the T of both adapters
   of one feed-forward sub-layer.
4  mark_only_lora_trainable with dropout: the adapter gradients keep the bits of the nothing-frozen run with the same seed."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lora_drop_restate as D  # noqa: E402
import lora_restate as LR  # noqa: E402
import test_lora_gpu as G0  # noqa: E402

SEED, P = G0.SEED, 0.1
bits16 = lambda t: t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
val16 = lambda t: LR.bf16_value(bits16(t))


def _model(name, targets, p=P):
    model, _, _, _, args = G0._pretrain(name, dict(r=8, alpha=16, targets=targets, dropout=p))
    G0._randomise_B(model)
    return model, args


def _run(model, args, train, seed, backward=True):
    model.train(train)
    model.set_dropout_seed(seed)
    G0._zero(model)
    losses = model(*args)
    if backward:
        sum(losses[:2]).sum().backward()                     # the MLM and region losses, as in tests/test_lora_gpu.py
    torch.cuda.synchronize()
    eng = model._last[0]
    taps = {k: t.clone() for k, t in eng.taps.items() if t is not None}
    return taps, G0._grads(model), eng, [float(x.detach()) for x in losses]


def _drop_problems(eng, plan, fns):
    """[(problem, its vk_dropout)] of the plan's LoRA dropout ops, in list order, and the index of the last such op"""
    from volta_amd import _lib as L
    kept = {ctypes.addressof(k): k for k in eng.keep if isinstance(k, ctypes.Array)}
    out, last = [], None
    for i, o in enumerate(plan.ops):
        if o[0] == L.OP_GENERIC and o[4].fn in fns:
            g = o[4]
            out += [(i, q, d) for q, d in zip(list(kept[g.p[0]])[:g.n[0]], list(kept[g.p[2]])[:g.n[0]])]
            last = i
    return out, last


def _buf_at(eng, ptr):
    return next(t for t in eng.bufs.values() if t.data_ptr() == ptr)


def _step_seed(eng):
    return int(eng.seed.cpu().item()) & 0xFFFFFFFFFFFFFFFF


# ---------------------------------------------------------------------------------------------- 1, 2
@pytest.mark.parametrize("name,targets", [("vilbert", ("query", "value")), ("uniter", ("query", "key", "value", "attn_out", "ffn_up", "ffn_down"))])
def test_eval_is_unmasked_and_train_replays_its_seed(name, targets):
    from volta_amd import _lib as L, lora
    model, args = _model(name, targets)
    arena = model.materialize()
    # ---- eval: nothing is masked
    taps_e, _, eng_e, loss_e = _run(model, args, False, SEED, backward=False)
    assert not _drop_problems(eng_e, eng_e.fwd, (L.FN_LORA_FWD_DROP, L.FN_LORA_PROJ_FWD_DROP))[0]
    taps_t, grads_t, eng_t, _ = _run(model, args, True, SEED)
    assert _drop_problems(eng_t, eng_t.fwd, (L.FN_LORA_FWD_DROP, L.FN_LORA_PROJ_FWD_DROP))[0]
    again_t, again_g, _, _ = _run(model, args, True, SEED)
    other_t, other_g, _, _ = _run(model, args, True, SEED + 1)
    lora.set_lora_dropout(model, 0.0)                         # the same model without the rate: new plans, the same arena
    assert model._arena is arena and lora.lora_dropout(model) == 0.0
    taps_e0, _, _, loss_e0 = _run(model, args, False, SEED, backward=False)
    taps_t0, grads_t0, eng_t0, _ = _run(model, args, True, SEED)
    assert not _drop_problems(eng_t0, eng_t0.fwd, (L.FN_LORA_FWD_DROP, L.FN_LORA_PROJ_FWD_DROP))[0]
    assert set(taps_e) == set(taps_e0) and len(taps_e) >= 8
    for k, t in taps_e0.items():
        assert torch.equal(t, taps_e[k]), ("eval", k)
    # the loss kernels sum their rows with float atomics: equality up to that reordering, as in tests/test_lora_gpu.py
    assert all((a != a and b != b) or abs(a - b) <= 144 * 2.0 ** -24 * abs(b) for a, b in zip(loss_e, loss_e0)), (loss_e, loss_e0)
    # ---- train: the base sites did not move -- what lies in front of the first adapted projection keeps its bits
    for k in ("emb_t", "emb_v"):
        assert torch.equal(taps_t[k], taps_t0[k]), k
    assert not torch.equal(taps_t["t0"], taps_t0["t0"])      # behind it the mask shows
    adapters = [k for k in grads_t if ".lora_" in k]
    assert adapters
    for k, t in taps_t.items():
        assert torch.equal(t, again_t[k]), ("same seed", k)
    for k in adapters:
        assert torch.equal(grads_t[k], again_g[k]), ("same seed", k)
        assert torch.isfinite(grads_t[k]).all() and float(grads_t[k].abs().max()) > 0.0, k
    assert not torch.equal(taps_t["t0"], other_t["t0"])
    assert any(not torch.equal(grads_t[k], other_g[k]) for k in adapters)


# ---------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("name", ["vilbert", "uniter"])
def test_wiring_of_the_lowest_attention_sublayer(name):
    from volta_amd import _lib as L
    targets = ("query", "key", "value") if name == "uniter" else ("query", "value")
    model, args = _model(name, targets)
    _, grads, eng, _ = _run(model, args, True, SEED)
    seed, c = _step_seed(eng), D.scale(P)
    fwd, _ = _drop_problems(eng, eng.fwd, (L.FN_LORA_FWD_DROP,))
    bwd, last = _drop_problems(eng, eng.bwd, (L.FN_LORA_BWD_DROP,))
    assert all(d.threshold == D.threshold(P) for _, _, d in fwd + bwd)
    x_in = {0: eng.taps["emb_t"], 1: eng.taps["emb_v"]}
    pre = model._arena_prefix
    checked = 0
    for col, t in enumerate(("query", "key", "value")):
        stems = {m: "bert.encoder.layer.0.attention_self.%s%s" % ("v_" if (m and name == "vilbert") else "", t) for m in (0, 1)}
        if stems[0] + ".lora_A" not in grads:
            continue
        src_A, src_B = {}, {}
        for m in (0, 1):
            if "L0_loraT%d%d" % (m, col) not in eng.bufs:      # vilbert: the lowest attention sub-layer is the text stream's alone
                assert name == "vilbert" and m == 1
                continue
            Tbuf = eng.bufs["L0_loraT%d%d" % (m, col)]
            site = next(d.site for _, q, d in fwd if q.T == Tbuf.data_ptr())
            # the sub-layer's backward op is the plan's last LoRA op: its dT is what the temporaries still hold
            q_b, d_b = next((q, d) for i, q, d in bwd if q.T == Tbuf.data_ptr())
            assert d_b.site == site and next(i for i, q, d in bwd if q.T == Tbuf.data_ptr()) == last
            X = val16(x_in[m]).reshape(-1, x_in[m].shape[-1])
            M, K = X.shape
            assert (q_b.M, q_b.K) == (M, K) and q_b.X == x_in[m].data_ptr()
            A = val16(eng.arena.view(pre + stems[m] + ".lora_A", "shadow"))
            keep = D.keep_mask(seed, site, M, K, P)
            assert 0.85 < keep.mean() < 0.95
            ref, e = D.ref_T(X, A, keep, c)
            assert LR.worst_bf16(bits16(Tbuf), ref, e) <= 1.0, (t, m)
            assert LR.worst_bf16(bits16(Tbuf), *LR.ref_T(X, A)) > 1.0, (t, m, "the unmasked T passes: the mask checks nothing")
            dT = val16(_buf_at(eng, q_b.dT))
            src_A.setdefault(stems[m], []).append((dT, X, keep, c))
            dqkv = val16(_buf_at(eng, q_b.dY - 2 * col * q_b.N))                # dY is column block `col` of the stream's 3N-wide dqkv
            assert dqkv.shape == (M, 3 * q_b.N) and q_b.ldy == 3 * q_b.N
            src_B.setdefault(stems[m], []).append((dqkv[:, col * q_b.N:(col + 1) * q_b.N], val16(Tbuf), 2.0))
        assert len(src_A) == 1 and len(src_A[stems[0]]) == (2 if name == "uniter" else 1)      # uniter: one adapter, the text rows then the vision rows
        for stem in src_A:
            ref, e = D.ref_dA(src_A[stem])
            assert LR.worst_f32(grads[stem + ".lora_A"].cpu().numpy(), ref, e) <= 1.0, stem
            ref, e = LR.ref_dB(src_B[stem])
            assert LR.worst_f32(grads[stem + ".lora_B"].cpu().numpy(), ref, e) <= 1.0, stem
            checked += 1
    assert checked == len(targets)


def test_wiring_of_a_feed_forward_sublayer():
    from volta_amd import _lib as L
    from volta_amd.modules import sublayer_schedule
    model, args = _model("vilbert", ("ffn_up", "ffn_down"))
    _, grads, eng, _ = _run(model, args, True, SEED)
    seed, c = _step_seed(eng), D.scale(P)
    fwd, _ = _drop_problems(eng, eng.fwd, (L.FN_LORA_PROJ_FWD_DROP,))
    bwd, _ = _drop_problems(eng, eng.bwd, (L.FN_LORA_PROJ_BWD_DROP,))
    by_T = {q.T: d.site for _, q, d in fwd}
    assert len(set(by_T.values())) == len(fwd) and all(by_T[q.T] == d.site for _, q, d in bwd) and len(bwd) == len(fwd)
    n = next(n for n, typ in sublayer_schedule(model.config) if typ == "ff" and ("L%d_loraTup0" % n) in eng.bufs and ("L%d_loraTup1" % n) in eng.bufs)
    pre = model._arena_prefix
    for m in (0, 1):
        v = "v_" if m else ""
        for which, holder, X in (("up", "intermediate.%sdense" % v, eng.taps["%s%d" % ("tv"[m], n - 1)]), ("dn", "output.%sdense" % v, eng.bufs["L%d_h%d" % (n, m)])):
            Tbuf = eng.bufs["L%d_loraT%s%d" % (n, which, m)]
            q, d = next((q, d) for _, q, d in fwd if q.T == Tbuf.data_ptr())
            Xv = val16(X).reshape(-1, X.shape[-1])
            assert q.X == X.data_ptr() and (q.M, q.K) == Xv.shape
            A = val16(eng.arena.view("%sbert.encoder.layer.%d.%s.lora_A" % (pre, n, holder), "shadow"))
            keep = D.keep_mask(seed, d.site, q.M, q.K, P)
            ref, e = D.ref_T(Xv, A, keep, c)
            assert LR.worst_bf16(bits16(Tbuf), ref, e) <= 1.0, (which, m)
            assert LR.worst_bf16(bits16(Tbuf), *LR.ref_T(Xv, A)) > 1.0, (which, m)
    assert all(torch.isfinite(g).all() and float(g.abs().max()) > 0 for k, g in grads.items() if ".lora_" in k)


# ---------------------------------------------------------------------------------------------- 4
def test_only_lora_trainable_keeps_the_bits_with_dropout():
    import test_frozen_backward_gpu as FB
    from volta_amd import _lib as L, lora
    model, loss_fn = FB._tasks("vilbert", "TASK1")
    lora.add_lora(model, r=8, alpha=16, dropout=P)
    G0._randomise_B(model)
    FB._step(model, loss_fn, 77)                             # nothing frozen
    assert _drop_problems(model._last[0], model._last[0].bwd, (L.FN_LORA_BWD_DROP,))[0]
    ref = G0._grads(model)
    keep = [n for n in ref if ref[n] is not None and ".lora_" in n]
    assert len(keep) == 24
    G0._zero(model)
    lora.mark_only_lora_trainable(model, also=("clfs_dict.",))
    G0._zero(model)
    FB._step(model, loss_fn, 77)
    got = G0._grads(model)
    eng = model._last[0]
    assert eng.pruned and eng.frozen and _drop_problems(eng, eng.bwd, (L.FN_LORA_BWD_DROP,))[0]
    for n in keep:
        assert torch.equal(got[n], ref[n]), n
