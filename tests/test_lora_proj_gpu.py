"""LoRA adapters on the attention-output and feed-forward projections end to end on the engine (targets attn_out, ffn_up, ffn_down of
volta_amd/lora.py), with the tiny configs, shape and helpers of tests/test_lora_gpu.py.

1  lora_B = 0 on attn_out + ffn_down changes nothing, to the bit; lora_A.grad is exactly zero, lora_B.grad finite and non-zero.
2  lora_B = 0 on ffn_up: lora_A.grad exactly zero; states and gradients within the gates of item 3 of the plain model's (not bitwise: the
   adapter path rounds the pre-activation u to bf16 before the GELU).
3  Random lora_B (ratio 0.3), the three new targets and all six: the engine against the oracle fed the merged fp32 weights, autograd through
   the merge giving the adapter gradients.  Gates of tests/test_engine_gpu.py as used in tests/test_lora_gpu.py: states 2e-2, gradients
   4e-2 / cosine 0.999 (query and key 0.1 / 0.995).  The new adapters meet the gate as it stands (measured: worst error 0.031, lowest
   cosine 0.99957 on vilbert with all six targets; 0.016 / 0.99988 on uniter), so the base-weight yardstick is not used.
4  mark_only_lora_trainable(also=head): adapter and head gradients keep the bits of the nothing-frozen run; the backward list is shorter.
5  AdamW over the trainable parameters only.   6  merge_lora on the GPU.   7  RetrievalScorer on a model with the new adapters."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_lora_gpu as TL  # noqa: E402  (_pretrain, _randomise_B, _grads, _zero)

SEED, SHAPE = TL.SEED, TL.SHAPE
NEW = ("attn_out", "ffn_up", "ffn_down")
ALL = ("query", "key", "value") + NEW


def _run(m, args, train):
    m.train(train)
    m.set_dropout_seed(SEED)
    TL._zero(m)
    losses = m(*args)
    sum(losses[:2]).sum().backward()                 # the MLM and region losses: their gradients do not read the atomically summed loss values
    torch.cuda.synchronize()
    eng = m._last[0]
    return {k: t.clone() for k, t in eng.taps.items() if t is not None}, TL._grads(m), eng, [float(x.detach()) for x in losses]


def _check_adapter_grads(grads):
    adapters = [k for k in grads if ".lora_" in k]
    assert adapters and all(grads[k] is not None for k in adapters)
    for k in adapters:
        g = grads[k]
        assert torch.isfinite(g).all(), k
        if k.endswith("lora_A"):
            assert float(g.abs().max()) == 0.0, k
        else:
            assert float(g.abs().max()) > 0.0, k
    return adapters


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", ["vilbert", "uniter"])
def test_zero_lora_B_on_attn_out_and_ffn_down_changes_nothing(name):
    from volta_amd import _lib as L
    plain, _, _, _, args = TL._pretrain(name)
    model, _, _, _, _ = TL._pretrain(name, dict(r=8, alpha=16, targets=("attn_out", "ffn_down")))
    for train in (False, True):
        taps_p, grads_p, _, loss_p = _run(plain, args, train)
        taps_l, grads_l, eng, loss_l = _run(model, args, train)
        assert sum(1 for o in eng.fwd.ops if o[0] == L.OP_GENERIC and o[4].fn == L.FN_LORA_PROJ_FWD) == len(eng.sublayer_ids)      # one per sub-layer
        # the loss kernels sum their rows with float atomics: "equal" is equality up to that reordering (tests/test_lora_gpu.py)
        assert all((a != a and b != b) or abs(a - b) <= 144 * 2.0 ** -24 * abs(b) for a, b in zip(loss_l, loss_p)), (train, loss_l, loss_p)
        for k, t in taps_p.items():
            assert torch.equal(t, taps_l[k]), (train, k)
        for k, g in grads_p.items():
            assert (g is None and grads_l[k] is None) or torch.equal(g, grads_l[k]), (train, k)
        _check_adapter_grads(grads_l)


# ---------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("name", ["vilbert", "uniter"])
def test_zero_lora_B_on_ffn_up_stays_within_the_gates(name):
    from test_engine_gpu import rel_err
    plain, _, _, _, args = TL._pretrain(name)
    model, _, _, _, _ = TL._pretrain(name, dict(r=8, alpha=16, targets=("ffn_up",)))
    taps_p, grads_p, _, loss_p = _run(plain, args, True)
    taps_l, grads_l, eng, loss_l = _run(model, args, True)
    _check_adapter_grads(grads_l)
    worst = [0.0, 0.0, 1.0]
    for k, t in taps_p.items():
        if t.dim() >= 2 and t.is_floating_point():
            e = rel_err(taps_l[k].float(), t.float())
            worst[0] = max(worst[0], e)
            assert e < 2e-2, (k, e)
    for a, b in zip(loss_l[:2], loss_p[:2]):
        assert abs(a - b) <= 1e-3 * max(abs(b), 1e-3) + 1e-4, (loss_l, loss_p)
    n = 0
    for k, g in grads_p.items():
        if g is None or float(g.norm()) < 1e-6:
            continue
        gl = grads_l[k].float()
        if k.endswith("key.bias"):          # zero in exact arithmetic (the softmax ignores a shift along the keys): both hold rounding noise,
            assert float(gl.norm()) <= 5e-3 and float(g.norm()) <= 5e-3, k          # gated as test_engine_gpu gates an expected-zero gradient
            continue
        e, cos = rel_err(gl, g.float()), float((gl * g).sum() / (gl.norm() * g.norm()))
        worst[1], worst[2] = max(worst[1], e), min(worst[2], cos)
        qk = "query." in k or "key." in k
        assert e <= (0.1 if qk else 4e-2) and cos >= (0.995 if qk else 0.999), (k, e, cos)
        n += 1
    print("ffn_up, B = 0 against the plain model: worst state %.3g, worst gradient %.3g, lowest cosine %.6f" % tuple(worst))
    assert n > 20


# ---------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("name,targets", [("vilbert", NEW), ("uniter", NEW), ("vilbert", ALL), ("uniter", ALL)])
def test_engine_against_oracle_with_merged_weights(name, targets):
    from oracle import volta_ref as R
    from test_engine_gpu import rel_err
    from volta_amd import lora
    model, rcfg, sd, batch, args = TL._pretrain(name, dict(r=8, alpha=16, targets=targets))
    ratios = TL._randomise_B(model, ratio=0.3)
    assert ratios and all(0.1 <= v <= 0.5 for v in ratios.values()), ratios
    s = lora.lora_scale(model)
    model.train()
    model.set_dropout_seed(SEED)
    lm, img, nsp = model(*args)
    torch.cuda.synchronize()
    eng = model._last[0]
    aliases = R.param_aliases(rcfg)
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k not in aliases}
    ad = {n: p.detach().cpu().clone().requires_grad_(True) for n, p in model.named_parameters() if ".lora_" in n}
    full = dict(leaves)
    for n in ad:
        if n.endswith(".lora_A"):
            stem = n[:-len(".lora_A")]
            full[stem + ".weight"] = leaves[stem + ".weight"] + s * (ad[stem + ".lora_B"] @ ad[n])
    for a, t in aliases.items():
        full[a] = full[t]
    taps = {}
    olm, oimg, onsp = R.forward_from_batch(full, rcfg, batch, train=True, philox_seed=SEED, taps=taps)
    seen = 0
    for key, ref in taps.items():
        if key not in eng.taps or ref is None or ref.dim() < 2:
            continue
        e = rel_err(eng.taps[key].float().cpu().view(ref.shape), ref.detach())
        assert e < 2e-2, (name, key, e)
        seen += 1
    assert seen >= 8
    for got, ref, nm in ((lm, olm, "lm"), (img, oimg, "img")):
        g, r = float(got.detach()), float(ref.detach())
        assert abs(g - r) <= 1e-3 * max(abs(r), 1e-3) + 1e-4, (name, nm, g, r)
    (lm + img).sum().backward()
    (olm + oimg).sum().backward()
    torch.cuda.synchronize()
    named = dict(model.named_parameters())
    bad, n_ad, worst_ad = [], 0, (0.0, 1.0)
    for k, leaf in list(leaves.items()) + list(ad.items()):
        g_ref = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
        assert named[k].grad is not None, k                  # no adapter (and no base parameter) is skipped
        g_got = named[k].grad.float().cpu()
        assert torch.isfinite(g_got).all(), k
        if float(g_ref.norm()) < 1e-6:
            assert ".lora_" not in k, (k, "an adapter with a zero reference gradient checks nothing")
            if float(g_got.norm()) > 5e-3:
                bad.append((k, "expected ~0", float(g_got.norm())))
            continue
        e = rel_err(g_got, g_ref)
        cos = float((g_got * g_ref).sum() / (g_got.norm() * g_ref.norm()))
        qk = "query." in k or "key." in k
        if e > (0.1 if qk else 4e-2) or cos < (0.995 if qk else 0.999):
            bad.append((k, e, cos, float(g_ref.norm())))
        if ".lora_" in k and not qk:
            worst_ad = (max(worst_ad[0], e), min(worst_ad[1], cos))
        n_ad += ".lora_" in k
    print("%s %s: worst adapter gradient error %.3g, lowest cosine %.6f" % (name, len(targets), worst_ad[0], worst_ad[1]))
    assert not bad, (name, bad[:12], len(bad))
    assert n_ad == len(ad) > 0


# ---------------------------------------------------------------------------------------------- 4, 5, 6
def _tasks_model(targets=NEW, r=8):
    import test_frozen_backward_gpu as FB
    from volta_amd import lora
    model, loss_fn = FB._tasks("vilbert", "TASK1")
    lora.add_lora(model, r=r, alpha=16, targets=targets)
    TL._randomise_B(model)
    return model, loss_fn, FB


def test_only_lora_trainable_keeps_the_bits():
    from volta_amd import lora
    model, loss_fn, FB = _tasks_model()
    FB._step(model, loss_fn, 77)                             # nothing frozen
    ref = TL._grads(model)
    n_full = len(model._last[0].bwd.ops)
    keep = [n for n in ref if ref[n] is not None and (".lora_" in n or n.startswith("clfs_dict."))]
    n_adapters = sum(".lora_" in n for n, _ in model.named_parameters())
    assert sum(".lora_" in n for n in keep) == n_adapters > 0 and len(keep) > n_adapters
    TL._zero(model)
    lora.mark_only_lora_trainable(model, also=("clfs_dict.",))
    runs = []
    for _ in range(2):
        TL._zero(model)
        FB._step(model, loss_fn, 77)
        runs.append(TL._grads(model))
    eng = model._last[0]
    assert eng.pruned and eng.frozen and len(eng.bwd.ops) < n_full
    named = dict(model.named_parameters())
    for n, g in runs[0].items():
        if n in keep:
            assert torch.equal(g, ref[n]), n                 # the bits of the nothing-frozen run
            assert torch.equal(g, runs[1][n]), n             # and of the same step once more
        elif not named[n].requires_grad:
            assert g is None, n
    arena = model._arena
    assert all(float(arena.view(n, "grad").abs().max()) == 0.0 for n in eng.pruned)
    assert not any(".lora_" in n for n in eng.pruned)


def test_adamw_moves_only_the_trainable_parameters():
    from volta_amd import lora
    from volta_amd.optimization import AdamW
    model, loss_fn, FB = _tasks_model()
    lora.mark_only_lora_trainable(model, also=("clfs_dict.",))
    model.materialize()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    opt = AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    losses = []
    for step in range(3):
        opt.zero_grad()
        losses.append(FB._step(model, loss_fn, 100 + step))
        opt.step()
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in losses), losses
    moved = 0
    for n, p in model.named_parameters():
        if ".lora_" in n:
            assert not torch.equal(p.detach(), before[n]), n
            moved += 1
        elif not p.requires_grad:
            assert torch.equal(p.detach(), before[n]), n
    assert moved > 0


def test_merge_on_the_gpu():
    """The reference's keys again, eval predictions within rel_err 2e-2 of those before, and the next plan has no LoRA op."""
    from test_engine_gpu import rel_err, CONFIGS
    from test_tasks_gpu import TASK_CFG
    from oracle import volta_ref as R
    from volta_amd import _lib as L, lora
    model, _, FB = _tasks_model(ALL)
    model.eval()
    rcfg = R.RefConfig(dict(CONFIGS["vilbert"], clf_hidden_size=1536))
    cb = {k: v.cuda() for k, v in R.synthetic_batch(rcfg, *SHAPE, seed=9, pad=True).items()}
    call = lambda: model(cb["input_ids"], cb["image_feat"], cb["image_loc"], "TASK1", cb["segment_ids"], cb["input_mask"], cb["image_mask"])[0].detach().float().clone()
    has = lambda: any(o[0] == L.OP_GENERIC and o[4].fn in (L.FN_LORA_FWD, L.FN_LORA_PROJ_FWD) for o in model._last[0].fwd.ops)
    plain_keys = {k for k in model.state_dict() if ".lora_" not in k}
    with torch.no_grad():
        pre = call()
        assert has()
        lora.merge_lora(model)
        assert set(model.state_dict()) == plain_keys == set(R.make_task_weights(rcfg, TASK_CFG, list(TASK_CFG), seed=4, std=0.04))
        post = call()
        assert not has()
    assert rel_err(post, pre) < 2e-2 and TASK_CFG["TASK1"]["num_labels"] == pre.shape[-1]


# ---------------------------------------------------------------------------------------------- 7
def test_retrieval_scorer_with_adapters():
    import test_retrieval_gpu as RT
    from volta_amd import lora
    model = RT._tiny("vilbert", zero_shot=False)
    lora.add_lora(model, r=8, alpha=16, targets=("ffn_up", "ffn_down", "attn_out"))
    TL._randomise_B(model)
    caps, imgs = RT._inputs(model.config, 5, 7, 20, 37, seed=11)
    want = RT._loop(model, caps, imgs)
    for chunk in (4, 1000):
        _, S, Lg = RT._score(model, caps, imgs, chunk)
        RT._check(S, Lg, want, False, ("lora_proj", chunk))
