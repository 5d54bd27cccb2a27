"""The retrieval scorer on the e4m3 projection path (`RetrievalScorer(..., projection_dtype="fp8")`) against the reference driver's loop on
the same model after `set_projection_dtype("fp8")`: the cases, inputs and helpers of tests/test_retrieval_gpu.py.  GPU only.

Gate: torch.equal on the logits, by that file's argument carried over to the e4m3 launches.  An activation row is quantised with a scale
of its own, a weight with one scale per output channel, the GELU copy with the static H8_MUL, and both tile shapes of the e4m3 GEMM walk K in
the same 128-deep steps without splitting it, so a pair's row comes out of every launch as it does in any other batch.  What is left is
WHICH e4m3 bits a sub-layer's first projection reads: the copy the LayerNorm in front of it wrote from its fp32 outputs, or -- behind an
embedding -- the row quantisation of the bf16 state.  The whole model reads the former wherever a sub-layer precedes; so must the pair plan,
whose first sub-layer follows a prefix that ran in another plan: the copy and its scales travel in the handle and through the pair gather.
The zero-shot probability is compared within the 8 ulp of tests/test_retrieval_gpu.py.

Distance to the fp32 oracle (test_distance_to_the_fp32_oracle): largest |logit - oracle logit| over the 35 pairs, reduced-depth models,
random weights, observed on MI355X:
    case                  bf16 scorer   fp8 scorer   largest |oracle logit|
    vilbert  VL-logit     0.02287       0.14427      0.98
    vilbert  zero-shot    0.01814       0.16701      1.09
    uniter   VL-logit     0.01255       0.11903      0.98
    uniter   zero-shot    0.02817       0.17424      0.68
The fp8 gate is at most 2 x the largest fp8 value observed (0.17424), the convention of tests/test_fp8_gpu.py; the bf16 column is for the
record and gates nothing.  profiles/retrieval_fp8.md holds the same table."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_retrieval_gpu import TASK_CFG, _check, _inputs, _loop, _tiny, _train_step  # noqa: E402

OP_GEMM_FP8 = 18
FP8_ORACLE_TOL = 0.348      # largest |logit - oracle logit| of the fp8 scorer: <= 2 x the 0.17424 observed (table above)


def _fp8_loop(model, caps, imgs, block=500):
    """the driver's loop on the model with its own switch on fp8; the switch is back on bf16 afterwards"""
    model.set_projection_dtype("fp8")
    try:
        return _loop(model, caps, imgs, block)
    finally:
        model.set_projection_dtype("bf16")


def _scorer(model, pair_chunk, dtype="fp8"):
    from volta_amd.modeling import BertForVLTasks
    from volta_amd.retrieval import RetrievalScorer
    return RetrievalScorer(model, "TASK8" if isinstance(model, BertForVLTasks) else None, pair_chunk=pair_chunk, projection_dtype=dtype)


def _score(model, caps, imgs, pair_chunk, dtype="fp8"):
    sc = _scorer(model, pair_chunk, dtype)
    S, Lg = sc.score_matrix(sc.encode_captions(*caps), sc.encode_images(*imgs), return_logits=True)
    return sc, S, Lg


@pytest.mark.parametrize("zero_shot", [False, True])
@pytest.mark.parametrize("name", ["vilbert", "lxmert", "uniter", "visualbert", "vlbert"])
def test_fp8_score_matrix_equals_the_fp8_driver_loop(name, zero_shot):
    model = _tiny(name, zero_shot)
    caps, imgs = _inputs(model.config, 5, 7, 20, 37, seed=11)
    want = _fp8_loop(model, caps, imgs)
    assert model._fp8 is False
    was = (model.training, model._step, model._last, dict(model._engines))
    for chunk in (4, 16, 1000):
        sc, S, Lg = _score(model, caps, imgs, chunk)
        _check(S, Lg, want, zero_shot, (name, chunk))
        pair = [e for k, e in sc._engines.items() if k[0] == "pair"]
        assert pair and all(e.fp8 and any(op[0] == OP_GEMM_FP8 for op in e.fwd.ops) for e in pair)
    one_c, one_i = [t[2:3] for t in caps], [t[4:5] for t in imgs]
    _, S, Lg = _score(model, one_c, one_i, 1000)
    _check(S, Lg, want[2:3, 4:5], zero_shot, (name, "1x1"))
    torch.cuda.synchronize()
    assert model._fp8 is False and (model.training, model._step) == was[:2] and model._last is was[2]
    assert set(model._engines) == set(was[3])


def test_fp8_full_depth_across_a_500_pair_block():
    """ctrl_vilbert_base, T = 38, 36 regions + the global feature; 520 images cross one of the driver's 500-pair boundaries."""
    from volta_amd.config import BertConfig
    from volta_amd.modeling import BertForVLTasks
    cfg = BertConfig.from_json_file(os.path.join(ROOT, "config", "ctrl_vilbert_base.json"))
    torch.manual_seed(3)
    model = BertForVLTasks(cfg, TASK_CFG, list(TASK_CFG)).cuda().eval()
    caps, imgs = _inputs(cfg, 3, 520, 38, 37, seed=5)
    want = _fp8_loop(model, caps, imgs)
    _, S, Lg = _score(model, caps, imgs, 500)
    _check(S, Lg, want, False, "ctrl_vilbert_base")


def test_the_projections_are_e4m3_and_the_hand_over_is_the_layernorm_copy():
    """The pair plan's forward list holds e4m3 GEMM launches where the bf16 scorer's holds none; the handles carry the copy of exactly the
    modalities whose prefix ends in a sub-layer; and the suffix reads it: another caption's e4m3 rows written over caption 2's change
    caption 2's scores and no other row (the bf16 rows, which the residual path reads, stay as they were)."""
    from volta_amd.retrieval import pair_gather_segments
    model = _tiny("vilbert", False)
    caps, imgs = _inputs(model.config, 5, 7, 20, 37, seed=11)
    want = _fp8_loop(model, caps, imgs)
    sc = _scorer(model, 16)
    c, i = sc.encode_captions(*caps), sc.encode_images(*imgs)
    assert torch.equal(sc.score_matrix(c, i), want[..., 0])
    H = model.config.hidden_size
    assert c.tensors["x8_t"].dtype == torch.uint8 and tuple(c.tensors["x8_t"].shape) == (5 * 20, -(-H // 128) * 128)
    assert c.tensors["xs_t"].dtype == torch.float32 and tuple(c.tensors["xs_t"].shape) == (5 * 20,)
    assert "x8_v" not in i.tensors and "xs_v" not in i.tensors                # vilbert's vision prefix is its embedding
    eng = next(e for k, e in sc._engines.items() if k[0] == "pair")
    assert [(n, s) for n, _, s in eng.pair_inputs] == pair_gather_segments(model.config, "fp8") and eng.pair_args.nseg == 6
    assert any(op[0] == OP_GEMM_FP8 for op in eng.fwd.ops)
    bf = _scorer(model, 16, "bf16")
    bf.score_matrix(bf.encode_captions(*caps), bf.encode_images(*imgs))
    assert not any(op[0] == OP_GEMM_FP8 for e in bf._engines.values() for op in e.fwd.ops)
    x8 = c.tensors["x8_t"].view(5, 20, -1)
    assert not torch.equal(x8[2], x8[0])
    x8[2] = x8[0].clone()
    bad = sc.score_matrix(c, i)
    assert not torch.equal(bad[2], want[2, :, 0])
    assert torch.equal(bad[[0, 1, 3, 4]], want[[0, 1, 3, 4], :, 0])
    # lxmert: both prefixes end in a sub-layer, both copies travel -- eight segments, the gather's limit
    lx = _tiny("lxmert", False)
    sl = _scorer(lx, 16)
    cl, il = sl.encode_captions(*caps), sl.encode_images(*imgs)
    assert "x8_t" in cl.tensors and "x8_v" in il.tensors and tuple(il.tensors["xs_v"].shape) == (7 * 37,)
    sl.score_matrix(cl, il)
    assert next(e for k, e in sl._engines.items() if k[0] == "pair").pair_args.nseg == 8


def test_fp8_scoring_leaves_the_model_state_alone():
    """Two identical bf16 models take the same training steps, one with fp8 scoring between its forward and backward: predictions, losses,
    gradients and weights stay equal, the model's switch stays on bf16, and a bf16 scorer built afterwards still equals the bf16 loop."""
    from volta_amd.optimization import AdamW
    a, b = _tiny("vilbert", False), _tiny("vilbert", False)
    caps, imgs = _inputs(a.config, 5, 7, 20, 37, seed=13)
    for m in (a, b):
        m.train()
        m.set_dropout_seed(77)
    opt_a, opt_b = AdamW(a.parameters(), lr=1e-3), AdamW(b.parameters(), lr=1e-3)
    sc = _scorer(a, 16)
    for step in range(2):
        pa, la = _train_step(a, opt_a, caps, imgs)
        engines = set(a._engines)
        sc.score_matrix(sc.encode_captions(*caps), sc.encode_images(*imgs))            # between the forward and its backward
        assert a._fp8 is False and set(a._engines) == engines
        la.backward()
        pb, lb = _train_step(b, opt_b, caps, imgs)
        lb.backward()
        assert torch.equal(pa, pb) and torch.equal(la, lb), step
        for (n, p), q in zip(a.named_parameters(), b.parameters()):
            assert (p.grad is None) == (q.grad is None), n
            assert p.grad is None or torch.equal(p.grad, q.grad), (step, n)
        assert a.training and a._step == b._step == step + 1
        opt_a.step()
        opt_b.step()
        opt_a.zero_grad()
        opt_b.zero_grad()
        for (n, p), q in zip(a.named_parameters(), b.parameters()):
            assert torch.equal(p, q), (step, n)
    # the fp8 scorer follows the updated weights; a bf16 scorer on the same model is still the bf16 loop
    S8 = sc.score_matrix(sc.encode_captions(*caps), sc.encode_images(*imgs))
    a.eval()
    assert torch.equal(S8, _fp8_loop(a, caps, imgs)[..., 0])
    _, S, _ = _score(a, caps, imgs, 16, "bf16")
    assert a._fp8 is False and torch.equal(S, _loop(a, caps, imgs)[..., 0])


def test_fp8_scores_follow_freshly_loaded_weights():
    """load_state_dict between two calls of one scorer: the e4m3 weight copies are re-quantised (weights_epoch), the second result is the
    fp8 loop on the new weights and differs from the first."""
    model = _tiny("lxmert", False)
    other = copy.deepcopy(_tiny("lxmert", False, seed=5).state_dict())
    caps, imgs = _inputs(model.config, 5, 7, 20, 37, seed=11)
    sc = _scorer(model, 16)
    S0 = sc.score_matrix(sc.encode_captions(*caps), sc.encode_images(*imgs)).clone()
    model.load_state_dict(other, strict=True)
    S1 = sc.score_matrix(sc.encode_captions(*caps), sc.encode_images(*imgs))
    assert not torch.equal(S0, S1)
    assert torch.equal(S1, _fp8_loop(model, caps, imgs)[..., 0])


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    from tests.retrieval_eval_fixture import EvalFixture
    return EvalFixture(tmp_path_factory.mktemp("retrieval_fp8_gpu"))


def test_evaluate_retrieval_fp8_equals_the_fp8_driver(fx):
    from test_retrieval_eval_gpu import _driver, _tiny as _eval_tiny
    from tests import ranks_restate as RR
    from volta_amd import datasets as D
    from volta_amd.retrieval import evaluate_retrieval
    model = _eval_tiny(False)
    ds = fx.dataset("coco_last")
    Nc, Ni = len(ds) // 2, 6
    model.set_projection_dtype("fp8")
    S = _driver(model, D.RetrievalEvalLoader(ds), Nc, Ni, False)
    model.set_projection_dtype("bf16")
    want_ir, want_top, want_tr = RR.ranks(S.astype(np.float32), ds.host_tables()["caption_image"], 20)
    res = evaluate_retrieval(model, ds, task_id="TASK8", pair_chunk=7, topk=20, projection_dtype="fp8")
    assert model._fp8 is False
    assert np.array_equal(res.score_matrix.cpu().numpy(), S.astype(np.float32))
    assert np.array_equal(res.rank_ir.cpu().numpy(), want_ir) and np.array_equal(res.rank_tr.cpu().numpy(), want_tr)
    assert res.results == [[v for v in row if v >= 0] for row in want_top.tolist()]
    assert res.image_retrieval == RR.metrics(want_ir) and res.text_retrieval == RR.metrics(want_tr[want_tr >= 0])


def _oracle_logits(name, zero_shot, caps, imgs, seed=4):
    """fp32 oracle (oracle/volta_ref.py) logits [Nc, Ni, classes] of every pair, from the weights _tiny(name, zero_shot, seed) loads"""
    from test_engine_gpu import CONFIGS
    from oracle import volta_ref as R
    rcfg = R.RefConfig(dict(CONFIGS[name], clf_hidden_size=1536))
    sd = R.make_weights(rcfg, seed=seed, std=0.04) if zero_shot else R.make_task_weights(rcfg, TASK_CFG, list(TASK_CFG), seed=seed, std=0.04)
    full = dict(sd)
    for alias, target in R.param_aliases(rcfg).items():
        full[alias] = sd[target]
    ids, seg, mask = [t.cpu() for t in caps]
    feat, loc, imask = [t.cpu() for t in imgs]
    Nc, Ni = ids.shape[0], feat.shape[0]
    rep_c = lambda t: t.repeat_interleave(Ni, 0)
    rep_i = lambda t: t.repeat(Nc, *[1] * (t.dim() - 1))
    with torch.no_grad():
        if zero_shot:
            _, _, pt, pv = R.bert_model(full, rcfg, rep_c(ids), rep_i(feat), rep_i(loc), rep_c(seg), rep_c(mask), rep_i(imask))
            out = R.linear(R.fuse_pooled(rcfg, pt, pv), full, "cls.bi_seq_relationship")
        else:
            out = R.tasks_forward(full, rcfg, TASK_CFG, "TASK8", rep_c(ids), rep_i(feat), rep_i(loc), rep_c(seg), rep_c(mask), rep_i(imask))
    return out.view(Nc, Ni, -1).float()


@pytest.mark.parametrize("zero_shot", [False, True])
@pytest.mark.parametrize("name", ["vilbert", "uniter"])
def test_distance_to_the_fp32_oracle(name, zero_shot):
    """The yardstick is the oracle, never the bf16 scorer: the bf16 figure is printed beside the fp8 one for the record only."""
    model = _tiny(name, zero_shot)
    caps, imgs = _inputs(model.config, 5, 7, 20, 37, seed=11)
    want = _oracle_logits(name, zero_shot, caps, imgs)
    err = {}
    for dtype in ("bf16", "fp8"):
        _, _, Lg = _score(model, caps, imgs, 16, dtype)
        assert Lg.shape == want.shape
        err[dtype] = float((Lg.cpu() - want).abs().max())
    print("oracle distance %s %s: bf16 %.5f fp8 %.5f (largest |oracle logit| %.4f)" % (name, "zero-shot" if zero_shot else "VL-logit", err["bf16"], err["fp8"],
                                                                                       float(want.abs().max())))
    assert err["fp8"] <= FP8_ORACLE_TOL, (name, zero_shot, err)
