"""The retrieval scorer (volta_amd/retrieval.py) against the reference driver's loop on the unchanged model (eval_retrieval.py:168-198:
each caption repeated against blocks of 500 images, `model(...)` per block): the reduced-depth configs of tests/test_engine_gpu.py in
VL-logit and zero-shot mode with ragged captions, ragged images and ragged pair chunks, ctrl_vilbert_base and ctrl_lxmert at full depth,
explicit pair lists, and a model whose state the scorer must leave alone.  GPU only.

Gate: the logits are compared with torch.equal.  Every launch of a forward computes a pair independently of the batch it sits in -- the
forward GEMMs do not split K, LayerNorm works per row, attention per (pair, head), the pair gather copies bytes -- and the scorer's lists are
built from the same builders, so a pair's logit must come out bit for bit as the loop's.  The one launch that looks across the batch is
VL-BERT's text position ids (shifted past the batch's shortest caption, the reference's quirk): the driver's batches hold one caption, and
so do the scorer's pair chunks for VL-BERT.  The zero-shot probability softmax(itm)[:, 0] is
taken by torch.softmax in both; it is compared within 8 ulp relative: p = 1 / (1 + exp(l1 - l0)), exp within 2 ulp, the add and the divide
half an ulp each, so each side is within 4 ulp of the exact value whichever vectorised path computed it."""
import copy
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASK_CFG = {"TASK8": {"type": "VL-logit"}}
ULP8 = 8 * 2.0 ** -23


def _tiny(name, zero_shot, seed=4):
    from test_engine_gpu import CONFIGS
    from oracle import volta_ref as R
    from volta_amd.config import BertConfig
    from volta_amd.modeling import BertForVLPreTraining, BertForVLTasks
    cd = dict(CONFIGS[name], clf_hidden_size=1536)
    rcfg = R.RefConfig(cd)
    if zero_shot:
        model = BertForVLPreTraining(BertConfig.from_dict(cd))
        model.load_state_dict(R.make_weights(rcfg, seed=seed, std=0.04), strict=True)
    else:
        model = BertForVLTasks(BertConfig.from_dict(cd), TASK_CFG, list(TASK_CFG))
        model.load_state_dict(R.make_task_weights(rcfg, TASK_CFG, list(TASK_CFG), seed=seed, std=0.04), strict=True)
    return model.cuda().eval()


def _inputs(cfg, Nc, Ni, T, Rv, seed):
    """Captions of different lengths ([CLS] ... [SEP], zero padding) and images with different region counts (the global feature first)."""
    g = torch.Generator().manual_seed(seed)
    V = cfg.vocab_size
    lens = torch.randint(max(3, T // 2), T + 1, (Nc,), generator=g)
    lens[0] = T
    ids = torch.randint(min(1000, V // 4), V, (Nc, T), generator=g)
    ar = torch.arange(T)[None]
    mask = (ar < lens[:, None]).long()
    ids[:, 0] = min(101, V - 2)
    ids[torch.arange(Nc), lens - 1] = min(102, V - 1)
    ids = ids * mask
    seg = torch.zeros(Nc, T, dtype=torch.long)
    nreg = torch.randint(max(2, Rv // 2), Rv + 1, (Ni,), generator=g)
    nreg[0] = Rv
    imask = (torch.arange(Rv)[None] < nreg[:, None]).long()
    feat = torch.rand(Ni, Rv, cfg.v_feature_size, generator=g) * 2.0 * imask[..., None]
    loc = torch.rand(Ni, Rv, cfg.num_locs, generator=g) * imask[..., None]
    return [t.cuda() for t in (ids, seg, mask)], [t.cuda() for t in (feat, loc, imask)]


def _loop(model, caps, imgs, block=500):
    """eval_retrieval.py:168-198 on the unchanged model: the raw logits [Nc, Ni, classes]."""
    from volta_amd.modeling import BertForVLTasks
    ids, seg, mask = caps
    feat, loc, imask = imgs
    Nc, Ni = ids.shape[0], feat.shape[0]
    rows = []
    with torch.no_grad():
        for c in range(Nc):
            row = []
            for i0 in range(0, Ni, block):
                n = min(block, Ni - i0)
                q, s, m = ids[c:c + 1].repeat(n, 1), seg[c:c + 1].repeat(n, 1), mask[c:c + 1].repeat(n, 1)
                f, l, im = feat[i0:i0 + n], loc[i0:i0 + n], imask[i0:i0 + n]
                if isinstance(model, BertForVLTasks):
                    row.append(model(q, f, l, "TASK8", s, m, im)[0].view(n, 1).float())
                else:
                    row.append(model(q, f, l, s, m, im)[2].float().clone())
            rows.append(torch.cat(row, 0))
    return torch.stack(rows, 0)


def _score(model, caps, imgs, pair_chunk):
    from volta_amd.retrieval import RetrievalScorer
    from volta_amd.modeling import BertForVLTasks
    sc = RetrievalScorer(model, "TASK8" if isinstance(model, BertForVLTasks) else None, pair_chunk=pair_chunk)
    S, Lg = sc.score_matrix(sc.encode_captions(*caps), sc.encode_images(*imgs), return_logits=True)
    return sc, S, Lg


def _check(S, Lg, want, zero_shot, tag):
    assert Lg.shape == want.shape, (tag, Lg.shape, want.shape)
    diff = (Lg - want).abs().max().item()
    assert torch.equal(Lg, want), (tag, "logits differ", diff)
    if zero_shot:
        p = torch.softmax(want, dim=2)[..., 0]
        assert bool(((S - p).abs() <= ULP8 * p.abs()).all()), (tag, (S - p).abs().max().item())
    else:
        assert torch.equal(S, want[..., 0]), tag


@pytest.mark.parametrize("zero_shot", [False, True])
@pytest.mark.parametrize("name", ["vilbert", "lxmert", "uniter", "visualbert", "vlbert"])
def test_score_matrix_equals_the_driver_loop(name, zero_shot):
    model = _tiny(name, zero_shot)
    caps, imgs = _inputs(model.config, 5, 7, 20, 37, seed=11)
    want = _loop(model, caps, imgs)
    was = (model.training, model._step, model._last, dict(model._engines))
    # pair_chunk 4: images in blocks of 4 + 3 per caption, prefixes in chunks of 4 + 1 / 4 + 3; 16: two captions per chunk (14, 14, 7 pairs;
    # vlbert: one caption per chunk, its text positions depend on the batch's shortest caption as in the driver's one-caption batches)
    for chunk in (4, 16, 1000):
        _, S, Lg = _score(model, caps, imgs, chunk)
        _check(S, Lg, want, zero_shot, (name, chunk))
    one_c, one_i = [t[2:3] for t in caps], [t[4:5] for t in imgs]
    _, S, Lg = _score(model, one_c, one_i, 1000)
    _check(S, Lg, want[2:3, 4:5], zero_shot, (name, "1x1"))
    torch.cuda.synchronize()
    assert (model.training, model._step) == was[:2] and model._last is was[2]
    assert set(model._engines) == set(was[3])


@pytest.mark.parametrize("zero_shot", [False, True])
@pytest.mark.parametrize("name", ["ctrl_vilbert_base", "ctrl_lxmert"])
def test_full_depth_across_500_pair_blocks(name, zero_shot):
    """T = 38, 36 regions + the global feature; 1 100 images cross two of the driver's 500-pair boundaries."""
    from volta_amd.config import BertConfig
    from volta_amd.modeling import BertForVLPreTraining, BertForVLTasks
    cfg = BertConfig.from_json_file(os.path.join(ROOT, "config", name + ".json"))
    torch.manual_seed(3)
    model = (BertForVLPreTraining(cfg) if zero_shot else BertForVLTasks(cfg, TASK_CFG, list(TASK_CFG))).cuda().eval()
    caps, imgs = _inputs(cfg, 3, 1100, 38, 37, seed=5)
    want = _loop(model, caps, imgs)
    _, S, Lg = _score(model, caps, imgs, 500)
    _check(S, Lg, want, zero_shot, name)


@pytest.mark.parametrize("name", ["lxmert", "vlbert"])
def test_explicit_pairs_equal_the_matrix_entries(name):
    """vlbert: its text positions follow the batch's shortest caption, so the scorer groups the pairs by caption -- shuffled pairs must
    still come back in the caller's order with the matrix's values."""
    from volta_amd.retrieval import RetrievalScorer
    model = _tiny(name, False)
    caps, imgs = _inputs(model.config, 5, 7, 20, 37, seed=12)
    sc = RetrievalScorer(model, "TASK8", pair_chunk=6)
    c, i = sc.encode_captions(*caps), sc.encode_images(*imgs)
    S = sc.score_matrix(c, i)
    g = torch.Generator().manual_seed(1)
    ci = torch.cat([torch.randint(0, 5, (20,), generator=g), torch.tensor([3, 3, 3, 0])]).cuda()
    ii = torch.cat([torch.randint(0, 7, (20,), generator=g), torch.tensor([6, 6, 0, 6])]).cuda()
    s = sc.score_pairs(c, i, ci, ii)
    assert torch.equal(s, S[ci, ii])
    with pytest.raises(ValueError):
        sc.score_pairs(c, i, ci, ii + 7)                                    # out of range
    with pytest.raises(ValueError):
        sc.score_pairs(c, i, ci, ii[:3])                                    # lengths differ
    with pytest.raises(ValueError):
        sc.encode_captions(caps[0], caps[1][:, :5], caps[2])              # mismatched shapes
    with pytest.raises(ValueError):
        sc.encode_images(imgs[0], imgs[1][..., :4], imgs[2])
    with pytest.raises(ValueError):
        sc.encode_images(imgs[0].cpu(), imgs[1].cpu(), imgs[2].cpu())      # not on the model's device
    with pytest.raises(ValueError):
        sc.score_matrix(i, c)                                              # sides swapped


def _train_step(model, opt, caps, imgs):
    ids, seg, mask = caps
    feat, loc, imask = imgs
    pred = model(ids, feat[:ids.shape[0]], loc[:ids.shape[0]], "TASK8", seg, mask, imask[:ids.shape[0]])[0]
    loss = (pred.float() * torch.linspace(-1.0, 1.0, pred.numel(), device=pred.device).view_as(pred)).sum()
    return pred, loss


def test_model_state_is_left_alone():
    """Scores after an AdamW step follow the step; scoring between a forward and its backward, or before the next training step, changes
    no gradient, loss or weight; `training` and the dropout step counter stay as they were."""
    from volta_amd.optimization import AdamW
    from volta_amd.retrieval import RetrievalScorer
    a, b = _tiny("vilbert", False), _tiny("vilbert", False)
    caps, imgs = _inputs(a.config, 5, 7, 20, 37, seed=13)
    for m in (a, b):
        m.train()
        m.set_dropout_seed(77)
    opt_a, opt_b = AdamW(a.parameters(), lr=1e-3), AdamW(b.parameters(), lr=1e-3)
    sc = RetrievalScorer(a, "TASK8", pair_chunk=16)
    for step in range(2):
        pa, la = _train_step(a, opt_a, caps, imgs)
        S = sc.score_matrix(sc.encode_captions(*caps), sc.encode_images(*imgs))        # between the forward and its backward
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
    # scores taken now follow the updated weights: equal to the loop on them (eval mode for the loop, as the driver runs it)
    S = sc.score_matrix(sc.encode_captions(*caps), sc.encode_images(*imgs))
    a.eval()
    want = _loop(a, caps, imgs)
    assert torch.equal(S, want[..., 0])


def test_a_wrong_prefix_fails_the_gate():
    """Two images' prefix rows swapped in the encoded handle: the suffix is computed with the wrong image for those columns, and the
    equality gate of test_score_matrix_equals_the_driver_loop catches it."""
    from volta_amd.retrieval import RetrievalScorer
    model = _tiny("vilbert", False)
    caps, imgs = _inputs(model.config, 5, 7, 20, 37, seed=11)
    want = _loop(model, caps, imgs)
    sc = RetrievalScorer(model, "TASK8", pair_chunk=16)
    c, i = sc.encode_captions(*caps), sc.encode_images(*imgs)
    assert torch.equal(sc.score_matrix(c, i), want[..., 0])
    x = i.tensors["x_v"].view(7, 37, -1)
    x[[1, 4]] = x[[4, 1]].clone()
    bad = sc.score_matrix(c, i)
    assert not torch.equal(bad, want[..., 0])
    assert torch.equal(bad[:, [0, 2, 3, 5, 6]], want[:, [0, 2, 3, 5, 6], 0])      # the other columns are untouched
