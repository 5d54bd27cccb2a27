"""A standalone BertModel as a trainable backbone: its forward against the task model's encoder, its gradients against the fp32 oracle
(final states, pooled vectors, every sub-layer's states), train-mode dropout replay, poolers without gradient, accumulation and stale
backwards, AdamW / clip_grad_norm_ over the arena plus torch tensors, and a custom torch head trained end to end.  True layer widths,
the reduced depth of tests/test_engine_gpu.py.  GPU only."""
import copy
import os
import sys

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-12))


def _setup(name, fusion=None, seed=4):
    from test_engine_gpu import CONFIGS
    from oracle import volta_ref as R
    from volta_amd.config import BertConfig
    from volta_amd.modeling import BertModel
    cd = dict(CONFIGS[name], clf_hidden_size=1536)
    if fusion:
        cd["fusion_method"] = fusion
    rcfg = R.RefConfig(cd)
    sd = R.make_weights(rcfg, seed=seed, std=0.04)
    model = BertModel(BertConfig.from_dict(cd))
    model.load_state_dict({k[len("bert."):]: v for k, v in sd.items() if k.startswith("bert.")}, strict=True)
    return model.cuda(), rcfg, sd, cd


def _call(model, cb, **kw):
    return model(cb["input_ids"], cb["image_feat"], cb["image_loc"], cb["segment_ids"], cb["input_mask"], cb["image_mask"], **kw)


def _leaves(R, rcfg, sd):
    aliases = R.param_aliases(rcfg)
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k not in aliases and k.startswith("bert.")}
    full = dict(leaves)
    for a, t in aliases.items():
        if t in leaves:
            full[a] = leaves[t]
    return leaves, full


def _check_grads(model, leaves, tag):
    named = {"bert." + k: p for k, p in model.named_parameters()}
    bad, checked = [], 0
    for k, leaf in leaves.items():
        if leaf.grad is None or k.endswith("key.bias"):        # d/d(key bias) is identically zero (softmax shift invariance)
            continue
        g = named[k].grad
        if leaf.grad.norm() < 1e-9:
            assert g is None or float(g.norm()) <= 1e-4, (tag, k)
            continue
        assert g is not None, (tag, k)
        tol = 0.12 if ("query." in k or "key." in k) else 6e-2         # tests/test_tasks_gpu.py, every position probed
        if leaf.grad.dim() == 1:
            tol = max(tol, 0.15)
        if "_pooler." in k:
            # one token per sample (B = 4) behind a ReLU: pooled values near 0 flip their mask under the bf16 forward noise -- the
            # pooled-output tolerances of tests/test_tasks_gpu.py (observed 0.06-0.10 on the pooler weights)
            tol = 0.25 if leaf.grad.dim() == 1 else 0.15
        e = rel(g.float().cpu(), leaf.grad)
        if e > tol:
            bad.append((k, round(e, 4), tol))
        checked += 1
    assert not bad, (tag, bad[:10], len(bad), checked)
    assert checked > 20, checked


def test_standalone_forward_equals_the_task_models_encoder(tmp_path):
    """BertModel.from_pretrained(<pre-training save>) strips the `bert.` prefix and, in eval mode, gives exactly what the task model's
    encode() gives for the same weights (same forward plan); the saved pre-training model's own encoder agrees within bf16 noise."""
    from test_engine_gpu import CONFIGS
    from oracle import volta_ref as R
    from volta_amd.config import BertConfig
    from volta_amd.modeling import BertForVLPreTraining, BertForVLTasks, BertModel
    task_cfg = {"TASK1": {"type": "VL-classifier", "num_labels": 10}}
    for name in ("vilbert", "uniter"):
        cd = dict(CONFIGS[name], clf_hidden_size=1536)
        rcfg = R.RefConfig(cd)
        cfg = BertConfig.from_dict(cd)
        pre = BertForVLPreTraining(cfg)
        pre.load_state_dict(R.make_weights(rcfg, seed=3, std=0.04), strict=True)
        d = tmp_path / name
        d.mkdir()
        pre.save_pretrained(str(d))
        bm = BertModel.from_pretrained(str(d), config=cfg).cuda().eval()
        tm = BertForVLTasks.from_pretrained(str(d), task_cfg, ["TASK1"], config=cfg).cuda().eval()
        pre = pre.cuda().eval()
        assert bm.embeddings.word_embeddings.weight.data_ptr() != tm.bert.embeddings.word_embeddings.weight.data_ptr()
        batch = R.synthetic_batch(rcfg, 4, 20, 36, seed=9, pad=True)
        cb = {k: v.cuda() for k, v in batch.items()}
        got, want, own = _call(bm, cb), _call(tm.bert, cb), _call(pre.bert, cb)
        for i in range(4):
            if want[i] is None:
                assert got[i] is None
                continue
            assert got[i].dtype == torch.float32 and torch.equal(got[i], want[i]), (name, i)
            assert rel(got[i], own[i]) <= 1e-2, (name, i, rel(got[i], own[i]))


@pytest.mark.parametrize("name,fusion", [("vilbert", None), ("lxmert", None), ("uniter", None), ("vlbert", "vl-bert_vqa")])
def test_gradient_parity_with_the_oracle(name, fusion):
    """loss = sum(probe * (seq_t, seq_v, pooled_t, pooled_v)) in eval mode: outputs and the gradient of every parameter against fp32
    autograd through oracle.volta_ref.bert_model."""
    _parity(name, fusion, train=False)


def test_gradient_parity_train_mode_dropout_replay():
    _parity("vilbert", None, train=True)


def _parity(name, fusion, train):
    from oracle import volta_ref as R
    model, rcfg, sd, _ = _setup(name, fusion)
    seed = 0x5EED1234
    model.train(train)
    model.set_dropout_seed(seed)
    batch = R.synthetic_batch(rcfg, 4, 20, 36, seed=9, pad=True)
    cb = {k: v.cuda() for k, v in batch.items()}
    outs = _call(model, cb)[:4]
    gen = torch.Generator().manual_seed(11)
    probes = [None if o is None else torch.randn(o.shape, generator=gen) for o in outs]
    sum((o * p.cuda()).sum() for o, p in zip(outs, probes) if o is not None).backward()
    torch.cuda.synchronize()
    leaves, full = _leaves(R, rcfg, sd)
    drop = R.Dropper(True, seed) if train else None
    want = R.bert_model(full, rcfg, batch["input_ids"], batch["image_feat"].clone(), batch["image_loc"], batch["segment_ids"],
                        batch["input_mask"], batch["image_mask"], drop=drop)
    sum((w * p).sum() for w, p in zip(want, probes) if w is not None).backward()
    for i, (o, w) in enumerate(zip(outs, want)):
        assert (o is None) == (w is None), (name, i)
        if o is not None:
            assert rel(o.detach().cpu(), w.detach()) <= 3e-2, (name, i, rel(o.detach().cpu(), w.detach()))
    _check_grads(model, leaves, (name, fusion, train))


def test_all_encoded_layers_gradients_match_the_oracle_taps():
    """output_all_encoded_layers=True with a probe on every entry: each intermediate state's gradient enters the backward at its
    sub-layer (ViLBERT: the vision stream enters late, its embedding backward runs aside)."""
    from oracle import volta_ref as R
    model, rcfg, sd, _ = _setup("vilbert")
    model.eval()
    batch = R.synthetic_batch(rcfg, 4, 20, 36, seed=9, pad=True)
    cb = {k: v.cuda() for k, v in batch.items()}
    seq_t, seq_v, pt, pv, _ = _call(model, cb, output_all_encoded_layers=True)
    ids = [n for n, _ in R.sublayer_schedule(rcfg)]
    assert len(seq_t) == len(seq_v) == len(ids)
    gen = torch.Generator().manual_seed(5)
    entries = list(seq_t) + list(seq_v) + [pt, pv]
    probes = [torch.randn(e.shape, generator=gen) for e in entries]
    sum((e * p.cuda()).sum() for e, p in zip(entries, probes)).backward()
    torch.cuda.synchronize()
    leaves, full = _leaves(R, rcfg, sd)
    taps = {}
    _, _, opt_, opv = R.bert_model(full, rcfg, batch["input_ids"], batch["image_feat"].clone(), batch["image_loc"], batch["segment_ids"],
                                    batch["input_mask"], batch["image_mask"], taps=taps)
    ref = [taps["t%d" % n] for n in ids] + [taps["v%d" % n] for n in ids] + [opt_, opv]
    for i, (e, r) in enumerate(zip(entries, ref)):
        assert rel(e.detach().cpu(), r.detach()) <= 3e-2, (i, rel(e.detach().cpu(), r.detach()))
    sum((r * p).sum() for r, p in zip(ref, probes)).backward()
    _check_grads(model, leaves, "all layers")


def test_poolers_without_gradient_stay_untouched():
    from oracle import volta_ref as R
    from volta_amd.optimization import AdamW
    model, rcfg, _, _ = _setup("vilbert")
    model.eval()
    batch = R.synthetic_batch(rcfg, 4, 20, 36, seed=9, pad=True)
    cb = {k: v.cuda() for k, v in batch.items()}
    head = nn.Linear(rcfg.v_hidden_size, 3).cuda()
    opt = AdamW(list(model.parameters()) + list(head.parameters()), lr=1e-3, weight_decay=0.01)
    before = {n: p.detach().clone() for n, p in model.named_parameters() if "pooler" in n}
    seq_t, seq_v, pt, pv, _ = _call(model, cb)
    head(seq_v).sum().backward()
    for n, p in model.named_parameters():
        if "pooler" in n:
            assert p.grad is None, n
    assert model.encoder.layer[7].output.v_dense.weight.grad is not None
    opt.step()
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        if "pooler" in n:
            assert torch.equal(p.detach(), before[n]), n


def test_two_backwards_accumulate_and_stale_backward_raises():
    from oracle import volta_ref as R
    model, rcfg, _, _ = _setup("uniter")
    model.eval()
    batch = R.synthetic_batch(rcfg, 4, 20, 36, seed=9, pad=True)
    cb = {k: v.cuda() for k, v in batch.items()}
    probe = torch.randn(4, 20, rcfg.hidden_size, generator=torch.Generator().manual_seed(1)).cuda()

    def loss():
        seq_t, seq_v, pt, pv, _ = _call(model, cb)
        return (seq_t * probe).sum() + pt.sum() + 0.5 * pv.sum() + seq_v.mean()

    loss().backward()
    one = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    loss().backward()
    for n, p in model.named_parameters():
        if n in one:
            assert torch.equal(p.grad, 2 * one[n]), n
    l1 = loss()
    l1.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second backward"):
        l1.backward()
    l2 = loss()
    loss()
    with pytest.raises(RuntimeError, match="overtaken"):
        l2.backward()
    with torch.no_grad():                    # no node, same values
        a = _call(model, cb)
    b = _call(model, cb)
    assert a[0].grad_fn is None and b[0].grad_fn is not None and torch.equal(a[0], b[0].detach())


def test_mixed_adamw_and_clip_match_the_oracle():
    """Groups as train_task.py:208-218 builds them (one per parameter; the head at its own lr), clip + AdamW for 3 steps against
    R.clip_grad_norm + R.adamw_step on the same gradients; a duplicated arena parameter; a state_dict round trip."""
    from oracle import volta_ref as R
    from volta_amd.optimization import AdamW, clip_grad_norm_
    model, rcfg, _, _ = _setup("uniter")
    model.eval()
    batch = R.synthetic_batch(rcfg, 4, 20, 36, seed=9, pad=True)
    cb = {k: v.cuda() for k, v in batch.items()}
    torch.manual_seed(0)
    vil_head = nn.Sequential(nn.Linear(rcfg.pooler_size, 192), nn.GELU(), nn.Linear(192, 7)).cuda()
    orig = model.encoder.layer[1].intermediate.dense.weight
    dup = nn.Parameter(orig.detach().clone())
    named = [("bert." + n, p) for n, p in model.named_parameters()] + [("vil_head." + n, p) for n, p in vil_head.named_parameters()] + [("dup.weight", dup)]
    no_decay = ["bias", "LayerNorm.bias", "LayerNorm.weight"]
    groups = [{"params": [p], "lr": 1e-4 if "vil_" in n else 2e-5, "weight_decay": 0.0 if any(nd in n for nd in no_decay) else 0.01}
              for n, p in named]
    opt = AdamW(groups, lr=2e-5, eps=1e-6, betas=(0.9, 0.98))
    ref_p = {n: p.detach().clone() for n, p in named}
    ref_m = {n: torch.zeros_like(p) for n, p in named}
    ref_v = {n: torch.zeros_like(p) for n, p in named}
    labels = torch.arange(4, device="cuda") % 7

    def fwd_bwd():
        _, _, pt, pv, _ = _call(model, cb)
        loss = nn.functional.cross_entropy(vil_head(pt * pv), labels)
        loss.backward()
        dup.grad = orig.grad.clone()
        return loss

    for step in range(1, 4):
        opt.zero_grad()
        fwd_bwd()
        grads = {n: p.grad.detach().clone() for n, p in named}
        norm = clip_grad_norm_([p for _, p in named], 0.5)
        want = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())))
        assert abs(float(norm) - want) <= 1e-6 * want, (float(norm), want)
        R.clip_grad_norm(list(grads.values()), 0.5)
        opt.step()
        torch.cuda.synchronize()
        for (n, p), g in zip(named, groups):
            R.adamw_step(ref_p[n], grads[n], ref_m[n], ref_v[n], step, g["lr"], beta1=0.9, beta2=0.98, eps=1e-6, weight_decay=g["weight_decay"])
            err = float((p.detach() - ref_p[n]).abs().max())
            assert err <= 2e-6, (step, n, err)
        assert torch.equal(dup.detach(), orig.detach()), step
    # state_dict round trip: resume from (weights, optimizer state) and take the same step twice
    snap = [p.detach().clone() for _, p in named]
    sd = copy.deepcopy(opt.state_dict())
    opt.zero_grad()
    fwd_bwd()
    clip_grad_norm_([p for _, p in named], 0.5)
    opt.step()
    first = [p.detach().clone() for _, p in named]
    with torch.no_grad():
        for (_, p), s in zip(named, snap):
            p.copy_(s)
    opt2 = AdamW([{"params": g["params"], "lr": g["lr"], "weight_decay": g["weight_decay"]} for g in groups], lr=2e-5, eps=1e-6, betas=(0.9, 0.98))
    opt2.load_state_dict(sd)
    opt2.zero_grad()
    fwd_bwd()
    clip_grad_norm_([p for _, p in named], 0.5)
    opt2.step()
    torch.cuda.synchronize()
    for (n, p), w in zip(named, first):
        assert torch.equal(p.detach(), w), n


def test_custom_head_trains_end_to_end(tmp_path):
    """The issue's example: BertModel.from_pretrained(<task checkpoint>) under a torch head, grouped AdamW, clip, 3 steps."""
    import volta_amd
    from oracle import volta_ref as R
    from volta_amd.config import BertConfig
    from volta_amd.modeling import BertForVLTasks
    from test_engine_gpu import CONFIGS
    cd = dict(CONFIGS["vilbert"], clf_hidden_size=1536)
    cfg = BertConfig.from_dict(cd)
    rcfg = R.RefConfig(cd)
    task_cfg = {"TASK1": {"type": "VL-classifier", "num_labels": 10}}
    tm = BertForVLTasks(cfg, task_cfg, ["TASK1"])
    tm.load_state_dict(R.make_task_weights(rcfg, task_cfg, ["TASK1"], seed=2, std=0.04), strict=True)
    tm.save_pretrained(str(tmp_path))
    K = 10

    class MyTask(nn.Module):
        def __init__(self, cfg):
            super().__init__()
            self.bert = volta_amd.modeling.BertModel.from_pretrained(str(tmp_path), config=cfg)
            self.head = nn.Sequential(nn.Linear(cfg.pooler_size, 1536), nn.GELU(), nn.Linear(1536, K))

        def forward(self, *batch):
            seq_t, seq_v, pooled_t, pooled_v, _ = self.bert(*batch)
            return self.head(pooled_t * pooled_v)

    model = MyTask(cfg).cuda().train()
    assert torch.equal(model.bert.t_pooler.dense.weight.detach().cpu(), tm.bert.t_pooler.dense.weight.detach())     # `bert.` stripped
    no_decay = ["bias", "LayerNorm.bias", "LayerNorm.weight"]
    groups = [{"params": [p for n, p in model.named_parameters() if not any(nd in n for nd in no_decay)], "weight_decay": 0.01},
              {"params": [p for n, p in model.named_parameters() if any(nd in n for nd in no_decay)], "weight_decay": 0.0}]
    opt = volta_amd.optimization.AdamW(groups, lr=1e-4)
    batch = R.synthetic_batch(rcfg, 8, 20, 36, seed=3, pad=True)
    cb = {k: v.cuda() for k, v in batch.items()}
    labels = torch.arange(8, device="cuda") % K
    watch = {n: p.detach().clone() for n, p in model.named_parameters()
             if n in ("bert.encoder.layer.2.attention_self.query.weight", "bert.t_pooler.dense.weight", "bert.v_pooler.dense.weight", "head.2.weight")}
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = nn.functional.cross_entropy(model(cb["input_ids"], cb["image_feat"], cb["image_loc"], cb["segment_ids"], cb["input_mask"],
                                                 cb["image_mask"]), labels)
        loss.backward()
        volta_amd.optimization.clip_grad_norm_(model.parameters(), 5.0)
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < losses[0], losses
    for n, w in watch.items():
        assert not torch.equal(dict(model.named_parameters())[n].detach(), w), n
