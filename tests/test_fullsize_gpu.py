"""Size-independent properties of the pre-training step at BASELINE.json's FULL sizes -- configs[1] ctrl_vilbert_base B=256, configs[2]
ctrl_lxmert B=256 and the per-GPU share of configs[3], ctrl_uniter_base B=512 (global batch 4096 over 8 GPUs); T=20, 36 regions --
where the CPU oracle is too slow to be the checker:
  * pairs are independent: permuting the batch leaves the three losses and the gradients unchanged;
  * the losses are per-row means: the full-batch MLM / region / ITM losses are the count-weighted means of two half batches,
    and the full-batch gradient is the same combination of the half-batch gradients (linearity of backward);
  * the same inputs give the same losses twice (no state leaks between steps).
Eval mode (dropout masks are tied to row positions, a permutation would move them).  GPU only."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(model, b, idx=None):
    from volta_amd.data import model_args
    if idx is not None:
        b = {k: (v[idx] if torch.is_tensor(v) else v) for k, v in b.items()}
    for p in model.parameters():
        p.grad = None
    lm, img, nsp = model(*model_args(b))
    (lm + img + nsp).sum().backward()
    torch.cuda.synchronize()
    g = model._arena.grad.detach().clone()
    n_lm = int((b["lm_label_ids"] != -1).sum())
    n_img = int((b["image_label"] == 1).sum())
    return [float(lm.detach()), float(img.detach()), float(nsp.detach())], g, (n_lm, n_img, b["is_match"].shape[0])


@pytest.mark.parametrize("name,B", [("ctrl_vilbert_base", 256), ("ctrl_lxmert", 256), ("ctrl_uniter_base", 512)])
def test_full_size_batch_properties(name, B):
    from volta_amd.config import BertConfig
    from volta_amd.modeling import BertForVLPreTraining
    from volta_amd.data import synthetic_batch
    cfg = BertConfig.from_json_file(os.path.join(ROOT, "config", name + ".json"))
    torch.manual_seed(1234)
    model = BertForVLPreTraining(cfg).cuda().eval()
    b = synthetic_batch(cfg, B, 20, 36, seed=1234, device="cuda")
    full, g_full, n_full = _run(model, b)
    again, g_again, _ = _run(model, b)
    for a, c in zip(full, again):                                   # same inputs, same losses (row sums are atomically accumulated: last-bit order effects,
        assert abs(a - c) <= 5e-6 * abs(a), (full, again)           # up to ~10 ulp observed over ctrl_lxmert's four visual losses)
    assert torch.equal(g_full, g_again)                              # no gradient reads a loss sum
    # ---- permutation of the pairs
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3)).cuda()
    lp, g_perm, _ = _run(model, b, perm)
    for a, c in zip(full, lp):
        assert abs(a - c) <= 2e-4 * abs(a), (full, lp)
    assert float((g_perm - g_full).norm() / g_full.norm()) <= 2e-3
    # ---- two half batches: count-weighted means of the losses, same combination of the gradients
    h0, g0, n0 = _run(model, b, torch.arange(0, B // 2, device="cuda"))
    h1, g1, n1 = _run(model, b, torch.arange(B // 2, B, device="cuda"))
    assert n0[0] + n1[0] == n_full[0] and n0[1] + n1[1] == n_full[1]
    for i in range(3):
        w0, w1 = n0[i] / n_full[i], n1[i] / n_full[i]
        comb = w0 * h0[i] + w1 * h1[i]
        assert abs(comb - full[i]) <= 3e-4 * abs(full[i]), (i, comb, full[i])
    # d(total)/dθ = Σ_i d(loss_i)/dθ and each loss_i combines with its own weights; check through the total with per-loss weights:
    # run the halves again with the upstream gradient of each loss scaled by its weight
    def weighted(idx, w):
        from volta_amd.data import model_args
        bb = {k: (v[idx] if torch.is_tensor(v) else v) for k, v in b.items()}
        for p in model.parameters():
            p.grad = None
        lm, img, nsp = model(*model_args(bb))
        (w[0] * lm + w[1] * img + w[2] * nsp).sum().backward()
        torch.cuda.synchronize()
        return model._arena.grad.detach().clone()
    gw = weighted(torch.arange(0, B // 2, device="cuda"), [n0[i] / n_full[i] for i in range(3)]) + \
        weighted(torch.arange(B // 2, B, device="cuda"), [n1[i] / n_full[i] for i in range(3)])
    assert float((gw - g_full).norm() / g_full.norm()) <= 5e-3
