"""The root models' cache of engine plans, pinned against its rule rather than against what the code happens to keep: the key is
(B, T, Rv, train, fp8, task_id, maps); a miss first drops every cached plan with the same train, task_id and maps (one plan per mode,
task head and map-keeping keeps memory bounded), then builds; every engine forward -- encode() included -- advances `_step` by one and
leaves (engine, tensors) in `_last`.  GPU only."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

A, B_ = "TASK1", "TASK13"
TASK_CFG = {A: {"type": "VL-classifier", "num_labels": 3129}, B_: {"type": "VL-tri-classifier"}}


def test_engine_cache_keys_eviction_step_counter_and_last():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_engine_gpu import CONFIGS
    from volta_amd.config import BertConfig
    from volta_amd.modeling import BertForVLTasks
    cfg = BertConfig.from_dict(dict(CONFIGS["gated"], clf_hidden_size=1536, visualization=True))
    model = BertForVLTasks(cfg, TASK_CFG, [A, B_]).cuda().eval()
    B, Rv = 2, 5
    g = torch.Generator().manual_seed(3)

    def inputs(T):
        return (torch.randint(0, cfg.vocab_size, (B, T), generator=g).cuda(), torch.randn(B, Rv, cfg.v_feature_size, generator=g).cuda(),
                torch.rand(B, Rv, cfg.num_locs, generator=g).cuda())

    def check(call, key, keys):
        step = model._step
        out = call()
        assert set(model._engines) == keys
        assert model._step == step + 1
        assert model._last[0] is model._engines[key]
        return out

    k1 = (B, 8, Rv, False, False, A, False)
    k2 = (B, 8, Rv, False, False, B_, False)
    k3 = (B, 9, Rv, False, False, A, False)
    k4 = (B, 8, Rv, False, False, None, False)
    k5 = (B, 8, Rv, False, False, A, True)
    assert model._engines == {} and model._step == 0 and model._last is None
    x8, x9 = inputs(8), inputs(9)
    check(lambda: model(*x8, A), k1, {k1})
    check(lambda: model(*x8, B_), k2, {k1, k2})                  # another task head: nothing to drop
    check(lambda: model(*x9, A), k3, {k2, k3})                   # same mode, task and maps at another shape: k1 goes
    check(lambda: model.encode(*x8), k4, {k2, k3, k4})           # no task head: a plan of its own
    out = check(lambda: model(*x8, A, output_all_attention_masks=True), k5, {k2, k3, k4, k5})       # kept maps: a plan of its own
    assert len(out[3][0]) == 1 and out[3][0][0] is not None      # the one attention sub-layer's maps came back
    check(lambda: model(*x9, A), k3, {k2, k3, k4, k5})           # a hit changes nothing
