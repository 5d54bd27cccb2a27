"""The standalone BertModel without a GPU: its parameter names and shapes are the reference's `bert.*` state_dict with the prefix
stripped, it refuses CPU execution, it is a root model only while no root model holds it, and the new C-ABI structs match the header."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _configs():
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_engine_gpu import CONFIGS
    return CONFIGS


@pytest.mark.parametrize("name", ["vilbert", "lxmert", "uniter", "visualbert", "vlbert"])
def test_state_dict_is_the_references_bert_subset(name):
    from oracle import volta_ref as R
    from volta_amd.config import BertConfig
    from volta_amd.modeling import BertModel
    cd = _configs()[name]
    rcfg = R.RefConfig(cd)
    want = {k[len("bert."):]: tuple(v) for k, v in R.param_shapes(rcfg).items() if k.startswith("bert.")}
    want.update({k[len("bert."):]: want[t[len("bert."):]] for k, t in R.param_aliases(rcfg).items() if k.startswith("bert.")})
    got = {k: tuple(v.shape) for k, v in BertModel(BertConfig.from_dict(cd)).state_dict().items()}
    assert got == want


def test_standalone_is_a_root_model_and_refuses_cpu_execution():
    from volta_amd.config import BertConfig
    from volta_amd.modeling import ArenaParameters, BertForVLPreTraining, BertModel
    cfg = BertConfig.from_dict(_configs()["gated"])
    bm = BertModel(cfg)
    assert isinstance(bm.parameters(), ArenaParameters) and bm.parameters().vk_model is bm
    assert all(p._vk_owner is bm for p in bm.parameters())
    assert "_vk_is_model" in bm.__dict__ and not getattr(BertModel, "_vk_is_model", False)     # the instance is the model, not the class
    with pytest.raises(RuntimeError, match="MI355X"):
        bm.materialize()
    ids = torch.zeros(2, 8, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        bm(ids, torch.zeros(2, 5, cfg.v_feature_size), torch.zeros(2, 5, cfg.num_locs))
    root = BertForVLPreTraining(cfg)
    assert "_vk_is_model" not in root.bert.__dict__ and not isinstance(root.bert.parameters(), ArenaParameters)
    assert all(p._vk_owner is root for p in root.parameters())


def test_plumbing_and_root_state_live_in_one_host_layer():
    """The engine plumbing resolves through the MRO to the one base class, for each of the three root models, and a constructed root
    model carries the whole root state while the BertModel nested in it carries none of it."""
    from volta_amd.config import BertConfig
    from volta_amd.modeling import BertForVLPreTraining, BertForVLTasks, BertModel, EngineHostModel
    plumbing = ("materialize", "set_dropout_seed", "set_projection_dtype", "_engine", "_prep_inputs", "_engine_forward", "_backward_begin",
                "_backward_run", "_run_step", "_init_root_state", "_adopt", "encode")
    state = {"_vk_is_model", "_arena", "_engines", "_step", "_seed_base", "_last", "_ddp", "_fwd_serial", "_fp8", "_task_dropout"}
    assert set(EngineHostModel._ROOT_STATE) == state
    cfg = BertConfig.from_dict(dict(_configs()["gated"], clf_hidden_size=256))
    for cls in (BertModel, BertForVLPreTraining, BertForVLTasks):
        assert issubclass(cls, EngineHostModel)
        for name in plumbing:
            assert name not in cls.__dict__, (cls.__name__, name)
            assert getattr(cls, name) is EngineHostModel.__dict__[name], (cls.__name__, name)
        assert not getattr(cls, "_vk_is_model", False)
    roots = [BertModel(cfg), BertForVLPreTraining(cfg), BertForVLTasks(cfg, {"TASK1": {"type": "VL-classifier", "num_labels": 5}}, ["TASK1"], dropout_prob=0.25)]
    for root in roots:
        assert state <= set(root.__dict__) and "_root" not in root.__dict__
        assert (root._arena, root._engines, root._step, root._seed_base, root._last, root._ddp, root._fwd_serial, root._fp8) == (None, {}, 0, None, None, None, 0, False)
        assert "_ddp" not in root._modules
        if root is not roots[0]:
            assert not state & set(root.bert.__dict__) and root.bert.__dict__["_root"] is root and "_root" not in root.bert._modules
    assert roots[0]._engines is not roots[1]._engines
    assert [r._task_dropout for r in roots] == [0.1, 0.1, 0.25]


def test_from_pretrained_strips_the_bert_prefix(tmp_path):
    from volta_amd.config import BertConfig
    from volta_amd.modeling import BertForVLTasks, BertModel
    cfg = BertConfig.from_dict(dict(_configs()["gated"], clf_hidden_size=256))
    tm = BertForVLTasks(cfg, {"TASK1": {"type": "VL-classifier", "num_labels": 5}}, ["TASK1"])
    with torch.no_grad():
        tm.bert.t_pooler.dense.weight.normal_()
    tm.save_pretrained(str(tmp_path))
    bm, info = BertModel.from_pretrained(str(tmp_path), config=cfg, output_loading_info=True)
    assert info["missing_keys"] == [] and info["unexpected_keys"] == []
    assert torch.equal(bm.t_pooler.dense.weight, tm.bert.t_pooler.dense.weight)
    assert not bm.training


def test_mixed_parameter_sets_are_checked_on_the_host():
    from volta_amd.config import BertConfig
    from volta_amd.modeling import BertModel
    from volta_amd.optimization import _split_params
    cfg = BertConfig.from_dict(_configs()["gated"])
    a, b = BertModel(cfg), BertModel(cfg)
    with pytest.raises(RuntimeError, match="different models"):
        _split_params([next(iter(a.parameters())), next(iter(b.parameters()))])
    with pytest.raises(RuntimeError, match="head.weight is not a contiguous CUDA float32 tensor"):
        _split_params([nn.Parameter(torch.zeros(3))], ["head.weight"])


def test_new_struct_layouts_match_the_header():
    from volta_amd import _lib as L
    pairs = {"vk_adamw_tensor": L.AdamwTensor, "vk_grad_seed_args": L.GradSeedArgs}
    src = '#include <stdio.h>\n#include "volta_hip.h"\nint main(void){' + "".join(
        'printf("%s %%zu\\n", sizeof(%s));' % (n, n) for n in pairs) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = subprocess.check_output([exe]).decode().split()
    sizes = dict(zip(out[0::2], map(int, out[1::2])))
    for name, cls in pairs.items():
        assert ctypes.sizeof(cls) == sizes[name], (name, ctypes.sizeof(cls), sizes[name])
    assert L.lib.vk_grad_sqnorm_list_work_floats() > 0
