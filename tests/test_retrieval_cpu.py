"""Host side of the retrieval scorer (volta_amd/retrieval.py): the split plan against hand-written expectations for the five ctrl_* configs
and the reduced-depth configs of tests/test_engine_gpu.py, the scorer's refusals, and the vk_pair_gather ABI (struct layout, host-side
argument checks).  No GPU needed."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _cfg(name):
    from volta_amd.config import BertConfig
    return BertConfig.from_json_file(os.path.join(ROOT, "config", name + ".json"))


def _tiny(name, **kw):
    from test_engine_gpu import CONFIGS
    from volta_amd.config import BertConfig
    return BertConfig.from_dict(dict(CONFIGS[name], clf_hidden_size=1536, **kw))


@pytest.mark.parametrize("name,text,vision,per_modality", [
    ("ctrl_vilbert_base", list(range(12)), [], True),                           # 6 text-only layers, then co-attention at 12
    ("ctrl_lxmert", list(range(18)), list(range(10)), True),                    # 9 text layers, 5 vision layers, cross-attention at 18
    ("ctrl_uniter_base", [], [], True),                                         # single stream from sub-layer 0, per-modality embeddings
    ("ctrl_visualbert_base", [], [], False),                                    # the embedding mixes the modalities
    ("ctrl_vl-bert_base", [], [], False),
])
def test_split_plan_ctrl_configs(name, text, vision, per_modality):
    from volta_amd.retrieval import split_plan
    assert split_plan(_cfg(name)) == (text, vision, per_modality)


@pytest.mark.parametrize("name,text,vision,per_modality", [
    ("vilbert", [0, 1], [], True), ("lxmert", [0, 1, 2, 3], [0, 1], True), ("uniter", [], [], True),
    ("visualbert", [], [], False), ("vlbert", [], [], False), ("gated", [], [], True),
])
def test_split_plan_reduced_configs(name, text, vision, per_modality):
    from volta_amd.retrieval import split_plan
    assert split_plan(_tiny(name)) == (text, vision, per_modality)


def test_split_plan_without_cross_attention_is_all_prefix():
    """A config whose streams never meet: every sub-layer runs per item (the suffix is the poolers and the head)."""
    from volta_amd.retrieval import split_plan
    cfg = _tiny("vilbert", tv_attn_sublayers=[], vt_attn_sublayers=[], tt_attn_sublayers=[0, 2, 4, 6], vv_attn_sublayers=[2, 6])
    assert split_plan(cfg) == ([0, 1, 2, 3, 4, 5, 6, 7], [2, 3, 6, 7], True)


TASK_CFG = {"TASK8": {"type": "VL-logit"}, "TASK1": {"type": "VL-classifier", "num_labels": 7}, "TASK9": {"type": "V-logit"}}


def test_scorer_refuses_what_it_cannot_score():
    from volta_amd.modeling import BertForVLPreTraining, BertForVLTasks, BertModel
    from volta_amd.retrieval import RetrievalScorer
    cfg = _tiny("vilbert")
    tasks = BertForVLTasks(cfg, TASK_CFG, list(TASK_CFG))
    for tid in ("TASK1", "TASK9", "TASK404", None):            # other task types, unknown ids, no id
        with pytest.raises(ValueError):
            RetrievalScorer(tasks, tid)
    with pytest.raises(ValueError):
        RetrievalScorer(BertModel(cfg))                         # a backbone has no scoring head
    pre = BertForVLPreTraining(cfg)
    with pytest.raises(ValueError):
        RetrievalScorer(pre, "TASK8")                           # zero-shot takes no task id
    for fusion in ("none", "vl-bert_vqa"):                       # no ITM head (encoders.py:744-747)
        with pytest.raises(ValueError):
            RetrievalScorer(BertForVLPreTraining(_tiny("vilbert", fusion_method=fusion)))
    with pytest.raises(ValueError, match="GPU"):
        RetrievalScorer(tasks, "TASK8")                         # the model is still on the CPU
    with pytest.raises(ValueError):
        RetrievalScorer(pre, pair_chunk=0)
    pre.set_projection_dtype("fp8")
    with pytest.raises(NotImplementedError):
        RetrievalScorer(pre)


def test_score_plans_are_eval_forward_only():
    from volta_amd.engine import StepEngine
    from volta_amd.retrieval import split_plan
    cfg = _tiny("lxmert")
    for kw in (dict(train=True, part="pair"), dict(train=False, part="both"), dict(train=False, part="text", fp8=True)):
        with pytest.raises(ValueError):
            StepEngine(cfg, None, 2, 20, 37, kw.pop("train"), heads="score", split=split_plan(cfg), **kw)


def test_pair_gather_struct_layout_matches_the_header():
    from volta_amd import _lib as L
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "volta_hip.h"\nint main(void){printf("%zu %zu %zu %zu\\n", sizeof(vk_pair_gather_args), ' \
          'offsetof(vk_pair_gather_args, cap_idx), offsetof(vk_pair_gather_args, n_items), offsetof(vk_pair_gather_args, ni)); return 0;}'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = list(map(int, subprocess.check_output([exe]).decode().split()))
    A = L.PairGatherArgs
    assert got == [ctypes.sizeof(A), A.cap_idx.offset, A.n_items.offset, A.ni.offset]
    assert "vk_pair_gather" in L.EXPORTS and hasattr(L.lib, "vk_pair_gather")


def test_pair_gather_rejects_bad_arguments_on_the_host():
    """Every check happens before a launch: a cross product that leaves the encoded items, half an index pair, segments that are empty,
    misaligned or unknown."""
    from volta_amd import _lib as L
    buf = (ctypes.c_uint8 * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16

    def args(**kw):
        a = L.PairGatherArgs()
        a.src[0], a.dst[0], a.bytes[0], a.side[0] = base, base + 1024, 64, 0
        a.src[1], a.dst[1], a.bytes[1], a.side[1] = base + 256, base + 2048, 32, 1
        a.nseg, a.npairs, a.c0, a.nc, a.i0, a.ni = 2, 6, 0, 2, 0, 3
        a.n_items[0], a.n_items[1] = 2, 3
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(a, k)[v[0]] = v[1]
            else:
                setattr(a, k, v)
        return a

    bad = [dict(nseg=0), dict(nseg=9), dict(npairs=7), dict(c0=1), dict(i0=1), dict(ni=0), dict(cap_idx=base),
           dict(bytes=(0, 62)), dict(bytes=(1, 0)), dict(side=(1, 2)), dict(src=(0, base + 2)), dict(dst=(1, None)), dict(n_items=(1, 0))]
    for kw in bad:
        assert L.lib.vk_pair_gather(ctypes.byref(args(**kw)), None) != 0, kw
        assert L.lib.vk_last_error().startswith(b"vk_pair_gather"), kw
    # nothing to copy: accepted without a launch
    assert L.lib.vk_pair_gather(ctypes.byref(args(npairs=0)), None) == 0
