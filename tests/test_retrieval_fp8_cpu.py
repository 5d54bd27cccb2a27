"""Host side of the retrieval scorer's e4m3 switch (volta_amd/retrieval.py, `projection_dtype`): which values are taken, which geometry is
refused and when (before the device check, so a model still on the CPU shows it), the score plan's own keyword, and the description of the
pair plan's gather segments for the reduced-depth configs of tests/test_engine_gpu.py in both precisions.  No GPU needed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TASK_CFG = {"TASK8": {"type": "VL-logit"}}
FAMILIES = ["vilbert", "lxmert", "uniter", "visualbert", "vlbert"]
# the geometry of config/vilbert_base.json on the reduced-depth vilbert schedule: a 1024-wide vision stream with 8 heads, and the
# co-attention sub-layer (2) projecting both streams to 1024 / 8 heads
WIDE = dict(v_hidden_size=1024, v_num_attention_heads=8, v_intermediate_size=1024, sublayer2attn_hidden_size={"2": 1024},
            sublayer2num_attention_heads={"2": 8})


def _tiny(name, **kw):
    from test_engine_gpu import CONFIGS
    from volta_amd.config import BertConfig
    return BertConfig.from_dict(dict(CONFIGS[name], clf_hidden_size=1536, **kw))


def test_projection_dtype_values():
    """Anything but None | "bf16" | "fp8" is a ValueError, raised for a model still on the CPU; the three values themselves get as far as
    the device check."""
    from volta_amd.modeling import BertForVLPreTraining
    from volta_amd.retrieval import RetrievalScorer
    pre = BertForVLPreTraining(_tiny("vilbert"))
    for bad in ("int8", "fp16", "", 8, True):
        with pytest.raises(ValueError, match="projection_dtype"):
            RetrievalScorer(pre, projection_dtype=bad)
    for good in (None, "bf16", "fp8"):
        with pytest.raises(ValueError, match="GPU"):
            RetrievalScorer(pre, projection_dtype=good)


def test_an_explicit_dtype_overrides_the_models_switch():
    """None refuses a model whose own switch is on fp8 and says what to pass; an explicit value is honoured whatever the switch says (the
    constructor then gets as far as the device check) and leaves the switch as it was."""
    from volta_amd.modeling import BertForVLPreTraining
    from volta_amd.retrieval import RetrievalScorer
    pre = BertForVLPreTraining(_tiny("vilbert"))
    pre.set_projection_dtype("fp8")
    with pytest.raises(NotImplementedError, match="pass projection_dtype='fp8' or 'bf16'"):
        RetrievalScorer(pre)
    for explicit in ("bf16", "fp8"):
        with pytest.raises(ValueError, match="GPU"):
            RetrievalScorer(pre, projection_dtype=explicit)
    assert pre._fp8 is True
    pre.set_projection_dtype("bf16")
    with pytest.raises(ValueError, match="GPU"):
        RetrievalScorer(pre, projection_dtype="fp8")
    assert pre._fp8 is False


def test_fp8_refuses_the_wide_geometry_before_the_device_check():
    from volta_amd.engine import wide_geometry
    from volta_amd.modeling import BertForVLTasks
    from volta_amd.retrieval import RetrievalScorer
    cfg = _tiny("vilbert", **WIDE)
    model = BertForVLTasks(cfg, TASK_CFG, list(TASK_CFG))                       # on the CPU
    with pytest.raises(NotImplementedError, match="768 text / 1024 vision"):
        RetrievalScorer(model, "TASK8", projection_dtype="fp8")
    for other in (None, "bf16"):                                                # bf16 scores this geometry: only the device is missing
        with pytest.raises(ValueError, match="GPU"):
            RetrievalScorer(model, "TASK8", projection_dtype=other)
    # the shipped wide config, and the shipped single-width ones
    from volta_amd.config import BertConfig
    load = lambda name: BertConfig.from_json_file(os.path.join(ROOT, "config", name + ".json"))
    what = wide_geometry(load("vilbert_base"))
    assert what is not None and "768 text / 1024 vision" in what and "per-sub-layer widths" in what
    for name in ("ctrl_vilbert_base", "ctrl_lxmert", "ctrl_uniter_base", "ctrl_visualbert_base", "ctrl_vl-bert_base"):
        assert wide_geometry(load(name)) is None, name
    for name in FAMILIES:
        assert wide_geometry(_tiny(name)) is None, name


def test_score_plans_take_their_precision_by_their_own_keyword():
    from volta_amd.engine import StepEngine
    from volta_amd.retrieval import split_plan
    cfg = _tiny("lxmert")
    for part in ("text", "image", "pair"):
        with pytest.raises(ValueError, match="projection_dtype"):
            StepEngine(cfg, None, 2, 20, 37, False, heads="score", part=part, split=split_plan(cfg), projection_dtype="int8")
    with pytest.raises(ValueError):                                             # the training plans' argument stays refused on a score plan
        StepEngine(cfg, None, 2, 20, 37, False, heads="score", part="text", split=split_plan(cfg), fp8=True, projection_dtype="fp8")
    with pytest.raises(ValueError, match="projection_dtype"):                   # and the score plans' keyword on a training plan
        StepEngine(cfg, None, 2, 20, 37, True, heads="pretrain", projection_dtype="fp8")


BF16_SEGS = {True: [("x_t", 0), ("x_v", 1), ("attention_mask", 0), ("image_attention_mask", 1)],
             False: [("input_ids", 0), ("token_type_ids", 0), ("image_feat", 1), ("image_loc", 1), ("attention_mask", 0), ("image_attention_mask", 1)]}


@pytest.mark.parametrize("dtype", [None, "bf16", "fp8"])
@pytest.mark.parametrize("name", FAMILIES)
def test_pair_gather_segments(name, dtype):
    """Never more than VK_PAIR_MAX_SEGS; the bf16 list is today's; under fp8 the e4m3 copy and its scales are listed for exactly the
    modalities whose prefix ends in a sub-layer (a non-empty split_plan list), behind the bf16 segments, each on its modality's side."""
    from volta_amd import _lib as L
    from volta_amd.retrieval import pair_gather_segments, split_plan
    cfg = _tiny(name)
    text, vision, per_modality = split_plan(cfg)
    segs = pair_gather_segments(cfg, dtype)
    assert len(segs) <= L.PAIR_MAX_SEGS and len(set(segs)) == len(segs)
    assert segs[:len(BF16_SEGS[per_modality])] == BF16_SEGS[per_modality]
    extra = segs[len(BF16_SEGS[per_modality]):]
    want = []
    if dtype == "fp8":
        want += [("x8_t", 0), ("xs_t", 0)] if text else []
        want += [("x8_v", 1), ("xs_v", 1)] if vision else []
    assert extra == want, (name, dtype, segs)


def test_pair_gather_segments_expectations_by_hand():
    """What the parametrised test derives from split_plan, written out: vilbert carries the text copy only (its vision prefix is the
    embedding), lxmert both (eight segments, the limit), uniter none (both prefixes are embeddings), visualbert / vlbert have no prefix."""
    from volta_amd import _lib as L
    from volta_amd.retrieval import pair_gather_segments
    names = lambda n: [s for s, _ in pair_gather_segments(_tiny(n), "fp8")][4:]
    assert names("vilbert") == ["x8_t", "xs_t"]
    assert names("lxmert") == ["x8_t", "xs_t", "x8_v", "xs_v"] and len(pair_gather_segments(_tiny("lxmert"), "fp8")) == L.PAIR_MAX_SEGS == 8
    assert names("uniter") == []
    for n in ("visualbert", "vlbert"):
        assert pair_gather_segments(_tiny(n), "fp8") == pair_gather_segments(_tiny(n), "bf16") == BF16_SEGS[False]
    with pytest.raises(ValueError):
        pair_gather_segments(_tiny("vilbert"), "int8")
