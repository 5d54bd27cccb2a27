"""Schedule independence of the step engine: every legal schedule of a command list gives the bits of the serial schedule.

The plan builder moves parts of the two command lists onto the executor's side stream by hand; what orders the two streams is the events
named at the top of volta_amd/engine/plan.py and hand-kept rules about who may share a scratch buffer.  The serial schedule
(vk_side_enable(0): control ops skipped, every block inline, in list order) is the reference.  tests/sched_perturb.py forces the
adversarial schedule: a bounded hold (vk_hold_cus, one wave, `hold_us`) opens every side block, so each block S runs AFTER the main-stream
launches M between its fork and its wait, where the serial order is S, then M.  A read of S's output, a store over S's input or a scratch
buffer shared by the two changes the result; the kernels are deterministic, so anything but equal bits is a missing edge.

Engine lists.  Per case, on one model and one cached engine, three replays of two steps -- batch A, then batch B (other token
ids, features, labels and dropout seed; A exists so that every engine buffer holds valid but DIFFERENT data when B starts: with
identical steps a stale read returns the right value).  Replay 1: A and B serial.  Replay 2: A serial, B with `late_side` on both lists.
Replay 3: A serial, B with the side stream on and nothing perturbed (natural timing).  After B: the whole gradient arena and every tap as
raw bits, the losses to 1e-5 relative (fp32 atomics in arrival order; no gradient reads them).  hold_us = 2 x the serial B step, measured
with two events around forward + backward (small-launch times vary by well under a factor of 2 from run to run); more than the
100 000 us vk_hold_cus accepts fails the test, nothing is clamped.  Every perturbed step must take at least 0.9 x holds x hold_us:
the side stream runs its blocks one after the other, so the holds add up -- unless they were skipped.
The stream the cases run on is one whose side stream shares no hardware queue with it (volta_amd/streams.py: two HIP streams on one queue
run in enqueue order; a hold on the side stream would then stall the main stream and prove nothing).
The census test pins that the cases' lists record and wait for every event of plan.py and all 8 ring slots, one slot twice in one list.
Two sensitivity cases remove one wait that is the only edge between its block and the main stream (EV_IMAGE_EMB_FWD from ViLBERT's
forward list, EV_DECODER_WGRAD from the `gated` backward list) and must then SEE a difference, confined to what that wait guards.

Pipelined AdamW.  tests/test_optim_gpu.py::test_pipelined_adamw_under_the_next_forward_changes_nothing with the optimizer's
stream held back by 2 x (forward + backward) before every step from the second on, alone and together with `late_side` lists.

Seen on the MI355X (B = 4, T = 20, 36 regions + the global one; three runs of the file, GPU_MAX_HW_QUEUES=4):
  stream    the current (default) stream and its side stream shared no queue in any of the runs: candidate 0 was kept every time
  case                    serial step us   hold_us       holds fwd + bwd   perturbed step us (holds x hold_us)   natural step us
  vilbert                 1642 - 1839      3284 - 3679    2 + 11           43756 (42692)                          1554 - 1849
  lxmert                  1538 - 2520      3076 - 5041    1 + 9            31769 (30760)                          1485 - 1590
  uniter / visualbert     1152 - 1878      2305 - 3757    1 + 6            16924 (16135)                          1105 - 1712
  vlbert                  1288 - 1769      2576 - 3538    1 + 6            18842 (18032)                          1244 - 1481
  gated / bigvocab         826 - 1004      1653 - 2009    1 + 4             8854 (8265)                            765 - 1051
  deep                    1215 - 1387      2430 - 2775    2 + 15           42426 (41310)                          1261 - 1894
  frozen-alternate        1586 - 1591      3173 - 3182    2 + 7            29615 (28557)                          1498 - 2435
  frozen-embeddings       1516 - 1901      3032 - 3802    2 + 10           37380 (36384)                          1460 - 1520
  frozen-decoder          1646 - 2091      3292 - 4182    2 + 11           43935 (42887)                          1550 - 1571
  frozen-image_embedding  1605 - 1612      3211 - 3224    2 + 10           39667 (38664)                          1534 - 1574
  lora                    2388 - 2395      4777 - 4791    2 + 1            16523 (14331)                          2403 - 2422
  tasks                   1516 - 1733      3033 - 3466    1 + 9            31356 (30330)                          1480 - 1543
  backbone                2590 - 2693      5181 - 5386    1 + 9            53392 (51810)                          2323 - 2665
  every case: gradient arena, taps and outputs of the perturbed and of the natural replay bit-equal to the serial one.
  sensitivity  ViLBERT without the wait for EV_IMAGE_EMB_FWD: 124 parameters' gradients and the taps t2-t7, v2-v7, seq_*, pooled_* differ
               (emb_t, emb_v, t0, t1, v0, v1 do not); `gated` without the wait for EV_DECODER_WGRAD: the word table's gradient and nothing else.
  census       recorded and waited for: 0-7, 11, 12, 13, 14, 15; `deep` records ring slots 0-3 twice.
  AdamW        forward + backward 1952 us, hold_us 3904; the loop of 4 steps: 15 ms plain, 75 ms with the late optimizer, 432 ms with the late
               optimizer and 13 late side blocks per step; master weights, both moments and the bf16 copies bit-equal in both.
  the file     19 tests in 12.3 s; the slowest is the AdamW test (3.5 s: three models), every other test takes 0.1 - 0.8 s.
"""
import ctypes as C
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sched_perturb as SP  # noqa: E402

SHAPE = (4, 20, 36)
BATCH_SEED = {"A": 7, "B": 9}                      # tests/test_engine_gpu.py: both leave B = 4 with labelled rows
DROP_SEED = {"A": 0x5EED1234, "B": 0xABCDEF12345}
LOSS_RTOL = 1e-5

# Depth, not width: 12 sub-layers, so that ring slots 0-3 are recorded twice in one backward list (sub-layers k and k + 8 share an event);
# the smallest widths the engine takes (64-wide heads), ViLBERT embeddings with a late vision stream (image-embedding blocks).
DEEP = dict(hidden_size=128, num_attention_heads=2, intermediate_size=512, pooler_size=128, v_hidden_size=128, v_num_attention_heads=2,
            v_intermediate_size=512, v_pooler_size=128, image_embeddings="vilbert", tt_attn_sublayers=[0, 2, 4, 8, 10],
            t_ff_sublayers=[1, 3, 5, 7, 9, 11], tv_attn_sublayers=[6], vt_attn_sublayers=[6], vv_attn_sublayers=[10], v_ff_sublayers=[7, 11])
LORA = dict(r=8, alpha=16, targets=("query", "key", "value", "attn_out", "ffn_up", "ffn_down"), dropout=0.1)
WORD = "bert.embeddings.word_embeddings.weight"
FROZEN = {        # arena name -> frozen?
    "alternate": lambda n: n.startswith(tuple("bert.encoder.layer.%d." % k for k in (1, 3, 5, 7))),      # ring events vanish, their neighbours stay
    "embeddings": lambda n: n.startswith(("bert.embeddings.", "bert.v_embeddings.")),      # word table frozen, still written with the decoder bias
    "decoder": lambda n: n in (WORD, "cls.predictions.bias"),        # the tied decoder's block alone: the word gradient's zero-fill branch (heads.py)
    "image_embedding": lambda n: n.startswith("bert.v_embeddings."),                        # no image-embedding block in the backward list
}


def _lib():
    from volta_amd import _lib as L
    return L


# ------------------------------------------------------------------------------------------------ the cases
class Case:
    """One model and what a training step on it is.  step(which) issues forward + backward of batch `which` ("A" / "B") on the current
    stream without a host synchronisation and returns what the step hands back (losses or outputs, detached copies)."""

    def __init__(self, model, step, loss_like):
        self.model, self.step, self.loss_like = model, step, loss_like      # loss_like: the outputs are loss sums (atomics): 1e-5, else bits
        self.arena = model.materialize()

    def engine(self):
        return self.model._last[0]


def _batches(rcfg):
    from oracle import volta_ref as R
    return {w: {k: v.cuda() for k, v in R.synthetic_batch(rcfg, *SHAPE, seed=s, pad=True).items()} for w, s in BATCH_SEED.items()}


def _begin(model, which):
    model.set_dropout_seed(DROP_SEED[which])
    for p in model.parameters():
        p.grad = None


def _pretrain_case(model, rcfg):
    cbs = _batches(rcfg)
    args = {w: (cb["input_ids"], cb["image_feat"], cb["image_loc"], cb["segment_ids"], cb["input_mask"], cb["image_mask"], cb["lm_label_ids"],
                cb["image_label"], cb["image_cls"], None, None, None, None, None, cb["is_match"]) for w, cb in cbs.items()}
    model.train()

    def step(which):
        _begin(model, which)
        out = model(*args[which])
        sum(out).sum().backward()
        return [x.detach().clone() for x in out]
    return Case(model, step, True)


def _config_case(name):
    from test_engine_gpu import build
    model, rcfg, _ = build(name)
    return _pretrain_case(model, rcfg)


def _deep_case():
    from test_engine_gpu import BASE
    from oracle import volta_ref as R
    from volta_amd.config import BertConfig
    from volta_amd.modeling import BertForVLPreTraining
    cd = dict(BASE, **DEEP)
    rcfg = R.RefConfig(cd)
    model = BertForVLPreTraining(BertConfig.from_dict(cd))
    model.load_state_dict(R.make_weights(rcfg, seed=2, std=0.04), strict=True)
    return _pretrain_case(model.cuda(), rcfg)


def _frozen_case(pattern):
    case = _config_case("vilbert")
    hit = 0
    for n, p in case.arena.param_list():
        if FROZEN[pattern](n):
            p.requires_grad_(False)
            hit += 1
    assert hit
    return case


def _lora_case():
    import test_lora_gpu as TL
    from volta_amd import lora
    model, rcfg, _, _, _ = TL._pretrain("vilbert", LORA)
    TL._randomise_B(model)
    lora.mark_only_lora_trainable(model)              # the base frozen, heads included
    return _pretrain_case(model, rcfg)


def _probes(shapes):
    gen = torch.Generator().manual_seed(5)
    return {w: [torch.randn(s, generator=gen).cuda() for s in shapes] for w in ("A", "B")}


def _tasks_case():
    import test_frozen_backward_gpu as FB
    from test_engine_gpu import CONFIGS
    from test_tasks_gpu import TASK_CFG
    from oracle import volta_ref as R
    model, _ = FB._tasks("vilbert", "TASK1")          # a BertForVLTasks in training mode (_heads_tasks); its closure's batch is not used
    cbs = _batches(R.RefConfig(dict(CONFIGS["vilbert"], clf_hidden_size=1536)))
    probes = _probes([(SHAPE[0], TASK_CFG["TASK1"]["num_labels"])])

    def step(which):
        _begin(model, which)
        cb = cbs[which]
        pred = model(cb["input_ids"], cb["image_feat"], cb["image_loc"], "TASK1", cb["segment_ids"], cb["input_mask"], cb["image_mask"])[0]
        assert pred.shape == probes[which][0].shape
        (pred * probes[which][0]).sum().backward()
        return [pred.detach().clone()]
    return Case(model, step, False)


def _backbone_case():
    import test_backbone_gpu as BB
    from volta_amd.modules import sublayer_schedule
    bert, rcfg, _, cd = BB._setup("vilbert")
    bert.train()
    cbs = _batches(rcfg)
    B, T, Rv = cbs["B"]["input_ids"].shape + cbs["B"]["image_feat"].shape[1:2]          # (the batch adds the global image feature to SHAPE's regions)
    n_sub = len(list(sublayer_schedule(bert.config)))
    probes = _probes([(B, T, cd["hidden_size"])] * n_sub + [(B, Rv, cd["v_hidden_size"])] * n_sub + [(B, cd["pooler_size"]), (B, cd["v_pooler_size"])])

    def step(which):
        _begin(bert, which)
        seq_t, seq_v, pt, pv, _ = BB._call(bert, cbs[which], output_all_encoded_layers=True)        # every state's gradient enters the backward list
        entries = list(seq_t) + list(seq_v) + [pt, pv]
        assert len(entries) == len(probes[which])
        sum((e * p).sum() for e, p in zip(entries, probes[which])).backward()
        return [e.detach().clone() for e in entries]
    return Case(bert, step, False)


def _named(fn, *a):
    return functools.partial(fn, *a)


CASES = {}
for _name in ("vilbert", "lxmert", "uniter", "visualbert", "vlbert", "gated", "bigvocab"):      # test_engine_gpu.CONFIGS, training mode
    CASES[_name] = _named(_config_case, _name)
CASES["deep"] = _deep_case
for _name in FROZEN:
    CASES["frozen-" + _name] = _named(_frozen_case, _name)
CASES.update({"lora": _lora_case, "tasks": _tasks_case, "backbone": _backbone_case})


@functools.lru_cache(maxsize=1)
def built(name):
    """The case's model, kept until another case is asked for (the sensitivity cases and the `vilbert` case share one)."""
    case = CASES[name]()
    torch.cuda.synchronize()
    return case


# ------------------------------------------------------------------------------------------------ a stream whose side stream runs beside it
def _independent(a, b):
    from volta_amd import streams
    return not streams.shares_queue(a, b) and not streams.shares_queue(b, a)


@pytest.fixture(scope="module")
def compute_stream():
    """The first of (the current stream, up to 8 new torch streams) whose executor side stream (vk_side_stream) shares no hardware queue
    with it, in either direction.  None found is a failure: on a shared queue the perturbation does not perturb."""
    from volta_amd import _lib as L
    tried = []
    for i, s in enumerate([torch.cuda.current_stream()] + [torch.cuda.Stream() for _ in range(8)]):
        side = L.lib.vk_side_stream(C.c_void_p(s.cuda_stream))
        assert side, "the executor opened no side stream"
        ok = _independent(s, int(side))
        tried.append(ok)
        if ok:
            print("\ncompute stream: candidate %d (%s) runs beside its side stream; candidates before it shared a queue: %d; GPU_MAX_HW_QUEUES=%s"
                  % (i, "the current stream" if i == 0 else "a new torch stream", i, os.environ.get("GPU_MAX_HW_QUEUES", "unset")))
            return s
    pytest.fail("no stream among %d candidates whose side stream runs on another hardware queue (GPU_MAX_HW_QUEUES=%s): a hold on the side "
                "stream would stall the main stream, and the perturbed schedule would be the serial one" % (len(tried), os.environ.get("GPU_MAX_HW_QUEUES", "unset")))


# ------------------------------------------------------------------------------------------------ the protocol
def _bits(t):
    t = t.detach().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _timed(fn, *a):
    """fn(*a) between two events on the current stream: (its result, a callable giving the microseconds once the stream got there)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn(*a)
    e1.record()

    def us():
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0
    return out, us


def _snapshot(case, outs):
    eng = case.engine()
    snap = dict(grad=case.arena.grad.clone(), taps={k: t.clone() for k, t in eng.taps.items() if t is not None}, outs=outs)
    torch.cuda.synchronize()
    return snap


def _replay(case, mode, hold_us=None, mutate=None):
    """Step A serial, then step B under `mode`: "serial", "natural" (side stream on, lists as built) or "late" (`late_side` on both lists,
    behind `mutate(fwd_ops, bwd_ops)` where a sensitivity case removes a wait).  -> (snapshot after B, B's microseconds, holds per list)."""
    with SP.serial():
        case.step("A")
    eng = case.engine()
    holds = (0, 0)
    if mode == "serial":
        with SP.serial():
            outs, us = _timed(case.step, "B")
    elif mode == "natural":
        outs, us = _timed(case.step, "B")
    else:
        f, b = eng.fwd.ops, eng.bwd.ops
        if mutate is not None:
            f, b = mutate(f, b)
        f, b = SP.late_side(f, hold_us), SP.late_side(b, hold_us)
        holds = (SP.count_holds(f), SP.count_holds(b))
        with SP.perturbed(eng, f, b):
            outs, us = _timed(case.step, "B")
    assert case.engine() is eng, "step B ran on another plan than step A"
    return _snapshot(case, outs), us(), holds


def _diff(case, ref, got):
    """What differs between two snapshots: (parameters whose gradient bits differ, gradient words that differ outside every parameter, taps
    that differ, outputs that differ -- loss-like outputs beyond 1e-5 relative)."""
    arena = case.arena
    params = []
    covered = torch.zeros(arena.grad.numel(), dtype=torch.bool, device=arena.grad.device)
    for n in arena.params:
        off, numel = arena.offset[n], arena.view(n, "grad").numel()
        covered[off:off + numel] = True
        if not torch.equal(_bits(ref["grad"][off:off + numel]), _bits(got["grad"][off:off + numel])):
            params.append(n)
    stray = int(((_bits(ref["grad"]) != _bits(got["grad"])) & ~covered).sum())
    taps = sorted(k for k in ref["taps"] if not _same_bits(ref["taps"][k], got["taps"][k]))
    assert set(ref["taps"]) == set(got["taps"])
    outs = []
    for i, (a, b) in enumerate(zip(ref["outs"], got["outs"])):
        if case.loss_like:
            a, b = float(a), float(b)
            if not (abs(a - b) <= LOSS_RTOL * abs(a) or (a != a and b != b)):
                outs.append((i, a, b))
        elif not _same_bits(a, b):
            outs.append(i)
    return dict(params=params, stray=stray, taps=taps, outs=outs)


def _clean(d):
    return not (d["params"] or d["stray"] or d["taps"] or d["outs"])


def _hold_us(serial_us):
    hold_us = int(2 * serial_us) + 1
    assert hold_us <= SP.HOLD_MAX_US, "the serial step takes %.0f us: 2 x that is more than vk_hold_cus holds for; the shape is too large for this test" % serial_us
    return hold_us


def _events_of(case):
    eng = case.engine()
    return [SP.events(eng.fwd.ops), SP.events(eng.bwd.ops)], [[o[0] for o in ops] for ops in (eng.fwd.ops, eng.bwd.ops)]


_CENSUS = {}


def _run_case(name, stream):
    """The three replays of one case; returns what the tests assert on and files the case's events for the census."""
    case = built(name)
    with torch.cuda.stream(stream):
        ref, serial_us, _ = _replay(case, "serial")
        hold_us = _hold_us(serial_us)
        late, late_us, holds = _replay(case, "late", hold_us)
        natural, natural_us, _ = _replay(case, "natural")
        torch.cuda.synchronize()
    _CENSUS[name] = _events_of(case)
    print("\n%s: serial step %.0f us, hold_us %d, holds %d forward + %d backward, perturbed step %.0f us (holds x hold_us = %d), natural step %.0f us"
          % (name, serial_us, hold_us, holds[0], holds[1], late_us, sum(holds) * hold_us, natural_us))
    return dict(case=case, ref=ref, late=late, natural=natural, late_us=late_us, hold_us=hold_us, holds=holds)


# ------------------------------------------------------------------------------------------------ sensitivity: a missing edge must show
def _sensitivity(stream, name, event, which_list):
    """Case `name` with the wait for `event` taken out of one list, `late_side` on both, against the serial bits.  The wait must be the only
    edge between its side block and the main stream (SP.implied_by): where a later wait covers it, no schedule shows that it is gone."""
    L = _lib()
    case = built(name)
    drop = lambda f, b: (SP.without_wait(f, event), b) if which_list == "fwd" else (f, SP.without_wait(b, event))
    with torch.cuda.stream(stream):
        ref, serial_us, _ = _replay(case, "serial")
        hold_us = _hold_us(serial_us)
        eng = case.engine()
        ops = eng.fwd.ops if which_list == "fwd" else eng.bwd.ops
        assert SP.implied_by(ops, event) is None, "%s: op %d waits for a block behind event %d's: its own wait is redundant here" % (name, SP.implied_by(ops, event), event)
        got, us, holds = _replay(case, "late", hold_us, mutate=drop)
        torch.cuda.synchronize()
    assert (eng.fwd.ops if which_list == "fwd" else eng.bwd.ops) is ops
    assert sum(o[0] == L.OP_WAIT_SIDE and o[1] == event for o in ops) == 1            # the wait is back, and it was the only one of its event
    assert us >= 0.9 * sum(holds) * hold_us, (us, holds, hold_us)
    d = _diff(case, ref, got)
    print("\n%s without the wait for event %d: %d parameters' gradients differ, taps that differ: %s" % (name, event, len(d["params"]), d["taps"]))
    return case, d


def test_removing_the_wait_for_the_image_embedding_shows_in_taps_and_gradients(compute_stream):
    """EV_IMAGE_EMB_FWD (forward list): without it the first vision sub-layer reads batch A's image embedding."""
    from volta_amd.engine.plan import EV_IMAGE_EMB_FWD
    case, d = _sensitivity(compute_stream, "vilbert", EV_IMAGE_EMB_FWD, "fwd")
    eng = case.engine()
    assert "emb_v" not in d["taps"] and "emb_t" not in d["taps"]              # the embedding itself arrives, late
    vision = {"v%d" % n for n in eng.sublayer_ids if eng.taps["v%d" % n].data_ptr() != eng.taps["emb_v"].data_ptr()}      # states behind the first vision sub-layer
    assert vision and vision <= set(d["taps"]), (sorted(vision), d["taps"])
    assert d["params"], "no gradient noticed the stale image embedding"


# ------------------------------------------------------------------------------------------------ every case: late side blocks change nothing
@pytest.mark.parametrize("name", list(CASES))
def test_late_side_blocks_give_the_serial_bits(name, compute_stream):
    r = _run_case(name, compute_stream)
    case, holds, hold_us = r["case"], r["holds"], r["hold_us"]
    begins = [sum(k == _lib().OP_SIDE_BEGIN for k in kinds) for kinds in _CENSUS[name][1]]
    assert list(holds) == begins and sum(holds) >= 2, (holds, begins)
    assert r["late_us"] >= 0.9 * sum(holds) * hold_us, "the holds did not run: %.0f us for %d holds of %d us" % (r["late_us"], sum(holds), hold_us)
    assert bool(r["ref"]["grad"].any()) and r["ref"]["taps"]
    late, natural = _diff(case, r["ref"], r["late"]), _diff(case, r["ref"], r["natural"])
    assert _clean(late), ("late side blocks against the serial schedule", name, late["params"][:8], len(late["params"]), late["stray"], late["taps"], late["outs"])
    assert _clean(natural), ("natural timing against the serial schedule", name, natural["params"][:8], len(natural["params"]), natural["stray"], natural["taps"],
                             natural["outs"])


def test_removing_the_wait_for_the_decoder_weight_gradient_shows_in_the_word_table_alone(compute_stream):
    """EV_DECODER_WGRAD (backward list): without it the text tables' backward adds into the word table's gradient before the tied decoder's
    weight gradient stores over it.  Nothing else may change: the damage is confined to what the edge guards.
    On the `gated` lists, not ViLBERT's: there the backward of sub-layer 5 waits for the weight-gradient block of sub-layer 7, which the
    one side stream runs behind the heads' block, so the main stream is behind EV_DECODER_WGRAD long before the text tables' backward
    whether or not it waits for it (SP.implied_by finds that wait; seen on the MI355X: ViLBERT without the wait, late side blocks,
    0 parameters differ).  `gated` has two sub-layers and no ring wait: the wait for EV_DECODER_WGRAD is the only edge."""
    from volta_amd.engine.plan import EV_DECODER_WGRAD
    _, d = _sensitivity(compute_stream, "gated", EV_DECODER_WGRAD, "bwd")
    assert d["params"] == [WORD], d["params"]
    assert not d["taps"] and not d["stray"] and not d["outs"], d


def test_census_every_event_is_recorded_and_waited_for_in_some_case(compute_stream):
    """Over the lists of all cases: every EV_* constant of plan.py and all 8 ring slots are recorded and are waited for (EV_IMAGE_EMB_BWD
    by the OP_JOIN that ends its list, as plan.py says); one list records a ring slot twice.  An event added to plan.py without a case
    here fails this test."""
    from volta_amd.engine import plan
    L = _lib()
    for name in CASES:
        if name not in _CENSUS:
            _run_case(name, compute_stream)
    named = {k: v for k, v in vars(plan).items() if k.startswith("EV_") and k != "EV_WGRAD_RING"}
    assert len(named) >= 5 and plan.EV_WGRAD_RING == 8
    want = set(named.values()) | set(range(plan.EV_WGRAD_RING))
    recorded, waited, twice = set(), set(), []
    for name, (evs, kinds) in _CENSUS.items():
        for (rec, wt), kk in zip(evs, kinds):
            recorded |= set(rec)
            waited |= wt
            if rec and kk[-1] == L.OP_JOIN:          # the final join waits for everything the list's side blocks recorded
                waited |= {e for e in rec if e == plan.EV_IMAGE_EMB_BWD}
            dup = sorted({e for e in rec if e < plan.EV_WGRAD_RING and rec.count(e) > 1})
            if dup:
                twice.append((name, dup))
    assert recorded >= want, ("never recorded", sorted(want - recorded))
    assert waited >= want, ("never waited for", sorted(want - waited))
    assert twice, "no list records a ring slot twice"
    print("\ncensus: recorded %s, waited %s, ring slots recorded twice in one list: %s" % (sorted(recorded), sorted(waited), twice))


# ------------------------------------------------------------------------------------------------ pipelined AdamW, its stream late
STEPS = 4


def _optimizer_run(stream, overlap, hold_us=None, late_lists=False):
    """Four steps of ViLBERT with a deferred clip and AdamW, another batch each step, no host synchronisation inside the loop.  hold_us: from
    the second step on a hold on the optimizer's stream right before opt.step(); late_lists: from the second step on the engine's lists
    under `late_side` as well."""
    import test_optim_gpu as TO
    from volta_amd import _lib as L
    from volta_amd.optimization import AdamW, clip_grad_norm_
    model, rcfg, _ = TO._build("vilbert")
    model.train()
    model.set_dropout_seed(21)
    model.materialize()
    opt = AdamW([{"params": [p], "weight_decay": 0.01} for p in model.parameters()], lr=5e-3, overlap_with_forward=overlap, overlap_ranges=5)
    batches = [TO._args(rcfg, seed=s) for s in (7, 9, 11, 13)]
    torch.cuda.synchronize()
    losses, times, ctx, holds = [], [], None, 0
    with torch.cuda.stream(stream):
        t_all = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t_all[0].record()
        try:
            for i in range(STEPS):
                if late_lists and i == 1:
                    eng = model._last[0]
                    f, b = SP.late_side(eng.fwd.ops, hold_us), SP.late_side(eng.bwd.ops, hold_us)
                    holds = SP.count_holds(f) + SP.count_holds(b)
                    ctx = SP.perturbed(eng, f, b)
                    ctx.__enter__()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = model(*batches[i])
                sum(out).sum().backward()
                e1.record()
                times.append((e0, e1))
                clip_grad_norm_(model.parameters(), 5.0, defer_to_optimizer=True)
                if hold_us is not None and opt._fused is not None and "stream" in opt._fused:
                    L.check(L.lib.vk_hold_cus(1, hold_us, 0, C.c_void_p(opt._fused["stream"].cuda_stream)))
                opt.step()
                opt.zero_grad()
                losses.append([x.detach().clone() for x in out])
        finally:
            if ctx is not None:
                ctx.__exit__(None, None, None)
        if overlap:
            assert model._arena.opt_pending is not None          # the last step is still owed a wait: the overlap is real
        opt.synchronize()
        t_all[1].record()
        torch.cuda.synchronize()
        if overlap:
            assert _independent(stream, opt._fused["stream"]), "the optimizer's stream shares a hardware queue with the compute stream"
    return dict(losses=[[float(x) for x in l] for l in losses], master=model._arena.master.clone(), m=opt._fused["m"].clone(), v=opt._fused["v"].clone(),
                shadow=model._arena.shadow.clone(), loop_us=t_all[0].elapsed_time(t_all[1]) * 1000.0, holds=holds,
                step_us=max(a.elapsed_time(b) for a, b in times[1:]) * 1000.0)         # (the first step also builds the plan, on the host)


def test_pipelined_adamw_on_a_late_stream_changes_nothing(compute_stream):
    """Every range update lands after the main stream has gone on to zero_grad and the next forward: the forward must be held by its range
    events, and nothing the optimizer still reads (gradients, clip coefficient) may be rewritten under it.  Run 3 makes the engine's side
    blocks late at the same time; its pipelined forward cuts the perturbed list by the remapped index tables."""
    ref = _optimizer_run(compute_stream, False)
    hold_us = _hold_us(ref["step_us"])
    runs = {"late optimizer": _optimizer_run(compute_stream, True, hold_us), "late optimizer and late side blocks": _optimizer_run(compute_stream, True, hold_us, True)}
    print("\npipelined AdamW: forward + backward %.0f us, hold_us %d; loop of %d steps: %.0f us plain, %s" % (
        ref["step_us"], hold_us, STEPS, ref["loop_us"], ", ".join("%.0f us %s (%d list holds per step)" % (r["loop_us"], k, r["holds"]) for k, r in runs.items())))
    assert ref["losses"][0] != ref["losses"][-1]                      # the model did move
    for tag, r in runs.items():
        assert r["loop_us"] >= 0.9 * (STEPS - 1) * (1 + r["holds"]) * hold_us, (tag, "the holds did not run", r["loop_us"], hold_us, r["holds"])
        for l0, l1 in zip(ref["losses"], r["losses"]):
            assert all(abs(a - b) <= LOSS_RTOL * max(abs(a), 1.0) for a, b in zip(l0, l1)), (tag, ref["losses"], r["losses"])
        for key in ("master", "m", "v", "shadow"):
            assert _same_bits(ref[key], r[key]), (tag, key, int((_bits(ref[key]) != _bits(r[key])).sum()))
