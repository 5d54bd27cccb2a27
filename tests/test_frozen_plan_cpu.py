"""The backward list of a plan built with frozen parameters (StepEngine(frozen=...)), checked on the CPU: plans build without a GPU,
as in tools/plan_signature.py, whose models, arenas and Renderer this module uses.

The tiny shape of that tool on each of the five families' pre-training plans, and on ViLBERT also a task plan and the backbone plan,
under seven frozen sets:
  a  both embeddings                                     e  one interior sub-layer only
  b  a + the sub-layers below the first cross-modal one  f  only the LayerNorm parameters of one sub-layer
  c  b + the first cross-modal sub-layer                 g  only `query` of one attention sub-layer
  d  every `bert.` parameter

A *block* is what the engine prunes as a whole ("Frozen parameters"); `blocks()` below restates the rule on its own.
One entry of the issue's list is mended here: "every wait_side(e) follows a side_end(e)" cannot be asked of the task and backbone
plans as it stands, because their text tables wait for EV_DECODER_WGRAD, which only the pre-training heads record, in the unpruned list
already.  The check exempts exactly the waits that dangle in the unpruned list of the same plan, so pruning may orphan none."""
import collections
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("plan_signature_frozen", os.path.join(ROOT, "tools", "plan_signature.py"))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)

PLANS = ["pretrain/%s/train-bf16" % f for f in S.FAMILIES] + ["tasks/vilbert/TASK1/train", "tasks/vilbert/TASK10/train", "backbone/vilbert/train"]
CASES = "abcdefg"


@pytest.fixture(scope="module")
def matrix():
    yield S.Matrix()


def build(matrix, pid, frozen=None):
    from volta_amd.engine import StepEngine
    _, key, kw = next(x for x in matrix.entries if x[0] == pid)
    cfg, arena = matrix.model(key)
    kw = dict(kw)
    extra = {} if frozen is None else dict(frozen=frozen)
    return StepEngine(cfg, arena, kw.pop("B"), kw.pop("T"), kw.pop("Rv"), kw.pop("train"), **kw, **extra)


def sublayers(cfg):
    from volta_amd.modules import sublayer_schedule
    return [n for n, _ in sublayer_schedule(cfg)]


def frozen_set(cfg, arena, case):
    names = list(arena.params)
    subs = sublayers(cfg)
    cross = set(cfg.tv_attn_sublayers) | set(cfg.vt_attn_sublayers)
    k_cross = next(k for k, n in enumerate(subs) if n in cross)
    under = lambda *pre: {n for n in names if n.startswith(pre)}
    layer = lambda n: under("bert.encoder.layer.%d." % n)
    emb = under("bert.embeddings.", "bert.v_embeddings.")
    attn = next(n for n in subs[1:] if any(".attention_self." in x for x in layer(n)))      # an interior attention sub-layer
    if case == "a":
        return emb
    if case == "b":
        return emb.union(*[layer(n) for n in subs[:k_cross]])
    if case == "c":
        return emb.union(*[layer(n) for n in subs[:k_cross + 1]])
    if case == "d":
        return under("bert.")
    if case == "e":
        return layer(subs[len(subs) // 2])
    if case == "f":
        return {n for n in layer(subs[len(subs) // 2]) if "LayerNorm" in n}
    if case == "g":
        return {n for n in layer(attn) if ".query." in n or ".v_query." in n}
    raise ValueError(case)


def blocks(arena, heads):
    """[[names]]: Linear = weight + bias; Q|K|V of one modality; LayerNorm = gamma + beta; one embedding prefix.  Pre-training heads: the
    tied decoder writes (word table, decoder bias) in one product, so the word table is left alone only if that pair is frozen too."""
    out = collections.OrderedDict()
    for n in arena.params:
        if n.startswith(("bert.embeddings.", "bert.v_embeddings.")):
            key = n.split("embeddings.")[0] + "embeddings."
        else:
            stem, leaf = n.rsplit(".", 1)
            mod = stem.rsplit(".", 1)
            key = mod[0] + "." + ("v_qkv" if mod[1].startswith("v_") else "qkv") if mod[1] in ("query", "key", "value", "v_query", "v_key", "v_value") else stem
        out.setdefault(key, []).append(n)
    return list(out.values())


def fully_frozen(arena, heads, frozen):
    """Names in blocks frozen as a whole, whose gradient range no op may write."""
    names = {n for blk in blocks(arena, heads) if all(x in frozen for x in blk) for n in blk}
    word = "bert.embeddings.word_embeddings.weight"
    if heads == "pretrain" and "cls.predictions.bias" not in frozen:
        names.discard(word)
    return names


GRAD = re.compile(r"(?<![\w:])grad\+(\d+)")


def grad_writes(eng):
    """Counter of byte offsets into the gradient arena that the backward list's structures point at."""
    r = S.Renderer(eng)
    text = "\n".join(r.ops("bwd", eng.bwd))
    assert r.unresolved == 0
    return collections.Counter(int(x) for x in GRAD.findall(text))


def ranges(arena, names):
    import math
    return sorted((4 * arena.offset[n], 4 * (arena.offset[n] + math.prod(arena.shape[n]))) for n in names)


def inside(off, rngs):
    return any(lo <= off < hi for lo, hi in rngs)


def events(eng):
    """(waits without an earlier record, as a set of events; the same as a list of op indices)"""
    from volta_amd import _lib as L
    seen, dangling = set(), []
    for i, o in enumerate(eng.bwd.ops):
        if o[0] == L.OP_SIDE_END:
            seen.add(o[1])
        if o[0] == L.OP_WAIT_SIDE and o[1] not in seen:
            dangling.append((i, o[1]))
    return dangling


def wgrad_problems(eng):
    """{(A, B): (M, N, K, lda, ldb)} of every TN problem of the backward list, operands as position-independent labels."""
    from volta_amd import _lib as L
    r = S.Renderer(eng)
    out = {}
    for kind, i0, i1, i2, a, b, c in eng.bwd.ops:
        if kind == L.OP_GEMM and (i0 & 0xFF) == L.TN:
            for q in a:
                out[(r.addr(q.A), r.addr(q.B))] = (q.M, q.N, q.K, q.lda, q.ldb)
    return out


@pytest.fixture(scope="module")
def unfrozen(matrix):
    cache = {}

    def get(pid):
        if pid not in cache:
            eng = build(matrix, pid)
            cache[pid] = (eng, S.render(eng)[0], grad_writes(eng), {e for _, e in events(eng)}, wgrad_problems(eng))
        return cache[pid]
    return get


@pytest.mark.parametrize("pid", PLANS)
def test_empty_frozen_set_is_the_unfrozen_plan(matrix, unfrozen, pid):
    text = unfrozen(pid)[1]
    for empty in (set(), None, ()):
        eng = build(matrix, pid, frozen=empty)
        assert S.render(eng)[0] == text
        assert not eng.pruned and not eng.frozen


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("pid", PLANS)
def test_pruned_backward_list(matrix, unfrozen, pid, case):
    from volta_amd import _lib as L
    base, base_text, base_writes, base_dangling, base_wgrad = unfrozen(pid)
    cfg, arena, heads = base.cfg, base.arena, base.heads
    frozen = frozen_set(cfg, arena, case)
    assert frozen
    eng = build(matrix, pid, frozen=frozen)
    text, unresolved = S.render(eng)
    assert unresolved == 0 and S.UNRESOLVED not in text
    # ---- nothing writes into a fully frozen block; everything else is written as often as in the unpruned list
    off_names = fully_frozen(arena, heads, frozen) - set(base.unused_params)
    off = ranges(arena, off_names)
    writes = grad_writes(eng)
    hit = sorted(o for o in writes if inside(o, off))
    assert not hit, "ops write into frozen gradient ranges at byte offsets %s" % hit[:8]
    assert eng.pruned >= off_names, sorted(off_names - eng.pruned)[:8]
    assert not [o for o in writes if inside(o, ranges(arena, eng.pruned))]          # what the engine reports as unwritten (the model clears it once) is
    want = collections.Counter({o: c for o, c in base_writes.items() if not inside(o, off)})
    word = "bert.embeddings.word_embeddings.weight"
    if heads == "pretrain" and word in frozen and word not in off_names:
        # the word table has two writers there: the text tables' scatter, gone with a frozen embedding, and the tied decoder's product,
        # which stays as long as the decoder bias trains
        emb_off = all(n in frozen for n in arena.params if n.startswith("bert.embeddings."))
        want[4 * arena.offset[word]] -= int(emb_off)
    assert writes == want, ("trainable blocks written differently", sorted((writes - want).items())[:8], sorted((want - writes).items())[:8])
    trainable_written = {n for n in arena.params if n not in off_names and any(inside(o, ranges(arena, [n])) for o in base_writes)}
    assert all(any(inside(o, ranges(arena, [n])) for o in writes) for n in trainable_written)
    # ---- events: pruning orphans no wait
    dangling = events(eng)
    assert all(e in base_dangling for _, e in dangling), dangling
    # ---- one mark per stage, as DistributedDataParallel's buckets expect
    assert len(eng.bwd_marks) == len(base.bwd_marks) and eng.param_ready_stage == base.param_ready_stage
    assert eng.bwd_marks == sorted(eng.bwd_marks) and eng.bwd_marks[-1] == len(eng.bwd.ops) - 1 and eng.bwd.ops[-1][0] == L.OP_JOIN
    # ---- the forward list and the buffers it writes do not change
    fwd = lambda t: t[t.index("# forward"):t.index("# backward")]
    assert fwd(text) == fwd(base_text)
    # ---- the remaining weight-gradient problems keep their K-chunks (operands, rows, strides)
    wg = wgrad_problems(eng)
    assert all(base_wgrad.get(k) == v for k, v in wg.items()), [k for k, v in wg.items() if base_wgrad.get(k) != v][:4]
    if case == "d":          # nothing of the encoder or the embeddings is left: every stage behind the heads is empty
        assert len(set(eng.bwd_marks)) == 1, eng.bwd_marks
    if case == "g":          # Q|K|V is one block: `query` alone prunes nothing
        assert text == base_text and not eng.frozen
    if case in "abcde":
        assert len(eng.bwd.ops) < len(base.bwd.ops)


def test_frozen_layernorm_takes_the_launch_without_column_sums(matrix, unfrozen):
    """Case f: the one LayerNorm backward job of the sub-layer has no partial records, no destination, and no TailJob sums it."""
    from volta_amd import _lib as L
    pid = "pretrain/vilbert/train-bf16"
    base = unfrozen(pid)[0]
    eng = build(matrix, pid, frozen=frozen_set(base.cfg, base.arena, "f"))
    jobs = lambda e: [x for o in e.bwd.ops if o[0] == L.OP_LN_BWD for x in (o[4], o[5]) if x is not None]
    bare = [j for j in jobs(eng) if not j.partial]
    assert len(bare) >= 1 and all(not j.dgamma and not j.dbeta for j in bare) and all(j.partial for j in jobs(base))
    tails = lambda e: sum(o[4].n[0] for o in e.bwd.ops if o[0] == L.OP_GENERIC and o[4].fn == L.FN_SIDE_TAIL)
    assert tails(eng) == tails(base) - len(bare)


def test_key_is_the_pruning_decision(matrix, unfrozen):
    """Two patterns that prune the same ops give one canonical set (what EngineHostModel keys its plans by); `query` alone gives the empty one."""
    from volta_amd.engine import canonical_frozen
    base = unfrozen("pretrain/vilbert/train-bf16")[0]
    cfg, arena = base.cfg, base.arena
    e = frozen_set(cfg, arena, "e")
    g = frozen_set(cfg, arena, "g")
    assert canonical_frozen(arena, g, "pretrain") == frozenset() == canonical_frozen(arena, (), "pretrain")
    assert canonical_frozen(arena, e | g, "pretrain") == canonical_frozen(arena, e, "pretrain") == frozenset(e)
