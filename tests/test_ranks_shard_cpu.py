"""The sharded rank calls on the host: the numpy restatement of the three steps (tests/ranks_shard_restate.py: rows at an offset, partial
column counts, sum and minimum) merged over W shards against the definition (tests/ranks_restate.py: the position in
np.argsort(-s, kind="stable"), NaN last, per row and per column), and the C boundary of `vk_retrieval_ranks_shard_rows`, `_shard_cols` and
`_finish` (exports, struct layout, host validation).  Integer outputs are compared for equality.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ranks_restate as RR  # noqa: E402
from tests import ranks_shard_restate as SR  # noqa: E402

CALLS = ("vk_retrieval_ranks_shard_rows", "vk_retrieval_ranks_shard_cols", "vk_retrieval_ranks_finish")


@pytest.fixture(scope="module")
def definition():
    return {name: (build(), ) for name, (build, _) in SR.CASES.items()}


@pytest.mark.parametrize("name", list(SR.CASES))
def test_merged_shards_equal_the_definition(definition, name):
    (S, ci), = definition[name]
    Nc, Ni = S.shape
    want = RR.ranks(S, ci, 20)
    assert want[0][2] == -1 and want[0][3] == -1 and want[2][1] == -1 and int((ci == 4).sum()) == 11
    for W in (1, 2, 3, 5, Nc + 2):
        got = SR.merged(S, ci, 20, W)
        for g, w, what in zip(got, want, ("rank_ir", "topk_ir", "rank_tr")):
            assert g.dtype == np.int32 and np.array_equal(g, w), (W, what, np.argwhere(g != w)[:8])


def test_the_tie_cases_are_what_they_claim():
    """equal scores in a column across a shard boundary, the target on the later and on the earlier side; local row indices would miscount"""
    S, ci = SR.case_ties()
    Nc = S.shape[0]
    for W, b, col in ((2, SR.shard_range(Nc, 2, 1)[0], 7), (3, SR.shard_range(Nc, 3, 1)[0], 9)):
        assert ci[b - 1] == col and ci[b] == col and S[b - 2, col] == S[b - 1, col] == S[b, col] == S[b + 1, col]
    image_ptr, image_captions = SR.csr(ci, S.shape[1])
    tk = SR.sortable(S[np.arange(Nc), np.clip(ci, 0, S.shape[1] - 1)])
    a, b = SR.shard_range(Nc, 2, 1)
    right = SR.shard_counts(S[a:b], a, tk, image_ptr, image_captions, Nc)
    local = SR.shard_counts(S[a:b], 0, tk, image_ptr, image_captions, Nc)          # the mistake: rows numbered from 0
    assert not np.array_equal(right, local)
    runs = [set(np.flatnonzero(ci[a:b] == 4)) != set() for a, b in (SR.shard_range(Nc, 3, r) for r in range(3))]
    assert runs == [True, True, True]                                             # the 11 captions of image 4 lie in all three shards


def test_sortable_words_order_like_the_definition():
    s = np.asarray([0.0, SR.NAN, -0.0, SR.INF, 1.0, -SR.INF, 1.0, -SR.NAN, -3.5, 2.0 ** -140], np.float32)
    sk = SR.sortable(s)
    assert sk[0] == sk[2] == 0x80000000 and sk[1] == sk[7] == 0 and sk[3] == 0xFF800000 and sk[5] == 0x007FFFFF
    assert np.lexsort((np.arange(len(s)), -sk.astype(np.int64))).tolist() == RR.order(s).tolist()


def test_shard_ranges_cover_the_captions_once():
    for Nc, W in ((37, 5), (37, 39), (600, 7), (1, 3)):
        r = [SR.shard_range(Nc, W, k) for k in range(W)]
        assert r[0][0] == 0 and r[-1][1] == Nc and all(a[1] == b[0] for a, b in zip(r, r[1:])) and all(b >= a for a, b in r)


# ------------------------------------------------------------------------------------------------ the C boundary
def test_shard_entries_are_exported_and_declared():
    from volta_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "volta_hip.h")).read(), flags=re.S)
    for name in CALLS:
        assert name in L.EXPORTS and hasattr(L.lib, name)
        assert re.search(r"\bint\s+%s\s*\(\s*const\s+vk_retrieval_ranks_shard_args\s*\*" % name, text), name
    assert "#define VK_RANKS_ACCUMULATE %d" % L.RANKS_ACCUMULATE in text


def test_shard_struct_layout_matches_the_header(tmp_path):
    from volta_amd import _lib as L
    fields = [n for n, _ in L.RetrievalRanksShardArgs._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "volta_hip.h"\nint main(void){printf("%zu\\n", sizeof(vk_retrieval_ranks_shard_args));' + "".join(
        'printf("%%zu\\n", offsetof(vk_retrieval_ranks_shard_args, %s));' % n for n in fields) + "return 0;}"
    c, exe = str(tmp_path / "s.c"), str(tmp_path / "s")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert ctypes.sizeof(L.RetrievalRanksShardArgs) == out[0]
    assert [getattr(L.RetrievalRanksShardArgs, n).offset for n in fields] == out[1:]


def _caller(fn_name):
    from volta_amd import _lib as L
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(**kw):
        v = dict(S=p, caption_image=p, image_ptr=p, image_captions=p, rank_ir=p, topk_ir=p, rank_tr=p, target_key=p, count=p, ld=4, Nc=6, Ni=4, K=2, row0=2,
                 nrows=3, flags=0)
        v.update(kw)
        a = L.RetrievalRanksShardArgs(*[v[n] for n, _ in L.RetrievalRanksShardArgs._fields_])
        rc = getattr(L.lib, fn_name)(ctypes.byref(a), None)
        return rc, L.lib.vk_last_error().decode()
    return call, p


READS = {"vk_retrieval_ranks_shard_rows": ("S", "caption_image", "rank_ir", "topk_ir", "target_key"),
         "vk_retrieval_ranks_shard_cols": ("S", "image_ptr", "image_captions", "target_key", "count"),
         "vk_retrieval_ranks_finish": ("image_ptr", "count", "rank_tr")}


@pytest.mark.parametrize("fn", CALLS)
def test_shard_host_validation_names_the_call(fn):
    """argument checks happen on the host before any launch and report through vk_last_error() with the call's name"""
    from volta_amd import _lib as L
    call, p = _caller(fn)
    for name in READS[fn]:
        rc, msg = call(**{name: None})
        assert rc != 0 and msg.startswith(fn + ": null pointer"), (name, msg)
    for kw in (dict(Nc=0), dict(Ni=0), dict(Nc=-3), dict(Ni=-1)):
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith(fn + ":") and "must be positive" in msg, kw
    assert getattr(L.lib, fn)(None, None) != 0 and L.lib.vk_last_error().decode().startswith(fn + ": null argument struct")
    if fn == "vk_retrieval_ranks_finish":
        return
    rc, msg = call(ld=3)
    assert rc != 0 and msg.startswith(fn + ": leading dimension 3")
    rc, msg = call(S=ctypes.c_void_p(p.value + 2))
    assert rc != 0 and msg.startswith(fn + ": S is not 4-byte aligned")
    for kw in (dict(row0=-1), dict(row0=4, nrows=3), dict(nrows=-1), dict(row0=2 ** 31 - 1, nrows=2 ** 31 - 1)):
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith(fn + ": rows [") and "not inside the 6 captions" in msg, kw
    if fn == "vk_retrieval_ranks_shard_rows":
        for k in (-1, 65):
            rc, msg = call(K=k)
            assert rc != 0 and msg.startswith(fn + ": top-k of %d" % k)
        assert call(K=0, topk_ir=None, nrows=0)[0] == 0
    else:
        rc, msg = call(flags=2)
        assert rc != 0 and msg.startswith(fn + ": unknown flags")
        rows = 65535 * 256 + 1
        rc, msg = call(Nc=rows + 5, row0=5, nrows=rows)
        assert rc != 0 and msg.startswith(fn + ": %d rows exceed" % rows)
    with pytest.raises(L.VoltaHipError, match=fn):
        L.check(call(ld=1)[0])


def test_an_empty_shard_is_legal_and_launches_nothing():
    """nrows == 0 returns success on a machine without a GPU: the row call does nothing, the column call with VK_RANKS_ACCUMULATE neither;
    S may then be NULL"""
    from volta_amd import _lib as L
    call, _ = _caller("vk_retrieval_ranks_shard_rows")
    assert call(nrows=0)[0] == 0 and call(nrows=0, S=None)[0] == 0 and call(nrows=0, row0=6)[0] == 0
    call, _ = _caller("vk_retrieval_ranks_shard_cols")
    assert call(nrows=0, flags=L.RANKS_ACCUMULATE)[0] == 0 and call(nrows=0, S=None, flags=L.RANKS_ACCUMULATE)[0] == 0


def test_group_without_a_process_group_is_refused_before_anything_else():
    import torch
    import torch.distributed as dist
    from volta_amd.retrieval import evaluate_retrieval
    assert not dist.is_initialized()
    with pytest.raises(ValueError, match="torch.distributed is not initialised"):
        evaluate_retrieval(torch.nn.Linear(2, 2), None, group=True)
    with pytest.raises(ValueError, match="not from Linear"):                       # without `group`: the scorer's refusal, as before
        evaluate_retrieval(torch.nn.Linear(2, 2), None)
