"""The step engine's plans, pinned by signature (tools/plan_signature.py): every plan of the tool's matrix -- the five embedding
families, bf16 and e4m3 sub-layers, the pre-training, task, backbone and score heads, the two benchmark shapes -- is built on the CPU and
its position-independent text hashed against tests/golden/plan_signatures.json.  A host-side edit of the engine that moves, adds or
re-binds a single op, buffer or patched input shows here, with no GPU."""
import importlib.util
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("plan_signature", os.path.join(ROOT, "tools", "plan_signature.py"))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)

IDS = S.Matrix().ids()              # building the list builds no model


@pytest.fixture(scope="module")
def matrix():
    """The models and arenas the plans of this module share, released when the module is done."""
    yield S.Matrix()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "plan_signatures.json")))


def test_golden_lists_exactly_the_matrix(golden):
    assert sorted(golden) == sorted(IDS)


@pytest.mark.parametrize("pid", IDS)
def test_plan_signature_matches_golden(matrix, golden, pid):
    text, unresolved = matrix.text(pid)
    assert unresolved == 0 and S.UNRESOLVED not in text, "an address of %s resolves to no buffer" % pid
    assert S.sha(text) == golden[pid], ("the plan %s differs from the recorded one; for a diff of its first differing ops against the parent's tree: "
                                        "python tools/plan_signature.py --check --only '^%s$' --base <checkout of the parent>" % (pid, pid))


def test_signature_is_independent_of_where_buffers_land():
    """The same plan built twice in one process, the second time on a new arena with an unrelated allocation alive in between."""
    pid = "pretrain/vilbert/train-fp8"
    eng1 = S.Matrix().build(pid)                 # stays alive: the second build cannot reuse its arena or buffers
    ballast = [torch.empty(n, dtype=torch.uint8) for n in (1 << 20, 12345, 3 << 20)]
    eng2 = S.Matrix().build(pid)
    assert eng1.arena.master.data_ptr() != eng2.arena.master.data_ptr() and len(ballast) == 3
    assert eng1.bufs["L0_qkv0"].data_ptr() != eng2.bufs["L0_qkv0"].data_ptr()
    first, second = S.render(eng1), S.render(eng2)
    assert first == second and first[1] == 0
    assert first[0].count("\n") > 500
