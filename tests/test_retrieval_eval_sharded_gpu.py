"""`evaluate_retrieval(..., group=...)`: the captions sharded over the ranks of a process group, against the unsharded call on the same model
and data -- every metric, `results`, both rank vectors, and each rank's score block bit for bit against the rows of the unsharded matrix.
A gloo group of one rank in this process, then two fresh child processes on GPU 0 over gloo (tests/retrieval_shard_child.py), a VL-logit
task model and a zero-shot `BertForVLPreTraining`; 20 captions, 6 images.  Integer outputs are compared for equality.  GPU only.

The ranks' score blocks come from pair chunks of another size than the unsharded run's (10 captions a rank against 20 at once): the scorer
pins that a pair's logit does not depend on the chunking (tests/test_retrieval_gpu.py), and the bit-equality asserted here rests on it."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tests import retrieval_shard_child as SC  # noqa: E402
from tests.retrieval_eval_fixture import EvalFixture  # noqa: E402

CHILD_SECONDS = 150
NC, NI = 20, 6


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    return EvalFixture(tmp_path_factory.mktemp("retrieval_eval_sharded"))


@pytest.fixture(scope="module")
def single(fx):
    """zero_shot -> (model, dataset, the unsharded result packed), computed once per kind"""
    from volta_amd.retrieval import evaluate_retrieval
    ds, cache = SC.dataset20(fx), {}

    def get(zero_shot):
        if zero_shot not in cache:
            model = SC.tiny_model(zero_shot)
            res = evaluate_retrieval(model, ds, task_id=None if zero_shot else "TASK8", pair_chunk=1000, topk=20)
            assert res.caption_range == (0, NC) and tuple(res.score_matrix.shape) == (NC, NI)
            cache[zero_shot] = (model, ds, res, SC.pack(res))
        return cache[zero_shot]
    return get


@pytest.fixture
def group_of_one(tmp_path):
    import torch.distributed as dist
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "store"), rank=0, world_size=1)
    yield dist
    dist.destroy_process_group()


def _same_numbers(got, want, where):
    for k in ("rank_ir", "rank_tr", "results", "image_retrieval", "text_retrieval"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (where, k, got[k], want[k])


def _same_block(got, want, where):
    a, b = (int(v) for v in got["caption_range"])
    block, rows = got["score_matrix"], want["score_matrix"][a:b]
    assert block.shape == rows.shape and block.dtype == np.float32
    differ = np.argwhere(block.view(np.uint32) != rows.view(np.uint32))
    assert len(differ) == 0, (where, "pairs (caption, image) whose score differs from the unsharded run:",
                              [(int(a + r), int(i), float(block[r, i]), float(rows[r, i])) for r, i in differ[:16]])


@pytest.mark.parametrize("zero_shot", [False, True], ids=["task", "zero_shot"])
def test_group_of_one_equals_the_unsharded_call(single, group_of_one, zero_shot):
    from volta_amd.parallel import DistributedDataParallel
    from volta_amd.retrieval import evaluate_retrieval
    model, ds, res, want = single(zero_shot)
    task = None if zero_shot else "TASK8"
    again = evaluate_retrieval(model, ds, task_id=task, pair_chunk=1000, topk=20)                 # `group=None` inside a group: today's path
    assert again.caption_range == (0, NC) and torch.equal(again.score_matrix, res.score_matrix)
    _same_numbers(SC.pack(again), want, "group=None")
    wrapped = DistributedDataParallel.__new__(DistributedDataParallel)                             # wrapped as the driver wraps it: unwrapped as now
    torch.nn.Module.__init__(wrapped)
    wrapped.module = model
    phases = []
    for who, grp in ((model, True), (wrapped, group_of_one.group.WORLD)):
        got = evaluate_retrieval(who, ds, task_id=task, pair_chunk=1000, topk=20, group=grp, phase_hook=phases.append)
        assert got.caption_range == (0, NC) and got.rank_ir.is_cuda and got.rank_tr.is_cuda and got.score_matrix.is_cuda
        assert got.image_retrieval == res.image_retrieval and got.text_retrieval == res.text_retrieval and got.results == res.results
        assert torch.equal(got.rank_ir, res.rank_ir) and torch.equal(got.rank_tr, res.rank_tr)
        assert torch.equal(got.score_matrix.view(torch.int32), res.score_matrix.view(torch.int32))
        _same_numbers(SC.pack(got), want, "group of one")
    assert phases == ["encode", "score", "ranks"] * 2
    k0 = evaluate_retrieval(model, ds, task_id=task, topk=0, group=True)                           # no top-k: three collectives, empty lists
    assert k0.results == [[]] * NC and torch.equal(k0.rank_ir, res.rank_ir) and torch.equal(k0.rank_tr, res.rank_tr)


def _run_children(tmp_path, zero_shot, world=2):
    """`world` fresh processes, each under its own time limit, no retry; stops at the first that fails.  The parent only waits."""
    store, outs, procs = str(tmp_path / "store"), [], []
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for r in range(world):
        outs.append(str(tmp_path / ("rank%d.npz" % r)))
        cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.join(ROOT, "tests", "retrieval_shard_child.py"), "--rank", str(r), "--world", str(world),
               "--store", store, "--root", str(tmp_path / ("root%d" % r)), "--out", outs[-1]] + (["--zero-shot"] if zero_shot else [])
        procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    pending, failed = set(range(world)), None
    while pending and failed is None:
        for r in sorted(pending):
            try:
                rc = procs[r].wait(timeout=0.05)
            except subprocess.TimeoutExpired:
                continue
            pending.discard(r)
            if rc != 0:
                failed = (r, rc)
                break
    for r in pending:                                                             # a rank failed: the others would wait for it in a collective
        procs[r].kill()
    logs = [p.communicate()[0] for p in procs]
    assert failed is None, "rank %d ended with status %d:\n%s" % (failed[0], failed[1], logs[failed[0]][-4000:])
    return [dict(np.load(o)) for o in outs]


@pytest.mark.parametrize("zero_shot", [False, True], ids=["task", "zero_shot"])
def test_two_processes_equal_the_unsharded_call(single, tmp_path, zero_shot):
    want = single(zero_shot)[3]
    torch.cuda.synchronize()                                                      # the parent leaves the GPU alone while the children run
    ranks = _run_children(tmp_path, zero_shot)
    assert [tuple(int(v) for v in r["caption_range"]) for r in ranks] == [(0, 10), (10, 20)]
    _same_numbers(ranks[0], ranks[1], "rank 0 against rank 1")
    for r, got in enumerate(ranks):
        _same_numbers(got, want, "rank %d against the unsharded run" % r)
        _same_block(got, want, "rank %d" % r)
    assert (want["rank_tr"][:5] >= 0).all() and want["rank_tr"][5] == -1          # the image without a caption is left out on every rank


def test_refusals(single, fx, tmp_path):
    import torch.distributed as dist
    from volta_amd.retrieval import evaluate_retrieval
    model, ds, _, _ = single(False)
    assert not dist.is_initialized()
    for grp in (True, "world", 0):
        with pytest.raises(ValueError, match="torch.distributed is not initialised"):
            evaluate_retrieval(model, ds, task_id="TASK8", group=grp)
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "store"), rank=0, world_size=1)
    try:
        with pytest.raises(ValueError, match="group must be None, True"):
            evaluate_retrieval(model, ds, task_id="TASK8", group="world")
        with pytest.raises(ValueError, match="unknown task id"):                   # the scorer's refusals, with its messages
            evaluate_retrieval(model, ds, task_id="TASK9", group=True)
        with pytest.raises(ValueError, match="pair_chunk must be positive"):
            evaluate_retrieval(model, ds, task_id="TASK8", pair_chunk=0, group=True)
        with pytest.raises(ValueError, match="topk"):
            evaluate_retrieval(model, ds, task_id="TASK8", topk=65, group=True)
        with pytest.raises(ValueError, match="not from"):
            evaluate_retrieval(torch.nn.Linear(2, 2), ds, group=True)
    finally:
        dist.destroy_process_group()
