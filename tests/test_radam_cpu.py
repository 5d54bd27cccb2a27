"""RAdam / PlainRAdam / WarmupConstantSchedule host side, no GPU: the step-size planner against the reference's recorded buffer
(tests/golden/radam_reference.npz, tools/make_radam_golden.py), the float64 restatement (tests/radam_restate.py) against the reference's
fp32 values, the new C ABI, and the constructors' checks."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from radam_restate import Restated  # noqa: E402

Z = np.load(os.path.join(HERE, "golden", "radam_reference.npz"))
N = len([k for k in Z.files if k.startswith("init_")])


def _lrs(s):
    return [float(Z["base_lr"][i] * Z["lr_factor"][s]) for i in range(N)]


def test_planner_reproduces_the_reference_buffer_exactly():
    """Per step: the 10-slot buffer and each stepping tensor's (step_size, rectified), bit for bit -- the first group's tensor taking group
    1's lr at step 2, the lagging tensors reusing (and, ten steps behind, overwriting) other groups' slots."""
    from volta_amd.optimization import radam_plan, radam_runs
    buf = [[None, None, None] for _ in range(10)]
    steps, uniform = [0] * N, 0
    foreign_lr_steps = 0
    for s in range(int(Z["steps"])):
        live = [bool(x) for x in Z["live"][s]]
        lrs = _lrs(s)
        runs, run_of = radam_runs(steps, live, lambda i: lrs[i], uniform)
        plan = radam_plan(buf, runs, 0.9, 0.999)
        for i in range(N):
            want_ss, want_n = Z["radam_step_size"][s][i], Z["radam_nsma"][s][i]
            r = (0 if run_of is None else run_of[i])
            if not live[i]:
                assert r == -1 and np.isnan(want_ss)
                continue
            assert plan[r][0] == want_ss, (s, i, plan[r][0], want_ss)
            assert plan[r][1] == (want_n >= 5), (s, i)
            own = __import__("radam_restate").step_size(lrs[i], steps[i] + 1, 0.9, 0.999)[0]
            foreign_lr_steps += own != want_ss
        got = np.array([[np.nan if x is None else float(x) for x in b] for b in buf])
        np.testing.assert_array_equal(got, Z["radam_buffer"][s])
        steps = [t + l for t, l in zip(steps, live)]
        uniform = steps[0] if all(t == steps[0] for t in steps) else None
    assert foreign_lr_steps >= 10        # the scenario really exercises steps taken with another group's (or an older) lr


def test_planner_uniform_case_is_one_run_without_a_walk():
    from volta_amd.optimization import radam_plan, radam_runs
    calls = []
    runs, run_of = radam_runs([7] * 600, [True] * 600, lambda i: calls.append(i) or 2e-5, uniform=7)
    assert runs == [(8, 2e-5)] and run_of is None and calls == [0]
    buf = [[None, None, None] for _ in range(10)]
    (ss, rect), = radam_plan(buf, runs, 0.9, 0.999)
    assert buf[8][0] == 8 and buf[8][2] == ss and rect
    # a second run at the same step count (another optimizer call at step 8) hits the slot: the first lr wins
    assert radam_plan(buf, [(8, 1e-4)], 0.9, 0.999) == [(ss, True)]


def _replay(tag, **variant):
    R = Restated([torch.from_numpy(Z["init_%d" % i]) for i in range(N)], plain=tag == "plain", **variant)
    worst = 0.0
    for s in range(int(Z["steps"])):
        grads = [torch.from_numpy(Z["grad_%d" % i][s]) if Z["live"][s][i] else None for i in range(N)]
        R.step(grads, _lrs(s), list(Z["wd"]))
        for i in range(N):
            worst = max(worst, R.excess(i, *(torch.from_numpy(Z["%s_%s_%d" % (tag, k, i)][s]) for k in "pmv")))
    return worst


@pytest.mark.parametrize("tag", ["radam", "plain"])
def test_restatement_matches_the_reference_within_the_fp32_bound(tag):
    """The gate is 2x the first-order fp32 bound derived in tests/radam_restate.py; the reference (fp32, CPU) must sit inside it and the
    plausible mistakes -- decay after the update (AdamW's order), each group's own lr for RAdam's step size -- far outside."""
    assert _replay(tag) <= 1.0
    assert _replay(tag, decay_after=True) > 10.0
    if tag == "radam":
        assert _replay(tag, own_lr=True) > 10.0


def test_warmup_constant_schedule():
    from volta_amd.optimization import WarmupConstantSchedule
    p = torch.nn.Parameter(torch.zeros(2))
    opt = torch.optim.SGD([p], lr=0.5)
    sch = WarmupConstantSchedule(opt, warmup_steps=2.5)             # train_task.py: warmup_proportion * steps is a float
    seen = []
    for _ in range(6):
        seen.append(opt.param_groups[0]["lr"])
        opt.step()
        sch.step()
    assert seen == [0.0, 0.5 / 2.5, 0.5 * 2 / 2.5, 0.5, 0.5, 0.5]
    sd = sch.state_dict()
    opt2 = torch.optim.SGD([torch.nn.Parameter(torch.zeros(2))], lr=0.5)
    sch2 = WarmupConstantSchedule(opt2, warmup_steps=100)
    sch2.load_state_dict(sd)
    assert sch2.warmup_steps == 2.5 and sch2.last_epoch == 6
    sch2.step()
    assert opt2.param_groups[0]["lr"] == 0.5
    opt3 = torch.optim.SGD([torch.nn.Parameter(torch.zeros(2))], lr=0.5)
    WarmupConstantSchedule(opt3, warmup_steps=0)
    assert opt3.param_groups[0]["lr"] == 0.5                         # no warm-up: full lr from the first step


def test_radam_struct_and_exports():
    from volta_amd import _lib as L
    src = '#include <stdio.h>\n#include "volta_hip.h"\nint main(void){printf("%zu %d\\n", sizeof(vk_radam_args), VK_RADAM_CLASSES);return 0;}'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        size, ncls = map(int, subprocess.check_output([exe]).decode().split())
    assert ctypes.sizeof(L.RadamArgs) == size and L.RADAM_CLASSES == ncls >= 16
    for name in ("vk_radam_step", "vk_radam_step_list"):
        assert name in L.EXPORTS and hasattr(L.lib, name)


def test_kernel_argument_checks_report_through_last_error():
    from volta_amd import _lib as L
    a = L.RadamArgs()
    a.beta1, a.beta2, a.one_minus_beta1, a.one_minus_beta2, a.eps, a.n = 0.9, 0.999, 0.1, 0.001, 1e-8, 1000
    assert L.lib.vk_radam_step(ctypes.byref(a), None) != 0 and b"multiple of 1024" in L.lib.vk_last_error()
    a.n, a.beta2 = 1024, 1.0
    assert L.lib.vk_radam_step(ctypes.byref(a), None) != 0 and b"betas" in L.lib.vk_last_error()
    a.beta2 = 0.999
    assert L.lib.vk_radam_step_list(ctypes.byref(a), None, 70000, 1, None) != 0 and b"70000 tensors" in L.lib.vk_last_error()


def test_constructors_validate_and_refuse_what_is_out_of_scope():
    from volta_amd.optimization import PlainRAdam, RAdam
    p, q = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(3))
    for cls in (RAdam, PlainRAdam):
        with pytest.raises(ValueError):
            cls([p], lr=-1.0)
        with pytest.raises(ValueError):
            cls([p], betas=(0.9, 1.0))
        with pytest.raises(ValueError):
            cls([p], eps=-1.0)
        with pytest.raises(RuntimeError, match="betas / eps"):
            cls([{"params": [p]}, {"params": [q], "betas": (0.8, 0.999)}])
        with pytest.raises(RuntimeError, match="betas / eps"):
            cls([{"params": [p]}, {"params": [q], "eps": 1e-6}])
        opt = cls([{"params": [p], "lr": 2e-5}, {"params": [q], "lr": 1e-4, "weight_decay": 0.01}], lr=2e-5)
        assert opt.defaults["eps"] == 1e-8 and opt.defaults["weight_decay"] == 0 and opt.defaults["betas"] == (0.9, 0.999)
        assert not hasattr(opt, "buffer") if cls is PlainRAdam else opt.buffer == [[None, None, None]] * 10
        with pytest.raises(TypeError):
            cls([p], overlap_with_forward=True)


def test_state_loaded_before_the_model_is_on_the_gpu_stays_on_the_host():
    """train_task.py:236-246: resume() loads the optimizer while the model is on the CPU; then `optimizer.state` tensors are moved with
    .cuda().  The loaded state is kept aside until the first setup on the GPU, and `optimizer.state` holds nothing to move."""
    from volta_amd.optimization import RAdam
    ps = [torch.nn.Parameter(torch.from_numpy(Z["init_%d" % i]).clone()) for i in range(N)]
    opt = RAdam([{"params": [p], "lr": float(Z["base_lr"][i]), "weight_decay": float(Z["wd"][i])} for i, p in enumerate(ps)], lr=1e-2)
    sd = {"state": {i: {"step": int(Z["radam_sd_mid_step"][i]), "exp_avg": torch.from_numpy(Z["radam_sd_mid_m_%d" % i]),
                        "exp_avg_sq": torch.from_numpy(Z["radam_sd_mid_v_%d" % i])} for i in range(N) if Z["radam_sd_mid_step"][i] > 0},
          "param_groups": opt.state_dict()["param_groups"]}
    opt.load_state_dict(sd)
    assert len(opt.state) == 0 and opt._fused is None
    back = opt.state_dict()
    assert sorted(back["state"]) == sorted(sd["state"]) and 5 not in back["state"]
    for i, st in back["state"].items():
        assert st["step"] == sd["state"][i]["step"] and torch.equal(st["exp_avg"], sd["state"][i]["exp_avg"])
    with pytest.raises(ValueError):
        opt.load_state_dict({"state": {0: {"step": 3, "exp_avg": torch.zeros(5), "exp_avg_sq": torch.zeros(5)}}, "param_groups": sd["param_groups"]})
