"""Records tests/golden/radam_reference.npz from the reference's own RAdam and PlainRAdam (volta/optimization.py), loaded by file path:

  python tools/make_radam_golden.py --reference /path/to/volta-checkout [--out tests/golden/radam_reference.npz]

Scenario (the constants below; the file records them for the tests): six small seeded fp32 tensors, one group each
(train_task.py:208-219 builds one group per parameter); group 0's lr differs from the others, groups 1 and 3 decay; every step sets the
lrs by hand (warm-up then decay); tensors miss gradients at chosen steps, so step counts diverge, lagging tensors reuse other groups'
buffer slots and, ten steps behind, overwrite them; one step has gradients 1000x larger.  Recorded per step: parameters, moments, the
buffer and each stepping tensor's (step_size, N_sma); the reference's state_dict() at the mid-point and at the end; and the run that a
FRESH optimizer loaded from the mid-point state_dict continues to (what train_task.py's resume() does).  Values only; tests never import
the reference."""
import argparse
import copy
import importlib.util
import os

import numpy as np
import torch

SHAPES = [(7,), (33,), (4, 5), (130,), (3, 3), (12,)]
BASE_LR = [1e-2, 3e-2, 3e-2, 3e-2, 3e-2, 3e-2]
WD = [0.0, 0.1, 0.0, 0.1, 0.0, 0.0]
STEPS, MID, BIG_STEP = 26, 12, 9
# global steps (1-based) at which a tensor has no gradient
MISSING = {0: [1], 2: [4, 5], 4: list(range(6, 16)), 5: list(range(1, 15))}


def lr_factor(s):
    """The hand-set schedule of global step s (1-based)."""
    return min(1.0, s / 4.0) * (1.0 - s / 40.0)


def scenario(seed=0):
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(sh, generator=g) for sh in SHAPES]
    grads = []
    for s in range(1, STEPS + 1):
        row = [torch.randn(sh, generator=g) * (1000.0 if s == BIG_STEP else 0.1) for sh in SHAPES]
        grads.append(row)
    return init, grads


def load_reference(root):
    spec = importlib.util.spec_from_file_location("volta_reference_optimization", os.path.join(root, "volta", "optimization.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Slot(list):
    """A buffer slot that logs the step size each parameter takes from it (index 2: written on a miss, read on a hit)."""
    log = []

    def __getitem__(self, k):
        v = list.__getitem__(self, k)
        if k == 2:
            Slot.log.append((v, list.__getitem__(self, 1)))
        return v

    def __setitem__(self, k, v):
        list.__setitem__(self, k, v)
        if k == 2:
            Slot.log.append((v, list.__getitem__(self, 1)))


def run(cls, init, grads, first, last, params=None, load=None, instrument=False):
    params = params or [torch.nn.Parameter(t.clone()) for t in init]
    opt = cls([{"params": [p], "lr": BASE_LR[i], "weight_decay": WD[i]} for i, p in enumerate(params)], lr=BASE_LR[0])
    if load is not None:
        opt.load_state_dict(load)
    if instrument:
        opt.buffer = [Slot([None, None, None]) for _ in range(10)]
    rec = dict(p=[], m=[], v=[], buf=[], ss=[], nsma=[], sd={})
    for s in range(first, last + 1):
        for i, grp in enumerate(opt.param_groups):
            grp["lr"] = BASE_LR[i] * lr_factor(s)
        for i, p in enumerate(params):
            p.grad = None if s in MISSING.get(i, ()) else grads[s - 1][i].clone()
        Slot.log = []
        opt.step()
        rec["p"].append([p.detach().clone() for p in params])
        rec["m"].append([opt.state[p]["exp_avg"].clone() if p in opt.state else torch.zeros_like(p) for p in params])
        rec["v"].append([opt.state[p]["exp_avg_sq"].clone() if p in opt.state else torch.zeros_like(p) for p in params])
        if instrument:
            rec["buf"].append(np.array([[np.nan if x is None else float(x) for x in list.__iter__(b)] for b in opt.buffer]))
            log = iter(Slot.log)
            ss, ns = np.full(len(params), np.nan), np.full(len(params), np.nan)
            for i, p in enumerate(params):
                if p.grad is not None:
                    ss[i], ns[i] = next(log)
            assert next(log, None) is None
            rec["ss"].append(ss)
            rec["nsma"].append(ns)
        if s in (MID, STEPS):
            rec["sd"][s] = copy.deepcopy(opt.state_dict())
    return rec, params


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository (volta/optimization.py is read from it)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "radam_reference.npz"))
    args = ap.parse_args()
    ref = load_reference(args.reference)
    init, grads = scenario()
    out = dict(steps=np.int64(STEPS), mid=np.int64(MID), big_step=np.int64(BIG_STEP), base_lr=np.array(BASE_LR), wd=np.array(WD),
               lr_factor=np.array([lr_factor(s) for s in range(1, STEPS + 1)]),
               live=np.array([[s not in MISSING.get(i, ()) for i in range(len(SHAPES))] for s in range(1, STEPS + 1)]))
    for i, t in enumerate(init):
        out["init_%d" % i] = t.numpy()
        out["grad_%d" % i] = torch.stack([grads[s][i] for s in range(STEPS)]).numpy()
    for tag, cls in (("radam", ref.RAdam), ("plain", ref.PlainRAdam)):
        rec, params = run(cls, init, grads, 1, STEPS, instrument=tag == "radam")
        for i in range(len(SHAPES)):
            for k in ("p", "m", "v"):
                out["%s_%s_%d" % (tag, k, i)] = torch.stack([r[i] for r in rec[k]]).numpy()
        for s, sd in rec["sd"].items():
            at = "mid" if s == MID else "end"
            out["%s_sd_%s_step" % (tag, at)] = np.array([sd["state"][i]["step"] if i in sd["state"] else 0 for i in range(len(SHAPES))])
            for i in range(len(SHAPES)):
                st = sd["state"].get(i)
                out["%s_sd_%s_m_%d" % (tag, at, i)] = (st["exp_avg"] if st else torch.zeros(SHAPES[i])).numpy().copy()
                out["%s_sd_%s_v_%d" % (tag, at, i)] = (st["exp_avg_sq"] if st else torch.zeros(SHAPES[i])).numpy().copy()
        if tag == "radam":
            out["radam_buffer"] = np.stack(rec["buf"])
            out["radam_step_size"] = np.stack(rec["ss"])
            out["radam_nsma"] = np.stack(rec["nsma"])
        # resume: a fresh optimizer, the mid-point weights and state_dict, the same gradients and lrs to the end
        mid_params = [torch.nn.Parameter(torch.from_numpy(out["%s_p_%d" % (tag, i)][MID - 1]).clone()) for i in range(len(SHAPES))]
        res, _ = run(cls, init, grads, MID + 1, STEPS, params=mid_params, load=copy.deepcopy(rec["sd"][MID]))     # torch's load keeps the tensors it is given
        for i in range(len(SHAPES)):
            for k in ("p", "m", "v"):
                out["%s_resumed_%s_%d" % (tag, k, i)] = torch.stack([r[i] for r in res[k]]).numpy()
    np.savez_compressed(args.out, **out)
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
