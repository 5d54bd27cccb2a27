"""Optimizer-side drop-ins for the reference's pre-training driver (train_concap.py:21,227-234,307-311):

  AdamW                  pytorch_transformers.optimization.AdamW  (same constructor / param-group semantics)
  WarmupLinearSchedule   pytorch_transformers.optimization.WarmupLinearSchedule
  RAdam, PlainRAdam      volta.optimization.RAdam / PlainRAdam  (train_task.py:27,227-228; see RAdam)
  LAMB                   apex.optimizers.FusedLAMB as the reference tree vendors it  (see LAMB)
  WarmupConstantSchedule pytorch_transformers.optimization.WarmupConstantSchedule  (train_task.py:24,233-234)
  clip_grad_norm_        torch.nn.utils.clip_grad_norm_

All parameters of a volta_amd model are views of one flat arena, so `step()` is ONE fused kernel over
(p, g, m, v) that also refreshes the bf16 weight copies used by the GEMMs, and the gradient norm / clip
coefficient never leave the device.  The arithmetic (decay after the Adam update with the un-corrected lr,
eps outside the bias correction) follows pytorch-transformers 1.1.0 and is pinned by the oracle tests."""
import ctypes as C
import math

import numpy as np
import torch
import weakref

from torch.optim import Optimizer
from torch.optim.lr_scheduler import LambdaLR

from . import _lib as L


def _split_params(params, labels=None):
    """(model, arena, foreign) of a parameter set that may mix ONE volta_amd model's arena parameters with plain CUDA fp32 tensors on the
    same device (a torch head trained on top of a standalone BertModel).  model / arena are None without arena parameters.  Anything else
    raises, naming the offending parameter by `labels[i]` (default: its position)."""
    labels = labels or ["parameter %d" % i for i in range(len(params))]
    owners, foreign = {}, []
    for p, lab in zip(params, labels):
        o = getattr(p, "_vk_owner", None)
        if o is not None:
            owners.setdefault(id(o), (o, lab))
        else:
            foreign.append((p, lab))
    if len(owners) > 1:
        (_, a), (_, b) = list(owners.values())[:2]
        raise RuntimeError("volta_amd optimizers take the parameters of at most one volta_amd model: %s and %s belong to different models" % (a, b))
    model = arena = None
    if owners:
        model = next(iter(owners.values()))[0]
        arena = model.materialize()
    dev = arena.device if arena is not None else None
    for p, lab in foreign:
        if not isinstance(p, torch.Tensor) or p.device.type != "cuda" or p.dtype != torch.float32 or not p.is_contiguous():
            raise RuntimeError("volta_amd optimizers: %s is not a contiguous CUDA float32 tensor nor a volta_amd model's parameter (%s)"
                               % (lab, (p.dtype, tuple(p.shape), str(p.device)) if isinstance(p, torch.Tensor) else type(p).__name__))
        dev = dev or p.device
        if p.device != dev:
            raise RuntimeError("volta_amd optimizers: %s is on %s, the other parameters on %s" % (lab, p.device, dev))
    return model, arena, [p for p, _ in foreign]


def _tensor_list(entries, device):
    """Device array of vk_adamw_tensor descriptors for [(p, g, m, v, class)] and the largest numel (the grid of the list launches)."""
    rows = [(p.data_ptr(), g.data_ptr(), m.data_ptr() if m is not None else 0, v.data_ptr() if v is not None else 0, p.numel(), c)
            for p, g, m, v, c in entries]
    host = (L.AdamwTensor * len(rows))(*[L.AdamwTensor(a, b, c_ or None, d or None, n, k, 0) for a, b, c_, d, n, k in rows])
    dev = torch.frombuffer(bytearray(host), dtype=torch.uint8).to(device, non_blocking=False)
    return dev, max((r[4] for r in rows), default=0)


def _chunks_of(arena, name):
    numel = 1
    for d in arena.shape[name]:
        numel *= d
    return arena.offset[name] // 1024, (arena.offset[name] + numel + 1023) // 1024


def _check_shared_chunks(arena, included, what, among=None):
    """Skipping works on whole 1024-element chunks; only the fused Q|K|V slot packs several tensors into one chunk, and
    those are frozen / trained together in every reference driver."""
    inc, exc = set(), set()
    for n in arena.params:
        if among is not None and n not in among:
            continue
        c0, c1 = _chunks_of(arena, n)
        (inc if n in included else exc).update(range(c0, c1))
    both = inc & exc
    if both:
        raise RuntimeError("volta_amd: parameters sharing an arena chunk (the fused query / key / value slot) must all be %s or none "
                           "of them (chunk %d)" % (what, min(both)))


class AdamW(Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, correct_bias=True, overlap_with_forward=False, overlap_ranges=8):
        """overlap_with_forward: issue the update as `overlap_ranges` launches over consecutive arena ranges (= forward order) on a stream
        of its own; the model's next forward waits range by range for the weights it is about to read, so the HBM-bound update of the late
        layers runs under the MFMA-bound forward of the early ones.  Same arithmetic, same results.  Opt-in because host code that reads
        parameters right after step() WITHOUT a device synchronisation (`p.cpu()` on the current stream) would race with that stream:
        call `optimizer.synchronize()` (or torch.cuda.synchronize()) before such reads."""
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[1]))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(eps))
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, correct_bias=correct_bias))
        self._fused = None
        self._overlap = (bool(overlap_with_forward), int(overlap_ranges))
        # known to the model's arena from construction on (not only from the first step): DistributedDataParallel(mode="zero1") refuses to
        # start a backward whose sharded gradients no volta_amd optimizer would pick up, and the reference's order is model -> DDP -> optimizer
        # -> first backward (train_concap.py:227-253).  Parameters that are not (yet) a materialised volta_amd model's stay lazy (_setup).
        try:
            _, arena, _ = _split_params([p for g in self.param_groups for p in g["params"]])
            if arena is not None:
                arena._vk_adamw = weakref.ref(self)
        except RuntimeError:
            pass

    def _setup(self):
        allp = [p for g in self.param_groups for p in g["params"]]
        labels = ["param_groups[%d]['params'][%d]" % (gi, i) for gi, g in enumerate(self.param_groups) for i in range(len(g["params"]))]
        model, arena, foreign = _split_params(allp, labels)
        if arena is None and not foreign:
            raise RuntimeError("volta_amd.AdamW: no parameters")
        byptr = {p.data_ptr(): n for n, p in arena.params.items()} if arena is not None else {}
        fids = {id(p) for p in foreign}
        # classes: groups with identical (initial lr, wd, betas, eps, correct_bias) share one class; chunks of parameters the
        # optimizer was not given (frozen: train_concap.py:200,213 builds its groups from requires_grad parameters) are skipped
        classes, cls_of_chunk = [], torch.full(((arena.total if arena is not None else 0) // 1024,), L.CHUNK_SKIP, dtype=torch.uint8)
        hyper = None
        spans, fspans = [], []
        for g in self.param_groups:
            h = (tuple(g["betas"]), g["eps"], g["correct_bias"])
            hyper = hyper or h
            if h != hyper:
                raise RuntimeError("volta_amd.AdamW: betas / eps / correct_bias must be common to all groups")
            key = (g.get("initial_lr", g["lr"]), g["weight_decay"])
            if key not in [c[0] for c in classes]:
                if len(classes) == 8:
                    raise RuntimeError("volta_amd.AdamW: more than 8 distinct (lr, weight_decay) classes")
                classes.append((key, g))
            ci = [c[0] for c in classes].index(key)
            for p in g["params"]:
                if id(p) in fids:              # outside the arena: moments of its own, stepped by vk_adamw_step_list
                    fspans.append(dict(p=p, cls=ci, m=torch.zeros_like(p), v=torch.zeros_like(p)))
                    continue
                n = byptr[p.data_ptr()]
                c0, c1 = _chunks_of(arena, n)
                cls_of_chunk[c0:c1] = ci
                spans.append((p, n, c0, c1))
        if arena is None:
            self._fused = dict(model=None, arena=None, classes=classes, spans=[], foreign=fspans, step=0)
            return
        _check_shared_chunks(arena, {n for _, n, _, _ in spans}, "given to the optimizer")
        arena._vk_adamw = weakref.ref(self)       # clip_grad_norm_ hands its coefficient to this optimizer's next step (see there)
        self._fused = dict(model=model, arena=arena, classes=classes, base_class=cls_of_chunk, spans=spans, masks={},
                           chunk_class=cls_of_chunk.to(arena.device), foreign=fspans,
                           m=torch.zeros_like(arena.master), v=torch.zeros_like(arena.master), step=0)

    def _chunk_class_for_step(self):
        """Parameters without a gradient this step are skipped like pytorch_transformers' AdamW does (`if p.grad is None:
        continue`): no moment update, no decay, and never a stale gradient left in the arena by an earlier step."""
        f = self._fused
        arena = f["arena"]
        missing = []
        for i, (p, n, c0, c1) in enumerate(f["spans"]):
            g = p.grad
            if g is None:
                missing.append(i)
            elif g.data_ptr() != arena.grad.data_ptr() + 4 * arena.offset[n]:
                raise RuntimeError("volta_amd.AdamW: the gradient of %s is not the engine's arena view (a foreign tensor was "
                                   "assigned to .grad); run backward through the model, or zero_grad(set_to_none=True)" % n)
        if not missing:
            return f["chunk_class"]
        key = tuple(missing)
        if key not in f["masks"]:
            if len(f["masks"]) > 16:
                f["masks"].clear()
            _check_shared_chunks(arena, {f["spans"][i][1] for i in range(len(f["spans"])) if i not in set(missing)}, "with a gradient this step",
                                 among={sp[1] for sp in f["spans"]})
            cc = f["base_class"].clone()
            for i in missing:
                cc[f["spans"][i][2]:f["spans"][i][3]] = L.CHUNK_SKIP
            f["masks"][key] = cc.to(arena.device)
        return f["masks"][key]

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        loss = closure() if closure is not None else None
        if self._fused is None:
            self._setup()
        f = self._fused
        arena = f["arena"]
        if f.get("foreign", ()) and self._zero1_reducer() is not None:
            raise NotImplementedError("volta_amd.AdamW: data-parallel mode 'zero1' with parameters outside the model's arena")
        f["step"] += 1
        a = L.AdamwArgs()
        if arena is None:                  # torch tensors only
            self._fill_hyper(a, f)
            self._step_foreign(a)
            return loss
        a.p, a.g, a.m, a.v = arena.master.data_ptr(), arena.grad.data_ptr(), f["m"].data_ptr(), f["v"].data_ptr()
        a.shadow, a.chunk_class = arena.shadow.data_ptr(), self._chunk_class_for_step().data_ptr()
        pend = getattr(arena, "pending_clip", None)
        clip = None
        if pend is not None:
            if pend[1] == self._grad_names():
                clip = pend[0]                     # the coefficient was computed over exactly the gradients this step consumes: folded into the pass
            else:
                flush_clip(arena)                  # another parameter set: applied to its gradients first
        a.clip = clip.data_ptr() if clip is not None else None
        arena.pending_clip = None
        a.n = arena.total
        self._fill_hyper(a, f, grad_scale)
        arena.sync_optimizer()         # an earlier pipelined step nobody waited for (two steps without a forward in between)
        red = self._zero1_reducer()
        if red is not None:
            self._step_zero1(a, arena, red)
        elif not self._overlap[0]:
            L.check(L.lib.vk_adamw_step(C.byref(a), L.stream_ptr()))
        else:
            self._step_pipelined(a, arena, clip)
        arena.mark_shadow_fresh()      # the kernel refreshed the bf16 copies itself
        self._step_foreign(a)          # same arguments (classes, step, scale, deferred clip), on the current stream
        return loss

    def _fill_hyper(self, a, f, grad_scale=1.0):
        """Class lr / wd, betas, eps, bias correction and gradient scale of this step into vk_adamw_args `a`."""
        g0 = self.param_groups[0]
        b1, b2 = g0["betas"]
        for i, (key, grp) in enumerate(f["classes"]):
            a.cls_lr_mult[i] = grp["lr"]          # current (scheduled) lr of the class
            a.cls_wd[i] = grp["weight_decay"]
        a.lr, a.beta1, a.beta2, a.eps = 1.0, b1, b2, g0["eps"]
        t = f["step"]
        a.step_mult = math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t) if g0["correct_bias"] else 1.0
        a.grad_scale = grad_scale

    def _step_foreign(self, a):
        """One vk_adamw_step_list launch over the tensors outside the arena that carry a gradient (the others are skipped, as
        pytorch_transformers' AdamW skips `p.grad is None`)."""
        f = self._fused
        live = [(t["p"], t["p"].grad, t["m"], t["v"], t["cls"]) for t in f.get("foreign", ()) if t["p"].grad is not None]
        if not live:
            return
        for p, g, _, _, _ in live:
            if g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape or g.device != p.device:
                raise RuntimeError("volta_amd.AdamW: the gradient of a tensor outside the arena must be a contiguous float32 tensor of its shape")
        key = tuple((p.data_ptr(), g.data_ptr()) for p, g, _, _, _ in live)
        if f.get("flist_key") != key:          # .grad tensors change when autograd allocates new ones (zero_grad(set_to_none=True))
            f["flist"], f["flist_max"] = _tensor_list(live, live[0][0].device)
            f["flist_key"] = key
        L.check(L.lib.vk_adamw_step_list(C.byref(a), L.ptr(f["flist"]), len(live), f["flist_max"], L.stream_ptr()))

    def _grad_names(self):
        """Names of this optimizer's parameters that carry a gradient now (the set a deferred clip coefficient must have been computed over);
        tensors outside the arena count as ("foreign", id)."""
        f = self._fused
        return frozenset([n for p, n, _, _ in f["spans"] if p.grad is not None] + [("foreign", id(t["p"])) for t in f.get("foreign", ()) if t["p"].grad is not None])

    def _zero1_reducer(self):
        """The data-parallel wrapper's reducer when it runs in mode "zero1" and the last backward left this rank with shards to step."""
        ddp = getattr(self._fused["model"], "_ddp", None) if self._fused else None
        red = getattr(ddp, "reducer", None)
        if red is None or red.mode != "zero1" or not (red.sharded or red.replicated):
            return None
        return red

    def _step_zero1(self, a, arena, red):
        """Sharded step (volta_amd/parallel.py, mode "zero1"): the fused kernel runs over the element ranges this rank owns -- its 1/world
        shard of every bucket plus the few replicated slots -- then the updated master weights are all-gathered and the bf16 copies re-cast.
        The moments of foreign shards are left alone; should the shard layout change (another batch shape compiles another bucket plan),
        they are gathered under the old layout first."""
        f = self._fused
        layout = tuple(red.sharded)
        prev = f.get("zero1_layout")
        if prev is not None and prev != layout:
            red.gather(f["m"], prev)
            red.gather(f["v"], prev)
        f["zero1_layout"] = layout
        base = (a.p, a.g, a.m, a.v, a.shadow, a.chunk_class)
        for lo, hi in red.owned():
            assert lo % 1024 == 0 and hi % 1024 == 0 and hi > lo, (lo, hi)
            a.p, a.g, a.m, a.v = base[0] + 4 * lo, base[1] + 4 * lo, base[2] + 4 * lo, base[3] + 4 * lo
            a.shadow, a.chunk_class = base[4] + 2 * lo, base[5] + lo // 1024
            a.n = hi - lo
            L.check(L.lib.vk_adamw_step(C.byref(a), L.stream_ptr()))
        f["model"]._ddp.gather_params(arena)

    def _step_pipelined(self, a, arena, clip):
        f = self._fused
        if "stream" not in f:
            n = max(1, min(self._overlap[1], arena.total // 1024))
            nchunks = arena.total // 1024
            from .streams import independent_stream, engine_streams
            ddp = getattr(f["model"], "_ddp", None)
            comm = getattr(getattr(ddp, "reducer", None), "stream", None)
            with torch.cuda.device(arena.device):          # clear of the compute, weight-gradient and communication streams' hardware queues
                f["stream"] = independent_stream(engine_streams(), device=arena.device, soft_avoid=[comm] if comm is not None else [])
            f["bounds"] = [nchunks * (i + 1) // n for i in range(n)]
            f["events"] = [torch.cuda.Event() for _ in range(n)]
        side, bounds, events = f["stream"], f["bounds"], f["events"]
        side.wait_stream(torch.cuda.current_stream())          # gradients, their norm and the clip coefficient are final
        if clip is not None:
            clip.record_stream(side)
        base = (a.p, a.g, a.m, a.v, a.shadow, a.chunk_class)
        with torch.cuda.stream(side):
            sp = C.c_void_p(side.cuda_stream)
            lo = 0
            for hi, ev in zip(bounds, events):
                if hi > lo:
                    off = lo * 1024
                    a.p, a.g, a.m, a.v = base[0] + 4 * off, base[1] + 4 * off, base[2] + 4 * off, base[3] + 4 * off
                    a.shadow, a.chunk_class = base[4] + 2 * off, base[5] + lo
                    a.n = (hi - lo) * 1024
                    L.check(L.lib.vk_adamw_step(C.byref(a), sp))
                ev.record(side)
                lo = hi
        arena.opt_pending = (bounds, events)

    def synchronize(self):
        """Current stream waits for a pipelined step (needed only before host code reads parameters without a device sync)."""
        if self._fused is not None and self._fused["arena"] is not None:
            self._fused["arena"].sync_optimizer()

    # ---- checkpoint interchange (volta/train_utils.py:295-340 saves optimizer.state_dict() of pytorch_transformers'
    # AdamW: per parameter {"step", "exp_avg", "exp_avg_sq"}, indexed in param_groups order)
    def _spans(self):
        """Per parameter in param_groups order: (arena offset, numel, shape) or, outside the arena, its foreign entry."""
        arena = self._fused["arena"]
        byptr = {p.data_ptr(): n for n, p in arena.params.items()} if arena is not None else {}
        fmap = {id(t["p"]): t for t in self._fused.get("foreign", ())}
        out = []
        for g in self.param_groups:
            for p in g["params"]:
                if id(p) in fmap:
                    out.append(fmap[id(p)])
                    continue
                n = byptr[p.data_ptr()]
                numel = 1
                for d in arena.shape[n]:
                    numel *= d
                out.append((arena.offset[n], numel, tuple(arena.shape[n])))
        return out

    def consolidate_state_dict(self):
        """Data-parallel mode "zero1": every rank holds the moments of its own shards only.  COLLECTIVE -- every rank calls it -- gathers
        them so that `state_dict()` (which the reference calls on rank 0 alone, volta/train_utils.py:295-316) has the whole state.
        A no-op without a sharded optimizer, so a driver may call it unconditionally in front of its `if default_gpu:` save."""
        self.synchronize()
        if self._fused is None:
            return
        f = self._fused
        red = self._zero1_reducer()
        if red is not None and f.get("zero1_layout"):
            red.gather(f["m"], f["zero1_layout"])
            red.gather(f["v"], f["zero1_layout"])
        f["zero1_consolidated_at"] = f["step"]

    def state_dict(self):
        """Collective-free (the reference's checkpoint flow enters it on one rank).  Under "zero1" the moments must have been gathered by
        `consolidate_state_dict()` since the last step; otherwise this raises instead of saving other ranks' stale shards."""
        self.synchronize()
        if self._fused is not None and self._fused.get("zero1_layout") and self._fused.get("zero1_consolidated_at") != self._fused["step"]:
            raise RuntimeError("volta_amd.AdamW.state_dict(): the optimizer state is sharded over the data-parallel ranks (mode 'zero1'); "
                               "call optimizer.consolidate_state_dict() on EVERY rank first, then state_dict() on the saving rank")
        sd = super().state_dict()
        if self._fused is not None and self._fused["step"] > 0:
            f = self._fused
            sd["state"] = {i: ({"step": f["step"], "exp_avg": sp["m"].clone(), "exp_avg_sq": sp["v"].clone()} if isinstance(sp, dict) else
                               {"step": f["step"], "exp_avg": f["m"][sp[0]:sp[0] + sp[1]].view(sp[2]).clone(),
                                "exp_avg_sq": f["v"][sp[0]:sp[0] + sp[1]].view(sp[2]).clone()})
                           for i, sp in enumerate(self._spans())}
        return sd

    def load_state_dict(self, state_dict):
        self.synchronize()
        state = state_dict.get("state", {})
        super().load_state_dict({"state": {}, "param_groups": state_dict["param_groups"]})
        if not state:
            return
        if self._fused is None:
            self._setup()
        f = self._fused
        spans = self._spans()
        if len(state) != len(spans):
            raise ValueError("volta_amd.AdamW.load_state_dict: the checkpoint holds %d parameter states, the optimizer %d parameters" % (len(state), len(spans)))
        steps = set()
        for i, sp in enumerate(spans):
            st = state[i] if i in state else state[str(i)]
            if isinstance(sp, dict):
                sp["m"].copy_(st["exp_avg"].reshape(sp["m"].shape))
                sp["v"].copy_(st["exp_avg_sq"].reshape(sp["v"].shape))
            else:
                o, n, shape = sp
                f["m"][o:o + n].copy_(st["exp_avg"].reshape(-1))
                f["v"][o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
            steps.add(int(st["step"]))
        if len(steps) != 1:
            raise ValueError("volta_amd.AdamW.load_state_dict: parameters at different step counts %s (one fused launch updates all of them)" % sorted(steps))
        f["step"] = steps.pop()

    def zero_grad(self, set_to_none=True):
        if self._fused is not None and self._fused["arena"] is not None:
            self._fused["arena"].pending_clip = None       # a coefficient nobody consumed dies with the gradients it was computed for
        for g in self.param_groups:
            for p in g["params"]:
                if set_to_none:
                    p.grad = None
                elif p.grad is not None:
                    p.grad.zero_()


def _radam_step_size(lr, t, beta1, beta2):
    """(step_size, N_sma) of step t in the reference's own expression order (volta/optimization.py:57-78, :143-165), in Python floats."""
    beta2_t = beta2 ** t
    N_sma_max = 2 / (1 - beta2) - 1
    N_sma = N_sma_max - 2 * t * beta2_t / (1 - beta2_t)
    if N_sma >= 5:
        step_size = (lr * math.sqrt((1 - beta2_t) * (N_sma - 4) / (N_sma_max - 4) * (N_sma - 2) / N_sma * N_sma_max / (N_sma_max - 2))
                     / (1 - beta1 ** t))
    else:
        step_size = lr / (1 - beta1 ** t)
    return step_size, N_sma


def radam_runs(steps, live, lr_of, uniform=None):
    """The stepping parameters of one RAdam step as runs of equal step count, in param_groups order.  steps[i]: parameter i's step count
    before this step, live[i]: it has a gradient, lr_of(i): its group's lr now.  Returns (runs, run_of): runs = [(t, lr of the run's first
    parameter)] with t the count after this step; run_of[i] = the run of parameter i, -1 when it does not step.  Within a run only the first
    parameter can miss the reference's buffer: every later one finds the slot it filled.  `uniform`: the common count, when the caller
    knows every parameter has it -- with every parameter live that is one run, found without a walk (run_of None: all in run 0)."""
    if uniform is not None and all(live):
        return [(uniform + 1, lr_of(0))], None
    runs, run_of, prev = [], [-1] * len(steps), None
    for i, t in enumerate(steps):
        if not live[i]:
            continue
        t += 1
        if t != prev:
            runs.append((t, lr_of(i)))
            prev = t
        run_of[i] = len(runs) - 1
    return runs, run_of


def radam_plan(buffer, runs, beta1, beta2):
    """The reference RAdam's shared step-size cache (volta/optimization.py:12,51-80) over `runs` (radam_runs): per run (step_size,
    rectified), `buffer` (10 slots [step, N_sma, step_size], slot = step % 10) updated in place exactly as the reference's loop leaves it.
    The first parameter to reach step t with slot t % 10 not holding t computes the step size from ITS group's lr and stores it; every
    later parameter at step t reuses it (another group's lr), until a different step count claims the slot."""
    out = []
    for t, lr in runs:
        b = buffer[int(t % 10)]
        if t == b[0]:
            N_sma, step_size = b[1], b[2]
        else:
            step_size, N_sma = _radam_step_size(lr, t, beta1, beta2)
            b[0], b[1], b[2] = t, N_sma, step_size
        out.append((step_size, N_sma >= 5))
    return out


class RAdam(Optimizer):
    """volta.optimization.RAdam (train_task.py:27,227-228, `--optim RAdam`): same constructor, param-group semantics, `buffer` and
    state_dict layout; one fused launch over the arena (vk_radam_step) plus one over tensors outside it (vk_radam_step_list) per step.

    Reference semantics kept on purpose: all parameters share the 10-slot step-size cache `self.buffer` (radam_plan), so the step size of
    a parameter can come from another group's lr; only the decay `-weight_decay * lr * p`, applied BEFORE the update, uses the group's own
    lr.  A parameter without a gradient is skipped and its step count stays behind.  Accepts one volta_amd model's parameters plus
    contiguous CUDA fp32 tensors, as AdamW does; clip_grad_norm_ defers its coefficient to this optimizer's next step the same way.
    Out of scope (raise): DistributedDataParallel(mode="zero1") (NotImplementedError), groups with different betas or eps (RuntimeError),
    and there is no overlap_with_forward form."""
    _plain = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[1]))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(eps))
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        if not self._plain:
            self.buffer = [[None, None, None] for _ in range(10)]
        self._hyper()
        self._fused = None
        self._pending = None        # a state loaded before the model was on the GPU (train_task.py:236-246): applied at the first setup
        try:                        # clip_grad_norm_ defers to this optimizer (see AdamW.__init__)
            _, arena, _ = _split_params([p for g in self.param_groups for p in g["params"]])
            if arena is not None:
                arena._vk_adamw = weakref.ref(self)
        except RuntimeError:
            pass

    def _name(self):
        return "volta_amd." + type(self).__name__

    def _hyper(self):
        """(beta1, beta2, eps) common to all groups: one launch steps all of them."""
        hs = {(tuple(g["betas"]), g["eps"]) for g in self.param_groups}
        if len(hs) != 1:
            raise RuntimeError("%s: betas / eps must be common to all groups (got %s)" % (self._name(), sorted(hs)))
        (b1, b2), eps = hs.pop()
        return float(b1), float(b2), float(eps)

    def _setup(self):
        allp = [p for g in self.param_groups for p in g["params"]]
        labels = ["param_groups[%d]['params'][%d]" % (gi, i) for gi, g in enumerate(self.param_groups) for i in range(len(g["params"]))]
        model, arena, foreign = _split_params(allp, labels)
        if arena is None and not foreign:
            raise RuntimeError("%s: no parameters" % self._name())
        byptr = {p.data_ptr(): n for n, p in arena.params.items()} if arena is not None else {}
        fids = {id(p) for p in foreign}
        ents = []                   # per parameter in param_groups order: (group index, arena name or None, chunk range, foreign record)
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                if id(p) in fids:
                    ents.append((gi, p, None, 0, 0, dict(p=p, m=torch.zeros_like(p), v=torch.zeros_like(p))))
                else:
                    n = byptr[p.data_ptr()]
                    c0, c1 = _chunks_of(arena, n)
                    ents.append((gi, p, n, c0, c1, None))
        f = dict(model=model, arena=arena, ents=ents, steps=[0] * len(ents), uniform=0, masks={})
        if arena is not None:
            arena._vk_adamw = weakref.ref(self)
            f.update(m=torch.zeros_like(arena.master), v=torch.zeros_like(arena.master))
        self._fused = f
        if self._pending is not None:
            self._apply_state(self._pending)
            self._pending = None

    def _grad_names(self):
        """Names of this optimizer's parameters that carry a gradient now (what a deferred clip coefficient must have been computed over)."""
        return frozenset(n if n is not None else ("foreign", id(p)) for _, p, n, _, _, _ in self._fused["ents"] if p.grad is not None)

    def _plan(self, live, b1, b2):
        """Per parameter: (step_size, rectified), or None for a parameter that does not step.  RAdam: the shared buffer (radam_plan);
        PlainRAdam: each parameter's own group lr and step count (volta/optimization.py:143-165)."""
        f, groups, ents = self._fused, self.param_groups, self._fused["ents"]
        lr_of = lambda i: groups[ents[i][0]]["lr"]
        if self._plain:
            memo = {}
            out = []
            for i, t in enumerate(f["steps"]):
                if not live[i]:
                    out.append(None)
                    continue
                key = (lr_of(i), t + 1)
                if key not in memo:
                    ss, N_sma = _radam_step_size(key[0], key[1], b1, b2)
                    memo[key] = (ss, N_sma >= 5)
                out.append(memo[key])
            return out
        runs, run_of = radam_runs(f["steps"], live, lr_of, f["uniform"])
        plan = radam_plan(self.buffer, runs, b1, b2)
        if run_of is None:
            return [plan[0]] * len(live)
        return [plan[r] if r >= 0 else None for r in run_of]

    def _chunk_map(self, cls_of):
        """Device chunk-class bytes for the arena parameters' classes (cached by the class tuple: a steady run reuses one map)."""
        f = self._fused
        arena = f["arena"]
        key = tuple(c for (_, _, n, _, _, _), c in zip(f["ents"], cls_of) if n is not None)
        cc = f["masks"].get(key)
        if cc is None:
            own = np.full(arena.total // 1024, -1, dtype=np.int16)
            for (_, _, n, c0, c1, _), c in zip(f["ents"], cls_of):
                if n is None:
                    continue
                for e in {c0, c1 - 1}:
                    if own[e] not in (-1, c):
                        raise RuntimeError("%s: parameters sharing an arena chunk (the fused query / key / value slot) must step together with "
                                           "the same lr, weight decay and step count (%s, chunk %d)" % (self._name(), n, e))
                own[c0:c1] = c
            own[own < 0] = L.CHUNK_SKIP
            if len(f["masks"]) > 16:
                f["masks"].clear()
            cc = f["masks"][key] = torch.from_numpy(own.astype(np.uint8)).to(arena.device)
        return cc

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        loss = closure() if closure is not None else None
        if self._fused is None:
            self._setup()
        f = self._fused
        arena, ents = f["arena"], f["ents"]
        red = getattr(getattr(f["model"], "_ddp", None), "reducer", None)
        if red is not None and red.mode == "zero1":
            raise NotImplementedError("%s: data-parallel mode 'zero1' shards the optimizer state for AdamW only; use mode 'allreduce' or "
                                      "'rs_ag'" % self._name())
        b1, b2, eps = self._hyper()
        live = []
        for gi, p, n, _, _, _ in ents:
            g = p.grad
            live.append(g is not None)
            if g is None:
                continue
            if n is not None:
                if g.data_ptr() != arena.grad.data_ptr() + 4 * arena.offset[n]:
                    raise RuntimeError("%s: the gradient of %s is not the engine's arena view (a foreign tensor was assigned to .grad); run "
                                       "backward through the model, or zero_grad(set_to_none=True)" % (self._name(), n))
            elif g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape or g.device != p.device:
                raise RuntimeError("%s: the gradient of a tensor outside the arena must be a contiguous float32 tensor of its shape" % self._name())
        if not any(live):
            return loss
        plan = self._plan(live, b1, b2)
        # classes: (decay = weight_decay * group lr, step size, rectified); the kernels look them up by class index
        classes, cls_of = {}, []
        for (gi, _, _, _, _, _), pl in zip(ents, plan):
            if pl is None:
                cls_of.append(L.CHUNK_SKIP)
                continue
            g = self.param_groups[gi]
            key = (g["weight_decay"] * g["lr"], pl[0], bool(pl[1]))
            if key not in classes:
                if len(classes) == L.RADAM_CLASSES:
                    raise RuntimeError("%s: more than %d distinct (lr, weight decay, step count) classes in one step" % (self._name(), L.RADAM_CLASSES))
                classes[key] = len(classes)
            cls_of.append(classes[key])
        a = L.RadamArgs()
        for (decay, ss, rect), c in classes.items():
            a.cls_decay[c], a.cls_step[c], a.cls_rect[c] = decay, ss, int(rect)
        a.beta1, a.beta2, a.one_minus_beta1, a.one_minus_beta2, a.eps, a.grad_scale = b1, b2, 1 - b1, 1 - b2, eps, grad_scale
        clip = None
        if arena is not None:
            pend = getattr(arena, "pending_clip", None)
            if pend is not None:
                if pend[1] == self._grad_names():
                    clip = pend[0]             # computed over exactly the gradients this step consumes: folded into the pass
                else:
                    flush_clip(arena)
            arena.pending_clip = None
            a.clip = clip.data_ptr() if clip is not None else None
            if any(l and e[2] is not None for l, e in zip(live, ents)):
                a.p, a.g, a.m, a.v = arena.master.data_ptr(), arena.grad.data_ptr(), f["m"].data_ptr(), f["v"].data_ptr()
                a.shadow, a.chunk_class, a.n = arena.shadow.data_ptr(), self._chunk_map(cls_of).data_ptr(), arena.total
                arena.sync_optimizer()
                L.check(L.lib.vk_radam_step(C.byref(a), L.stream_ptr()))
                arena.mark_shadow_fresh()
        flive = [(e[5]["p"], e[5]["p"].grad, e[5]["m"], e[5]["v"], c) for l, e, c in zip(live, ents, cls_of) if l and e[2] is None]
        if flive:
            key = tuple((p.data_ptr(), g.data_ptr(), c) for p, g, _, _, c in flive)
            if f.get("flist_key") != key:
                f["flist"], f["flist_max"] = _tensor_list(flive, flive[0][0].device)
                f["flist_key"] = key
            L.check(L.lib.vk_radam_step_list(C.byref(a), L.ptr(f["flist"]), len(flive), f["flist_max"], L.stream_ptr()))
        steps = f["steps"]
        if f["uniform"] is not None and all(live):
            f["uniform"] += 1
            for i in range(len(steps)):
                steps[i] += 1
        else:
            for i, l in enumerate(live):
                steps[i] += l
            f["uniform"] = steps[0] if steps and all(t == steps[0] for t in steps) else None
        return loss

    def zero_grad(self, set_to_none=True):
        if self._fused is not None and self._fused["arena"] is not None:
            self._fused["arena"].pending_clip = None
        for g in self.param_groups:
            for p in g["params"]:
                if set_to_none:
                    p.grad = None
                elif p.grad is not None:
                    p.grad.zero_()

    def synchronize(self):
        if self._fused is not None and self._fused["arena"] is not None:
            self._fused["arena"].sync_optimizer()

    # ---- checkpoints: the reference's layout, {"step", "exp_avg", "exp_avg_sq"} per parameter that has stepped, indexed in param_groups
    # order; `buffer` is not part of it (volta/optimization.py keeps it outside `state`), so it starts empty after a load
    def state_dict(self):
        self.synchronize()
        sd = super().state_dict()
        f = self._fused
        if f is None:
            sd["state"] = {i: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()} for i, st in (self._pending or {}).items()}
            return sd
        out = {}
        for i, ((_, p, n, _, _, fr), t) in enumerate(zip(f["ents"], f["steps"])):
            if t == 0:
                continue
            if fr is not None:
                m, v = fr["m"].clone(), fr["v"].clone()
            else:
                o, k = f["arena"].offset[n], p.numel()
                m, v = f["m"][o:o + k].view(p.shape).clone(), f["v"][o:o + k].view(p.shape).clone()
            out[i] = {"step": t, "exp_avg": m, "exp_avg_sq": v}
        sd["state"] = out
        return sd

    def load_state_dict(self, state_dict):
        self.synchronize()
        state = state_dict.get("state", {})
        super().load_state_dict({"state": {}, "param_groups": state_dict["param_groups"]})
        self._hyper()
        if not self._plain:
            self.buffer = [[None, None, None] for _ in range(10)]
        allp = [p for g in self.param_groups for p in g["params"]]
        st = {}
        for k, s in state.items():
            i = int(k)
            if not 0 <= i < len(allp):
                raise ValueError("%s.load_state_dict: state for parameter %d, the optimizer has %d" % (self._name(), i, len(allp)))
            if int(s["step"]) < 1 or s["exp_avg"].numel() != allp[i].numel() or s["exp_avg_sq"].numel() != allp[i].numel():
                raise ValueError("%s.load_state_dict: parameter %d's state does not fit it (step %s, %d / %d elements for %d)"
                                 % (self._name(), i, s["step"], s["exp_avg"].numel(), s["exp_avg_sq"].numel(), allp[i].numel()))
            st[i] = {"step": int(s["step"]), "exp_avg": s["exp_avg"].detach().float().cpu().clone(),
                     "exp_avg_sq": s["exp_avg_sq"].detach().float().cpu().clone()}
        if self._fused is None and not all(p.device.type == "cuda" for p in allp):
            self._pending = st          # the model is not on the GPU yet (train_task.py: resume() before model.to(device))
            return
        if self._fused is None:
            self._setup()
        self._apply_state(st)

    def _apply_state(self, st):
        f = self._fused
        for i, (_, p, n, _, _, fr) in enumerate(f["ents"]):
            s = st.get(i)
            m = s["exp_avg"].reshape(-1) if s is not None else 0.0
            v = s["exp_avg_sq"].reshape(-1) if s is not None else 0.0
            if fr is not None:
                dm, dv = fr["m"].view(-1), fr["v"].view(-1)
            else:
                o, k = f["arena"].offset[n], p.numel()
                dm, dv = f["m"][o:o + k], f["v"][o:o + k]
            if s is None:
                dm.zero_(); dv.zero_()
            else:
                dm.copy_(m); dv.copy_(v)
            f["steps"][i] = s["step"] if s is not None else 0
        steps = f["steps"]
        f["uniform"] = steps[0] if steps and all(t == steps[0] for t in steps) else None


class PlainRAdam(RAdam):
    """volta.optimization.PlainRAdam (volta/optimization.py:96-169): RAdam with each parameter's step size from its own group's lr and
    step count, and no shared buffer.  Same kernels, same scope."""
    _plain = True


# numpy mirrors of vk_lamb_tensor / vk_lamb_piece / vk_lamb_group (include/volta_hip.h): the tables are built as arrays, not row by row
_LAMB_TENSOR = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("shadow", "<u8"), ("numel", "<i8"), ("cls", "<i4"),
                         ("group", "<i4"), ("piece0", "<i4"), ("npieces", "<i4")])
_LAMB_PIECE = np.dtype([("offset", "<i8"), ("tensor", "<i4"), ("count", "<i4")])
_LAMB_GROUP = np.dtype([("piece0", "<i4"), ("piece1", "<i4"), ("max_grad_norm", "<f4"), ("reserved_", "<i4")])
assert (_LAMB_TENSOR.itemsize, _LAMB_PIECE.itemsize, _LAMB_GROUP.itemsize) == (C.sizeof(L.LambTensor), C.sizeof(L.LambPiece), C.sizeof(L.LambGroup))


def lamb_tables(rows, max_norms, piece=L.LAMB_PIECE):
    """The host tables of vk_lamb_step for `rows` = [(p, g, m, v, shadow or 0, numel, class, group)] (addresses as integers, groups
    ascending) and the groups' max_grad_norm (<= 0 or None: no clipping): (tensors, pieces, groups) as numpy record arrays.  Every tensor
    is tiled exactly once by consecutive pieces of at most `piece` elements, in offset order (64-bit offsets); a piece never crosses a
    tensor, so tensors that share an arena chunk (the biases of a fused query / key / value slot) get pieces, and norms, of their own."""
    T = np.zeros(len(rows), dtype=_LAMB_TENSOR)
    for k, name in enumerate(("p", "g", "m", "v", "shadow", "numel", "cls", "group")):
        T[name] = [r[k] for r in rows]
    numel = T["numel"].astype(np.int64)
    if len(rows) and (numel.min() < 0 or np.any(np.diff(T["group"]) < 0) or T["group"].min() < 0 or T["group"].max() >= len(max_norms)):
        raise ValueError("lamb_tables: negative numel, or groups that do not ascend within 0 .. %d" % (len(max_norms) - 1))
    npc = (numel + piece - 1) // piece
    first = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(npc)])
    if first[-1] >= 2 ** 31:
        raise ValueError("lamb_tables: %d pieces" % first[-1])
    T["piece0"], T["npieces"] = first[:-1], npc
    P = np.zeros(int(first[-1]), dtype=_LAMB_PIECE)
    owner = np.repeat(np.arange(len(rows), dtype=np.int64), npc)
    P["tensor"] = owner
    P["offset"] = (np.arange(len(P), dtype=np.int64) - first[owner]) * piece
    P["count"] = np.minimum(piece, numel[owner] - P["offset"])
    G = np.zeros(len(max_norms), dtype=_LAMB_GROUP)
    G["max_grad_norm"] = [float(x) if x is not None and x > 0 else 0.0 for x in max_norms]
    ends = np.zeros(len(max_norms), dtype=np.int64)          # pieces of groups 0 .. n, cumulative
    np.add.at(ends, T["group"], npc)
    ends = np.cumsum(ends)
    G["piece1"] = ends
    G["piece0"][1:] = ends[:-1]
    return T, P, G


class LAMB(Optimizer):
    """apex.optimizers.FusedLAMB as the reference tree vendors it (apex/apex/optimizers/fused_lamb.py over apex/csrc/multi_tensor_lamb.cu):
    same constructor, param-group semantics (`group["step"]` counts per group, and advances every step) and state_dict layout; Adam
    moments, then one trust ratio lr * |p| / |update| per parameter tensor -- query, key and value of a fused slot are three tensors with
    three ratios.  One vk_lamb_step call per step (csrc/lamb.hip: six launches whatever the number of parameters) over the arena views and
    the tensors outside the arena alike; lr, step, the clip divisor and a deferred clip_grad_norm_ coefficient reach the kernels without a
    host read or a rebuilt table.  The semantics are spelled out at vk_lamb_step in include/volta_hip.h.

    Differences from apex, on purpose:
      * `.grad` keeps its bits across step() (apex overwrites it with the update): gradient accumulation and the data-parallel reducer
        read that arena.  The second stage recomputes the update instead.
      * max_grad_norm None or <= 0 disables this optimizer's own clipping (the vendored kernel would divide by it).
      * global_grad_norm=True takes ONE gradient norm over all groups, as later apex versions do; the default, False, is the vendored
        behaviour: one norm per param group, over the tensors of that group stepped this call.
      * the norm is that of the gradient the step consumes: g * grad_scale * (deferred clip coefficient).
    Accepts what RAdam accepts: one volta_amd model's parameters plus contiguous CUDA fp32 tensors.  lr, weight_decay and max_grad_norm
    may differ per group (at most 64 distinct (lr, weight_decay, step) combinations in one step); betas, eps, bias_correction and
    grad_averaging are common to all groups.  Out of scope (raise): amsgrad (RuntimeError, as apex), DistributedDataParallel(mode="zero1")
    (NotImplementedError), and there is no overlap_with_forward form."""

    def __init__(self, params, lr=1e-3, bias_correction=True, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, amsgrad=False,
                 adam_w_mode=True, grad_averaging=True, set_grad_none=True, max_grad_norm=1.0, global_grad_norm=False):
        if amsgrad:
            raise RuntimeError("volta_amd.LAMB does not support the AMSGrad variant.")
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[1]))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(eps))
        super().__init__(params, dict(lr=lr, bias_correction=bias_correction, betas=betas, eps=eps, weight_decay=weight_decay,
                                      grad_averaging=grad_averaging, max_grad_norm=max_grad_norm))
        self.adam_w_mode = 1 if adam_w_mode else 0
        self.set_grad_none = set_grad_none
        self.global_grad_norm = bool(global_grad_norm)
        self._hyper()
        self._fused = None
        self._pending = None        # a state loaded before the model was on the GPU: applied at the first setup (see RAdam)
        try:                        # clip_grad_norm_ defers to this optimizer (see AdamW.__init__)
            model, arena, _ = _split_params([p for g in self.param_groups for p in g["params"]])
        except RuntimeError:
            model = arena = None
        if arena is not None:
            self._refuse_zero1(model)
            arena._vk_adamw = weakref.ref(self)

    def _hyper(self):
        """(beta1, beta2, eps, bias_correction, grad_averaging) common to all groups: one call steps all of them."""
        hs = {(tuple(g["betas"]), g["eps"], bool(g["bias_correction"]), bool(g["grad_averaging"])) for g in self.param_groups}
        if len(hs) != 1:
            raise RuntimeError("volta_amd.LAMB: betas / eps / bias_correction / grad_averaging must be common to all groups (got %s)" % sorted(hs))
        (b1, b2), eps, bc, ga = hs.pop()
        return float(b1), float(b2), float(eps), bc, ga

    @staticmethod
    def _refuse_zero1(model):
        red = getattr(getattr(model, "_ddp", None), "reducer", None)
        if red is not None and red.mode == "zero1":
            raise NotImplementedError("volta_amd.LAMB: data-parallel mode 'zero1' shards the optimizer state for AdamW only, and a trust ratio "
                                      "needs whole tensors; use mode 'allreduce' or 'rs_ag'")

    def _setup(self):
        allp = [p for g in self.param_groups for p in g["params"]]
        labels = ["param_groups[%d]['params'][%d]" % (gi, i) for gi, g in enumerate(self.param_groups) for i in range(len(g["params"]))]
        model, arena, foreign = _split_params(allp, labels)
        if arena is None and not foreign:
            raise RuntimeError("volta_amd.LAMB: no parameters")
        byptr = {p.data_ptr(): n for n, p in arena.params.items()} if arena is not None else {}
        fids = {id(p) for p in foreign}
        ents = []                   # per parameter in param_groups order: (group index, parameter, arena name or None, moments outside the arena)
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                if id(p) in fids:
                    ents.append((gi, p, None, dict(m=torch.zeros_like(p), v=torch.zeros_like(p))))
                else:
                    ents.append((gi, p, byptr[p.data_ptr()], None))
        f = dict(model=model, arena=arena, ents=ents, stepped=[False] * len(ents), tables={}, last=None)
        if arena is not None:
            arena._vk_adamw = weakref.ref(self)
            f.update(m=torch.zeros_like(arena.master), v=torch.zeros_like(arena.master))
        self._fused = f
        if self._pending is not None:
            self._apply_state(self._pending)
            self._pending = None

    def _grad_names(self):
        """Names of this optimizer's parameters that carry a gradient now (what a deferred clip coefficient must have been computed over)."""
        return frozenset(n if n is not None else ("foreign", id(p)) for _, p, n, _ in self._fused["ents"] if p.grad is not None)

    def _moments(self, i):
        """(exp_avg, exp_avg_sq) of parameter i as flat views."""
        f = self._fused
        _, p, n, fr = f["ents"][i]
        if fr is not None:
            return fr["m"].view(-1), fr["v"].view(-1)
        o, k = f["arena"].offset[n], p.numel()
        return f["m"][o:o + k], f["v"][o:o + k]

    def _tables(self, key, rows, labels, max_norms, device):
        """Host and device tables, scratch and ratio table for this (liveness, pointer, class) pattern: built once, reused while it holds."""
        f = self._fused
        t = f["tables"].get(key)
        if t is None:
            T, P, G = lamb_tables(rows(), max_norms)
            nbytes = L.lib.vk_lamb_work_bytes(T.ctypes.data, len(T), P.ctypes.data, len(P), G.ctypes.data, len(G))
            if nbytes <= 0:
                raise L.VoltaHipError(L.lib.vk_last_error().decode())
            dev = [torch.from_numpy(x.view(np.uint8).reshape(-1).copy()).to(device) for x in (T, P, G)]
            if len(f["tables"]) > 4:
                f["tables"].clear()
            t = f["tables"][key] = dict(host=(T, P, G), dev=dev, work=torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device), nbytes=nbytes,
                                        table=torch.zeros(len(T), 4, device=device), labels=labels())
        return t

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        loss = closure() if closure is not None else None
        if self._fused is None:
            self._setup()
        f = self._fused
        arena, ents = f["arena"], f["ents"]
        self._refuse_zero1(f["model"])
        b1, b2, eps, bias_correction, grad_averaging = self._hyper()
        for g in self.param_groups:                    # apex: every group's counter advances, with or without gradients in it
            g["step"] = g.get("step", 0) + 1
        if arena is not None and f.get("fixed") is None:
            # what does not change while the arena stands: per arena parameter (p, expected g, m, v, shadow, numel)
            pb, gb, mb, vb, sb = (x.data_ptr() for x in (arena.master, arena.grad, f["m"], f["v"], arena.shadow))
            f["fixed"] = [None if n is None else (pb + 4 * arena.offset[n], gb + 4 * arena.offset[n], mb + 4 * arena.offset[n], vb + 4 * arena.offset[n],
                                                  sb + 2 * arena.offset[n], p.numel()) for _, p, n, _ in ents]
        fixed = f.get("fixed")
        live, fptr, groups_live = [], [], set()
        for i, (gi, p, n, fr) in enumerate(ents):
            g = p.grad
            live.append(g is not None)
            if g is None:
                continue
            groups_live.add(gi)
            if n is not None:
                if g.data_ptr() != fixed[i][1]:
                    raise RuntimeError("volta_amd.LAMB: the gradient of %s is not the engine's arena view (a foreign tensor was assigned to "
                                       ".grad); run backward through the model, or zero_grad(set_to_none=True)" % n)
            elif g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape or g.device != p.device:
                raise RuntimeError("volta_amd.LAMB: the gradient of a tensor outside the arena must be a contiguous float32 tensor of its shape")
            else:
                fptr.append((p.data_ptr(), g.data_ptr()))
        if not groups_live:
            f["last"] = None
            return loss
        # classes: what the kernels look up per tensor -- (lr, weight decay, step count) of its group; groups without a live tensor need none
        classes, cls_of_group = {}, {}
        for gi in sorted(groups_live):
            g = self.param_groups[gi]
            key = (float(g["lr"]), float(g["weight_decay"]), int(g["step"]) if bias_correction else 0)
            if key not in classes:
                if len(classes) == L.LAMB_CLASSES:
                    raise RuntimeError("volta_amd.LAMB: more than %d distinct (lr, weight decay, step count) classes in one step" % L.LAMB_CLASSES)
                classes[key] = len(classes)
            cls_of_group[gi] = classes[key]
        max_norms = tuple(g["max_grad_norm"] for g in self.param_groups)

        def rows():
            out, k = [], 0
            for i, ((gi, p, n, fr), l) in enumerate(zip(ents, live)):
                if not l:
                    continue
                if n is not None:
                    out.append(fixed[i] + (cls_of_group[gi], gi))
                else:
                    out.append(fptr[k] + (fr["m"].data_ptr(), fr["v"].data_ptr(), 0, p.numel(), cls_of_group[gi], gi))
                    k += 1
            return out

        def labels():
            return [n if n is not None else i for i, ((_, _, n, _), l) in enumerate(zip(ents, live)) if l]

        key = (tuple(live), tuple(fptr), tuple(sorted(cls_of_group.items())), max_norms)
        t = self._tables(key, rows, labels, max_norms, ents[0][1].device)
        a = L.LambArgs()
        T, P, G = t["host"]
        a.tensors, a.pieces, a.groups = T.ctypes.data, P.ctypes.data, G.ctypes.data
        a.d_tensors, a.d_pieces, a.d_groups = (x.data_ptr() for x in t["dev"])
        a.work, a.work_bytes, a.table = t["work"].data_ptr(), t["nbytes"], t["table"].data_ptr()
        a.ntensors, a.npieces, a.ngroups = len(T), len(P), len(G)
        a.flags = ((L.LAMB_ADAM_W_MODE if self.adam_w_mode else 0) | (L.LAMB_GRAD_AVERAGING if grad_averaging else 0)
                   | (L.LAMB_GLOBAL_NORM if self.global_grad_norm else 0))
        b1f, b2f = float(np.float32(b1)), float(np.float32(b2))      # the betas the kernels use: apex takes its powers of the fp32 values too
        for (lr, wd, st), c in classes.items():
            a.cls_lr[c], a.cls_wd[c] = lr, wd
            a.cls_bc1[c], a.cls_bc2[c] = (1.0 - b1f ** st, 1.0 - b2f ** st) if bias_correction else (1.0, 1.0)
        a.beta1, a.beta2, a.eps, a.grad_scale = b1, b2, eps, grad_scale
        clip = None
        if arena is not None:
            pend = getattr(arena, "pending_clip", None)
            if pend is not None:
                if pend[1] == self._grad_names():
                    clip = pend[0]             # computed over exactly the gradients this step consumes: folded into the pass
                else:
                    flush_clip(arena)
            arena.pending_clip = None
            arena.sync_optimizer()
        a.clip = clip.data_ptr() if clip is not None else None
        L.check(L.lib.vk_lamb_step(C.byref(a), L.stream_ptr()))
        if arena is not None and any(l and e[2] is not None for l, e in zip(live, ents)):
            arena.mark_shadow_fresh()          # stage 2 refreshed the bf16 copies of what it wrote
        stepped = f["stepped"]
        for i, l in enumerate(live):
            if l:
                stepped[i] = True
        f["last"] = t
        return loss

    def trust_ratios(self):
        """{arena name, or position in param_groups order for a tensor outside the arena: (ratio / lr, |p|, |update|)} of the last step --
        |p| before the update; parameters skipped in that step are absent.  One device-to-host copy, made here and nowhere else."""
        t = self._fused["last"] if self._fused is not None else None
        if t is None:
            return {}
        rows = t["table"].cpu().tolist()
        return {lab: (r[1], r[2], r[3]) for lab, r in zip(t["labels"], rows)}

    def zero_grad(self, set_to_none=None):
        if set_to_none is None:
            set_to_none = self.set_grad_none
        if self._fused is not None and self._fused["arena"] is not None:
            self._fused["arena"].pending_clip = None
        for g in self.param_groups:
            for p in g["params"]:
                if set_to_none:
                    p.grad = None
                elif p.grad is not None:
                    p.grad.zero_()

    def synchronize(self):
        if self._fused is not None and self._fused["arena"] is not None:
            self._fused["arena"].sync_optimizer()

    # ---- checkpoints: apex's layout -- param_groups[i]["step"], and {"exp_avg", "exp_avg_sq"} per parameter that has stepped, indexed in
    # param_groups order
    def state_dict(self):
        self.synchronize()
        sd = super().state_dict()
        f = self._fused
        if f is None:
            sd["state"] = {i: {k: v.clone() for k, v in st.items()} for i, st in (self._pending or {}).items()}
            return sd
        out = {}
        for i, (_, p, _, _) in enumerate(f["ents"]):
            if f["stepped"][i]:
                m, v = self._moments(i)
                out[i] = {"exp_avg": m.view(p.shape).clone(), "exp_avg_sq": v.view(p.shape).clone()}
        sd["state"] = out
        return sd

    def load_state_dict(self, state_dict):
        self.synchronize()
        state = state_dict.get("state", {})
        super().load_state_dict({"state": {}, "param_groups": state_dict["param_groups"]})
        self._hyper()
        allp = [p for g in self.param_groups for p in g["params"]]
        st = {}
        for k, s in state.items():
            i = int(k)
            if not 0 <= i < len(allp):
                raise ValueError("volta_amd.LAMB.load_state_dict: state for parameter %d, the optimizer has %d" % (i, len(allp)))
            if s["exp_avg"].numel() != allp[i].numel() or s["exp_avg_sq"].numel() != allp[i].numel():
                raise ValueError("volta_amd.LAMB.load_state_dict: parameter %d's state does not fit it (%d / %d elements for %d)"
                                 % (i, s["exp_avg"].numel(), s["exp_avg_sq"].numel(), allp[i].numel()))
            st[i] = {"exp_avg": s["exp_avg"].detach().float().cpu().clone(), "exp_avg_sq": s["exp_avg_sq"].detach().float().cpu().clone()}
        if self._fused is None and not all(p.device.type == "cuda" for p in allp):
            self._pending = st          # the model is not on the GPU yet: applied at the first setup
            return
        if self._fused is None:
            self._setup()
        self._apply_state(st)

    def _apply_state(self, st):
        f = self._fused
        for i in range(len(f["ents"])):
            s = st.get(i)
            dm, dv = self._moments(i)
            if s is None:
                dm.zero_(); dv.zero_()
            else:
                dm.copy_(s["exp_avg"].reshape(-1)); dv.copy_(s["exp_avg_sq"].reshape(-1))
            f["stepped"][i] = s is not None


class WarmupLinearSchedule(LambdaLR):
    """Linear warm-up from 0 to 1 over `warmup_steps`, then linear decay to 0 at `t_total`."""

    def __init__(self, optimizer, warmup_steps, t_total, last_epoch=-1):
        self.warmup_steps = warmup_steps
        self.t_total = t_total
        super().__init__(optimizer, self.lr_lambda, last_epoch=last_epoch)

    def lr_lambda(self, step):
        if step < self.warmup_steps:
            return float(step) / float(max(1, self.warmup_steps))
        return max(0.0, float(self.t_total - step) / float(max(1.0, self.t_total - self.warmup_steps)))


class WarmupConstantSchedule(LambdaLR):
    """Linear warm-up from 0 to 1 over `warmup_steps`, then 1 (pytorch_transformers 1.1.0; train_task.py:233-234, the default schedule)."""

    def __init__(self, optimizer, warmup_steps, last_epoch=-1):
        self.warmup_steps = warmup_steps
        super().__init__(optimizer, self.lr_lambda, last_epoch=last_epoch)

    def lr_lambda(self, step):
        if step < self.warmup_steps:
            return float(step) / float(max(1.0, self.warmup_steps))
        return 1.0


def flush_clip(arena):
    """Apply a clip coefficient that is still waiting for an optimizer step to the gradients it was computed over (and forget it)."""
    pend = getattr(arena, "pending_clip", None)
    arena.pending_clip = None
    if pend is None:
        return
    out, names = pend[0], pend[1]
    foreign = pend[2] if len(pend) > 2 else ()          # gradients of tensors outside the arena that the norm covered
    names = frozenset(n for n in names if isinstance(n, str))
    if len(names) == sum(p.grad is not None for _, p in arena.param_list()) == len(arena.param_list()):
        arena.grad.mul_(out[1])
    else:
        for n in names:
            arena.view(n, "grad").mul_(out[1])
    for g in foreign:
        g.mul_(out[1])


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, defer_to_optimizer=None, pre_scale=1.0):
    """Global L2 norm of the gradients and clipping by max_norm / (norm + 1e-6) when that is < 1 (torch.nn.utils.clip_grad_norm_ as
    train_concap.py:307 calls it).  Returns the norm as a 0-dim DEVICE tensor (no host synchronisation).
    Where the scaling happens: when a `volta_amd.AdamW` has been built on this model's parameters, the coefficient is handed to its
    next `step()`, which folds it into its single pass over the gradients (saves one read + write of the 968 MB gradient arena); it is
    applied at once instead when no such optimizer exists, when the next step consumes another set of gradients, before the next
    backward, and by `flush_clip(model.materialize())` for code that reads `.grad` between the two calls.  `defer_to_optimizer=False`
    forces the eager form, `True` the deferred one."""
    if float(norm_type) != 2.0:
        raise NotImplementedError("only the L2 norm is supported")
    model = None
    whole = False
    owner = getattr(parameters, "vk_model", None)          # modeling.ArenaParameters: `model.parameters()` of a volta_amd model
    if owner is not None and not parameters.started and owner.__dict__.get("_arena") is not None:
        model, arena = owner, owner.materialize()          # the whole arena, no need to walk 600 tensors
        whole = True
    foreign = []
    if model is None:
        params = [parameters] if isinstance(parameters, torch.Tensor) else list(parameters)
        model, arena, foreign = _split_params(params)
        if arena is None:
            if not foreign:
                raise RuntimeError("clip_grad_norm_: no parameters")
            return _clip_foreign_only(foreign, max_norm, pre_scale)
        given = {p.data_ptr() for p in params}
    flush_clip(arena)                                       # two clips in a row: the first one's scaling is part of what the second measures
    # parameters without a gradient (frozen, or an unused head) are left out, as torch.nn.utils.clip_grad_norm_ does
    plist, gviews = arena.param_list(), arena.grad_views()
    have = []
    for (n, p), g in zip(plist, gviews):
        if not whole and p.data_ptr() not in given:
            continue
        if p.grad is None:
            continue
        if not (p.grad is g or p.grad.data_ptr() == g.data_ptr()):
            raise RuntimeError("clip_grad_norm_: the gradient of %s is not attached to the engine's arena (run backward first)" % n)
        have.append(n)
    if not have and not any(p.grad is not None for p in foreign):
        raise RuntimeError("clip_grad_norm_: gradients are not attached to the engine's arena (run backward first)")
    flive = [p for p in foreign if p.grad is not None]
    if flive and _red_mode(model) == "zero1":
        raise NotImplementedError("clip_grad_norm_: data-parallel mode 'zero1' with parameters outside the model's arena")
    mask = None
    if len(have) != len(plist):
        cache = arena.__dict__.setdefault("_clip_masks", {})
        key = tuple(have)
        if key not in cache:
            if len(cache) > 16:
                cache.clear()
            _check_shared_chunks(arena, set(have), "part of the norm")
            cc = torch.full((arena.total // 1024,), L.CHUNK_SKIP, dtype=torch.uint8)
            for n in have:
                c0, c1 = _chunks_of(arena, n)
                cc[c0:c1] = 0
            cache[key] = cc.to(arena.device)
        mask = cache[key]
    # per-slot sums of squares, then one fixed-order sum: a function of the gradient values alone, so a rank that owns only part of the
    # arena (data-parallel mode "zero1") and receives the other ranks' slot sums obtains the same bits as one that holds everything
    nchunks = arena.total // 1024
    npad = nchunks + (nchunks & 1)                     # an even count: the first-level sums follow the slot sums as doubles
    if not hasattr(arena, "norm_chunks"):
        arena.norm_chunks = torch.zeros(npad + 256, device=arena.device)
    sums = arena.norm_chunks[:npad]
    if flive:
        # tensors outside the arena: one sum of squares each in the slots behind the chunk sums, then the same fixed-order sum over all
        nf = len(flive)
        npad = nchunks + nf + ((nchunks + nf) & 1)
        buf = arena.__dict__.get("norm_slots")
        if buf is None or buf.numel() < npad + 256:
            buf = arena.__dict__["norm_slots"] = torch.zeros(npad + 256, device=arena.device)
        sums = buf[:npad]
        sums[nchunks + nf:].zero_()
        ents = [(p, p.grad, None, None, 0) for p in flive]
        for p in flive:
            if p.grad.dtype != torch.float32 or not p.grad.is_contiguous() or p.grad.device != arena.device:
                raise RuntimeError("clip_grad_norm_: the gradient of a tensor outside the arena must be a contiguous float32 tensor on %s" % arena.device)
        flist, fmax = _tensor_list(ents, arena.device)
        work = torch.empty(nf * L.lib.vk_grad_sqnorm_list_work_floats(), device=arena.device)
        L.check(L.lib.vk_grad_sqnorm_list(L.ptr(flist), nf, fmax, L.ptr(work), L.ptr(sums[nchunks:]), L.stream_ptr()))
    out = torch.empty(2, device=arena.device)
    ddp = getattr(model, "_ddp", None)
    red = getattr(ddp, "reducer", None)
    if red is not None and red.mode == "zero1" and (red.sharded or red.replicated):
        sums.zero_()
        mine = [(lo + red.rank * s, lo + (red.rank + 1) * s) for lo, hi, s in red.sharded] + (list(red.replicated) if red.rank == 0 else [])
        for lo, hi in mine:
            L.check(L.lib.vk_grad_sqnorm_chunks(L.ptr(arena.grad), lo // 1024, (hi - lo) // 1024, L.ptr(mask), L.ptr(sums), L.stream_ptr()))
        torch.distributed.all_reduce(sums, group=red.pg)        # every slot has one contributor: the sum adds zeros, exactly
    else:
        L.check(L.lib.vk_grad_sqnorm_chunks(L.ptr(arena.grad), 0, nchunks, L.ptr(mask), L.ptr(sums), L.stream_ptr()))
    L.check(L.lib.vk_grad_norm_from_chunks(L.ptr(sums), npad, pre_scale, float(max_norm), L.ptr(out), L.stream_ptr()))
    names = frozenset(have + [("foreign", id(p)) for p in flive])
    if defer_to_optimizer is None:
        # the reference's plain call: defer when the optimizer that will consume these gradients is ours and steps exactly this set
        opt = getattr(arena, "_vk_adamw", None)
        opt = opt() if opt is not None else None
        defer_to_optimizer = opt is not None and opt._fused is not None and opt._fused["arena"] is arena and opt._grad_names() == names
    arena.pending_clip = (out, names, [p.grad for p in flive]) if flive else (out, names)
    if not defer_to_optimizer:
        flush_clip(arena)
    return out[0]


def _red_mode(model):
    red = getattr(getattr(model, "_ddp", None), "reducer", None)
    return red.mode if red is not None and (red.sharded or red.replicated) else None


def _clip_foreign_only(params, max_norm, pre_scale):
    """clip_grad_norm_ over torch tensors alone (no volta_amd model among them): the same kernels, applied at once."""
    live = [p for p in params if p.grad is not None]
    if not live:
        raise RuntimeError("clip_grad_norm_: no parameter carries a gradient")
    dev = live[0].device
    nf = len(live)
    npad = nf + (nf & 1)
    sums = torch.zeros(npad + 256, device=dev)
    flist, fmax = _tensor_list([(p, p.grad, None, None, 0) for p in live], dev)
    work = torch.empty(nf * L.lib.vk_grad_sqnorm_list_work_floats(), device=dev)
    L.check(L.lib.vk_grad_sqnorm_list(L.ptr(flist), nf, fmax, L.ptr(work), L.ptr(sums), L.stream_ptr()))
    out = torch.empty(2, device=dev)
    L.check(L.lib.vk_grad_norm_from_chunks(L.ptr(sums), npad, pre_scale, float(max_norm), L.ptr(out), L.stream_ptr()))
    for p in live:
        p.grad.mul_(out[1])
    return out[0]
