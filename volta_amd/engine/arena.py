"""Flat parameter storage: fp32 master, bf16 shadow and fp32 gradient arenas, and the e4m3 weight copies of the fp8 path."""
import math

import torch

from .. import _lib as L
from .._lib import check, ptr
from .plan import _round_up

CHUNK = 1024
NO_DECAY = ("bias", "LayerNorm.bias", "LayerNorm.weight")


class ParamArena:
    """Flat master / shadow / gradient storage; re-points every Parameter at its slice."""

    def __init__(self, model, device, prefix=""):
        named = [(prefix + n, p) for n, p in model.named_parameters()]
        byname = dict(named)
        slots, seen = [], set()
        for name, p in named:
            if name in seen:
                continue
            group = [name]
            for q in ("query", "v_query"):
                tag = ".attention_self.%s." % q
                if tag in name and name.rsplit(".", 1)[1] in ("weight", "bias"):      # not a projection's LoRA adapters: slots of their own
                    pre, suf = name.split(tag)
                    kq = q.replace("query", "")
                    group = ["%s.attention_self.%s%s.%s" % (pre, kq, k, suf) for k in ("query", "key", "value")]
            assert all(g in byname for g in group), group
            seen.update(group)
            slots.append(group)
        self.offset, self.shape = {}, {}
        classes = []
        off = 0
        for group in slots:
            start = off
            for g in group:
                self.offset[g] = off
                self.shape[g] = tuple(byname[g].shape)
                off += byname[g].numel()
            off = _round_up(off, CHUNK)
            nd = any(k in group[0] for k in NO_DECAY)
            assert all(any(k in g for k in NO_DECAY) == nd for g in group)
            classes += [1 if nd else 0] * ((off - start) // CHUNK)
        self.total = off
        self.device = device
        self.master = torch.zeros(self.total, dtype=torch.float32, device=device)
        self.shadow = torch.zeros(self.total, dtype=torch.bfloat16, device=device)
        self.grad = torch.zeros(self.total, dtype=torch.float32, device=device)
        self.chunk_class = torch.tensor(classes, dtype=torch.uint8, device=device)
        self.names = [n for n, _ in named]
        self.params = byname
        with torch.no_grad():
            for name, p in named:
                v = self.view(name)
                v.copy_(p.data.to(device=device, dtype=torch.float32))
                p.data = v
                p.grad = None
        self.shadow_version = -1
        self.weights_epoch = 0          # bumped whenever the master weights changed (torch-side edits, fused AdamW)
        self.fp8_sites = {}             # data_ptr of an fp32 master view -> (view [N, K], q uint8 [N, Kp], scale [N])
        self.fp8_epoch = -1
        self._plist = self._gviews = None       # param_list() / grad_views(), built on first use
        self.opt_pending = None         # (range bounds, events) of a pipelined optimizer step still in flight (optimization.py)
        self.frozen_memo = None         # (requires_grad pattern, its pruning decision) of the last forward (modeling._frozen_signature)
        self.grad_plan = None           # weak reference to the plan whose backward wrote `grad` last (modeling._backward_begin)
        lora = getattr(model, "lora_config", None)
        self.lora_scale = lora["alpha"] / lora["r"] if lora else None      # alpha / r of the model's LoRA adapters (volta_amd/lora.py)

    def view(self, name, which="master"):
        buf = getattr(self, which)
        o = self.offset[name]
        return buf[o:o + math.prod(self.shape[name])].view(self.shape[name])

    def param_list(self):
        if self._plist is None or len(self._plist) != len(self.params):
            self._plist = list(self.params.items())
        return self._plist

    def grad_views(self):
        """One view of the gradient arena per parameter, created once (the hot loop only re-attaches them)."""
        if self._gviews is None or len(self._gviews) != len(self.params):
            self._gviews = [self.view(n, "grad") for n in self.params]
        return self._gviews

    def span(self, names, which, shape):
        """Contiguous view over consecutive tensors of one slot (the fused Q|K|V block)."""
        buf = getattr(self, which)
        o = self.offset[names[0]]
        for a, b in zip(names[:-1], names[1:]):
            assert self.offset[b] == self.offset[a] + math.prod(self.shape[a])
        return buf[o:o + math.prod(shape)].view(shape)

    def intact(self):
        return all(p.data_ptr() == self.master.data_ptr() + 4 * self.offset[n] for n, p in self.params.items())

    def param_version(self):
        """Sum of the parameters' own version counters.  Every Parameter was re-pointed with `p.data = view`, which gives
        it a counter of ITS OWN: `load_state_dict`, `p.copy_()`, `p.add_()` (torch optimizers, EMA under no_grad) bump it
        and leave `master._version` alone, so the base tensor's counter says nothing about them."""
        return sum(p._version for p in self.params.values()) + self.master._version

    def refresh_shadow(self, force=False):
        """bf16 copies of the weights, rebuilt whenever a parameter was written through torch since the last refresh.
        The fused AdamW refreshes the shadow inside its own launch and calls mark_shadow_fresh().  Not seen by any version
        counter: in-place edits through `p.data` (`p.data.mul_()`): call invalidate_shadow() after those."""
        v = self.param_version()
        if force or self.shadow_version != v:
            self.sync_optimizer()
            check(L.lib.vk_cast_f32_bf16(ptr(self.master), ptr(self.shadow), self.total, L.stream_ptr()))
            self.shadow_version = v
            self.weights_epoch += 1

    def mark_shadow_fresh(self):
        self.shadow_version = self.param_version()
        self.weights_epoch += 1

    def fp8_weight(self, w):
        """e4m3 copy (+ per-output-channel scales) of the fp32 master weight view `w` [N, K], registered for refresh_fp8()."""
        key = w.data_ptr()
        if key not in self.fp8_sites:
            N, K = w.shape
            Kp = _round_up(K, 128)
            self.fp8_sites[key] = (w, torch.zeros(N, Kp, dtype=torch.uint8, device=self.device), torch.ones(N, dtype=torch.float32, device=self.device))
            self.fp8_epoch = -1
        return self.fp8_sites[key][1:]

    def refresh_fp8(self):
        """Re-quantise the registered weights from the fp32 masters when they changed (one row kernel per weight matrix)."""
        if self.fp8_epoch == self.weights_epoch:
            return
        for w, q, sc in self.fp8_sites.values():
            N, K = w.shape
            check(L.lib.vk_quant_rows_fp8(ptr(w), 1, w.stride(0), ptr(q), q.stride(0), ptr(sc), N, K, None, L.stream_ptr()))
        self.fp8_epoch = self.weights_epoch

    def invalidate_shadow(self):
        self.shadow_version = -1

    def sync_optimizer(self):
        """Make the current stream wait for a pipelined optimizer step still in flight on its own stream."""
        pend = self.opt_pending
        if pend:
            cur = torch.cuda.current_stream()
            for ev in pend[1]:
                cur.wait_event(ev)
            self.opt_pending = None
