"""float64 restatement of the LAMB contract of include/volta_hip.h (vk_lamb_step), written from the header's text, with a first-order bound
on how far ANY fp32 implementation of that contract may lie from it, deliberately wrong contracts for the gate checks, and the case table
that tests/test_lamb_cpu.py and tests/test_lamb_kernels_gpu.py share.  Needs torch alone (any device: the model-level GPU test runs it on
the device).

Notation as in tests/optim_restate.py: u = 2^-24, one rounding of an fp32 result r costs at most u|r|; every gate is 2x a first-order
bound; `ratio` (optim_restate's) is the only comparator.  The fp32 scalars (lr, wd, betas, eps, grad_scale, clip[1], max_grad_norm, bc1,
bc2) are taken as exact doubles; 1 - beta is exact in fp32 for beta in [0.5, 1].  E* are bounds on |implementation - restatement|; Ep
is carried from step to step, because the implementation continues from ITS p, m and v.

  gs   = fl(grad_scale * clip)         one rounding;  g1 = fl(g * gs): eg = 2u|g1|   (0 when gs == 1: exact)
  S_n  = sum g^2 over group n          a piece's sum meets <= N = 1024 rounded squares in fp32, in any order, then goes to double:
                                       eS = (N + 1) u relative
  norm = fl(fl32(sqrt(S)) * |gs|)      eN = eS / 2 + 4u relative (sqrt, cast, product, and gs's own rounding)
  c    = norm / mx  if mx > 0 and norm > mx, else 1
                                       Ec = c (eN + u) where it divides; where the restatement says 1 but norm (1 + eN) > mx an
                                       implementation may divide: Ec = norm (1 + eN) / mx - 1 + u; else exactly 1, Ec = 0
  g2   = g1 / c                        Eg = eg / c + |g2| Ec / c + u|g2|   (the last term 0 when c == 1 with Ec == 0: exact)
  mode 0, wd != 0:  g2 = g2 + wd p     Eg <- Eg + wd Ep + u|wd p| + u|g2|
  m    = b1 m + b3 g2                  Em <- b1 Em + b3 Eg + 4u M,  M = b1 M + b3|g2| >= |m|
  v    = b2 v + (1 - b2) g2^2          Ev <- b2 Ev + 6u v + 2 (1 - b2)|g2| Eg
  mh   = m / bc1 ; vh = v / bc2        Emh = Em / bc1 + u|mh| ;  Evh = Ev / bc2 + u vh
  den  = sqrt(vh) + eps                Dden = min(Evh / (2 sqrt vh), sqrt Evh) + 2u den
  r    = mh / den                      Er = (Emh + |r| Dden) / max(den - Dden, den / 2) + u|r|
  mode 1, wd != 0:  upd = r + wd p     Eu = Er + wd Ep + u|wd p| + u|upd|             (else upd = r, Eu = Er)
  |p_t| = fl32(sqrt(P_t))              the implementation takes the norm of ITS p: | |p + e| - |p| | <= |e|_2; the sum as for S, the
                                       square root and the cast round once each:  Epn = |Ep|_2 + |p_t| ((N + 1) u / 2 + 2u)
  |u_t|                                Eun = |Eu|_2 + |u_t| ((N + 1) u / 2 + 2u)
  trust = |p_t| / |u_t|                Et = (Epn + trust Eun) / max(|u_t| - Eun, |u_t| / 2) + u trust ;  1, Et = 0, when a norm is 0
  ratio = lr trust                     Erat = lr Et + u ratio                          (exactly lr when a norm is 0)
  p    = p - ratio upd                 Ep <- Ep + ratio Eu + |upd| Erat + u|ratio upd| + u|p|
This is where the norm errors enter p: |upd| Erat.

`Lamb64.VARIANTS` are deliberately wrong contracts; tests/test_lamb_cpu.py checks that each lies outside the gates on some case."""
import collections
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from optim_restate import U, f32, ratio  # noqa: E402,F401

PIECE = 1024                   # VK_LAMB_PIECE
E_SUM = (PIECE + 1) * U        # relative error of a sum of squares whose pieces are fp32
NSTEPS = 2                     # steps every case of the table runs

Hyper = collections.namedtuple("Hyper", "b1 b2 eps bias_correction grad_averaging adam_w global_norm")


def hyper(b1=0.9, b2=0.999, eps=1e-6, bias_correction=True, grad_averaging=True, adam_w=True, global_norm=False):
    return Hyper(f32(b1), f32(b2), f32(eps), bool(bias_correction), bool(grad_averaging), bool(adam_w), bool(global_norm))


def bias_corrections(h, step):
    """(bc1, bc2) as the contract's host computes them: 1 - beta^step from the fp32 betas, rounded to fp32; 1 without bias correction."""
    if not h.bias_correction:
        return 1.0, 1.0
    return f32(1.0 - h.b1 ** step), f32(1.0 - h.b2 ** step)


class Lamb64:
    """tensors: [(name, p, m, v, group, slot)] (flat or shaped fp32 / fp64 tensors on one device; `slot` names the arena slot for the
    whole-slot variant); groups: [dict(lr, wd, max_norm, step)] -- step counts BEFORE the next step, as in param_groups."""
    VARIANTS = ("slot_ratio", "pnorm_after", "decay_other_mode", "no_grad_averaging", "no_bias_correction", "no_clip_divisor", "other_norm_scope")

    def __init__(self, tensors, groups, h, variant=None):
        assert variant is None or variant in self.VARIANTS
        self.names = [t[0] for t in tensors]
        self.group = {t[0]: t[4] for t in tensors}
        self.slot = {t[0]: t[5] for t in tensors}
        self.p = {t[0]: t[1].detach().double().reshape(-1).clone() for t in tensors}
        self.m = {t[0]: t[2].detach().double().reshape(-1).clone() for t in tensors}
        self.v = {t[0]: t[3].detach().double().reshape(-1).clone() for t in tensors}
        self.M = {n: x.abs() for n, x in self.m.items()}
        self.Ep = {n: torch.zeros_like(x) for n, x in self.p.items()}
        self.Em = {n: torch.zeros_like(x) for n, x in self.p.items()}
        self.Ev = {n: torch.zeros_like(x) for n, x in self.p.items()}
        self.groups = [dict(g) for g in groups]
        self.h, self.variant = h, variant
        self.last = {}

    @torch.no_grad()
    def step(self, grads, grad_scale=1.0, clip=None):
        """grads: {name: fp32 gradient, or None / absent for a skipped tensor}.  Leaves self.last[name] = dict(ratio, trust, pn, un and
        their bounds Eratio, Etrust, Epn, Eun) for the tensors stepped."""
        h, var = self.h, self.variant
        for g in self.groups:
            g["step"] = g.get("step", 0) + 1
        live = [n for n in self.names if grads.get(n) is not None]
        self.last = {}
        if not live:
            return
        gs = f32(grad_scale) * (f32(clip) if clip is not None else 1.0)
        g1 = {n: grads[n].detach().to(self.p[n].device).double().reshape(-1) * gs for n in live}
        eg = {n: (2 * U * g1[n].abs() if gs != 1.0 else torch.zeros_like(g1[n])) for n in live}
        # clip divisor per group
        S = [0.0] * len(self.groups)
        for n in live:
            S[self.group[n]] += float((grads[n].detach().double() ** 2).sum())
        global_norm = h.global_norm != (var == "other_norm_scope")
        cdiv = []
        for gi, g in enumerate(self.groups):
            Sn = sum(S) if global_norm else S[gi]
            norm, eN = math.sqrt(Sn) * abs(gs), E_SUM / 2 + 4 * U
            mx = g["max_norm"]
            mx = f32(mx) if mx is not None and mx > 0 else 0.0
            if var == "no_clip_divisor" or mx <= 0:
                cdiv.append((1.0, 0.0))
            elif norm > mx:
                cdiv.append((norm / mx, norm / mx * (eN + U)))
            elif norm * (1 + eN) > mx:
                cdiv.append((1.0, norm * (1 + eN) / mx - 1 + U))
            else:
                cdiv.append((1.0, 0.0))
        adam_w = h.adam_w != (var == "decay_other_mode")
        b3 = (1 - h.b1) if h.grad_averaging != (var == "no_grad_averaging") else 1.0
        upd, Eu, new = {}, {}, {}
        for n in live:
            g = self.groups[self.group[n]]
            wd = f32(g["wd"])
            c, Ec = cdiv[self.group[n]]
            bc1, bc2 = (1.0, 1.0) if var == "no_bias_correction" else bias_corrections(h, g["step"])
            p, Ep = self.p[n], self.Ep[n]
            g2 = g1[n] / c
            Eg = eg[n] / c + g2.abs() * Ec / c + (U * g2.abs() if (c != 1.0 or Ec != 0.0) else 0.0)
            if not adam_w and wd != 0.0:
                g2 = g2 + wd * p
                Eg = Eg + wd * Ep + U * (wd * p).abs() + U * g2.abs()
            m = h.b1 * self.m[n] + b3 * g2
            M = h.b1 * self.M[n] + b3 * g2.abs()
            Em = h.b1 * self.Em[n] + b3 * Eg + 4 * U * M
            v = h.b2 * self.v[n] + (1 - h.b2) * g2 * g2
            Ev = h.b2 * self.Ev[n] + 6 * U * v + 2 * (1 - h.b2) * g2.abs() * Eg
            mh, vh = m / bc1, v / bc2
            Emh, Evh = Em / bc1 + U * mh.abs(), Ev / bc2 + U * vh
            den = vh.sqrt() + h.eps
            Dden = torch.minimum(Evh / (2 * vh.sqrt()).clamp_min(1e-300), Evh.sqrt()) + 2 * U * den
            r = mh / den
            Er = (Emh + r.abs() * Dden) / torch.maximum(den - Dden, den / 2) + U * r.abs()
            if adam_w and wd != 0.0:
                u = r + wd * p
                E = Er + wd * Ep + U * (wd * p).abs() + U * u.abs()
            else:
                u, E = r, Er
            upd[n], Eu[n], new[n] = u, E, (m, M, Em, v, Ev)
        # norms per tensor (per slot for the wrong variant), trust ratios, update
        def scope(n):
            return [k for k in live if self.slot[k] == self.slot[n]] if var == "slot_ratio" else [n]

        for n in live:
            g = self.groups[self.group[n]]
            lr = f32(g["lr"])
            ks = scope(n)
            P = sum(float((self.p[k] ** 2).sum()) for k in ks)
            Uu = sum(float((upd[k] ** 2).sum()) for k in ks)
            EP2 = sum(float((self.Ep[k] ** 2).sum()) for k in ks)
            EU2 = sum(float((Eu[k] ** 2).sum()) for k in ks)
            pn, un = math.sqrt(P), math.sqrt(Uu)
            Epn = math.sqrt(EP2) + pn * (E_SUM / 2 + 2 * U)
            Eun = math.sqrt(EU2) + un * (E_SUM / 2 + 2 * U)
            if var == "pnorm_after" and pn != 0 and un != 0:
                pn = float(((self.p[n] - lr * (pn / un) * upd[n]) ** 2).sum()) ** 0.5
            if pn != 0 and un != 0:
                trust = pn / un
                Et = (Epn + trust * Eun) / max(un - Eun, un / 2) + U * trust
            else:
                trust, Et = 1.0, 0.0
            rat = lr * trust
            Erat = lr * Et + (U * rat if Et else 0.0)
            p, u = self.p[n], upd[n]
            q = p - rat * u
            self.Ep[n] = self.Ep[n] + rat * Eu[n] + u.abs() * Erat + U * (rat * u).abs() + U * q.abs()
            self.p[n] = q
            self.m[n], self.M[n], self.Em[n], self.v[n], self.Ev[n] = new[n]
            self.last[n] = dict(ratio=rat, trust=trust, pn=pn, un=un, Eratio=Erat, Etrust=Et, Epn=Epn, Eun=Eun)

    def excess(self, name, p=None, m=None, v=None):
        return max([ratio(got, want, err) for got, want, err in ((p, self.p[name], self.Ep[name]), (m, self.m[name], self.Em[name]),
                                                                 (v, self.v[name], self.Ev[name])) if got is not None] + [0.0])

    def excess_table(self, name, row):
        """row = (ratio, trust, |p|, |u|) of the implementation's table against the last step's values."""
        w = self.last[name]
        return max(ratio(row[0], w["ratio"], w["Eratio"]), ratio(row[1], w["trust"], w["Etrust"]), ratio(row[2], w["pn"], w["Epn"]),
                   ratio(row[3], w["un"], w["Eun"]))


# ============================================================================================ the case table
# One layout for every case: an "arena" of chunk-aligned slots plus tensors outside it.  (name, numel, group, slot, offset): offset = element
# offset in the arena, or None for a tensor outside it (`FOREIGN_SHIFT` floats off a 16-byte boundary).  Group 0 decays, group 1 does not;
# the tensors of a group are consecutive, as in param_groups order.
Spec = collections.namedtuple("Spec", "name numel group slot offset")
LAYOUT = [
    Spec("t1", 1, 0, "t1", 1024), Spec("t3", 3, 0, "t3", 2048), Spec("t1023", 1023, 0, "t1023", 3072), Spec("t1024", 1024, 0, "t1024", 4096),
    Spec("t1025", 1025, 0, "t1025", 5120), Spec("t2053", 2 * 1024 + 5, 0, "t2053", 7168), Spec("zero_p", 100, 0, "zero_p", 10240),
    Spec("skipme", 300, 0, "skipme", 12288),                                    # between two live tensors, in the table and in memory
    Spec("w_q", 384, 0, "w_qkv", 13312), Spec("w_k", 384, 0, "w_qkv", 13696), Spec("w_v", 384, 0, "w_qkv", 14080),      # w_k straddles a chunk boundary
    Spec("f_big", 517, 0, "f_big", None),
    Spec("b_q", 64, 1, "b_qkv", 0), Spec("b_k", 64, 1, "b_qkv", 64), Spec("b_v", 64, 1, "b_qkv", 128),                  # the bias-slot trap: one chunk
    Spec("zero_u", 100, 1, "zero_u", 11264),                                    # g = m = v = 0 and no decay: the update is all zero
    Spec("f_odd", 37, 1, "f_odd", None),
]
ARENA_TOTAL = 15360
FOREIGN_SHIFT = {"f_big": 0, "f_odd": 1}

Case = collections.namedtuple("Case", "id h step0 lr wd max_norm grad_scale clip skip seed")


def _cases():
    out = []

    def add(id, step0=0, lr=(1e-3, 2e-3), wd=(0.01, 0.0), max_norm=(1.0, 1.0), grad_scale=1.0, clip=None, skip=(), **kw):
        out.append(Case(id, hyper(**kw), step0, lr, wd, max_norm, grad_scale, clip, tuple(skip), 500 + len(out)))
    add("base-clip-bites")
    add("l2mode-step3", step0=2, lr=(0.02, 0.01), wd=(0.1, 0.0), adam_w=False)
    add("noavg-nobias-step3-deferred", step0=2, max_norm=(1e9, 1e9), clip=0.37, grad_averaging=False, bias_correction=False)
    add("biglr-bigwd-noclip", lr=(0.05, 0.05), wd=(0.25, 0.0), max_norm=(None, None))
    add("skip-deferred-scale", clip=0.71, grad_scale=0.5, skip=("skipme",))
    add("global-norm", max_norm=(1.0, 0.5), global_norm=True)
    add("group-norms", max_norm=(1.0, 0.5))
    add("noclip-noavg", max_norm=(None, 0.0), grad_averaging=False)
    add("l2mode-nobias-step1", wd=(0.01, 0.0), adam_w=False, bias_correction=False, max_norm=(1e9, 1.0))
    return out


CASES = _cases()


def lamb_inputs(case):
    """{name: dict(p, m, v, gs=[NSTEPS gradients or None])} in fp32 on the CPU.  |g| log-uniform over 1e-4 .. 1, one element in 16 with
    g = 0 in the first step; m and v start non-zero, so that the clip divisor matters from the first step on."""
    gen = torch.Generator().manual_seed(case.seed)
    out = {}
    for s in LAYOUT:
        n = s.numel
        p = torch.randn(n, generator=gen)
        m = torch.randn(n, generator=gen) * 0.01
        v = torch.rand(n, generator=gen) * 1e-3 + 1e-8
        gs = []
        for k in range(NSTEPS):
            g = torch.pow(10.0, torch.rand(n, generator=gen) * 4 - 4) * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
            if k == 0:
                g[torch.rand(n, generator=gen) < 1.0 / 16] = 0.0
            gs.append(g.float())
        if s.name == "zero_p":
            p.zero_()
        if s.name == "zero_u":
            m.zero_(); v.zero_()
            gs = [torch.zeros(n) for _ in gs]
        if s.name in case.skip:
            gs = [None] * NSTEPS
        out[s.name] = dict(p=p.float(), m=m.float(), v=v.float(), gs=gs)
    return out


def case_groups(case):
    return [dict(lr=case.lr[i], wd=case.wd[i], max_norm=case.max_norm[i], step=case.step0) for i in range(2)]


def restated(case, inp, variant=None):
    return Lamb64([(s.name, inp[s.name]["p"], inp[s.name]["m"], inp[s.name]["v"], s.group, s.slot) for s in LAYOUT], case_groups(case), case.h, variant)


def step_grads(inp, k):
    return {n: d["gs"][k] for n, d in inp.items()}
