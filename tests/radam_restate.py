"""float64 restatement of the reference's RAdam and PlainRAdam (volta/optimization.py:9-169) for tests/test_radam_*.py, written from the
reference's text -- its own buffer walk, not volta_amd's planner -- together with a per-element bound on how far ANY fp32 implementation
of the same element function may lie from it.

Derivation of the bound (u = 2^-24, one rounding of an fp32 result r costs at most u|r|; the fp32 constants beta, 1 - beta, the decay
factor and the step size are each within u relative of their double values):
  g'   = fl(g * clip)                 eg = u|g'|   (0 when clip == 1: the product is exact)
  m    = b1 m + (1-b1) g'             3 roundings / constant errors, each at most u * M with M = b1 M + (1-b1)|g'| >= |m|:
                                      Em <- b1 Em + 4u M + (1-b1) eg
  v    = b2 v + (1-b2) g'^2           every term positive, 5 roundings / constant errors relative to v:
                                      Ev <- b2 Ev + 6u v + 2 (1-b2) |g'| eg
  p   -= d p                          Ep <- Ep (1 + d) + u d|p| + u|p_new|
  rectified:  r = m / (sqrt(v) + eps) |sqrt(a) - sqrt(b)| <= min(|a-b| / (2 sqrt b), sqrt|a-b|), sqrt and + round once each:
                                      Dden = min(Ev / (2 sqrt v), sqrt Ev) + 2u den
                                      Er = (Em + |r| Dden) / (den - Dden) + u|r|      (den - Dden floored at den / 2)
              p -= s r                Ep <- Ep + s Er + u s|r| + u|p_new|
  otherwise   p -= s m                Ep <- Ep + s Em + u s|m| + u|p_new|
The gates are 2x these first-order bounds (the factor covers the neglected products of two error terms)."""
import math

import torch

U = 2.0 ** -24


def step_size(lr, t, beta1, beta2):
    """volta/optimization.py:57-78 in its own expression order."""
    beta2_t = beta2 ** t
    N_sma_max = 2 / (1 - beta2) - 1
    N_sma = N_sma_max - 2 * t * beta2_t / (1 - beta2_t)
    if N_sma >= 5:
        ss = lr * math.sqrt((1 - beta2_t) * (N_sma - 4) / (N_sma_max - 4) * (N_sma - 2) / N_sma * N_sma_max / (N_sma_max - 2)) / (1 - beta1 ** t)
    else:
        ss = lr / (1 - beta1 ** t)
    return ss, N_sma


class Restated:
    """RAdam (plain=False) or PlainRAdam over a list of tensors, one group each (lrs / wds per tensor), in float64 on the tensors' device.
    Deliberately wrong variants for the gate checks: decay_after (decay after the update, as AdamW does), own_lr (every tensor's step size
    from its own group's lr, ignoring the shared buffer)."""

    def __init__(self, params, plain=False, betas=(0.9, 0.999), eps=1e-8, decay_after=False, own_lr=False):
        self.p = [t.detach().double().clone() for t in params]
        z = lambda: [torch.zeros_like(t) for t in self.p]
        self.m, self.v, self.M, self.Ep, self.Em, self.Ev = z(), z(), z(), z(), z(), z()
        self.steps = [0] * len(self.p)
        self.buffer = [[None, None, None] for _ in range(10)]
        self.plain, self.b1, self.b2, self.eps = plain, betas[0], betas[1], eps
        self.decay_after, self.own_lr = decay_after, own_lr
        self.last = []                 # (step_size, rectified) per tensor of the last step, None where it did not step

    def load(self, ps, steps, ms, vs):
        """Weights and a reference state_dict's content (step 0 = no entry), taken as exact; the buffer starts empty, as after the
        reference's load."""
        self.p = [t.detach().double().clone() for t in ps]
        self.Ep, self.Em, self.Ev = [torch.zeros_like(t) for t in self.p], [torch.zeros_like(t) for t in self.p], [torch.zeros_like(t) for t in self.p]
        self.steps = list(steps)
        self.m = [t.detach().double().clone() for t in ms]
        self.v = [t.detach().double().clone() for t in vs]
        self.M = [t.abs() for t in self.m]
        self.buffer = [[None, None, None] for _ in range(10)]

    def _plan(self, i, lr):
        t = self.steps[i]
        if self.plain or self.own_lr:
            ss, N_sma = step_size(lr, t, self.b1, self.b2)
            return ss, N_sma
        b = self.buffer[int(t % 10)]
        if t == b[0]:
            return b[2], b[1]
        ss, N_sma = step_size(lr, t, self.b1, self.b2)
        b[0], b[1], b[2] = t, N_sma, ss
        return ss, N_sma

    @torch.no_grad()
    def step(self, grads, lrs, wds, clip=1.0):
        b1, b2 = self.b1, self.b2
        self.last = []
        for i, g in enumerate(grads):
            if g is None:
                self.last.append(None)
                continue
            g = g.to(self.p[i].device).double() * clip
            eg = U * g.abs() if clip != 1.0 else torch.zeros_like(g)
            self.v[i] = b2 * self.v[i] + (1 - b2) * g * g
            self.Ev[i] = b2 * self.Ev[i] + 6 * U * self.v[i] + 2 * (1 - b2) * g.abs() * eg
            self.m[i] = b1 * self.m[i] + (1 - b1) * g
            self.M[i] = b1 * self.M[i] + (1 - b1) * g.abs()
            self.Em[i] = b1 * self.Em[i] + 4 * U * self.M[i] + (1 - b1) * eg
            self.steps[i] += 1
            ss, N_sma = self._plan(i, lrs[i])
            rect = N_sma >= 5
            self.last.append((ss, rect))
            d = wds[i] * lrs[i]
            p, m, v = self.p[i], self.m[i], self.v[i]
            if d != 0 and not self.decay_after:
                p = p - d * p
                self.Ep[i] = self.Ep[i] * (1 + d) + U * d * self.p[i].abs() + U * p.abs()
            if rect:
                den = v.sqrt() + self.eps
                dden = torch.minimum(self.Ev[i] / (2 * v.sqrt()).clamp_min(1e-300), self.Ev[i].sqrt()) + 2 * U * den
                r = m / den
                er = (self.Em[i] + r.abs() * dden) / torch.maximum(den - dden, den / 2) + U * r.abs()
                q = p - ss * r
                self.Ep[i] = self.Ep[i] + ss * er + U * ss * r.abs() + U * q.abs()
            else:
                q = p - ss * m
                self.Ep[i] = self.Ep[i] + ss * self.Em[i] + U * ss * m.abs() + U * q.abs()
            if d != 0 and self.decay_after:
                q = q - d * q
            self.p[i] = q

    def excess(self, i, p=None, m=None, v=None):
        """max over elements of |x - restated| / (2 * bound) for the given fp32 results of tensor i (> 1: outside the gate)."""
        worst = 0.0
        for got, want, err in ((p, self.p[i], self.Ep[i]), (m, self.m[i], self.Em[i]), (v, self.v[i], self.Ev[i])):
            if got is None:
                continue
            diff = (got.to(want.device).double().reshape(want.shape) - want).abs()
            worst = max(worst, float((diff / (2 * err + 1e-30)).max()))
        return worst
