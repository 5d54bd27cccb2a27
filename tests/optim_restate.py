"""float64 restatements of the optimizer and reduction contracts of include/volta_hip.h (the optimizer block, vk_sum_slabs_*, vk_side_tail,
vk_mul_bf16, vk_cast_f32_bf16, vk_axpy_f32), written from the header's text, each with a per-element bound on how far ANY fp32
implementation of the same contract may lie from it, and the case table that tests/test_optim_cpu.py and kernel-level GPU tests share.
Needs no GPU; only full_chunks() imports volta_amd (the built library must be there: the engine's own arena sizing is the source of
the full-size chunk count), everything else needs torch alone.

Notation: u = 2^-24, one rounding of an fp32 result r costs at most u|r|.  Every gate is 2x a first-order bound (the factor covers the
neglected products of two error terms and the double-precision roundings of the restatement itself); `ratio` is the only place that
compares, and 2 and u are its only literals.

AdamW element function (pytorch-transformers order; the fp32 scalars lr, betas, eps, step_mult, grad_scale, clip[1] and the class arrays
are taken as exact doubles, 1 - beta is exact in fp32 for beta in [0.5, 1]):
  gs   = fl(grad_scale * clip)        one rounding;  g' = fl(g * gs): eg = 2u|g'|  (0 when gs == 1: the product is exact)
  m    = b1 m + (1-b1) g'             two products and a sum (a fused form has fewer), each at most u * M with M = b1 M + (1-b1)|g'| >= |m|,
                                      and one more for an implementation that rounds 1 - b1 from a double:
                                      Em <- b1 Em + 4u M + (1-b1) eg
  v    = b2 v + (1-b2) g'^2           every term positive, up to 5 roundings relative to v:
                                      Ev <- b2 Ev + 6u v + 2 (1-b2) |g'| eg
  den  = sqrt(v) + eps                |sqrt(a) - sqrt(b)| <= min(|a-b| / (2 sqrt b), sqrt|a-b|), sqrt and + round once each:
                                      Dden = min(Ev / (2 sqrt v), sqrt Ev) + 2u den
  r    = m / den                      Er = (Em + |r| Dden) / (den - Dden) + u|r|        (den - Dden floored at den / 2; the division rounds once)
  step = fl(fl(lr * mult_c) * step_mult)   2u relative;  q = p - step r:  the product and the difference round once each
                                      Ep <- Ep + step Er + 3u step|r| + u|q|
  d    = fl(fl(lr * mult_c) * wd_c)   2u relative;  p = q - d q, only when d > 0:
                                      Ep <- Ep + 3u d|q| + u|p|
`AdamW64.VARIANTS` are deliberately wrong element functions for the gate checks.

Sums of squares.  A sum of N non-negative fp32 terms, each the rounded square of an input, added in fp32 in ANY order, lies within
(1 + u)^(N + 1) - 1 ~ (N + 1) u relative of the exact sum.  N is the number of elements that can meet in fp32 before the contract goes to double:
  * vk_grad_sqnorm_chunks: the sum of one 1024-element chunk is a float, "a function of that chunk's data alone"       N_CHUNK = 1024
  * vk_grad_norm_clip(_masked): `partial` holds vk_grad_norm_workspace_floats() = NORM_BLOCKS floats, one per workgroup of 256 lanes that
    strides over the n / 4 float4 groups; what one workgroup sees meets in fp32, the partials are added in double     n_partial(n)
  * vk_grad_sqnorm_list: "double partials"; the four squares of one 16-byte group meet in fp32, and the slot itself is a float
    (one more rounding)                                                                                                N_LIST = 4 (+ 1)
The norm is fl(fl32(sqrt(S)) * pre_scale): a relative error e of S gives e / 2, then sqrt, the cast and the product round once each:
En = norm (e / 2 + 3u).  coef = min(1, max_norm / (norm + 1e-6)): the sum and the quotient round once each, Ed = En + u d,
Ec = c Ed / (d - Ed) + u c; max_norm <= 0 gives exactly 1 (bound 0).

Slab sums: dst[i] = sum_s src[s * stride + i], sequential in s.  nslabs - 1 additions: gate (nslabs - 1) u sum_s |x_s|; and because the order is
the contract and additions cannot contract, the sequential fp32 sum is the bitwise expectation.  vk_side_tail kind 0 is the same statement;
kind 1 is a column sum over count (+ count2) records (+ the old value when accumulating) in no stated order: (count + count2 + 1) u sum|x|.
vk_axpy_f32: y + alpha x with the product rounded or fused: u|alpha x| + u|y + alpha x|.

Bit statements (torch on the CPU rounds to nearest even): vk_cast_f32_bf16 = RNE; vk_mul_bf16 = RNE of the fp32 product of two bf16 values
(16 significant bits: exact in fp32 while it stays normal); vk_sum_slabs_bf16 = RNE of the sequential fp32 sum; AdamW's bf16 shadow = RNE
of the fp32 p the kernel itself wrote."""
import collections
import math

import torch

U = 2.0 ** -24
CHUNK = 1024
SKIP = 255                     # VK_CHUNK_SKIP
N_CHUNK = 1024
N_LIST = 4
E_LIST = (N_LIST + 1 + 1) * U    # relative: the group of four in fp32, then the float slot
NORM_BLOCKS = 1024             # vk_grad_norm_workspace_floats()
SQ_GROUPS = 128                # "256 floats of scratch" = 128 doubles: the first level of vk_grad_norm_from_chunks
TAIL_MAX_JOBS = 16
NCUS = (1, 24, 256)
NARROW_U = 8                   # 2048-element blocks (two chunks) one workgroup of vk_adamw_step_on has in flight per trip


def f32(x):
    """The fp32 value nearest to x, as a Python float (an exact double)."""
    return float(torch.tensor(x, dtype=torch.float32))


def ratio(got, want, bound):
    """max over elements of |got - want| / (2 * bound); > 1 is outside the gate.  A zero bound admits only the exact value."""
    want = torch.as_tensor(want, dtype=torch.float64)
    got = torch.as_tensor(got).to(want.device).double().reshape(want.shape)
    bound = torch.as_tensor(bound, dtype=torch.float64, device=want.device).expand(want.shape)
    diff = (got - want).abs()
    r = torch.where(bound > 0, diff / (2 * bound), torch.where(diff == 0, torch.zeros_like(diff), torch.full_like(diff, math.inf)))
    r = torch.where(torch.isnan(diff), torch.full_like(diff, math.inf), r)
    return float(r.max()) if r.numel() else 0.0


# ============================================================================================ AdamW
Hyper = collections.namedtuple("Hyper", "lr b1 b2 eps step_mult grad_scale clip mult wd")
MULT8 = (1.0, 0.5, 2.0, 1.5, 0.25, 3.0, 0.75, 1.25)
WD8 = (0.01, 0.0, 0.1, 0.05, 0.02, 0.0, 0.03, 0.2)


def hyper(lr=1e-3, b1=0.9, b2=0.999, eps=1e-6, step_mult=1.7, grad_scale=1.0, clip=None, mult=MULT8, wd=WD8):
    return Hyper(f32(lr), f32(b1), f32(b2), f32(eps), f32(step_mult), f32(grad_scale), None if clip is None else f32(clip),
                 tuple(f32(x) for x in mult), tuple(f32(x) for x in wd))


class AdamW64:
    """The element function over flat arrays; cls_elem holds each element's class (anything outside 0..7 takes no part)."""
    VARIANTS = ("decay_first", "decay_step", "eps_inside", "no_step_mult", "no_clip", "no_cls_mult")

    def __init__(self, p, m, v, cls_elem, h, variant=None):
        assert variant is None or variant in self.VARIANTS
        self.p, self.m, self.v = p.double().clone(), m.double().clone(), v.double().clone()
        self.M = self.m.abs()
        self.Ep, self.Em, self.Ev = torch.zeros_like(self.p), torch.zeros_like(self.p), torch.zeros_like(self.p)
        c = cls_elem.to(self.p.device).long()
        self.live = (c >= 0) & (c <= 7)
        c = c.clamp(0, 7)
        self.mult = torch.tensor(h.mult, dtype=torch.float64, device=self.p.device)[c]
        self.wd = torch.tensor(h.wd, dtype=torch.float64, device=self.p.device)[c]
        self.h, self.variant = h, variant

    @torch.no_grad()
    def step(self, g):
        h, var = self.h, self.variant
        gs = h.grad_scale * (h.clip if h.clip is not None and var != "no_clip" else 1.0)
        g = g.to(self.p.device).double() * gs
        eg = 2 * U * g.abs() if gs != 1.0 else torch.zeros_like(g)
        m = h.b1 * self.m + (1 - h.b1) * g
        M = h.b1 * self.M + (1 - h.b1) * g.abs()
        Em = h.b1 * self.Em + 4 * U * M + (1 - h.b1) * eg
        v = h.b2 * self.v + (1 - h.b2) * g * g
        Ev = h.b2 * self.Ev + 6 * U * v + 2 * (1 - h.b2) * g.abs() * eg
        lrc = h.lr * (self.mult if var != "no_cls_mult" else 1.0)
        step = lrc * (h.step_mult if var != "no_step_mult" else 1.0)
        d = (step if var == "decay_step" else lrc) * self.wd
        d = d if torch.is_tensor(d) else torch.full_like(self.p, d)
        p, Ep = self.p, self.Ep
        if var == "decay_first":
            p = p - d * p
        den = (v + h.eps).sqrt() if var == "eps_inside" else v.sqrt() + h.eps
        dden = torch.minimum(Ev / (2 * v.sqrt()).clamp_min(1e-300), Ev.sqrt()) + 2 * U * den
        r = m / den
        er = (Em + r.abs() * dden) / torch.maximum(den - dden, den / 2) + U * r.abs()
        q = p - step * r
        Ep = Ep + step * er + 3 * U * step * r.abs() + U * q.abs()
        if var != "decay_first":
            q2 = q - d * q
            Ep = Ep + torch.where(d > 0, 3 * U * d * q.abs() + U * q2.abs(), torch.zeros_like(q))
            q = q2
        else:                                          # the wrong variant carries the same two terms: only its values differ
            Ep = Ep + torch.where(d > 0, 3 * U * d * q.abs() + U * q.abs(), torch.zeros_like(q))
        L = self.live
        self.p, self.m, self.v, self.M = torch.where(L, q, self.p), torch.where(L, m, self.m), torch.where(L, v, self.v), torch.where(L, M, self.M)
        self.Ep, self.Em, self.Ev = torch.where(L, Ep, self.Ep), torch.where(L, Em, self.Em), torch.where(L, Ev, self.Ev)

    def excess(self, p=None, m=None, v=None):
        return max([ratio(got, want, err) for got, want, err in ((p, self.p, self.Ep), (m, self.m, self.Em), (v, self.v, self.Ev))
                    if got is not None] + [0.0])


AdamCase = collections.namedtuple("AdamCase", "id nch cls_mode cls_off h shadow seed")
ADAM_STEPS = 3


def _adam_cases():
    out = []

    def add(nch, cls_mode, cls_off=0, shadow=True, **kw):
        out.append(AdamCase("nch%d-%s%s%s%s" % (nch, cls_mode, "-off%d" % cls_off if cls_off else "", "" if shadow else "-noshadow",
                                               "".join("-%s%s" % (k[:2], "%g" % v if isinstance(v, float) else "x") for k, v in sorted(kw.items()))),
                            nch, cls_mode, cls_off, hyper(**kw), shadow, 100 + len(out)))
    add(1, "null")
    add(2, "mixed", clip=0.71)
    add(3, "allskip", cls_off=1)
    add(7, "lastlive", cls_off=2)                       # an odd count
    add(15, "firstlive", cls_off=3)                     # 2 * 8 * ncus - 1 for ncus = 1
    add(16, "mixed", cls_off=1)
    add(17, "mixed", cls_off=2, shadow=False)
    add(383, "mixed", cls_off=3, grad_scale=0.5)        # 2 * 8 * 24 - 1
    add(384, "mixed", clip=0.31, grad_scale=4.0)
    add(385, "mixed", cls_off=1)
    add(3 * 384 + 5, "mixed", cls_off=2, clip=0.71, grad_scale=0.5)     # three trips of 24 workgroups and a ragged tail
    add(4095, "mixed", cls_off=3)                       # 2 * 8 * 256 - 1
    add(4096, "null", shadow=False)
    add(4097, "mixed", cls_off=1, clip=0.9)
    add(2 * 4096 + 5, "mixed", cls_off=2)               # two trips of 256 workgroups and a ragged tail
    add(9, "mixed", lr=0.05, wd=tuple(25 * w for w in WD8))      # lr * wd up to 0.25: separates the decay-order variants in one step
    return out


ADAM_CASES = _adam_cases()


def chunk_classes(nch, mode, gen):
    """uint8 [nch] or None."""
    if mode == "null":
        return None
    c = (torch.arange(nch) % 8).to(torch.uint8)
    if mode == "mixed":
        c[torch.rand(nch, generator=gen) < 0.15] = SKIP
        if nch >= 2:
            c[-1] = 7                                   # the ragged last chunk is live, with a class of its own multiplier
    elif mode == "allskip":
        c[:] = SKIP
    elif mode == "lastlive":
        c[:-1] = SKIP
    elif mode == "firstlive":
        c[1:] = SKIP
    else:
        raise ValueError(mode)
    return c


def adam_data(n, gen):
    """fp32 p, m, v and ADAM_STEPS gradients of n elements: |g| log-uniform over 1e-6 .. 1e2, one element in 16 with g = 0 and v = 0 (half of
    those with m = 0 too), everything else normal and finite through three steps."""
    p = torch.randn(n, generator=gen)
    m = torch.randn(n, generator=gen) * 0.01
    v = torch.rand(n, generator=gen) * 1e-3 + 1e-8
    gs = []
    zero = torch.rand(n, generator=gen) < 1.0 / 16
    for _ in range(ADAM_STEPS):
        mag = torch.pow(10.0, torch.rand(n, generator=gen) * 8 - 6)
        g = mag * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
        gs.append(g.float())
    gs[0][zero] = 0.0
    v[zero] = 0.0
    m[zero & (torch.rand(n, generator=gen) < 0.5)] = 0.0
    m[zero] *= 1e-3                                     # m / eps stays a moderate number
    return p.float(), m.float(), v.float(), gs


def adam_inputs(case):
    gen = torch.Generator().manual_seed(case.seed)
    cls = chunk_classes(case.nch, case.cls_mode, gen)
    p, m, v, gs = adam_data(case.nch * CHUNK, gen)
    return dict(p=p, m=m, v=v, gs=gs, cls=cls)


def cls_elem(cls, nch):
    return (torch.zeros(nch, dtype=torch.uint8) if cls is None else cls).repeat_interleave(CHUNK)


def narrow_owner(nch, ncus):
    """How often each chunk is visited by vk_adamw_step_on's walk: workgroup b takes the 2048-element blocks b + (k * NARROW_U + u) * ncus,
    halves sub = 0 / 1 of its 512 threads take the two chunks of a block; a trip starts while its first block begins inside the arena."""
    seen = [0] * nch
    for b in range(ncus):
        blk = b
        while blk * 2 < nch:
            for u in range(NARROW_U):
                for sub in range(2):
                    c = (blk + u * ncus) * 2 + sub
                    if c < nch:
                        seen[c] += 1
            blk += ncus * NARROW_U
    return seen


# list form: (numel, cls, which of p / g / m / v starts off a 16-byte boundary, by how many floats)
LIST_NUMELS = (1, 2, 3, 4, 5, 1023, 1024, 1025, 4099, 1024 * 1024 + 1)
LIST_CLS = (0, 7, SKIP, 8, -1)


def list_table():
    out, k = [], 0
    for numel in LIST_NUMELS:
        out.append((numel, 0 if numel != 5 else 7, None, 0))
    for which in "pgmv":
        for off in (1, 2, 3):
            out.append(((5, 1025, 4099, 7, 1023)[k % 5], (0, 7, 3, 5)[k % 4], which, off))
            k += 1
    for c in LIST_CLS:
        out.append((1027, c, None, 0))
        out.append((6, c, "g", 1))
    for i in range(12):
        out.append((17 * i + 1, i % 8, None, 0))
    assert len(out) >= 40
    return out


# ============================================================================================ sums of squares, norm, clip
def n_partial(n):
    """fp32 terms that can meet in one workgroup's partial of vk_grad_norm_clip: 256 lanes, 4 elements per group, ceil(groups / lanes of the grid)."""
    return 4 * 256 * -(-(n // 4) // (NORM_BLOCKS * 256))


def chunk_sums64(g, cls=None):
    """double [nch]: exact sums of squares per 1024-element chunk, 0 for skipped chunks."""
    s = (g.double().view(-1, CHUNK) ** 2).sum(1)
    if cls is not None:
        s = torch.where(cls.to(s.device) == SKIP, torch.zeros_like(s), s)
    return s


def norm_clip64(S, eS, pre_scale, max_norm):
    """(norm, En, coef, Ec) from the exact total S with relative error eS; pre_scale / max_norm fp32 values as doubles."""
    norm = math.sqrt(S) * pre_scale
    En = abs(norm) * (eS / 2 + 3 * U)
    if max_norm <= 0:
        return norm, En, 1.0, 0.0
    d = norm + f32(1e-6)
    Ed = En + U * d
    c = max_norm / d
    Ec = c * Ed / (d - Ed) + U * c
    return norm, En, min(1.0, c), Ec


def group_ranges(total):
    """First level of vk_grad_norm_from_chunks: SQ_GROUPS contiguous runs of ceil(total / SQ_GROUPS) chunk sums (the last ones short or empty)."""
    per = -(-total // SQ_GROUPS)
    return [(min(i * per, total), min(i * per + per, total)) for i in range(SQ_GROUPS)]


NormCase = collections.namedtuple("NormCase", "id total mask pre_scale max_mode")
FULL = "full"                   # the chunk count of the ctrl_vilbert_base arena: resolved by the tests through the engine's arena sizing
NORM_CASES = [NormCase("t2-none", 2, "none", 1.0, "above"), NormCase("t2-end", 2, "end", 0.5, "zero"),
              NormCase("t126-start", 126, "start", 1.0, "below"), NormCase("t128-middle", 128, "middle", 1.0 / 3, "ulp"),
              NormCase("t130-end", 130, "end", 3.0, "above"), NormCase("t258-mixed", 258, "mixed", 0.125, "below"),
              NormCase("t258-none", 258, "none", 1.0, "ulp"), NormCase("full-mixed", FULL, "mixed", 1.0 / 256, "below")]
HEAVY = 10                      # exponent of the heavy chunks: 2^20 times a plain chunk's share of the sum


def _base():
    gen = torch.Generator().manual_seed(77)
    b = torch.randn(8, CHUNK, generator=gen).float()
    return b, (b.double() ** 2).sum(1)


BASE, BASESQ = _base()


def norm_plan(total, mode):
    """(exponents int64 [total], mask uint8 [total] or None, heavy live chunks, heavy skipped chunk or None).  Chunk c of the gradient is
    BASE[c % 8] * 2^exp[c] (exact in fp32), so its sum of squares is BASESQ[c % 8] * 4^exp[c].  The worst-case bound (N + 1) u is far above
    one plain chunk's share of a large arena, so the first, the middle and the last live chunk are heavy and one skipped chunk is heavy:
    the totals notice those; every other chunk is held by the elementwise check of its own sum."""
    c = torch.arange(total)
    exp = (c * 7) % 5 - 2
    mask = None
    if mode != "none":
        mask = torch.zeros(total, dtype=torch.uint8)
        run = max(1, total // 5)
        if mode in ("start", "mixed"):
            mask[:run] = SKIP
        if mode in ("middle", "mixed"):
            mask[total // 2: total // 2 + run] = SKIP
        if mode in ("end", "mixed"):
            mask[total - run:] = SKIP
        if total == 2:
            mask[0] = 0
    live = c if mask is None else c[mask != SKIP]
    heavy = sorted({int(live[0]), int(live[len(live) // 2]), int(live[-1])})
    exp[heavy] = HEAVY
    hskip = None
    if mask is not None:
        hskip = int(c[mask == SKIP][-1])
        exp[hskip] = HEAVY
    return exp, mask, heavy, hskip


def norm_grad(exp, device="cpu", lo=0, hi=None):
    """fp32 gradient of chunks [lo, hi) of a plan."""
    hi = len(exp) if hi is None else hi
    c = torch.arange(lo, hi, device=device)
    return (BASE.to(device)[c % 8] * torch.pow(2.0, exp[lo:hi].to(device).float())[:, None]).reshape(-1)


def plan_sums64(exp, mask):
    s = BASESQ[torch.arange(len(exp)) % 8] * torch.pow(4.0, exp.double())
    return s if mask is None else torch.where(mask == SKIP, torch.zeros_like(s), s)


def chunk_ranges(total):
    """(chunk0, nchunks) sub-ranges for vk_grad_sqnorm_chunks: chunk0 > 0, nchunks in {1, 2, 3, 5} (none a multiple of the 4 chunks one
    workgroup takes), up to the last chunk."""
    out = [(1, 1), (1, 2), (3, 3), (total // 2, 5), (max(total - 5, 1), 5), (total - 1, 1)]
    return sorted({(c0, k) for c0, k in out if c0 >= 1 and c0 + k <= total})


def shard_plans(total):
    """Disjoint covers of [0, total) by 2, 3 and 7 ranges (chunk0, nchunks) at seeded random cuts, each in shuffled order: what the ranks
    of the zero1 mode compute one range each."""
    gen = torch.Generator().manual_seed(total)
    plans = []
    for parts in (2, 3, 7):
        if parts > total:
            continue
        cut = sorted(set([0, total] + (torch.randperm(total - 1, generator=gen)[:parts - 1] + 1).tolist()))
        ranges = [(a, b - a) for a, b in zip(cut, cut[1:])]
        plans.append([ranges[i] for i in torch.randperm(len(ranges), generator=gen).tolist()])
    return plans


def max_norm_for(mode, norm):
    return {"above": f32(norm * 2), "below": f32(norm / 2), "ulp": f32(norm), "zero": 0.0}[mode]


# ============================================================================================ slab sums, tail, axpy, cast, mul
def slabs64(src):
    """src [nslabs, n] -> (double sum, bound)."""
    d = src.double()
    return d.sum(0), (src.shape[0] - 1) * U * d.abs().sum(0)


def slabs_seq32(src):
    a = src[0].clone()
    for s in range(1, src.shape[0]):
        a += src[s]
    return a


def tail_cols64(rec, rec2=None, old=None):
    """rec [count, 2, H] (+ rec2 [count2, 2, H]) -> (dgamma | dbeta as [2, H] double, bound)."""
    s, a, n = rec.double().sum(0), rec.double().abs().sum(0), rec.shape[0]
    if rec2 is not None:
        s, a, n = s + rec2.double().sum(0), a + rec2.double().abs().sum(0), n + rec2.shape[0]
    if old is not None:
        s, a = s + old.double(), a + old.double().abs()
    return s, (n + 1) * U * a


def axpy64(y, x, alpha):
    ax = alpha * x.double()
    w = y.double() + ax
    return w, U * ax.abs() + U * w.abs()


GRID_SLABS = 2048 * 256 * 4           # elements one pass of the capped slab-sum grid covers
GRID_CAST = 4096 * 256 * 8            # elements one pass of the capped cast / mul grid covers
SLAB_NS = (1, 3, 4, 5, 1027, GRID_SLABS + 1)
SLAB_COUNTS = (1, 2, 7)


def slab_strides(n):
    """Elements between slabs: the tightest multiple of 4, and one with a gap (NaN in the tests) between the slabs."""
    return ((n + 3) // 4 * 4, (n + 3) // 4 * 4 + 8)


def list_max_numels(true_max):
    """max_numel values vk_grad_sqnorm_list must not depend on: the true maximum and two larger ones."""
    return (true_max, true_max + 1, 3 * true_max + 7)


SlabBf = collections.namedtuple("SlabBf", "id nslabs rows row_len dyn")
SLAB_BF = [SlabBf("s1-r1x4", 1, 1, 4, None), SlabBf("s2-r257x4-mid", 2, 257, 4, 100), SlabBf("s7-r33x32-zero", 7, 33, 32, 0),
           SlabBf("s7-r33x32-more", 7, 33, 32, 40), SlabBf("s2-r33x36-mid", 2, 33, 36, 17), SlabBf("s2-cap-null", 2, GRID_SLABS // 4 + 1, 4, None),
           SlabBf("s2-cap-mid", 2, GRID_SLABS // 4 + 1, 4, GRID_SLABS // 4 - 5)]
CAST_NS = (1, 7, 8, 9, 2055, GRID_CAST + 1)
MulCase = collections.namedtuple("MulCase", "id rows row_len dyn")
MUL_CASES = [MulCase("r1x8", 1, 8, None), MulCase("r2x8-zero", 2, 8, 0), MulCase("r257x8-mid", 257, 8, 100), MulCase("r33x24-more", 33, 24, 50),
             MulCase("cap-null", GRID_CAST // 8 + 1, 8, None), MulCase("cap-mid", GRID_CAST // 8 + 1, 8, GRID_CAST // 8 - 3)]
# (kind, n or H, count, count2 or None, accumulate): 16 jobs of one launch
TAIL_JOBS = [(0, 1, 1, None, 0), (1, 8, 3, None, 0), (0, 3, 2, None, 0), (1, 24, 16, 5, 1), (0, 5, 7, None, 0), (1, 100, 17, None, 1),
             (0, 1027, 2, None, 0), (1, 768, 40, 20, 0), (1, 1000, 15, 33, 1), (0, 4, 7, None, 0), (1, 1, 1, 1, 0), (0, 2048, 1, None, 0),
             (1, 17, 31, None, 0), (0, 1030, 7, None, 0), (1, 1024, 2, 3, 1), (0, 7, 2, None, 0)]


def cast_specials():
    """fp32 bit patterns: +-0, ties to even both ways, the largest finite value (rounds to inf), +-inf, NaN, denormals."""
    bits = [0x00000000, 0x80000000, 0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0xFF7FFFFF,
            0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC12345, 0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80008001, 0x00400000]
    return torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in bits], dtype=torch.int32).view(torch.float32)


def full_chunks(name="ctrl_vilbert_base"):
    """Chunks of the full-size parameter arena, from config/ through the engine's own arena sizing (on the meta device: nothing is allocated)."""
    import os
    from volta_amd.config import BertConfig
    from volta_amd.engine import ParamArena
    from volta_amd.modeling import BertForVLPreTraining
    cfg = BertConfig.from_json_file(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config", name + ".json"))
    with torch.device("meta"):
        model = BertForVLPreTraining(cfg)
    total = ParamArena(model, torch.device("meta"), prefix=model._arena_prefix).total
    assert total % CHUNK == 0
    return total // CHUNK
