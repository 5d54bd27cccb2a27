"""float64 restatements of the visual-target loss family (csrc/vislosses.hip: vk_vis_loss_fwd/_bwd in four kinds, vk_pool_fuse_*,
vk_text_end_rows), of vk_pool_mul_* (csrc/heads.hip), vk_grad_seed (csrc/backbone.hip) and vk_pair_gather (csrc/pairs.hip), with
per-element error gates derived from the roundings the kernels have, the input makers and the case tables that
tests/test_vis_restate_cpu.py, tests/test_vislosses_kernels_gpu.py and tests/test_seed_gather_kernels_gpu.py run.  No GPU, no kernel.

Contract restated (include/volta_hip.h, "The visual targets other than kl_1601").  n = min(*count, max_rows); row i < n predicts grid
position p = pos[i]; x = logits[i, :V], w = weight, g = *gscale:
  MSE    row = w / V sum_c (x_c - t_c)^2                       t = target[p]        dlogits = g w / (n V) 2 (x - t)
  HUBER  row = w / V sum_c h(x_c - t_c), h(d) = d^2 / 2 (|d| < 1) | |d| - 1/2      dlogits = g w / (n V) clamp(x - t, -1, 1)
  XENT   row = w c (lse(x) - x[l]), l = clamp(labels[p], 0, V - 1), c = conf[p] | 1  dlogits = g w c / n (exp(x - lse) - onehot_l)
  NCE    s_j = <sample_j, x>, sample_0 = target[p], sample_j = target[neg_index[p * n_neg + j - 1]] (j = 1 .. n_neg)
         row = w (lse(s) - s_0)                                                     dlogits = g w / n sum_j (exp(s_j - lse) - [j = 0]) sample_j
  *loss_sum += sum_i row_i (atomics, any order); lse[i] (XENT, NCE) and aux[i, 0 .. n_neg] = s (NCE) are saved; dlogits columns [V, ldd)
  of rows < n are +0; nothing else is written.

Gates.  u = 2^-24.  Every gate below is F = 2 times the first-order bound E (tests/test_heads_gpu.py takes the same factor), and a
bf16 output adds half a bf16 ulp of |ref| + F E for its own round to nearest even (attn_restate.half_ulp_bf16).  T = 2^-126 covers
results flushed to zero below the normal range.  depth(V) = ceil(V / 256) + 6 + 3: the serial adds of one thread, the six levels of
the wave reduction and the three cross-wave adds of vl_block_sum.

  MSE / HUBER row.  d = fl(x - t) is off by u |d| (the inputs are exact), so d d (or d d / 2: the half is exact) by 2u and its product
    by one more: 3u per term.  The linear HUBER branch |d| - 1/2 with |d| >= 1 has |d| <= 2 (|d| - 1/2): u |d| + u (|d| - 1/2) <= 3u per
    term as well, and at |d| = 1 the two branches agree in value and slope, so a d that rounds across the switch changes nothing to
    first order.  All terms are non-negative: E_row = (3 + depth(V) + 2) u w / V sum_c term_c; the last 2 are the rounding of w * s
    and of the division by V.  V = 256 k: k_u = 3 + k + 9 + 2.
  MSE / HUBER dlogits.  g w / (n V): the product, the integer product n V (exact below 2^24) and the quotient, 2u; d, u; clamp and
    doubling exact; the product with the factor, u.  E = 4u |ref|.
  XENT lse.  (tests/test_heads_gpu.py lines 5-13, re-counted for this kernel, which has no running rescale.)  y = fl(x - max) <= 0 is
    off by u |y|; __expf(y) = exp2(fl(y log2 e)): the constant and the product round, u |y| each, and v_exp_f32 is good to one ulp, taken
    as 2u: each term carries u (3 |y| + 2), |y| <= Rg = max - min of the row.  (The heads' docstring counts 2 Rg: it takes x - max as
    exact.)  The sum adds depth(V) u, its logarithm __logf = log2(s) ln 2 three roundings relative to log s, and the final add u |lse|:
    E_lse = u (3 Rg + depth(V) + 2 + 3 log s + |lse|).  V = 1: Rg = 0, s = 1, lse = x exactly -- the gate is u |x| + 12u, the result
    is in fact exact.
  XENT row.  w c (lse - x_l): E = w c (E_lse + 3u |lse - x_l|): the difference, and one rounding each for weight and conf.
  XENT dlogits.  p = __expf(fl(x - lse')) with the kernel's saved lse' within F E_lse of lse: relative u (3 |x - lse| + 2) + F E_lse.
    p - onehot rounds once, g w c / n three times (two products, the quotient), the product with it once:
    E = |g w c / n| (p (u (3 |x - lse| + 2) + F E_lse) + 5u |p - onehot|) + T.
  NCE score.  Each lane adds 4 products per trip over ceil(V / 256) trips, serially (a fused multiply-add only removes roundings),
    then six reduction levels: E_s_j = (4 ceil(V / 256) + 8) u sum_c |t_c x_c|, that is (V / 64 + 8) u at V = 256 k.
  NCE lse.  attn_restate's Else with n = n_neg + 1 scores and this kernel's exponent error:
    Eexp_j = u (3 |s_j - lse| + 2); r = sum_j P_j (E_s_j + Eexp_j); E_lse = r + gamma2(n) + 4u log n + 8u + u |lse|
    (gamma2(n) = 2 n u / (1 - 2 n u) >= the at most min(n - 1, 9) adds the kernel has).
  NCE row.  w (lse - s_0): E = w (E_lse + E_s_0 + 3u |lse - s_0|).
  NCE dlogits.  q_j = (exp(s'_j - lse') - [j = 0]) g w / n from the SAVED scores and lse:
    E_q_j = |g w / n| (P_j (E_s_j + Eexp_j + F E_lse) + 4u |P_j - [j = 0]|) + T; dlogits_c = sum_j q_j sample_j[c] is n serial
    multiply-adds: E = sum_j E_q_j |sample_j[c]| + n u sum_j |q_j sample_j[c]|.
  loss_sum.  The atomics add the n rows to what stands there in any order: after k forwards over a start value s0,
    gate = k sum_i F E_row_i + F (k n) u (|s0| + k sum_i |row_i|).  The forward is not deterministic and is not asserted to be.

Exact cases (no gate: the expected bits are the float64 value rounded to nearest even, `bf16_bits`):
  * fusions with p = 0: the product of two bf16 values has 16 significant bits, their sum at most 8 + (exponent span 2^-6 .. 2^3 of
    `pooled_inputs`) = 18: both exact in fp32, one rounding to bf16.  With p > 0 the fp32 constant 1 / (1 - p) and the product with it
    round before the bf16 store: within one bf16 ulp of the exactly rounded value, and the share of elements that differ is held
    under twice the share a plain numpy fp32 evaluation (`fuse_fp32`) leaves on the same inputs.
  * vk_grad_seed (at most one fp32 add, one round to bf16), vk_pair_gather, vk_text_end_rows, vk_nce_negatives.
  * the exact-integer family: x, t small integers, weight and V powers of two: every NCE score, every MSE / HUBER row sum and the
    MSE loss_sum are exact in fp32 whatever the order of the adds."""
import math
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
F = 2.0
MSE, NCE, XENT, HUBER = 1, 2, 3, 5           # VK_VIS_*
KIND_NAME = {MSE: "mse", NCE: "nce", XENT: "xent", HUBER: "huber"}
NCE_MAX_SAMPLES = 128
FUSE_MUL, FUSE_SUM, FUSE_TEXT = 0, 1, 2
GRID_B, GRID_R = 3, 5
LABELLED = (0, 3, 4, 7, 9, 12, 14)           # grid positions of the labelled rows: index 0 and index B * R - 1 among them
LABEL_POISON = 1 << 40
LOSS_START = 3.0
XR = 3                                       # guard rows past max_rows in every row buffer


def gamma2(n):
    return 2 * n * U / (1 - 2 * n * U)


def depth(V):
    return math.ceil(V / 256) + 6 + 3


# ------------------------------------------------------------------------------------------------ bf16 helpers (numpy)
def half_ulp_bf16(x):
    """Half a bf16 ulp at |x| (float64 array): 2^-134 at 0 and in the subnormal range (attn_restate.half_ulp_bf16)."""
    _, e = np.frexp(np.abs(x))
    e = np.where(x == 0, -125, np.maximum(e, -125))
    return np.ldexp(1.0, e - 9)


def bf16_bits(x):
    """float64 -> bf16 bit patterns (uint16), ONE round to nearest even from the float64 value (no detour over fp32)."""
    x = np.asarray(x, np.float64)
    _, e = np.frexp(np.abs(x))
    e = np.maximum(e, -125)                                  # subnormals: fixed quantum 2^-133
    q = np.rint(np.ldexp(np.abs(x), 8 - e))                  # |x| in units of 2^(e - 8); rint is ties-to-even
    v = np.copysign(np.ldexp(q, e - 8), x).astype(np.float32)  # exact: 8 significant bits
    return (v.view(np.uint32) >> 16).astype(np.uint16)


def f32_to_bf16_bits(x):
    """fp32 -> bf16 bits, round to nearest even on the bit pattern (no NaN among the values the tests pass)."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    with np.errstate(invalid="ignore"):                       # canaries and poison are signalling-NaN patterns
        return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def ordered(bits):
    """bf16 bits -> integers in value order (+0 and -0 both 0): the difference of two is their distance in bf16 steps."""
    b = np.asarray(bits, np.uint16).astype(np.int64)
    return np.where(b < 0x8000, b, -(b & 0x7FFF))


def bf16_gate(ref, E):
    return F * E + half_ulp_bf16(np.abs(ref) + F * E)


def worst(got, ref, gate):
    """max |got - ref| / gate over the elements (inf where got is NaN or infinite), for an empty array 0."""
    got, ref, gate = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(gate, np.float64)
    if got.size == 0:
        return 0.0
    d = np.abs(got - ref)
    d = np.where(np.isfinite(got), d, np.inf)
    return float((d / gate).max())


# ------------------------------------------------------------------------------------------------ loss cases and inputs
Case = namedtuple("Case", "id kind V n_neg family conf ld ldd max_rows count gscale weight")


def _round_up(v, m):
    return -(-v // m) * m


def _case(kind, V, i, n_neg=0, family="gauss", conf=False, count=None, extra=None):
    """Layout choices cycled by i, so that each kind meets ld = V and V + 12, ldd = V and V rounded up to 64 plus 64, max_rows equal to
    and above the number of labelled rows, and the three values of gscale."""
    nl = len(LABELLED)
    max_rows = nl + (2 if (i // 2) % 2 else 0) if extra is None else nl + extra
    ld = V if i % 2 == 0 else V + 12
    ldd = V if (i // 2 + i) % 2 == 0 else _round_up(V, 64) + 64
    gscale = (1.0, 0.7, 2.0 ** -10)[i % 3]
    weight = 2.0 if family == "int" else 1.7
    cnt = nl if count is None else count
    cid = "%s%s-V%d%s-%s-ld%d-ldd%d-mr%d-n%d-g%d" % (KIND_NAME[kind], "+conf" if conf else "", V, "-neg%d" % n_neg if kind == NCE else "", family,
                                                     ld, ldd, max_rows, cnt, i % 3)
    return Case(cid, kind, V, n_neg, family, conf, ld, ldd, max_rows, cnt, gscale, weight)


VS = (1, 63, 255, 256, 257, 400, 1601, 2048)
NCE_VS = (4, 252, 256, 260, 2048)
NCE_NEGS = (1, 2, 3, 4, 126, 127)


def loss_cases():
    out, i = [], 0
    for kind in (MSE, HUBER, XENT):
        for V in VS:
            for conf in ((False, True) if kind == XENT else (False,)):
                out.append(_case(kind, V, i, conf=conf))
                i += 1
        out += [_case(kind, 1601, 0), _case(kind, 1601, 3), _case(kind, 1601, 1)]     # odd ldd = V = 1601 with ld = V and V + 12, and the padded one
    for V in NCE_VS:
        for nn in NCE_NEGS:
            out.append(_case(NCE, V, i, n_neg=nn))
            i += 1
    for V in (63, 257, 1601, 2048):                                 # wide rows: scores near +100 and -100
        out.append(_case(XENT, V, i, family="wide", conf=V == 257))
        i += 1
    for V, nn in ((4, 3), (260, 127), (2048, 4), (2048, 127)):
        out.append(_case(NCE, V, i, n_neg=nn, family="wide"))
        i += 1
    for kind in (MSE, HUBER):                                       # exact integers
        for V in (1, 256, 2048):
            out.append(_case(kind, V, i, family="int"))
            i += 1
    for V, nn in ((4, 1), (256, 126), (2048, 127), (2048, 3)):
        out.append(_case(NCE, V, i, n_neg=nn, family="int"))
        i += 1
    for kind, V, nn in ((MSE, 257, 0), (HUBER, 400, 0), (XENT, 257, 0), (NCE, 260, 5)):   # the device-side count: 0, 1, and max_rows < and > labelled
        for cnt, extra in ((0, 0), (0, 2), (1, 0), (1, 2)):
            out.append(_case(kind, V, i, n_neg=nn, conf=kind == XENT, count=cnt, extra=extra))
            i += 1
    seen, uniq = set(), []
    for c in out:                                                   # the cycled layouts may repeat a hand-picked one
        if c.id not in seen:
            seen.add(c.id)
            uniq.append(c)
    return uniq


def over_count_cases():
    """*count above max_rows (the engine cannot produce it: required away in the header): only the write set is checked."""
    nl = len(LABELLED)
    return [_case(kind, V, 1, n_neg=nn, count=nl + 2, extra=0) for kind, V, nn in ((MSE, 257, 0), (HUBER, 63, 0), (XENT, 400, 0), (NCE, 260, 4))]


def case_seed(case):
    import zlib
    return zlib.crc32(case.id.encode()) & 0xFFFF


def make_inputs(case, seed=None, grid=(GRID_B, GRID_R), labelled=LABELLED, neg=None):
    """The contract's inputs as numpy arrays with everything outside them poisoned:
      logits  fp32 [max_rows + XR, ld]: rows < nl hold predictions in columns < V; NaN in the pad columns and in every other row
      target  fp32 [B R, V]: rows that are labelled (MSE, HUBER, NCE) or drawn as a labelled row's negative (NCE), NaN elsewhere
      labels  int64 [B R]: 2^40 at unlabelled positions; conf fp32 [B R]: NaN there
      pos     int32 [max_rows + XR]: the labelled positions, then 0
      neg     int32 [B R, n_neg]: negatives of the labelled positions; every other row points at a NaN row of target (or at row 0).
    `neg` given (vk_nce_negatives' output, [B R, n_neg]): used as it stands."""
    rng = np.random.default_rng(case_seed(case) if seed is None else seed)
    BR, nl, V, kind = grid[0] * grid[1], len(labelled), case.V, case.kind
    given = neg
    rows = case.max_rows + XR
    pos = np.zeros(rows, np.int32)
    pos[:nl] = labelled
    x = rng.standard_normal((nl, V)).astype(np.float32)
    inp = dict(case=case, pos=pos, nl=nl, target=None, labels=None, conf=None, neg=None)
    if kind in (MSE, HUBER):
        t = rng.standard_normal((BR, V)).astype(np.float32) * np.float32(2.0 if kind == HUBER else 1.0)   # |x - t| on both sides of 1
        if case.family == "int":
            x = rng.integers(-3, 4, (nl, V)).astype(np.float32)
            t = rng.integers(-3, 4, (BR, V)).astype(np.float32)
            if kind == HUBER:
                t = t * np.float32(0.5)                       # differences in halves: both branches, every term a multiple of 1/8
        used = np.zeros(BR, bool)
        used[list(labelled)] = True
        t[~used] = np.nan
        inp["target"] = t
    elif kind == XENT:
        labels = np.full(BR, LABEL_POISON, np.int64)
        labels[list(labelled)] = rng.integers(0, V, nl)
        if case.family == "wide":
            for r, own in ((1, True), (2, False)):            # rows with +100 and -100; the label on the peak (p - 1 cancels) and off it
                hi, lo = (int(c) for c in rng.choice(V, 2, replace=False))
                x[r, hi], x[r, lo] = 100.0 + x[r, hi], -100.0 + x[r, lo]
                labels[labelled[r]] = hi if own else lo
        inp["labels"] = labels
        if case.conf:
            conf = np.full(BR, np.nan, np.float32)
            conf[list(labelled)] = rng.random(nl).astype(np.float32)
            inp["conf"] = conf
    else:
        nn = case.n_neg
        t = rng.standard_normal((BR, V)).astype(np.float32)
        x = x * np.float32(0.05)
        if case.family == "int":
            x = rng.integers(-3, 4, (nl, V)).astype(np.float32)
            t = rng.integers(-3, 4, (BR, V)).astype(np.float32)
        neg = np.zeros((BR, nn), np.int32)
        used = np.zeros(BR, bool)
        for p in labelled:
            others = np.array([q for q in range(BR) if q != p])
            neg[p] = rng.choice(others, nn, replace=True) if given is None else given[p]
            used[p] = True
            used[neg[p]] = True
        if case.family == "wide":                             # row 1: score_0 near +100, the first negative's near -100
            p = labelled[1]
            ab = np.stack([t[p], t[neg[p, 0]]]).astype(np.float64)                    # x in their span with <t_p, x> = 100, <t_neg, x> = -100
            x[1] = (np.linalg.solve(ab @ ab.T, np.array([100.0, -100.0])) @ ab).astype(np.float32)
        t[~used] = np.nan
        poison = int(np.flatnonzero(~used)[0]) if (~used).any() else 0
        for q in range(BR):
            if q not in labelled:
                neg[q] = poison if given is None else given[q]
        inp["target"], inp["neg"] = t, neg
    logits = np.full((rows, case.ld), np.nan, np.float32)
    logits[:nl, :V] = x
    inp["logits"] = logits
    return inp


# ------------------------------------------------------------------------------------------------ float64 restatement of the losses
def _lse64(s):
    m = s.max(-1, keepdims=True)
    return (m + np.log(np.exp(s - m).sum(-1, keepdims=True)))[..., 0]


def restate(inp):
    """-> dict: n; rows [n] (weighted row losses) + g_rows; lse [n] + g_lse (XENT, NCE); aux [n, n_neg + 1] + g_aux (NCE);
    dlogits [n, V] = d(sum rows / max(n, 1)) / d logits x gscale + g_dlogits (bf16 gate).  weight and gscale are taken as the fp32
    values the kernel receives."""
    c = inp["case"]
    V, kind = c.V, c.kind
    n = min(c.count, c.max_rows, inp["nl"])
    w, g = float(np.float32(c.weight)), float(np.float32(c.gscale))
    x = inp["logits"][:n, :V].astype(np.float64)
    pos = inp["pos"][:n]
    out = dict(n=n)
    nd = max(n, 1)
    if kind in (MSE, HUBER):
        t = inp["target"][pos].astype(np.float64)
        d = x - t
        term = d * d if kind == MSE else np.where(np.abs(d) < 1.0, 0.5 * d * d, np.abs(d) - 0.5)
        out["rows"] = w * term.sum(1) / V
        out["g_rows"] = F * (3 + depth(V) + 2) * U * out["rows"]
        dl = g * w / (nd * V) * (2.0 * d if kind == MSE else np.clip(d, -1.0, 1.0))
        out["dlogits"], out["g_dlogits"], out["e_dlogits"] = dl, bf16_gate(dl, 4 * U * np.abs(dl)), F * (4 * U * np.abs(dl))
    elif kind == XENT:
        lab = np.clip(inp["labels"][pos], 0, V - 1)
        cf = inp["conf"][pos].astype(np.float64) if inp["conf"] is not None else np.ones(n)
        lse = _lse64(x) if n else np.zeros(0)
        rg = (x.max(1) - x.min(1)) if n else np.zeros(0)
        logs = lse - (x.max(1) if n else 0.0)
        e_lse = U * (3 * rg + depth(V) + 2 + 3 * logs + np.abs(lse))
        xl = x[np.arange(n), lab]
        out["lse"], out["g_lse"] = lse, F * e_lse
        out["rows"] = w * cf * (lse - xl)
        out["g_rows"] = F * w * cf * (e_lse + 3 * U * np.abs(lse - xl))
        p = np.exp(x - lse[:, None])
        oh = np.zeros_like(p)
        oh[np.arange(n), lab] = 1.0
        sc = (g * w * cf / nd)[:, None]
        dl = sc * (p - oh)
        E = np.abs(sc) * (p * (U * (3 * np.abs(x - lse[:, None]) + 2) + F * e_lse[:, None]) + 5 * U * np.abs(p - oh)) + TINY
        out["dlogits"], out["g_dlogits"], out["e_dlogits"] = dl, bf16_gate(dl, E), F * E
    else:
        nn = c.n_neg
        ns = nn + 1
        tg = inp["target"].astype(np.float64)
        idx = np.concatenate([pos[:, None].astype(np.int64), inp["neg"][pos].astype(np.int64)], 1)      # [n, ns] sample rows
        smp = tg[idx]                                                                                    # [n, ns, V]
        s = np.einsum("njc,nc->nj", smp, x)
        e_s = (4 * math.ceil(V / 256) + 8) * U * np.einsum("njc,nc->nj", np.abs(smp), np.abs(x))
        lse = _lse64(s) if n else np.zeros(0)
        P = np.exp(s - lse[:, None])
        e_exp = U * (3 * np.abs(s - lse[:, None]) + 2)
        r = (P * (e_s + e_exp)).sum(1)
        e_lse = r + gamma2(ns) + 4 * U * math.log(ns) + 8 * U + U * np.abs(lse)
        out["aux"], out["g_aux"] = s, F * e_s + TINY
        out["lse"], out["g_lse"] = lse, F * e_lse
        out["rows"] = w * (lse - s[:, 0])
        out["g_rows"] = F * w * (e_lse + e_s[:, 0] + 3 * U * np.abs(lse - s[:, 0]))
        oh = np.zeros_like(P)
        oh[:, 0] = 1.0
        sc = g * w / nd
        q = sc * (P - oh)
        e_q = abs(sc) * (P * (e_s + e_exp + F * e_lse[:, None]) + 4 * U * np.abs(P - oh)) + TINY
        dl = np.einsum("nj,njc->nc", q, smp)
        E = np.einsum("nj,njc->nc", e_q, np.abs(smp)) + ns * U * np.einsum("nj,njc->nc", np.abs(q), np.abs(smp))
        out["dlogits"], out["g_dlogits"], out["e_dlogits"] = dl, bf16_gate(dl, E), F * E
    return out


def loss_sum_gate(ref, start=LOSS_START, k=1):
    """Gate of *loss_sum after k forwards over `start` (module docstring)."""
    n = ref["n"]
    return k * float(ref["g_rows"].sum()) + F * k * n * U * (abs(start) + k * float(np.abs(ref["rows"]).sum())) + (0.0 if n == 0 else TINY)


def check_loss(ref, got, case, start=LOSS_START, k=1):
    """Worst |got - ref| / gate per output of one forward + backward.  got: dict with loss (float: *loss_sum after k forwards), lse [n],
    aux [n, n_neg + 1], dlogits (bf16 VALUES as float, [n, V]).  -> {name: ratio}; a ratio above 1 is a failure."""
    n = ref["n"]
    res = {}
    want = start + k * float(ref["rows"].sum())
    gate = loss_sum_gate(ref, start, k)
    res["loss_sum"] = 0.0 if float(got["loss"]) == want else (abs(float(got["loss"]) - want) / gate if gate > 0 and math.isfinite(float(got["loss"])) else math.inf)
    if n == 0:
        return res
    if "lse" in ref:
        res["lse"] = worst(got["lse"], ref["lse"], ref["g_lse"])
    if "aux" in ref:
        res["aux"] = worst(got["aux"], ref["aux"], ref["g_aux"])
    res["dlogits"] = worst(got["dlogits"], ref["dlogits"], ref["g_dlogits"])
    return res


def fp32_share(got, ref):
    """What of the dlogits error the final bf16 round cannot explain, against the fp32 part F E of the gate alone: max over the elements of
    (|got - ref| - half a bf16 ulp of got) / (F E).  The ratio against the whole gate always comes close to 1, because a correctly
    rounded bf16 value may sit half an ulp away and the fp32 terms are small beside that; this figure is the one that shows how much
    of the DERIVED bound the arithmetic uses.  Reported, not asserted (the assertion is the whole gate)."""
    if ref["n"] == 0:
        return 0.0
    got = np.asarray(got, np.float64)
    d = np.abs(got - ref["dlogits"]) - half_ulp_bf16(got)
    with np.errstate(divide="ignore"):                        # an exactly zero gradient has a zero fp32 gate: d < 0 there
        return float(np.maximum(d / ref["e_dlogits"], 0.0).max())


def exact_checks(ref, got, case, start=LOSS_START, k=1):
    """The exact-integer family: -> list of failures (strings).  NCE: aux equals float64 bit for bit; MSE / HUBER: every row sum is
    exact, so *loss_sum after k forwards is the exactly representable float64 sum."""
    bad = []
    if case.family != "int" or ref["n"] == 0:
        return bad
    if case.kind == NCE:
        if not np.array_equal(np.asarray(got["aux"], np.float64), ref["aux"]):
            bad.append("aux differs from the exact integer scores")
    else:
        want = start + k * float(ref["rows"].sum())
        assert float(np.float32(want)) == want, "the maker must keep the integer loss sum representable"
        if float(got["loss"]) != want:
            bad.append("loss_sum %r is not the exact %r" % (float(got["loss"]), want))
    return bad


# ------------------------------------------------------------------------------------------------ pooled-vector fusions
FUSE_B = (1, 5)
FUSE_P = (1, 3, 255, 256, 257, 1024)
FUSE_DROP = (0.0, 0.1, 0.5)
FUSE_SEED, FUSE_SITE = 0x5EED00F00D5, 23        # high 32 bits non-zero


def pooled_inputs(B, P, seed):
    """bf16 bit patterns: pt, pv post-ReLU (zero where dead: +0 and -0 both; live magnitudes within [2^-6, 8]) and dp (both signs, same span)."""
    rng = np.random.default_rng(seed)

    def draw(relu):
        v = rng.standard_normal((B, P))
        mag = np.clip(np.abs(v), 2.0 ** -6, 8.0)
        bits = bf16_bits(np.copysign(mag, v))
        if relu:
            dead = v < 0
            bits = np.where(dead, np.where(rng.random((B, P)) < 0.5, 0x8000, 0x0000), bits).astype(np.uint16)
            if B * P >= 2:
                bits.reshape(-1)[0], bits.reshape(-1)[1] = 0x0000, 0x8000       # both zeros present whenever there is room
        return bits

    return draw(True), draw(True), draw(False)


def keep_scale64(B, P, p, word_bug=False):
    """float64 [B, P]: 1 / (1 - p) where the element is kept, 0 where dropped; all ones at p = 0."""
    if p <= 0:
        return np.ones((B, P))
    from oracle import volta_ref as R
    if word_bug:                                  # the keep word taken as w[0] of the block instead of w[c & 3]
        u = R.philox_u32(FUSE_SEED, FUSE_SITE, B, _round_up(P, 4))
        u = np.repeat(u[:, 0::4], 4, 1)[:, :P]
        keep = u >= np.uint32(min(int(p * 4294967296.0), 0xFFFFFFFF))
    else:
        keep = R.philox_keep_mask(FUSE_SEED, FUSE_SITE, (B, P), p).numpy()
    return np.where(keep, 1.0 / (1.0 - p), 0.0)


def fuse_restate(pt, pv, dp, mode, p, keep=None):
    """float64 forward and backward of out = dropout(pt * pv | pt + pv | pt) through the poolers' ReLUs (dead: pt, pv not > 0 -> +0).
    pt, pv, dp: bf16 bits.  -> out, dyt, dyv (dyv None in text mode) as float64; signs of zero follow IEEE like the kernel's fp32."""
    a, b, d = bf16_value(pt), bf16_value(pv), bf16_value(dp)
    ks = keep_scale64(*a.shape, p) if keep is None else keep
    v = a if mode == FUSE_TEXT else (a + b if mode == FUSE_SUM else a * b)
    out = v * ks
    g = d * ks
    if mode == FUSE_TEXT:
        return out, np.where(a > 0, g, 0.0), None
    dyt = np.where(a > 0, g if mode == FUSE_SUM else g * b, 0.0)
    dyv = np.where(b > 0, g if mode == FUSE_SUM else g * a, 0.0)
    return out, dyt, dyv


def fuse_fp32(pt, pv, dp, mode, p, keep=None):
    """The same formulas in plain numpy fp32, rounded to bf16 bits: what fp32 arithmetic leaves of the exactly rounded value."""
    f = np.float32
    a, b, d = bf16_value(pt).astype(f), bf16_value(pv).astype(f), bf16_value(dp).astype(f)
    ks = (keep_scale64(*a.shape, p) if keep is None else keep) > 0
    ks = np.where(ks, f(1.0 / (1.0 - p)) if p > 0 else f(1.0), f(0.0)).astype(f)
    v = a if mode == FUSE_TEXT else (a + b if mode == FUSE_SUM else a * b)
    out = f32_to_bf16_bits(v * ks)
    g = d * ks
    z = np.zeros_like(g)
    if mode == FUSE_TEXT:
        return out, f32_to_bf16_bits(np.where(a > 0, g, z)), None
    dyt = np.where(a > 0, g if mode == FUSE_SUM else g * b, z)
    dyv = np.where(b > 0, g if mode == FUSE_SUM else g * a, z)
    return out, f32_to_bf16_bits(dyt), f32_to_bf16_bits(dyv)


def check_fused(got_bits, ref64, p, np_bits=None):
    """-> (failure or None, share of elements that are not the exactly rounded value, worst distance in bf16 steps).  p = 0: bit
    equality.  p > 0: within one step, and the share at most twice the numpy fp32 evaluation's (`np_bits`)."""
    want = bf16_bits(ref64)
    got_bits = np.asarray(got_bits, np.uint16)
    if p <= 0:
        bad = int((got_bits != want).sum())
        return ("%d element(s) differ from the exactly rounded value" % bad if bad else None), bad / max(want.size, 1), 0
    if np.isnan(bf16_value(got_bits)).any():
        return "NaN in the output", 1.0, -1
    steps = np.abs(ordered(got_bits) - ordered(want))
    zero_sign = (got_bits != want) & (steps == 0)
    share = float((steps != 0).mean())
    cap = 2.0 * float((np.abs(ordered(np_bits) - ordered(want)) != 0).mean())
    if zero_sign.any():
        return "%d zero(s) of the wrong sign" % int(zero_sign.sum()), share, int(steps.max())
    if int(steps.max()) > 1:
        return "worst element %d bf16 steps away" % int(steps.max()), share, int(steps.max())
    if share > cap:
        return "share %.4f%% of inexactly rounded elements above the cap %.4f%%" % (100 * share, 100 * cap), share, int(steps.max())
    return None, share, int(steps.max())


# ------------------------------------------------------------------------------------------------ the small exact kernels
TEXT_T = (1, 2, 63, 64, 65, 200)


def text_ids(T, seed=0):
    """int64 [6, T]: captions with 0, 1, 2 and T non-zero ids, one ragged, one with a ZERO IN ITS INTERIOR (the count, not the position of
    the first zero, is the contract)."""
    rng = np.random.default_rng(seed + T)
    ids = rng.integers(1, 30000, (6, T)).astype(np.int64)
    for b, k in enumerate((0, 1, 2, T, max(T // 2, 1))):
        ids[b, min(k, T):] = 0
    if T >= 3:
        ids[5, 1] = 0
    return ids


def text_end_rows_restate(ids):
    B, T = ids.shape
    return (np.arange(B) * T + np.maximum((ids != 0).sum(1) - 2, 0)).astype(np.int32)


def grad_seed_restate(src, stride_b, stride_l, B, L, H, dst_bits, row0, ld, y_bits, ldy, accumulate):
    """vk_grad_seed in fp32 numpy: src a flat fp32 array (or None), dst_bits uint16 [rows, ld] (the prefilled buffer), y_bits uint16
    [B L, ldy] or None.  -> the expected dst bits.  One fp32 add at most, then one round to nearest even."""
    out = dst_bits.copy()
    if src is None and accumulate:
        return out
    b, l, h = np.meshgrid(np.arange(B), np.arange(L), np.arange(H), indexing="ij")
    x = src[b * stride_b + l * stride_l + h].reshape(B * L, H).astype(np.float32) if src is not None else np.zeros((B * L, H), np.float32)
    if y_bits is not None:
        yv = bf16_value(y_bits[:, :H])
        with np.errstate(invalid="ignore"):
            x = np.where(yv > 0, x, np.float32(0.0)).astype(np.float32)      # !(y > 0): NaN, -0, +0 and negatives close the gate
    if accumulate:
        x = x + bf16_value(dst_bits[row0:row0 + B * L, :H]).astype(np.float32)
    out[row0:row0 + B * L, :H] = f32_to_bf16_bits(x)
    return out


def pair_gather_restate(src, nbytes, items):
    """src uint8 [n_items * nbytes], items int [npairs] -> uint8 [npairs * nbytes]; an item outside [0, n_items) gives zero bytes."""
    rowsv = src.reshape(-1, nbytes)
    items = np.asarray(items, np.int64)
    ok = (items >= 0) & (items < rowsv.shape[0])
    out = rowsv[np.where(ok, items, 0)].copy()
    out[~ok] = 0
    return out.reshape(-1)
