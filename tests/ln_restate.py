"""float64 restatement of the fused (dropout +) residual + LayerNorm contract (include/volta_hip.h: vk_ln_args, vk_ln_bwd_args) for
tests/test_ln_cpu.py and tests/test_ln_kernels_gpu.py, with elementwise error gates derived from the rounding points the kernels
(csrc/layernorm.hip) actually have, an fp32/bf16 emulation of the kernels' arithmetic (to show the gates are not too tight, and -- with
planted bugs -- not too loose), the dispatch restated, and the case table that the GPU test runs.

Contract restated, on the bf16 / fp32 inputs exactly as given (s = the fp32 dropout scale 1/(1-p), keep = Philox word >= threshold):
  z    = keep_pre s d + x + addvec                            (x, addvec optional; the SAVED z is bf16(z))
  mean = sum_i z_i / H ;  var = sum_i (z_i - mean)^2 / H ;  rstd = 1 / sqrt(var + 1e-12)
  y    = keep_post s (gamma (z - mean) rstd + beta) out_scale
  y8, y8_scale = vk_quant_rows_fp8 of the UNROUNDED y: y8_scale = max_i |y_i| / 448 (1 for a zero row), y8 = e4m3(y / y8_scale)
Keep masks: element (row, c) takes word c & 3 of Philox-4x32-7(counter = (c >> 2, prow, site, 0)) (oracle.volta_ref.philox_u32), where
rows [0, split_row) belong to seg[0], the rest to seg[1], r' = row - segment start, prow = (r' / div) mul + r' % div + off (div == 0:
prow = r') and site = seg[].site.  A device row count `dyn` limits the rows to min(*dyn, M); rows past it are neither read nor written.
Backward, restated on ITS OWN inputs (dy, the stored bf16 z, the fp32 mean and rstd, gamma) so that it does not depend on the forward:
  xh = (z - mean) rstd ;  gy = keep_post s out_scale dy ;  gx = gy gamma ;  s1 = sum_i gx_i / H ;  s2 = sum_i gx_i xh_i / H
  dz = rstd (gx - s1 - xh s2) ;  dd = keep_pre s dz ;  dgamma_c = sum_rows gy xh ;  dbeta_c = sum_rows gy   (+ the prior value when
  accumulate bit 0 is set)

Rounding points of the kernels and their first-order bounds.  u = 2^-24 (fp32 unit roundoff).  A sum whose every term passes through at
most D fp32 adds has error <= D u sum|terms| (Higham, Accuracy and Stability, 4.2; the depths below are those of the kernels' trees: 4-wide
lanes, 64-lane butterfly, 16-row workgroups).  Divides, sqrtf and reciprocals are given one ulp = 2u each (correctly rounded or not).
 forward (ln_fwd_kernel):
  Ez    = u (pre |s d| + [x] |keep s d + x| + [addvec] |z|)                  the fp32 add chain of z, each link only where it exists
  Emean = mean_i Ez_i + Df u mean_i |z_i| + 2u |mean|                          H-term sum: Df = 3 (quad) + H/256 chunks + 6 (wave); the divide
  c_i   = z_i - mean ;  Ec_i = Ez_i + u |c_i|                                  the subtraction; Emean is a COMMON shift of every c_i:
  Evar  = mean_i 2 |c_i| Ec_i + Emean^2 + (Dq + 1) u var + 2u var              sum_i c_i = 0, so the shift enters var only as its square.
                                                                               Dq = 4 H/256 + 6 (sequential in the lane), + 1 for the square
  Erstd = rstd (Evar / (2 (var + eps)) + 6u)                                   the add of eps (and eps' own rounding), sqrtf, the reciprocal
  Exh_i = rstd (Ec_i + Emean) + |c_i| Erstd + u |xh_i|                         Emean rstd is the cancellation term (>= |mean| u rstd): what a
                                                                               row with a large mean and a small spread loses
  Eo_i  = |gamma_i| Exh_i + u |gamma_i xh_i| + u |o_i|                         the affine o = gamma xh + beta (fused or not)
  Ey_i  = keep s out_scale Eo_i + (post + 1) u |y_i|                           post-dropout scale, out_scale
  Esc   = max_i Ey_i / 448 + 2u y8_scale                                       |max|y^| - max|y|| <= max|y^ - y|; the divide
 backward (ln_bwd_kernel, ln_bwd_finalize_kernel):
  Egy   = (1 + post) u |gy| ;  Exh = 2u |xh| ;  Egx = |gamma| Egy + u |gx|
  Es1   = mean_i Egx_i + Db u mean_i |gx_i| + 2u |s1|                          Db = 4 H/256 + 6
  Ep_i  = |xh_i| Egx_i + |gx_i| Exh_i + u |gx_i xh_i|
  Es2   = mean_i Ep_i + Db u mean_i |gx_i xh_i| + 2u |s2|
  Ea_i  = Egx_i + Es1 + u |gx_i - s1| + |xh_i| Es2 + |s2| Exh_i + u |xh_i s2| + u |a_i|      a = gx - s1 - xh s2
  Edz_i = rstd Ea_i + u |dz_i| ;  Edd_i = keep s Edz_i + pre u |dd_i|
  Edgamma_c = sum_rows (|xh| Egy + |gy| Exh + u |gy xh|) + Dm u sum_rows |gy xh| (+ u |result| with accumulate bit 0)
  Edbeta_c  = sum_rows Egy + Dm u sum_rows |gy|                                 M-term column sums: Dm = 4 (rows of a wave) + 3 (waves) +
                                                                               ceil(records / 16) + 15 (finalize)
Every gate is G = 1.25 times its first-order bound (the neglected products of two relative errors are far below a quarter of it) plus
2^-126 (results flushed below the fp32 normal range) plus, for a bf16 output (y, the saved z, dz, dd), half a bf16 ulp of (|ref| + G E):
its own round to nearest even.  mean, rstd, y8_scale, dgamma and dbeta are fp32 outputs: G E alone.  The de-quantised y8 y8_scale lies
within (gate of y) + (half an e4m3 ulp at |y| / y8_scale) y8_scale: y^ / sc^ * sc^ is y^ to 4u, far inside the half bf16 ulp the gate of
y already carries.  Gates are elementwise functions of the case's data; there is no global tolerance.

Planted bugs (emulate_*(bug=...)) and the cases named for each (PLANTED): one_pass_var (offset rows: mean 64, spread 0.5),
eps_outside (spike rows whose variance is near or below eps), h_minus_1 (H = 768 and 2048: seen by rstd only), div_nch (H = 260, 516,
1284: a partly filled last chunk), bwd_no_out_scale (out_scale 0.5), bwd_no_post_mask (post-dropout), dd_no_scale (pre-dropout),
seg_not_rebased (split_row mid-tensor), seg_map_ignored (the single-stream seg tuples), finalize_drops_last, acc_overwrites (accumulate
bit 0), dyn_ignored (dyn < M)."""
import math
import os
import re
import zlib
from collections import namedtuple

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
G = 1.25
EPS = 1e-12
SEED = 0x9E3779B97F4A7C15                    # high 32 bits non-zero: the key's second word matters
MODES = {"none": (0.0, 0, 1.0), "pre": (0.1, 0, 1.0), "post": (0.1, 1, 1.0), "post05": (0.5, 1, 0.5)}     # p, post, out_scale
FWD_KEYS = ("y", "z", "mean", "rstd")
BWD_KEYS = ("dz", "dd", "dgamma", "dbeta")


def half_ulp_bf16(x):
    """Half a bf16 ulp at |x| (float64): the error bound of one round to nearest even; 2^-134 at 0."""
    _, e = torch.frexp(x.abs())
    e = torch.where(x == 0, torch.full_like(e, -125), e.clamp_min(-125))
    return torch.ldexp(torch.ones_like(x), e - 9)


def half_ulp_e4m3(x):
    """Half an OCP e4m3 ulp at |x| (float64): 3 mantissa bits, subnormal spacing 2^-9 below 2^-6."""
    _, e = torch.frexp(x.abs())
    e = torch.where(x == 0, torch.full_like(e, -5), e.clamp_min(-5))
    return torch.ldexp(torch.ones_like(x), e - 5)


# ------------------------------------------------------------------------------------------------ dispatch restated
def nch(H):
    return (H + 255) // 256


def fwd_template(H):
    """NCH of the ln_fwd_kernel instantiation vk_ln_fwd_pair launches for H."""
    n = nch(H)
    return n if n <= 4 else 8


def bwd_template(H):
    """NCH of the ln_bwd_kernel instantiation vk_ln_bwd_pair launches for H."""
    n = nch(H)
    return n if n <= 4 else 6 if n <= 6 else 8


def partial_rows(M):
    """vk_ln_bwd_partial_rows: one [2, H] record per 16-row workgroup."""
    return (M + 15) // 16


def parse_switches(path=None):
    """The `switch (nch)` statements of layernorm.hip: {"fwd": ({case: NCH}, default NCH), "bwd": ...}."""
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "volta_amd", "csrc", "layernorm.hip")
    src = open(path).read()
    out = {}
    for kind in ("fwd", "bwd"):
        cases, default = {}, None
        for line in src.splitlines():
            m = re.search(r"ln_%s_kernel<(\d+)>, grid" % kind, line)
            if not m:
                continue
            labels = re.findall(r"case (\d+):", line)
            for lab in labels:
                cases[int(lab)] = int(m.group(1))
            if "default:" in line:
                default = int(m.group(1))
        out[kind] = (cases, default)
    return out


# ------------------------------------------------------------------------------------------------ cases
Case = namedtuple("Case", "id M H mode profile split seg addvec x z dd dyn y8 acc")


def _c(M, H, mode="none", profile="randn", split=False, seg="rows", addvec=False, x=True, z="own", dd=True, dyn=None, y8=False, acc=0, name=None):
    tags = [mode, profile] + (["split"] if split else []) + ([seg] if seg != "rows" else []) + (["addvec"] if addvec else []) \
        + ([] if x else ["xnull"]) + (["z" + z] if z != "own" else []) + ([] if dd else ["ddnull"]) \
        + (["dyn%d" % dyn] if dyn is not None else []) + (["y8"] if y8 else []) + (["acc"] if acc else [])
    return Case(name or "M%d-H%d-%s" % (M, H, "-".join(tags)), M, H, mode, profile, split, seg, addvec, x, z, dd, dyn, y8, acc)


CASES = [
    # every H: each forward {1, 2, 3, 4, 8} and backward {1, 2, 3, 4, 6, 8} instantiation with a full and a partly filled last chunk
    _c(33, 4), _c(17, 64, "pre", split=True), _c(33, 252, "post", "offset"), _c(33, 256, "post05", "wide", split=True),
    _c(33, 260, "pre", "offset", addvec=True), _c(33, 512, "none", "wide"), _c(33, 516, "post", split=True, addvec=True),
    _c(33, 768, "pre", "wide", split=True), _c(33, 1000, "post05", "offset"), _c(33, 1024, "none", "offset", addvec=True),
    _c(33, 1284, "pre", split=True), _c(33, 1536, "post", "wide", split=True, addvec=True), _c(33, 1792, "post05", split=True),
    _c(33, 2048, "pre", "offset", split=True, addvec=True),
    # every M: one row, partly filled workgroups of 4 (forward) and 16 (backward) rows, one past them, many records
    _c(1, 768, "post", split=True), _c(3, 260, "pre", split=True), _c(4, 1536, "none", "wide"), _c(5, 516, "post05", "offset", split=True),
    _c(15, 1284, "post", split=True), _c(15, 2044, "pre", "wide", split=True), _c(16, 768, "pre", "wide", split=True), _c(17, 2048),
    _c(1000, 768, "pre", split=True),
    _c(1000, 1024, "post", "wide", split=True), _c(1000, 1536, "post05", "offset", split=True),
    _c(14592, 768, "pre", split=True),                       # the bench workload's text stream: 912 partial records
    # the engine's single-stream seg tuples (site, T, T + R, 0) / (site, R, T + R, T), T = 5, R = 3
    _c(33, 768, "post", split=True, seg="single"), _c(1000, 768, "pre", split=True, seg="single"),
    _c(17, 260, "post05", split=True, seg="single", addvec=True), _c(16, 1536, "post", seg="single_v", addvec=True, x=False),
    # optional pointers
    _c(33, 768, "pre", split=True, x=False), _c(33, 516, "post", z="null"), _c(33, 768, "pre", split=True, z="alias"),
    _c(17, 1284, "none", x=False, z="alias"), _c(33, 1024, "pre", split=True, dd=False), _c(15, 260, "post", dd=False),
    # device row counts: 0, 1, M - 1, M, M + 5
    _c(33, 768, "pre", split=True, dyn=0), _c(33, 768, "pre", split=True, dyn=1), _c(33, 768, "pre", split=True, dyn=32),
    _c(33, 768, "pre", split=True, dyn=33), _c(33, 768, "pre", split=True, dyn=38), _c(17, 516, "post", dyn=16),
    _c(1000, 1536, "none", dyn=517), _c(16, 260, "pre", dyn=0),
    # data profiles (offset and wide also run above)
    _c(33, 768, "none", "spike"), _c(17, 1284, "post", "spike", split=True), _c(33, 260, "post05", "spike"),
    # ill-conditioned on purpose (identical elements per row: var = 0, rstd = 1e6 amplifies the rounding of the mean into xh): only
    # finiteness and the gate of `mean` are asserted for this one case
    _c(33, 768, "none", "const", name="const-M33-H768"),
    # row-quantised e4m3 copy
    _c(33, 768, "none", y8=True), _c(17, 516, "post", "wide", split=True, y8=True), _c(1000, 1024, "pre", split=True, y8=True),
    _c(5, 1536, "post05", "offset", y8=True), _c(16, 256, "none", "spike", y8=True),
    # accumulate bit 0 onto a known dgamma / dbeta
    _c(33, 768, "pre", split=True, acc=1), _c(1000, 516, "post", acc=1), _c(17, 1536, "none", dyn=9, acc=1),
]
CASE = {c.id: c for c in CASES}
assert len(CASE) == len(CASES)

# bug -> (cases named for it, outputs of which at least one must miss its gate on every named case)
PLANTED = {
    "one_pass_var": (("M33-H252-post-offset", "M33-H2048-pre-offset-split-addvec", "M1000-H1536-post05-offset-split"), ("rstd", "y")),
    "eps_outside": (("M33-H768-none-spike", "M33-H260-post05-spike"), ("rstd", "y")),
    "h_minus_1": (("M33-H768-pre-wide-split", "M17-H2048-none-randn", "M33-H4-none-randn"), ("rstd",)),
    "div_nch": (("M33-H260-pre-offset-addvec", "M33-H516-post-randn-split-addvec", "M33-H1284-pre-randn-split", "M33-H4-none-randn"),
                ("mean", "rstd", "y", "dz")),
    "bwd_no_out_scale": (("M33-H256-post05-wide-split", "M1000-H1536-post05-offset-split"), ("dz", "dgamma", "dbeta")),
    "bwd_no_post_mask": (("M33-H252-post-offset", "M1-H768-post-randn-split", "M33-H1792-post05-randn-split"), ("dz", "dgamma", "dbeta")),
    "dd_no_scale": (("M17-H64-pre-randn-split", "M33-H1284-pre-randn-split"), ("dd",)),
    "seg_not_rebased": (("M33-H516-post-randn-split-addvec", "M16-H768-pre-wide-split", "M1000-H768-pre-randn-split"), ("y", "z", "dd", "dz")),
    "seg_map_ignored": (("M33-H768-post-randn-split-single", "M1000-H768-pre-randn-split-single", "M16-H1536-post-randn-single_v-addvec-xnull"),
                        ("y", "z", "dd", "dz")),
    "finalize_drops_last": (("M33-H768-pre-wide-split", "M1-H768-post-randn-split", "M1000-H1024-post-wide-split"), ("dgamma", "dbeta")),
    "acc_overwrites": (("M33-H768-pre-randn-split-acc", "M1000-H516-post-randn-acc", "M17-H1536-none-randn-dyn9-acc"), ("dgamma", "dbeta")),
    "dyn_ignored": (("M33-H768-pre-randn-split-dyn1", "M33-H768-pre-randn-split-dyn32", "M1000-H1536-none-randn-dyn517"), ("dgamma", "dbeta")),
}
BUGS = tuple(PLANTED)


def case_seed(case):
    return zlib.crc32(case.id.encode()) & 0xFFFFFF


def case_rows(case):
    """Rows the launch covers: min(*dyn, M)."""
    return case.M if case.dyn is None else min(case.dyn, case.M)


def case_segs(case):
    """(split_row, [(site, div, mul, off)] * 2) of a case."""
    split = (2 * case.M) // 3 if case.split else case.M
    if case.seg == "rows":
        return split, [(11, 0, 0, 0), (12, 0, 0, 0)]
    if case.seg == "single":
        return split, [(21, 5, 8, 0), (21, 3, 8, 5)]
    assert case.seg == "single_v" and not case.split
    return split, [(21, 3, 8, 5), (21, 0, 0, 0)]


def drop_rows(M, split, segs, bug=None):
    """(Philox row, site) of every row under the two-segment mapping of vk_ln_args.seg."""
    rows = np.arange(M, dtype=np.int64)
    si = rows >= split
    r = rows if bug == "seg_not_rebased" else np.where(si, rows - split, rows)
    prow, site = np.zeros(M, np.int64), np.zeros(M, np.int64)
    for k, (s, div, mul, off) in enumerate(segs):
        sel = si == bool(k)
        site[sel] = s
        prow[sel] = r[sel] if (div <= 0 or bug == "seg_map_ignored") else (r[sel] // div) * mul + r[sel] % div + off
    return prow, site


def keep_mask(M, H, p, split, segs, bug=None, seed=SEED):
    """Bool [M, H]: the kernels' keep decision, from oracle.volta_ref.philox_u32 under the restated row mapping."""
    from oracle import volta_ref as R
    prow, site = drop_rows(M, split, segs, bug)
    thr = np.uint32(min(int(p * 4294967296.0), 0xFFFFFFFF))
    keep = np.ones((M, H), bool)
    for s in np.unique(site):
        sel = site == s
        w = R.philox_u32(seed, int(s), int(prow[sel].max()) + 1, H)
        keep[sel] = w[prow[sel]] >= thr
    return torch.from_numpy(keep)


def make_inputs(case):
    """The tensors of a case, exactly as the kernels receive them: d, x, dy bf16 [M, H]; gamma, beta, addvec, dgamma0, dbeta0 fp32 [H]."""
    g = torch.Generator().manual_seed(case_seed(case))
    M, H = case.M, case.H
    p, post, out_scale = MODES[case.mode]
    sign = torch.where(torch.rand(M, 1, generator=g) < 0.5, -1.0, 1.0)
    scale_rows = torch.logspace(-3, 2, M)[torch.randperm(M, generator=g)][:, None] if M > 1 else torch.ones(1, 1)

    def profile(second):
        if case.profile == "randn":
            return torch.randn(M, H, generator=g)
        if case.profile == "offset":
            return sign * 64.0 + 0.5 * torch.randn(M, H, generator=g)
        if case.profile == "wide":
            return scale_rows * torch.randn(M, H, generator=g)
        if case.profile == "spike":             # amplitudes over 1e-6 .. 1e2: the small ones put var near and below eps
            t = torch.zeros(M, H)
            if not second:
                amp = sign[:, 0] * 10.0 ** (torch.rand(M, generator=g) * 8 - 6)
                t[torch.arange(M), torch.randint(0, H, (M,), generator=g)] = amp
            return t
        assert case.profile == "const"
        return (3.0 * torch.randn(M, 1, generator=g)).expand(M, H).contiguous()

    inp = dict(M=M, H=H, p=p, post=post, out_scale=out_scale, scale=float(np.float32(1.0 / (1.0 - p))) if p > 0 else 1.0)
    inp["d"] = profile(False).bfloat16()
    inp["x"] = profile(True).bfloat16() if case.x else None
    inp["gamma"] = 1 + 0.1 * torch.randn(H, generator=g)
    inp["beta"] = 0.1 * torch.randn(H, generator=g)
    inp["addvec"] = 0.5 * torch.randn(H, generator=g) if case.addvec else None
    inp["dy"] = torch.randn(M, H, generator=g).bfloat16()
    inp["dgamma0"], inp["dbeta0"] = torch.randn(H, generator=g), torch.randn(H, generator=g)
    inp["split"], inp["segs"] = case_segs(case)
    inp["keep"] = keep_mask(M, H, p, inp["split"], inp["segs"]) if p > 0 else None
    return inp


# ------------------------------------------------------------------------------------------------ float64 restatement and gates
def _gate16(ref, E):
    return G * E + half_ulp_bf16(ref.abs() + G * E) + TINY


def restate_fwd(inp, rows=None, y8=False):
    """Float64 forward on rows [0, rows) with the gates of the module docstring: y, z, mean, rstd (+ y8 = y, sc) and a 'g_' gate each."""
    M, H = inp["M"], inp["H"]
    n = M if rows is None else rows
    p, post, os_, s = inp["p"], inp["post"], inp["out_scale"], inp["scale"]
    pre_on, post_on = p > 0 and not post, p > 0 and bool(post)
    km = (inp["keep"][:n].double() * s) if p > 0 else torch.ones(n, H, dtype=torch.float64)
    one = torch.ones(n, H, dtype=torch.float64)
    dd = inp["d"][:n].double() * (km if pre_on else one)
    Ez = U * dd.abs() if pre_on else torch.zeros(n, H, dtype=torch.float64)
    z = dd
    if inp["x"] is not None:
        z = z + inp["x"][:n].double()
        Ez = Ez + U * z.abs()
    if inp["addvec"] is not None:
        z = z + inp["addvec"].double()
        Ez = Ez + U * z.abs()
    gamma, beta = inp["gamma"].double(), inp["beta"].double()
    Df, Dq = 3 + nch(H) + 6, 4 * nch(H) + 6
    mean = z.mean(-1, keepdim=True)
    Emean = Ez.mean(-1, keepdim=True) + Df * U * z.abs().mean(-1, keepdim=True) + 2 * U * mean.abs()
    c = z - mean
    Ec = Ez + U * c.abs()
    var = (c * c).mean(-1, keepdim=True)
    Evar = (2 * c.abs() * Ec).mean(-1, keepdim=True) + Emean ** 2 + (Dq + 3) * U * var
    rstd = 1.0 / torch.sqrt(var + EPS)
    Erstd = rstd * (Evar / (2 * (var + EPS)) + 6 * U)
    xh = c * rstd
    Exh = rstd * (Ec + Emean) + c.abs() * Erstd + U * xh.abs()
    o = gamma * xh + beta
    Eo = gamma.abs() * Exh + U * (gamma * xh).abs() + U * o.abs()
    kpost = km if post_on else one
    y = kpost * o * os_
    Ey = kpost * os_ * Eo + (2 if post_on else 1) * U * y.abs()
    out = dict(rows=n, z=z, g_z=_gate16(z, Ez), y=y, g_y=_gate16(y, Ey), mean=mean[:, 0], g_mean=(G * Emean + TINY)[:, 0],
               rstd=rstd[:, 0], g_rstd=(G * Erstd + TINY)[:, 0])
    if y8:
        amax = y.abs().amax(-1, keepdim=True) if n else torch.zeros(0, 1, dtype=torch.float64)
        sc = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
        Esc = (Ey.amax(-1, keepdim=True) if n else amax) / 448.0 + 2 * U * sc
        out.update(sc=sc[:, 0], g_sc=(G * Esc + TINY)[:, 0], y8=y, g_y8=out["g_y"] + half_ulp_e4m3(y / sc) * sc)
    return out


def backward_inputs(fwd):
    """The backward's own inputs, from the restatement alone: the stored bf16 z and the fp32 mean and rstd."""
    return fwd["z"].bfloat16(), fwd["mean"].float(), fwd["rstd"].float()


def restate_bwd(inp, zb, mean, rstd, rows=None, dd=True, acc=0):
    """Float64 backward on rows [0, rows) from dy, the stored bf16 z [M, H], fp32 mean / rstd [M] and gamma: dz, dd, dgamma, dbeta and
    their gates.  acc bit 0: dgamma / dbeta are added to inp['dgamma0'] / inp['dbeta0']."""
    M, H = inp["M"], inp["H"]
    n = M if rows is None else rows
    p, post, os_, s = inp["p"], inp["post"], inp["out_scale"], inp["scale"]
    pre_on, post_on = p > 0 and not post, p > 0 and bool(post)
    km = (inp["keep"][:n].double() * s) if p > 0 else torch.ones(n, H, dtype=torch.float64)
    one = torch.ones(n, H, dtype=torch.float64)
    gamma = inp["gamma"].double()
    mean, rstd = mean[:n].double()[:, None], rstd[:n].double()[:, None]
    Db = 4 * nch(H) + 6
    Dm = 4 + 3 + (partial_rows(M) + 15) // 16 + 15
    xh = (zb[:n].double() - mean) * rstd
    Exh = 2 * U * xh.abs()
    gy = inp["dy"][:n].double() * os_ * (km if post_on else one)
    Egy = (2 if post_on else 1) * U * gy.abs()
    gx = gy * gamma
    Egx = gamma.abs() * Egy + U * gx.abs()
    s1 = gx.mean(-1, keepdim=True)
    Es1 = Egx.mean(-1, keepdim=True) + Db * U * gx.abs().mean(-1, keepdim=True) + 2 * U * s1.abs()
    pr = gx * xh
    Ep = xh.abs() * Egx + gx.abs() * Exh + U * pr.abs()
    s2 = pr.mean(-1, keepdim=True)
    Es2 = Ep.mean(-1, keepdim=True) + Db * U * pr.abs().mean(-1, keepdim=True) + 2 * U * s2.abs()
    a = gx - s1 - xh * s2
    Ea = Egx + Es1 + U * (gx - s1).abs() + xh.abs() * Es2 + s2.abs() * Exh + U * (xh * s2).abs() + U * a.abs()
    dz = rstd * a
    Edz = rstd * Ea + U * dz.abs()
    out = dict(rows=n, dz=dz, g_dz=_gate16(dz, Edz))
    if dd:
        kpre = km if pre_on else one
        ddv = kpre * dz
        out.update(dd=ddv, g_dd=_gate16(ddv, kpre * Edz + (U * ddv.abs() if pre_on else 0.0)))
    q = gy * xh
    dg, Edg = q.sum(0), (xh.abs() * Egy + gy.abs() * Exh + U * q.abs()).sum(0) + Dm * U * q.abs().sum(0)
    db, Edb = gy.sum(0), Egy.sum(0) + Dm * U * gy.abs().sum(0)
    if acc & 1:
        dg, db = dg + inp["dgamma0"].double(), db + inp["dbeta0"].double()
        Edg, Edb = Edg + U * dg.abs(), Edb + U * db.abs()
    out.update(dgamma=dg, g_dgamma=G * Edg + TINY, dbeta=db, g_dbeta=G * Edb + TINY, E_dgamma=Edg, E_dbeta=Edb)
    return out


def ratio(got, ref, gate):
    """max over elements of |got - ref| / gate (inf where a NaN appears; 0 for an empty tensor)."""
    if ref.numel() == 0:
        return 0.0
    d = (got.double() - ref).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, math.inf), d)
    return float((d / gate).max())


def worst(got, ref, gate):
    """(ratio, flat index, got, ref, gate) at the worst element, for assertion messages."""
    if ref.numel() == 0:
        return 0.0, -1, 0.0, 0.0, 0.0
    d = (got.double() - ref).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, math.inf), d)
    rr = (d / gate).reshape(-1)
    i = int(rr.argmax())
    return float(rr[i]), i, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(gate.reshape(-1)[i])


def ratios(got, ref, keys):
    """{key: ratio} over the rows the reference covers; inf if `got` wrote a row past them or left one of them unwritten (NaN marks
    an unwritten element of the emulation's outputs)."""
    n, res = ref["rows"], {}
    for key in keys:
        if key not in ref or got.get(key) is None:
            continue
        if key in ("dgamma", "dbeta"):
            res[key] = ratio(got[key], ref[key], ref["g_" + key])
            continue
        r = ratio(got[key][:n], ref[key], ref["g_" + key])
        if not bool(torch.isnan(got[key][n:]).all()):
            r = math.inf
        res[key] = r
    return res


# ------------------------------------------------------------------------------------------------ fp32 / bf16 emulation of the kernels
F = np.float32


def _bf(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def _lanes(a, H):
    """[n, H] -> [n, chunks, 64 lanes, 4]: the kernels' element ownership (chunk j, lane l: columns j * 256 + 4 l .. + 3), zero past H."""
    n, k = a.shape[0], nch(H)
    out = np.zeros((n, k * 256), F)
    out[:, :H] = a
    return out.reshape(n, k, 64, 4)


def _wave_sum(v):
    """wave_sum's DPP tree over [n, 64] lane values: quads, half rows, rows, row pairs, the wave."""
    for _ in range(6):
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


def _f32(t):
    return None if t is None else t.float().numpy()


def _keep(inp, bug):
    if inp["p"] <= 0:
        return None
    if bug in ("seg_not_rebased", "seg_map_ignored"):
        return keep_mask(inp["M"], inp["H"], inp["p"], inp["split"], inp["segs"], bug).numpy()
    return inp["keep"].numpy()


def emulate_fwd(inp, rows=None, y8=False, bug=None):
    """ln_fwd_kernel in fp32 numpy: the add chain of z, the lane-then-wave sums of the two-pass statistics, the affine, the bf16 stores
    and the row-wise e4m3 copy.  Outputs are [M, ...] with NaN in rows the launch does not write.  `bug` plants one defect (BUGS)."""
    M, H = inp["M"], inp["H"]
    n = M if (rows is None or bug == "dyn_ignored") else rows
    p, post, os_, s = inp["p"], inp["post"], F(inp["out_scale"]), F(inp["scale"])
    keep = _keep(inp, bug)
    z = _f32(inp["d"])[:n]
    if p > 0 and not post:
        z = np.where(keep[:n], z * s, F(0))
    if inp["x"] is not None:
        z = z + _f32(inp["x"])[:n]
    if inp["addvec"] is not None:
        z = z + _f32(inp["addvec"])
    zl = _lanes(z, H)
    valid = _lanes(np.ones((n, H), F), H) > 0
    k = nch(H)
    Hdiv = F(fwd_template(H) * 256 if bug == "div_nch" else H)
    acc = np.zeros((n, 64), F)
    for j in range(k):
        acc = acc + (((zl[:, j, :, 0] + zl[:, j, :, 1]) + zl[:, j, :, 2]) + zl[:, j, :, 3])
    mean = _wave_sum(acc) / Hdiv
    sq = np.zeros((n, 64), F)
    for j in range(k):
        for r in range(4):
            t = zl[:, j, :, r] if bug == "one_pass_var" else np.where(valid[:, j, :, r], zl[:, j, :, r] - mean[:, None], F(0))
            sq = sq + t * t
    var = _wave_sum(sq) / (F(H - 1) if bug == "h_minus_1" else Hdiv)
    if bug == "one_pass_var":
        var = var - mean * mean
    rstd = F(1) / (np.sqrt(var) + F(EPS)) if bug == "eps_outside" else F(1) / np.sqrt(var + F(EPS))
    o = _f32(inp["gamma"]) * ((z - mean[:, None]) * rstd[:, None]) + _f32(inp["beta"])
    if p > 0 and post:
        o = np.where(keep[:n], o * s, F(0))
    o = (o * os_).astype(F)

    def full(a, shape):
        out = np.full(shape, np.nan, F)
        out[:n] = a
        return torch.from_numpy(out)
    out = dict(z=full(_bf(z), (M, H)), y=full(_bf(o), (M, H)), mean=full(mean, (M,)), rstd=full(rstd, (M,)))
    if y8:
        amax = np.abs(o).max(-1) if n else np.zeros(0, F)
        sc = np.where(amax > 0, amax / F(448), F(1)).astype(F)
        inv = (F(1) / sc).astype(F)
        q = torch.from_numpy(np.clip(o * inv[:, None], -448, 448).astype(F)).to(torch.float8_e4m3fn).float().numpy()
        out.update(sc=full(sc, (M,)), y8=full(q * sc[:, None], (M, H)))
    return out


def emulate_bwd(inp, zb, mean, rstd, rows=None, dd=True, acc=0, bug=None):
    """ln_bwd_kernel + ln_bwd_finalize_kernel in fp32 numpy: per row the sequential lane sums and wave sums of s1 / s2, per column the
    4 rows of a wave, the 4 waves of a 16-row workgroup (one partial record each) and the finalize's 16 strided sums."""
    M, H = inp["M"], inp["H"]
    n = M if (rows is None or bug == "dyn_ignored") else rows
    p, post, os_, s = inp["p"], inp["post"], F(inp["out_scale"]), F(inp["scale"])
    keep = _keep(inp, bug)
    k = nch(H)
    Hdiv = F(bwd_template(H) * 256 if bug == "div_nch" else H)
    mean, rstd = mean.numpy().astype(F)[:n, None], rstd.numpy().astype(F)[:n, None]
    gy = _f32(inp["dy"])[:n] * (F(1) if bug == "bwd_no_out_scale" else os_)
    if p > 0 and post and bug != "bwd_no_post_mask":
        gy = np.where(keep[:n], gy * s, F(0))
    xv = (_f32(zb)[:n] - mean) * rstd
    gx = gy * _f32(inp["gamma"])
    gxl, pl = _lanes(gx, H), _lanes(gx * xv, H)
    s1, s2 = np.zeros((n, 64), F), np.zeros((n, 64), F)
    for j in range(k):
        for r in range(4):
            s1 = s1 + gxl[:, j, :, r]
            s2 = s2 + pl[:, j, :, r]
    s1, s2 = (_wave_sum(s1) / Hdiv)[:, None], (_wave_sum(s2) / Hdiv)[:, None]
    o = (rstd * (gx - s1 - xv * s2)).astype(F)

    def full(a):
        out = np.full((M, H), np.nan, F)
        out[:n] = a
        return torch.from_numpy(out)
    out = dict(dz=full(_bf(o)), dd=None)
    if dd:
        if p > 0 and not post:
            o = np.where(keep[:n], o * (F(1) if bug == "dd_no_scale" else s), F(0))
        out["dd"] = full(_bf(o))
    nblk = partial_rows(M)
    res = []
    for q in (gy * xv, gy):
        t = np.zeros((nblk * 16, H), F)
        t[:n] = q
        t = t.reshape(nblk, 4, 4, H)                                   # [workgroup, row of the wave, wave, column]
        w = ((t[:, 0] + t[:, 1]) + t[:, 2]) + t[:, 3]
        rec = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]                 # one partial record per workgroup
        if bug == "finalize_drops_last":
            rec = rec[:-1]
        pad = np.zeros(((len(rec) + 15) // 16 * 16, H), F)
        pad[:len(rec)] = rec
        pad = pad.reshape(-1, 16, H)
        st = np.zeros((16, H), F)
        for i in range(pad.shape[0]):
            st = st + pad[i]
        tot = st[0]
        for i in range(1, 16):
            tot = tot + st[i]
        res.append(tot)
    if acc & 1 and bug != "acc_overwrites":
        res = [_f32(inp["dgamma0"]) + res[0], _f32(inp["dbeta0"]) + res[1]]
    out["dgamma"], out["dbeta"] = torch.from_numpy(res[0].astype(F)), torch.from_numpy(res[1].astype(F))
    return out
