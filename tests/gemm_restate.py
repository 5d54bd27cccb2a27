"""Float64 restatement of one vk_gemm_problem (csrc/gemm.hip, gemm256.hip, gemm4w.hip, gemm_common.h) with derived per-element error
bounds, the two input families of the GEMM kernel tests, guarded output buffers and the comparison.  CPU only (numpy + torch for bf16).

The reference.  The operands are taken as the kernel sees them: storage arrays [rows, ld] of bf16 values, the contraction length K, the
device count `dyn` (rows of C in NT / NN, rows of the contraction in TN), the previous contents of C and bias_grad for F32_ACC.  The
ragged-K contract of NT / NN (include/volta_hip.h: lda padded to a multiple of 64, the pad written as 0) is asserted, not assumed; the
contraction then runs over K columns in float64.

The bounds -- derived, none tuned.  Products of two bf16 values (8 significant bits each) are exact in fp32, so the only error of the
accumulator is that of summing Kc terms in fp32 in some order, bias included:
    mag   = |A| . |B| + |bias|  (+ |C_prev| for F32_ACC)           e_acc = (Kc + 4) * 2^-24 * mag
(Kc additions of relative error 2^-24 each against the running magnitude <= mag, and 4 more for bias, the previous C, a split
accumulation's second summation and the epilogue's own add; Kc is the contraction length after `dyn` in TN).
    F32, F32_ACC, bias_grad (mag = sum |A| (+ |bias_grad_prev|))    |out - ref| <= e_acc
    bf16 outputs: one round-to-nearest-even (pack2bf and f2bf both are; 8 significant bits, so half an ulp is 2^-8 relative)
                                                                    |out - f(ref)| <= e_f + 2^-8 * (|f(ref)| + e_f)
    BF16, RELU   e_f = e_acc                    ADDR   e_f = e_acc + |R| * 2^-24
    MULR         e_f = |R| * e_acc + |R * ref| * 2^-24
    GELU         e_f = 1.13 * e_acc + e_formula(u)         (max |gelu'| = 1.129)
    C2 (gelu')   e_f = 0.80 * e_acc + e_formula'(u)        (max |gelu''| = 2 phi(0) = 0.798)
e_formula is the error of the kernel's OWN erf polynomial (gelu_both in csrc/common.h: Abramowitz-Stegun 7.1.26 with exp2 and a
reciprocal) evaluated in fp32, against float64 erf.  gelu_both_f32() below restates that formula in numpy float32 and
measure_formula_error() measures it on a dense grid over [-12, 12] (tests/test_gemm_restate_cpu.py asserts the constants below still
cover the measurement): measured 4.64e-7 absolute = 1.77e-7 relative to max(|x|, 1) for the value, 2.98e-7 absolute for the derivative
(rounded up to 1.8e-7 and 3.0e-7 below).
The bounds use FOUR times the measured numbers -- the hardware's v_exp_f32 and v_rcp_f32 are 1-ulp approximations that numpy's correctly
rounded exp2 and division do not reproduce:
    e_formula(u) = 4 * 1.8e-7 * max(|u|, 1)          e_formula'(u) = 4 * 3.0e-7
That is a bound against the reference formula, never against a kernel's output.

The integer family makes "subtly wrong" visible at any magnitude: operands in [-4, 4], bias, R and the previous C in [-8, 8], all
integers.  Every product and every partial sum in any order is then an integer below 2^24 (asserted from mag), i.e. exact in fp32, so
the expected output is BITWISE the float64 result rounded once to bf16, or exactly the integer in fp32 (BF16, ADDR, MULR, RELU, F32,
F32_ACC, bias_grad).  The issue that asked for these tests names 256 terms as the family's limit; the condition that matters is
mag * 8 < 2^24, which holds up to the 352 terms of the K-depth cases (352 * 16 * 8 + 64 < 2^24) and is what the code asserts.  A zero
is compared without its sign (a sum of -0 products is +0 in the MFMA accumulator and may be -0 in numpy).  GELU stays on the Gaussian
family."""
import numpy as np
import torch

NT, NN, TN = 0, 1, 2
BF16, GELU, MULR, ADDR, F32, RELU, F32_ACC = range(7)
LAYOUT_NAMES = {NT: "NT", NN: "NN", TN: "TN"}
EPI_NAMES = {BF16: "BF16", GELU: "GELU", MULR: "MULR", ADDR: "ADDR", F32: "F32", RELU: "RELU", F32_ACC: "F32_ACC"}
F32_EPIS = (F32, F32_ACC)

U24, U8 = 2.0 ** -24, 2.0 ** -8
FORMULA_VALUE_REL_MEASURED = 1.8e-7     # |gelu_both_f32 - float64| / max(|x|, 1), dense grid over [-12, 12]
FORMULA_DERIV_ABS_MEASURED = 3.0e-7     # |gelu'_f32 - float64|
FORMULA_FACTOR = 4.0                    # margin for v_exp_f32 / v_rcp_f32 (1 ulp each), see the module docstring
GUARD = 256                             # sentinel elements in front of and behind every output buffer
EXTRA_ROWS = 3                          # sentinel rows behind row M - 1


# ---- number formats ----------------------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """float array -> uint16 bit patterns of the bf16 nearest to each value (round to nearest even, through fp32)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return r.astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def tensor_f64(t):
    """bf16 / fp32 torch tensor (any device) -> float64 numpy array of the same shape"""
    return t.detach().cpu().double().numpy()


def drop_zero_sign(bits, width):
    """bit patterns with -0 mapped to +0 (uint16 for bf16, uint32 for fp32)"""
    bits = np.array(bits)
    bits[bits == (0x8000 if width == 16 else 0x80000000)] = 0
    return bits


# ---- the kernel's GELU formula in numpy float32, and float64 GELU ------------------------------------------------------------------
def gelu_both_f32(x):
    """gelu_both of csrc/common.h, operation by operation, in numpy float32 (exp2 and the reciprocal correctly rounded)."""
    f = np.float32
    x = np.asarray(x, dtype=f)
    e = np.exp2((x * x) * f(-0.72134752044448170)).astype(f)
    t = (f(1.0) / (np.abs(x) * f(0.3275911 * 0.70710678118654752) + f(1.0))).astype(f)
    poly = ((((f(0.5 * 1.061405429) * t - f(0.5 * 1.453152027)) * t + f(0.5 * 1.421413741)) * t - f(0.5 * 0.284496736)) * t + f(0.5 * 0.254829592)) * t
    half_erf = (f(0.5) - poly * e).astype(f)
    cdf = f(0.5) + np.copysign(half_erf, x)
    return (x * cdf).astype(f), (x * f(0.39894228040143268) * e + cdf).astype(f)


def gelu64(u):
    """(gelu(u), gelu'(u)) in float64 with erf"""
    u = np.asarray(u, dtype=np.float64)
    cdf = 0.5 * (1.0 + torch.erf(torch.from_numpy(u / np.sqrt(2.0))).numpy())
    pdf = np.exp(-0.5 * u * u) / np.sqrt(2.0 * np.pi)
    return u * cdf, cdf + u * pdf


def measure_formula_error(points=2_400_001):
    """(max |value error| / max(|x|, 1), max |value error|, max |derivative error|) of gelu_both_f32 against float64 over [-12, 12]"""
    x = np.linspace(-12.0, 12.0, points).astype(np.float32)
    y, d = gelu_both_f32(x)
    y64, d64 = gelu64(x.astype(np.float64))
    ev = np.abs(y.astype(np.float64) - y64)
    return float((ev / np.maximum(np.abs(x), 1.0)).max()), float(ev.max()), float(np.abs(d.astype(np.float64) - d64).max())


def e_formula_value(u):
    return FORMULA_FACTOR * FORMULA_VALUE_REL_MEASURED * np.maximum(np.abs(u), 1.0)


def e_formula_deriv(u):
    return np.full_like(np.asarray(u, dtype=np.float64), FORMULA_FACTOR * FORMULA_DERIV_ABS_MEASURED)


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def contract(layout, M, N, K, A, B, dyn=None):
    """(acc, |A|.|B|, rows of C the launch writes, contraction length used, column sums of A and of |A| (TN) or None).
    A, B: float64 storage arrays [rows, ld] of the operands as the kernel sees them."""
    rows, Kc = M, K
    if dyn is not None:
        if layout == TN:
            Kc = min(int(dyn), K)
        else:
            rows = min(int(dyn), M)
    if layout != TN:
        pad_end = min(A.shape[1], (K + 63) // 64 * 64)
        assert not A[:M, K:pad_end].any(), "NT / NN with a ragged K: the pad columns of A up to the next multiple of 64 must be zero"
        a = A[:M, :K]
        b = B[:N, :K].T if layout == NT else B[:K, :N]
    else:
        a, b = A[:Kc, :M].T, B[:Kc, :N]
    acc, mag = a @ b, np.abs(a) @ np.abs(b)
    sums = (a.sum(axis=1), np.abs(a).sum(axis=1)) if layout == TN else None
    return acc, mag, rows, Kc, sums


def reference(layout, epi, M, N, K, A, B, bias=None, R=None, dyn=None, c_prev=None, bg_prev=None, want_bias_grad=False, parts=None):
    """Float64 value and error bound of every output element of one problem.
    A, B, R: float64 storage arrays [rows, ld]; bias: [>= N]; c_prev [M, N] and bg_prev [M]: previous contents (F32_ACC).
    `parts` may carry a cached contract() result.  Returns a dict: rows (of C written), Kc, C / C_bound [M, N], C2 / C2_bound (GELU),
    bias_grad / bias_grad_bound [M] (TN with want_bias_grad)."""
    acc, mag, rows, Kc, sums = parts if parts is not None else contract(layout, M, N, K, A, B, dyn)
    u, mag = acc.copy(), mag.copy()
    if bias is not None and epi != MULR:          # the MULR epilogue takes no bias (gemm_epilogue: has_bias)
        u += bias[:N]
        mag += np.abs(bias[:N])
    if epi == F32_ACC:
        u += c_prev
        mag += np.abs(c_prev)
    e_acc = (Kc + 4) * U24 * mag
    out = {"rows": rows, "Kc": Kc}
    r = R[:M, :N] if epi in (MULR, ADDR) else None
    if epi in F32_EPIS:
        out["C"], out["C_bound"] = u, e_acc
    else:
        if epi == BF16:
            f, e_f = u, e_acc
        elif epi == RELU:
            f, e_f = np.maximum(u, 0.0), e_acc
        elif epi == ADDR:
            f, e_f = u + r, e_acc + np.abs(r) * U24
        elif epi == MULR:
            f, e_f = u * r, np.abs(r) * e_acc + np.abs(r * u) * U24
        else:
            f, d = gelu64(u)
            e_f = 1.13 * e_acc + e_formula_value(u)
            e_d = 0.80 * e_acc + e_formula_deriv(u)
            out["C2"], out["C2_bound"] = d, e_d + U8 * (np.abs(d) + e_d)
        out["C"], out["C_bound"] = f, e_f + U8 * (np.abs(f) + e_f)
    if want_bias_grad:
        assert layout == TN
        s, smag = sums
        if epi == F32_ACC:
            s, smag = s + bg_prev, smag + np.abs(bg_prev)
        out["bias_grad"], out["bias_grad_bound"] = s, (Kc + 4) * U24 * smag
    out["mag_max"] = float(mag.max()) if mag.size else 0.0
    return out


# ---- guarded buffers --------------------------------------------------------------------------------------------------------------
def sentinel(n, dtype):
    """n elements of a position-dependent NaN pattern (a copy from a neighbouring element does not reproduce it)"""
    i = np.arange(n, dtype=np.int64)
    if dtype == torch.bfloat16:
        return torch.from_numpy((0x7FC0 | ((i * 7 + 3) & 0x3F)).astype(np.uint16).view(np.int16)).view(torch.bfloat16)
    return torch.from_numpy((0x7FC00000 | ((i * 2654435761) & 0x3FFFFF)).astype(np.uint32).view(np.int32)).view(torch.float32)


def raw_bits(t):
    """tensor -> numpy array of its bit patterns (uint16 for bf16, uint32 for fp32)"""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.view(torch.int32).numpy().view(np.uint32)


class Guarded:
    """An output of `rows` x `cols` elements at leading dimension `ld`, `col0` columns into a wider buffer, with GUARD sentinel elements
    in front and behind and EXTRA_ROWS sentinel rows below; `prev` (a [rows, cols] tensor) gives the written region its previous contents
    (F32_ACC), everything else is sentinel.  flat: the CPU master copy; view(t): the kernel's view of a (device) copy t of flat."""

    def __init__(self, rows, cols, ld, col0, dtype, prev=None):
        assert ld >= col0 + cols and (GUARD + col0) * (2 if dtype == torch.bfloat16 else 4) % 16 == 0
        self.rows, self.cols, self.ld, self.col0, self.dtype = rows, cols, ld, col0, dtype
        self.flat = sentinel(2 * GUARD + (rows + EXTRA_ROWS) * ld, dtype)
        if prev is not None:
            self.view(self.flat)[:rows, :cols] = prev.to(dtype)
        self.before = raw_bits(self.flat).copy()

    def view(self, flat):
        return flat[GUARD + self.col0:].as_strided((self.rows + EXTRA_ROWS, self.ld - self.col0), (self.ld, 1))

    def index(self, rows, c0, c1):
        """flat indices of the elements [0, rows) x [c0, c1)"""
        return (GUARD + self.col0 + np.arange(rows)[:, None] * self.ld + np.arange(c0, c1)[None, :]).reshape(-1)


class Worst:
    """worst |err| / bound and the count of bf16 elements that are not the exactly rounded float64 value, over many comparisons"""

    def __init__(self):
        self.ratio, self.inexact, self.bf16_elems = 0.0, 0, 0

    def merge(self, other):
        self.ratio = max(self.ratio, other.ratio)
        self.inexact += other.inexact
        self.bf16_elems += other.bf16_elems


def compare(name, g, got_flat, ref, bound, rows, exact, zero_cols=0, worst=None):
    """One Guarded output against its reference.  got_flat: the buffer after the launch.  Rows [0, rows) x columns [0, g.cols) must hold
    the reference (bitwise with exact=True, else within `bound`), columns [g.cols, zero_cols) of those rows exact zeros, and every other
    element of the buffer its bits from before the launch.  Returns a list of messages, empty when all holds."""
    msgs = []
    got = raw_bits(got_flat)
    touched = np.zeros(got.size, dtype=bool)
    idx = g.index(rows, 0, g.cols)
    touched[idx] = True
    if zero_cols > g.cols:
        zi = g.index(rows, g.cols, zero_cols)
        touched[zi] = True
        bad = np.flatnonzero(got[zi] != 0)
        if bad.size:
            msgs.append("%s: %d pad elements of columns [%d, %d) are not exact zeros" % (name, bad.size, g.cols, zero_cols))
    changed = np.flatnonzero((got != g.before) & ~touched)
    if changed.size:
        off = changed[0] - GUARD - g.col0
        msgs.append("%s: %d elements outside the output were written (first at flat %d: row %d, column %d)"
                    % (name, changed.size, changed[0], off // g.ld, off % g.ld))
    if rows == 0 or g.cols == 0:
        return msgs
    is16 = g.dtype == torch.bfloat16
    gb = got[idx].reshape(rows, g.cols)
    ref, bound = ref[:rows], bound[:rows]
    val = bf16_value(gb) if is16 else gb.view(np.float32).astype(np.float64)
    want_bits = bf16_bits(ref) if is16 else ref.astype(np.float32).view(np.uint32)
    width = 16 if is16 else 32
    if exact:
        bad = np.argwhere(drop_zero_sign(gb, width) != drop_zero_sign(want_bits, width))
        if bad.size:
            r_, c_ = bad[0]
            msgs.append("%s: %d of %d elements differ bitwise from the exact result (first at [%d, %d]: got %r, want %r)"
                        % (name, len(bad), gb.size, r_, c_, float(val[r_, c_]), float(ref[r_, c_])))
    else:
        err = np.abs(val - ref)
        with np.errstate(invalid="ignore"):
            bad = np.argwhere(~(err <= bound))         # a NaN output fails
        if bad.size:
            r_, c_ = bad[0]
            msgs.append("%s: %d of %d elements beyond their bound (first at [%d, %d]: got %r, want %r, bound %.3g)"
                        % (name, len(bad), gb.size, r_, c_, float(val[r_, c_]), float(ref[r_, c_]), float(bound[r_, c_])))
        if worst is not None:
            pos = bound > 0
            with np.errstate(invalid="ignore", divide="ignore"):
                if pos.any():
                    worst.ratio = max(worst.ratio, float(np.nanmax(np.where(pos, err / np.where(pos, bound, 1.0), 0.0))))
            if is16:
                worst.inexact += int((drop_zero_sign(gb, 16) != drop_zero_sign(want_bits, 16)).sum())
                worst.bf16_elems += gb.size
    return msgs


# ---- cases: inputs, buffers, reference and check of one problem -------------------------------------------------------------------
def _up(x, m):
    return (x + m - 1) // m * m


class Case:
    """One problem with everything a launch and its check need, built on the CPU from a seed.
    family "gauss": A ~ N(0, 1), B ~ N(0, 1 / K) (u = acc + bias is of order 1: the curved part of GELU), bias, R, previous C ~ N(0, 1);
    family "int": the integer family of the module docstring.
    NT / NN: A is [M, lda], lda = K rounded up to 64 with zero pad columns (`lda` may name a larger one); NT's B is [N, K rounded up
    to 8] -- NOT padded to 64: the kernel's K-steps run into the next row there and meet A's zeros --, NN's [K, N rounded up to 8, + 8];
    TN: A [K, M up to 8], B [K, N up to 8].  Pad columns of B (and of TN's A) hold 1.0: finite, as the contract allows.
    C sits `col0` = 8 columns into a buffer of leading dimension ldc; ldr = ldc + ldr_extra; dyn: device count or None."""

    def __init__(self, layout, epi, M, N, K, family, seed, ldc=None, ldr_extra=0, n_store=0, dyn=None, bias_grad=False, with_bias=True,
                 lda=None, c8=8):
        assert family in ("gauss", "int") and not (family == "int" and epi == GELU)
        self.layout, self.epi, self.M, self.N, self.K, self.family = layout, epi, M, N, K, family
        self.dyn, self.n_store, self.bias_grad = dyn, n_store, bias_grad
        g = torch.Generator().manual_seed(seed)
        integer = family == "int"

        def draw(shape, lim, scale=1.0):
            if integer:
                return torch.randint(-lim, lim + 1, shape, generator=g).float()
            return torch.randn(shape, generator=g) * scale

        bscale = 1.0 / max(K, 1) ** 0.5
        if layout == TN:
            self.lda, self.ldb = _up(M, 8), _up(N, 8)
            A, B = torch.ones(K, self.lda), torch.ones(K, self.ldb)
            A[:, :M], B[:, :N] = draw((K, M), 4), draw((K, N), 4, bscale)
        else:
            self.lda = lda if lda is not None else _up(K, 64)
            A = torch.zeros(M, self.lda)
            A[:, :K] = draw((M, K), 4)
            if layout == NT:
                self.ldb = _up(K, 8)
                B = torch.ones(N, self.ldb)
                B[:, :K] = draw((N, K), 4, bscale)
            else:
                self.ldb = _up(N, 8) + 8
                B = torch.ones(K, self.ldb)
                B[:, :N] = draw((K, N), 4, bscale)
        self.A, self.B = A.to(torch.bfloat16), B.to(torch.bfloat16)
        self.bias = draw((N,), 8) if (with_bias and epi not in (MULR, F32_ACC)) else None
        f32 = epi in F32_EPIS
        out_dtype = torch.float32 if f32 else torch.bfloat16
        ncols = max(N, n_store)
        self.ldc = ldc if ldc is not None else _up(ncols, 4) + 12
        assert self.ldc >= c8 + ncols
        self.R = None
        self.ldr = 0
        if epi in (MULR, ADDR):
            self.ldr = self.ldc + ldr_extra
            self.R = draw((M, self.ldr), 8).to(torch.bfloat16)
        c_prev = draw((M, N), 8) if epi == F32_ACC else None
        bg_prev = draw((M,), 8) if (epi == F32_ACC and bias_grad) else None
        self.c_prev = tensor_f64(c_prev) if c_prev is not None else None
        self.bg_prev = tensor_f64(bg_prev) if bg_prev is not None else None
        self.out = {"C": Guarded(M, N, self.ldc, c8, out_dtype, prev=c_prev)}
        if epi == GELU:
            self.out["C2"] = Guarded(M, N, self.ldc, c8, out_dtype)
        if bias_grad:
            self.out["bias_grad"] = Guarded(1, M, M, 0, torch.float32, prev=bg_prev.view(1, M) if bg_prev is not None else None)
        self._A64, self._B64 = tensor_f64(self.A), tensor_f64(self.B)
        self._R64 = tensor_f64(self.R) if self.R is not None else None
        self._bias64 = tensor_f64(self.bias) if self.bias is not None else None
        self._parts = None
        self._ref = {}

    def ident(self):
        return "%s %s %dx%dx%d %s dyn=%s" % (LAYOUT_NAMES[self.layout], EPI_NAMES[self.epi], self.M, self.N, self.K, self.family, self.dyn)

    def ref(self, passes=1):
        """the reference after `passes` launches in a row (F32_ACC accumulates; the bounds of the passes add)"""
        if passes in self._ref:
            return self._ref[passes]
        if self._parts is None:
            self._parts = contract(self.layout, self.M, self.N, self.K, self._A64, self._B64, self.dyn)
        c_prev, bg_prev, carried, carried_bg = self.c_prev, self.bg_prev, 0.0, 0.0
        for _ in range(passes):
            r = reference(self.layout, self.epi, self.M, self.N, self.K, self._A64, self._B64, self._bias64, self._R64, self.dyn,
                          c_prev, bg_prev, self.bias_grad, parts=self._parts)
            r["C_bound"] = r["C_bound"] + carried
            c_prev, carried = r["C"], r["C_bound"]
            if self.bias_grad:
                r["bias_grad_bound"] = r["bias_grad_bound"] + carried_bg
                bg_prev, carried_bg = r["bias_grad"], r["bias_grad_bound"]
        if self.family == "int":
            assert r["mag_max"] * 8 * passes + 64 < 2 ** 24, "integer family: partial sums must stay exact in fp32"
        self._ref[passes] = r
        return r

    def check(self, got, passes=1, worst=None):
        """got: {"C": flat buffer after the launch(es), "C2": ..., "bias_grad": ...}.  Returns the list of failures."""
        r = self.ref(passes)
        exact = self.family == "int"
        zero_cols = self.n_store if self.epi == F32 else 0
        msgs = compare("C", self.out["C"], got["C"], r["C"], r["C_bound"], r["rows"], exact, zero_cols, worst)
        if self.epi == GELU:
            msgs += compare("C2", self.out["C2"], got["C2"], r["C2"], r["C2_bound"], r["rows"], False, 0, worst)
        if self.bias_grad:
            msgs += compare("bias_grad", self.out["bias_grad"], got["bias_grad"], r["bias_grad"].reshape(1, -1),
                            r["bias_grad_bound"].reshape(1, -1), 1, exact, 0, worst)
        return ["%s: %s" % (self.ident(), m) for m in msgs]
