"""Float64 restatement of the LoRA entry points (include/volta_hip.h: vk_lora_fwd / vk_lora_bwd, csrc/lora.hip) with derived bounds, the two
input families of the kernel tests and sentinel buffers.  CPU only (numpy).

The contract, per problem (X [M, K], A [r, K], B [N, r] bf16; s = the problem's scale as fp32):
    T   = bf16(sum_k X[m,k] A[j,k])
    Y   = bf16(Y + s sum_j T[m,j] B[n,j])                 reads the stored T
    dT  = bf16(s sum_n dY[m,n] B[n,j])
    dB  = s sum_m dY[m,n] T[m,j]      (fp32)              summed over every problem that names the same dB, + the previous dB with `accumulate`
    dA  = sum_m dT[m,j] X[m,k]        (fp32)              reads the stored dT
    dX  = bf16(dX + sum_c sum_j dT_c[m,j] A_c[j,k])       over the problems c that name the same dX

The bounds -- derived, none tuned.  A product of two bf16 values is exact in fp32, so an fp32 accumulator differs from the float64 sum only
by the roundings of Kc additions in some order, each relative 2^-24 against a running magnitude <= mag = sum |a||b| (+ |previous value|):
    e_acc = (Kc + 4) * 2^-24 * mag
The 4 covers what is not a term of the sum: the multiplication by s, the add of the previous value, the second level of a blocked or
lane-wise summation, and one spare.  Kc is K for T, r for Y, N for dT, the rows of all sources for dA / dB, r times the number of adapters
for dX.  fp32 outputs: |out - ref| <= e_acc.  bf16 outputs take one round-to-nearest-even (8 significant bits: half an ulp is 2^-8 relative):
    |out - ref| <= e_acc + 2^-8 * (|ref| + e_acc)
Each stage is checked on its own: the restatement of Y and dX, and of dA, starts from the bits of T / dT that the kernel itself stored, so no
bound has to carry a neighbouring stage's rounding flip.

The integer family makes a wrong index visible at any magnitude.  Every operand is a small integer and sparse enough that T, dT and the
updated Y / dX stay integers of magnitude <= 256 (exact in bf16) and every partial sum is an integer below 2^24 (exact in fp32, in any
order): X and dY have four entries of +-1 per row, A two entries of +-1 per column, B four entries from {-1, 1, 2} per row (an asymmetric
set: a transposed or sign-flipped B changes the result), previous Y / dX values lie in [-8, 8], s = 2.  Then |T| <= 4, |s T B^T| <= 64,
|dT| <= 16, |sum_c dT_c A_c| <= 3 * 32, and the expected outputs are BITWISE the float64 results (a zero compared without its sign)."""
import numpy as np

U24, U8 = 2.0 ** -24, 2.0 ** -8
GUARD = 256            # sentinel elements in front of and behind every buffer
EXTRA_ROWS = 3         # sentinel rows behind row M - 1


# ---- number formats
def bf16_bits(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def drop_zero_sign(bits, width):
    bits = np.array(bits)
    bits[bits == (0x8000 if width == 16 else 0x80000000)] = 0
    return bits


def sentinels16(n, start=0):
    """position-dependent bf16 NaNs"""
    i = np.arange(start, start + n, dtype=np.uint64)
    return (0x7F81 + (i % 125)).astype(np.uint16)


def sentinels32(n, start=0):
    """position-dependent fp32 NaNs"""
    i = np.arange(start, start + n, dtype=np.uint64)
    return (0x7FC00001 + (i % 65521)).astype(np.uint32)


# ---- the reference: every function returns (ref, e_acc) in float64
def e_acc(kc, mag):
    return (kc + 4) * U24 * mag


def bound_bf16(ref, e):
    return e + U8 * (np.abs(ref) + e)


def ref_T(X, A):
    """X [M, K], A [r, K] -> T before rounding [M, r]"""
    return X @ A.T, e_acc(X.shape[1], np.abs(X) @ np.abs(A).T)


def ref_Y(Yprev, T, B, s):
    """T: the VALUES of the stored bf16 T [M, r]; B [N, r]"""
    s = float(np.float32(s))
    return Yprev + s * (T @ B.T), e_acc(B.shape[1], np.abs(Yprev) + s * (np.abs(T) @ np.abs(B).T))


def ref_dT(dY, B, s):
    s = float(np.float32(s))
    return s * (dY @ B), e_acc(B.shape[0], s * (np.abs(dY) @ np.abs(B)))


def ref_dB(sources, prev=None):
    """sources: [(dY [M, N], T values [M, r], s)] of every problem that names this dB, in list order; prev: previous contents or None"""
    ref = sum(float(np.float32(s)) * (dY.T @ T) for dY, T, s in sources)
    mag = sum(float(np.float32(s)) * (np.abs(dY).T @ np.abs(T)) for dY, T, s in sources)
    if prev is not None:
        ref, mag = ref + prev, mag + np.abs(prev)
    return ref, e_acc(sum(dY.shape[0] for dY, _, _ in sources), mag)


def ref_dA(sources, prev=None):
    """sources: [(dT values [M, r], X [M, K])]"""
    ref = sum(dT.T @ X for dT, X in sources)
    mag = sum(np.abs(dT).T @ np.abs(X) for dT, X in sources)
    if prev is not None:
        ref, mag = ref + prev, mag + np.abs(prev)
    return ref, e_acc(sum(X.shape[0] for _, X in sources), mag)


def ref_dX(dXprev, members):
    """members: [(dT values [M, r], A [r, K])] of the problems that name this dX"""
    ref = dXprev + sum(dT @ A for dT, A in members)
    mag = np.abs(dXprev) + sum(np.abs(dT) @ np.abs(A) for dT, A in members)
    return ref, e_acc(sum(A.shape[0] for _, A in members), mag)


# ---- comparisons: the worst ratio |out - ref| / bound (<= 1 passes), computed where the bound is positive and exact equality elsewhere
def worst_bf16(out_bits, ref, e):
    out = bf16_value(out_bits)
    assert np.isfinite(out).all(), "non-finite output"
    return _ratio(np.abs(out - ref), bound_bf16(ref, e))


def worst_f32(out, ref, e):
    out = np.asarray(out, dtype=np.float64)
    assert np.isfinite(out).all(), "non-finite output"
    return _ratio(np.abs(out - ref), e)


def _ratio(err, bound):
    zero = bound == 0
    assert (err[zero] == 0).all(), "a value whose bound is zero differs"
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


def exact_bf16(out_bits, ref):
    """the integer family: bitwise the float64 result"""
    want = bf16_bits(ref)
    assert (bf16_value(want) == ref).all(), "the expected value is not representable in bf16: the family's premise is broken"
    return np.array_equal(drop_zero_sign(out_bits, 16), drop_zero_sign(want, 16))


def exact_f32(out, ref):
    assert (np.abs(ref) < 2 ** 24).all() and (ref == np.round(ref)).all(), "not an integer below 2^24: the family's premise is broken"
    return np.array_equal(np.asarray(out, dtype=np.float64), ref)


# ---- input families
def _sparse_rows(rng, rows, cols, per_row, values):
    out = np.zeros((rows, cols))
    for i in range(rows):
        idx = rng.choice(cols, size=min(per_row, cols), replace=False)
        out[i, idx] = rng.choice(values, size=len(idx))
    return out


def family(kind, rng, M, K, N, r):
    """One problem's operands as float64 arrays of bf16-representable values: X, A, B, dY, Yprev, dXprev; and its scale."""
    if kind == "gauss":
        q = lambda a: bf16_value(bf16_bits(a))
        return dict(X=q(rng.standard_normal((M, K))), A=q(rng.uniform(-1, 1, (r, K)) / np.sqrt(K)), B=q(rng.standard_normal((N, r)) * 0.05),
                    dY=q(rng.standard_normal((M, N)) * 0.01), Yprev=q(rng.standard_normal((M, N))), dXprev=q(rng.standard_normal((M, K)) * 0.01),
                    s=2.0)
    assert kind == "int"
    return dict(X=_sparse_rows(rng, M, K, 4, [-1.0, 1.0]), A=_sparse_rows(rng, K, r, 2, [-1.0, 1.0]).T.copy(),
                B=_sparse_rows(rng, N, r, 4, [-1.0, 1.0, 2.0]), dY=_sparse_rows(rng, M, N, 4, [-1.0, 1.0]),
                Yprev=rng.integers(-8, 9, (M, N)).astype(np.float64), dXprev=rng.integers(-8, 9, (M, K)).astype(np.float64), s=2.0)
