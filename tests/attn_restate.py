"""float64 restatement of volta's BertGatedSelfAttention core (volta/encoders.py:258-340) for tests/test_attention_*.py, with elementwise
error gates derived from the rounding points the kernels (csrc/attention.hip, csrc/attention_generic.hip) actually have, an fp32/bf16
emulation of the MFMA kernels' arithmetic (to show the gates are not too tight, and -- with planted bugs -- not too loose), and the case
table that the GPU test runs.

Contract restated (one launch, gate[mq][mk] enables block (query modality mq, key modality mk)):
  s   = Q_mq K^T / sqrt(dh) + mask            over the JOINT key set [text keys | vision keys] that mq attends (enabled blocks only)
  lse = logsumexp_j s ;  P = exp(s - lse)      (the forward saves lse per query row, (b * nh + h) * Lq + q)
  P~  = P * keep / (1 - p)                     keep of element (query row, key) of block (mq, mk): word key & 3 of
                                               Philox-4x32-7(counter = (key >> 2, drow, site[mq][mk], 0)), drow = (b * nh + h) * Lq + q
  ctx = sum over blocks of P~ V
  dP = dO V^T ;  delta = sum_j P~ dP = dO . ctx ;  dS = P (keep/(1-p) dP - delta)
  dV = P~^T dO ;  dK = dS^T Q / sqrt(dh) ;  dQ = dS K / sqrt(dh)      (dK, dV summed over the query modalities that attend mk)

Gates.  u = 2^-24 (fp32 unit roundoff), ub = 2^-8 (bf16 unit roundoff: P, dS and P~ are rounded to bf16 before the MFMAs),
gamma2(n) = 2nu / (1 - 2nu): the error of an fp32 sum of n products of bf16 values (exact in fp32) under ANY summation tree, with each
add allowed 2u instead of u so that an MFMA whose internal adds truncate is covered too (Higham, Accuracy and Stability, 4.2).  Per
element (query row i, key j of the joint set, n keys):
  Es_ij  = (gamma2(dh) + 3u) scale (|q_i|.|k_j|) + u |s_ij|
           the fp32 score: the QK^T MFMA / fp32 dot (gamma2), the fp32 constant scale, q * scale (generic) or acc * scale (MFMA), and
           the rounding of s * scale + mask (attention.hip:218, :409, :475; attention_generic.hip `g_dot(..) + mask`).  The last term is
           NOT negligible: at mask = -10000 one fp32 rounding is up to 4.9e-4.
  Eexp_ij = (2 |s_ij - lse_i| + 4) u           __expf(x) = exp2(x log2 e): the product rounds (u |x|), log2 e rounds (u |x|), v_exp_f32 is
                                               good to one ulp (2u).  |s - max| <= |s - lse|, so the one form covers forward and backward.
  r_i    = sum_j P_ij (Es_ij + Eexp_ij)        a common shift of the scores (the row max) cancels in P; what remains is each term's own
                                               error against the weighted mean of all of them
  RP_ij  = Es_ij + Eexp_ij + r_i + gamma2(n) + 4u     relative error of the forward's fp32 P~ (sum of n exps, 1/sum, * inv, * 1/(1-p)
                                               whose fp32 constant is off by u)
  EP_ij  = P~_ij RP_ij + 2^-126                absolute; the floor covers exp results flushed to zero below the fp32 normal range
  Else_i = r_i + gamma2(n) + 4u log(n) + 8u + u |lse_i|     lse = m + log(sum): log(sum) <= log n, __logf good to a few ulp, final add
  Ectx   = EP @ |V| + (ub + gamma2(n)) (P~ @ |V|)     P~ rounded to bf16 before the PV MFMA (attention.hip:259), fp32 accumulation.
           The generic kernels keep P in fp32 and sit inside the same gate.
Backward (the kernels recompute P from the SAVED lse, attention.hip:409/:475, attention_generic.hip `__expf(sc - lse)`):
  RPb_ij = Es_ij + Eexp_ij + G Else_i + 4u    the kernel's lse lies within its own gate G Else
  Edp_ij = gamma2(dh) (|dO_i|.|v_j|)
  Edelta_i = |dO_i|.Gctx_i + gamma2(dh) (|dO_i|.|ctx_i|) + sum_j P~_ij (RPb_ij |dP_ij| + Edp_ij) + gamma2(n) sum_j P~_ij |dP_ij|
           delta from the STORED bf16 ctx (delta_rows, attention.hip:74; generic phase 2), whose error is its gate Gctx; or (generic
           phase 1) the fp32 sum of P~ dP.  The sum of both forms bounds either.
  EdS0_ij = P_ij RPb_ij |keep dP_ij - delta_i| + P_ij (keep Edp_ij + Edelta_i) + 4u P_ij (keep |dP_ij| + |delta_i|)
  EdS_ij  = EdS0_ij + ub (|dS_ij| + EdS0_ij)   dS rounded to bf16 before the dK / dQ MFMAs (attention.hip:416, :482)
  EdQ   = scale (EdS @ |K| + gamma2(n) |dS| @ |K|) + u |dQ|           final * scale (attention.hip:495)
  EdK   = scale (EdS^T @ |Q| + gamma2(nq) |dS|^T @ |Q|) + u |dK|      summed over the attending query modalities (nq queries)
  EdV   = (P~ (RPb + ub) + 2^-126)^T @ |dO| + gamma2(nq) P~^T @ |dO|  P~ rounded to bf16 before the dV MFMA (attention.hip:416)
Every gate is G = 1.25 times its first-order bound -- the neglected products of two relative errors are below 1e-2 of the bound, since
every relative term above is at most ~ub -- plus, for a bf16 output, half a bf16 ulp of (|ref| + G E): its own round to nearest even
(the final bf16 store).  lse and probs are fp32 outputs: G E alone.  Gates are elementwise; there is no global scale."""
import math
from collections import namedtuple

import numpy as np
import torch

U = 2.0 ** -24
UB = 2.0 ** -8
TINY = 2.0 ** -126
G = 1.25
LDS_LIMIT = 160 * 1024

GATES = {"tt": [[1, 0], [0, 0]], "tt+vv": [[1, 0], [0, 1]], "tv+vt": [[0, 1], [1, 0]], "all": [[1, 1], [1, 1]],
         "tt+tv": [[1, 1], [0, 0]]}
SITES = [[11, 12], [21, 22]]                 # distinct Philox site per block
SEED = 0x9E3779B97F4A7C15                    # high 32 bits non-zero: the key's second word matters
DISTS = {"uniform": 0.25, "mid": 1.5, "peaked": 3.0}   # std of q and k entries; score std = its square (0.06, 2.25, 9: max ~ +-30)


def gamma2(n):
    return 2 * n * U / (1 - 2 * n * U)


def half_ulp_bf16(x):
    """Half a bf16 ulp at |x| (float64): the error bound of one round to nearest even; 2^-134 at 0."""
    _, e = torch.frexp(x.abs())
    e = torch.where(x == 0, torch.full_like(e, -125), e.clamp_min(-125))
    return torch.ldexp(torch.ones_like(x), e - 9)


# ------------------------------------------------------------------------------------------------ inputs
def lengths(B, L, g):
    """Per batch element: full, 1, ragged, none (every key masked), cycled."""
    out = []
    for b in range(B):
        k = b % 4
        out.append(L if k == 0 else 1 if k == 1 else int(torch.randint(1, L + 1, (1,), generator=g)) if k == 2 else 0)
    return torch.tensor(out)


def make_inputs(B, nh, dh, T, R, dist="mid", seed=0):
    """bf16 rows [B*L, H] of Q, K, V, dO per modality, fp32 additive masks [B, L] (0 / -10000)."""
    g = torch.Generator().manual_seed(seed)
    H, Ls, sd = nh * dh, [T, R], DISTS[dist]
    inp = dict(B=B, nh=nh, dh=dh, L=Ls, dist=dist, q=[], k=[], v=[], do=[], mask=[], lens=[])
    for m in range(2):
        n = B * Ls[m]
        inp["q"].append((torch.randn(n, H, generator=g) * sd).bfloat16())
        inp["k"].append((torch.randn(n, H, generator=g) * sd).bfloat16())
        inp["v"].append((torch.randn(n, H, generator=g) * 1.5).bfloat16())
        inp["do"].append(torch.randn(n, H, generator=g).bfloat16())
        lens = lengths(B, Ls[m], g)
        inp["lens"].append(lens)
        inp["mask"].append(((torch.arange(Ls[m])[None] >= lens[:, None]).float() * -10000.0).contiguous())
    return inp


def heads(t, B, L, nh, dh, dtype=torch.float64):
    """[B*L, H] rows -> [B, nh, L, dh]."""
    return t.to(dtype).reshape(B, L, nh, dh).transpose(1, 2)


def rows(t):
    """[B, nh, L, dh] -> [B*L, H]."""
    B, nh, L, dh = t.shape
    return t.transpose(1, 2).reshape(B * L, nh * dh)


def keep_mask(seed, site, B, nh, Lq, Lk, p, row_shift=0):
    """Bool [B, nh, Lq, Lk]: the kernels' keep decision (oracle.volta_ref.philox_keep_mask's stream), optionally with every drow shifted."""
    from oracle import volta_ref as R
    n = B * nh * Lq
    w = R.philox_u32(seed, site, n + row_shift, Lk)[row_shift:]
    thr = np.uint32(min(int(p * 4294967296.0), 0xFFFFFFFF))
    return torch.from_numpy(np.ascontiguousarray(w >= thr)).view(B, nh, Lq, Lk)


def keeps(inp, gate, p, seed=SEED, sites=SITES):
    B, nh, Ls = inp["B"], inp["nh"], inp["L"]
    return [[keep_mask(seed, sites[i][j], B, nh, Ls[i], Ls[j], p) if (p > 0 and gate[i][j]) else None for j in range(2)] for i in range(2)]


def blocks(gate, mq):
    return [mk for mk in range(2) if gate[mq][mk]]


# ------------------------------------------------------------------------------------------------ float64 restatement and gates
def restate(inp, gate, p, keep=None):
    """Closed-form float64 forward and backward on the bf16-rounded inputs, with the gates of the module docstring.
    Returns dict: ctx/lse/dq/dk/dv[m] (rows layout [B*L, H] / [B*nh*L]) and probs[mq][mk] [B, nh, Lq, Lk], each with a 'g_' gate."""
    B, nh, dh, Ls = inp["B"], inp["nh"], inp["dh"], inp["L"]
    scale = 1.0 / math.sqrt(dh)
    keep = keep if keep is not None else keeps(inp, gate, p)
    q = [heads(inp["q"][m], B, Ls[m], nh, dh) for m in range(2)]
    k = [heads(inp["k"][m], B, Ls[m], nh, dh) for m in range(2)]
    v = [heads(inp["v"][m], B, Ls[m], nh, dh) for m in range(2)]
    do = [heads(inp["do"][m], B, Ls[m], nh, dh) for m in range(2)]
    mask = [inp["mask"][m].double() for m in range(2)]
    out = {key: [None, None] for key in ("ctx", "lse", "dq", "dk", "dv", "g_ctx", "g_lse", "g_dq", "g_dk", "g_dv")}
    out["probs"], out["g_probs"] = [[None, None], [None, None]], [[None, None], [None, None]]
    dk = [torch.zeros_like(k[m]) for m in range(2)]
    dv = [torch.zeros_like(v[m]) for m in range(2)]
    edk = [torch.zeros_like(k[m]) for m in range(2)]
    edv = [torch.zeros_like(v[m]) for m in range(2)]
    adk = [torch.zeros_like(k[m]) for m in range(2)]
    adv = [torch.zeros_like(v[m]) for m in range(2)]
    nq = [sum(Ls[mq] for mq in range(2) if gate[mq][mk]) for mk in range(2)]
    for mq in range(2):
        bl = blocks(gate, mq)
        if not bl:
            continue
        K = torch.cat([k[mk] for mk in bl], 2)
        V = torch.cat([v[mk] for mk in bl], 2)
        M = torch.cat([mask[mk][:, None, None, :].expand(B, 1, 1, Ls[mk]) for mk in bl], 3)
        KP = torch.cat([(keep[mq][mk].double() / (1 - p)) if keep[mq][mk] is not None else torch.ones(B, nh, Ls[mq], Ls[mk], dtype=torch.float64)
                        for mk in bl], 3)
        n = K.shape[2]
        s = q[mq] @ K.transpose(-1, -2) * scale + M
        lse = torch.logsumexp(s, -1, keepdim=True)
        P = torch.exp(s - lse)
        Pt = P * KP
        ctx = Pt @ V
        # forward gates
        Es = (gamma2(dh) + 3 * U) * scale * (q[mq].abs() @ K.abs().transpose(-1, -2)) + U * s.abs()
        Eexp = (2 * (s - lse).abs() + 4) * U
        r = (P * (Es + Eexp)).sum(-1, keepdim=True)
        RP = Es + Eexp + r + gamma2(n) + 4 * U
        EP = Pt * RP + TINY
        Vabs = V.abs()
        Ectx = EP @ Vabs + (UB + gamma2(n)) * (Pt @ Vabs)
        Else = r + gamma2(n) + 4 * U * math.log(n) + 8 * U + U * lse.abs()
        gctx = G * Ectx + half_ulp_bf16(ctx.abs() + G * Ectx)
        out["ctx"][mq], out["g_ctx"][mq] = rows(ctx), rows(gctx)
        out["lse"][mq], out["g_lse"][mq] = lse.reshape(-1), (G * Else).reshape(-1)
        off = 0
        for mk in bl:
            sl = slice(off, off + Ls[mk])
            out["probs"][mq][mk], out["g_probs"][mq][mk] = Pt[..., sl], G * EP[..., sl]
            off += Ls[mk]
        # backward
        dP = do[mq] @ V.transpose(-1, -2)
        delta = (do[mq] * ctx).sum(-1, keepdim=True)
        dS = P * (KP * dP - delta)
        RPb = Es + Eexp + G * Else + 4 * U
        Edp = gamma2(dh) * (do[mq].abs() @ Vabs.transpose(-1, -2))
        Edelta = ((do[mq].abs() * gctx).sum(-1, keepdim=True) + gamma2(dh) * (do[mq].abs() * ctx.abs()).sum(-1, keepdim=True)
                  + (Pt * (RPb * dP.abs() + Edp)).sum(-1, keepdim=True) + gamma2(n) * (Pt * dP.abs()).sum(-1, keepdim=True))
        EdS0 = P * RPb * (KP * dP - delta).abs() + P * (KP * Edp + Edelta) + 4 * U * P * (KP * dP.abs() + delta.abs())
        EdS = EdS0 + UB * (dS.abs() + EdS0)
        dq = dS @ K * scale
        Edq = scale * (EdS @ K.abs() + gamma2(n) * (dS.abs() @ K.abs())) + U * dq.abs()
        out["dq"][mq] = rows(dq)
        out["g_dq"][mq] = rows(G * Edq + half_ulp_bf16(dq.abs() + G * Edq))
        EPb = Pt * (RPb + UB) + TINY
        off = 0
        for mk in bl:
            sl = slice(off, off + Ls[mk])
            off += Ls[mk]
            dk[mk] += dS[..., sl].transpose(-1, -2) @ q[mq] * scale
            edk[mk] += scale * (EdS[..., sl].transpose(-1, -2) @ q[mq].abs())
            adk[mk] += scale * (dS[..., sl].abs().transpose(-1, -2) @ q[mq].abs())
            dv[mk] += Pt[..., sl].transpose(-1, -2) @ do[mq]
            edv[mk] += EPb[..., sl].transpose(-1, -2) @ do[mq].abs()
            adv[mk] += Pt[..., sl].transpose(-1, -2) @ do[mq].abs()
    for mk in range(2):
        if not nq[mk]:
            continue
        Edk = edk[mk] + gamma2(nq[mk]) * adk[mk] + U * dk[mk].abs()
        Edv = edv[mk] + gamma2(nq[mk]) * adv[mk]
        out["dk"][mk], out["g_dk"][mk] = rows(dk[mk]), rows(G * Edk + half_ulp_bf16(dk[mk].abs() + G * Edk))
        out["dv"][mk], out["g_dv"][mk] = rows(dv[mk]), rows(G * Edv + half_ulp_bf16(dv[mk].abs() + G * Edv))
    return out


def ratio(got, ref, gate):
    """max over elements of |got - ref| / gate (inf where a NaN appears)."""
    d = (got.double() - ref).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, math.inf), d)
    return float((d / gate).max())


def worst(got, ref, gate):
    """(ratio, flat index, got, ref, gate) at the worst element, for assertion messages."""
    d = (got.double() - ref).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, math.inf), d)
    rr = (d / gate).reshape(-1)
    i = int(rr.argmax())
    return float(rr[i]), i, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(gate.reshape(-1)[i])


# ------------------------------------------------------------------------------------------------ fp32 / bf16 emulation of the MFMA kernels
def _bf(x):
    return x.bfloat16().float()


BUGS = ("drop_key", "mask_ignored", "per_block_softmax", "drow_shift", "site_shift", "no_keep_scale", "other_scale", "lse_row_shift",
        "dk_no_scale", "dq_no_scale", "delta_row_shift")


def emulate(inp, gate, p, bug=None, bug_arg=None, seed=SEED, sites=SITES):
    """The MFMA kernels' arithmetic in fp32 with their bf16 rounding points (fp32 sums in torch's order stand in for the MFMA's):
    scores acc * scale + mask, P = exp(s - max) / sum * keep-scale rounded to bf16, ctx stored as bf16; backward P = exp(s - lse) from the
    saved lse, delta = dO . bf16 ctx, P~ and dS rounded to bf16, dK / dQ * scale, bf16 stores.  `bug` plants one defect (BUGS)."""
    B, nh, dh, Ls = inp["B"], inp["nh"], inp["dh"], inp["L"]
    f32 = torch.float32
    scale = torch.tensor(1.0 / math.sqrt(128 if dh == 64 else 64) if bug == "other_scale" else 1.0 / math.sqrt(dh), dtype=f32)
    kscale = torch.tensor(1.0 / (1.0 - p), dtype=f32) if bug != "no_keep_scale" else torch.tensor(1.0, dtype=f32)
    q = [heads(inp["q"][m], B, Ls[m], nh, dh, f32) for m in range(2)]
    k = [heads(inp["k"][m], B, Ls[m], nh, dh, f32) for m in range(2)]
    v = [heads(inp["v"][m], B, Ls[m], nh, dh, f32) for m in range(2)]
    do = [heads(inp["do"][m], B, Ls[m], nh, dh, f32) for m in range(2)]
    mask = [inp["mask"][m].clone() for m in range(2)]
    if bug == "mask_ignored":
        for m in range(2):
            mask[m][bug_arg] = 0.0
    kp = [[None, None], [None, None]]
    for i in range(2):
        for j in range(2):
            if not gate[i][j]:
                continue
            if p > 0:
                site = sites[i][j] + (1 if bug == "site_shift" else 0)
                km = keep_mask(seed, site, B, nh, Ls[i], Ls[j], p, row_shift=1 if bug == "drow_shift" else 0)
                kp[i][j] = torch.where(km, kscale, torch.tensor(0.0, dtype=f32))
            else:
                kp[i][j] = torch.ones(B, nh, Ls[i], Ls[j], dtype=f32)
    out = {key: [None, None] for key in ("ctx", "lse", "dq", "dk", "dv")}
    dk32 = [torch.zeros_like(k[m]) for m in range(2)]
    dv32 = [torch.zeros_like(v[m]) for m in range(2)]
    saved = {}
    for mq in range(2):
        bl = blocks(gate, mq)
        if not bl:
            continue
        K = torch.cat([k[mk] for mk in bl], 2)
        V = torch.cat([v[mk] for mk in bl], 2)
        M = torch.cat([mask[mk][:, None, None, :].expand(B, 1, 1, Ls[mk]) for mk in bl], 3)
        KP = torch.cat([kp[mq][mk] for mk in bl], 3)
        s = (q[mq] @ K.transpose(-1, -2)) * scale + M
        if bug == "drop_key":                 # key bug_arg = (modality, index) never seen
            mk_d, j = bug_arg
            if mk_d in bl:
                s[..., (0 if bl[0] == mk_d else Ls[bl[0]]) + j] = -math.inf
        if bug == "per_block_softmax" and len(bl) == 2:
            parts = s.split([Ls[mk] for mk in bl], -1)
            e = torch.cat([torch.softmax(t, -1) for t in parts], -1)
            lse = torch.logsumexp(s, -1, keepdim=True)
            Pn = e
        else:
            mx = s.amax(-1, keepdim=True)
            e = torch.exp(s - mx)
            sm = e.sum(-1, keepdim=True)
            Pn = e * (1.0 / sm)
            lse = mx + torch.log(sm)
        Pb = _bf(Pn * KP)
        ctx = _bf(Pb @ V)
        out["ctx"][mq], out["lse"][mq] = rows(ctx), lse.reshape(-1)
        saved[mq] = (bl, K, V, KP, s, lse, ctx)
    for mq, (bl, K, V, KP, s, lse, ctx) in saved.items():
        if bug == "lse_row_shift":
            lse = torch.roll(lse, 1, 2)
        P = torch.exp(s - lse)
        dP = do[mq] @ V.transpose(-1, -2)
        delta = (do[mq] * ctx).sum(-1, keepdim=True)
        if bug == "delta_row_shift":
            delta = torch.roll(delta, 1, 2)
        pd = _bf(P * KP)
        ds = _bf(P * (dP * KP - delta))
        out["dq"][mq] = rows(_bf((ds @ K) * (1.0 if bug == "dq_no_scale" else scale)))
        off = 0
        for mk in bl:
            sl = slice(off, off + Ls[mk])
            off += Ls[mk]
            dk32[mk] += ds[..., sl].transpose(-1, -2) @ q[mq]
            dv32[mk] += pd[..., sl].transpose(-1, -2) @ do[mq]
    for mk in range(2):
        if gate[0][mk] or gate[1][mk]:
            out["dk"][mk] = rows(_bf(dk32[mk] * (1.0 if bug == "dk_no_scale" else scale)))
            out["dv"][mk] = rows(_bf(dv32[mk]))
    return out


def worst_ratio(got, ref, keys=("ctx", "lse", "dq", "dk", "dv")):
    """max ratio over the given outputs and modalities: {key: ratio}."""
    res = {}
    for key in keys:
        for m in range(2):
            if ref[key][m] is None:
                continue
            res[(key, m)] = ratio(got[key][m], ref[key][m], ref["g_" + key][m])
    return res


# ------------------------------------------------------------------------------------------------ dispatch restated (attention.hip:552-647)
def mfma_instance(T, R, dh):
    """Template <TP, RP, DHT> vk_gated_attn_fwd / _bwd pick when the MFMA kernels serve the launch."""
    bigT, bigR = T > 32, R > 64
    if dh == 128:
        return (32, 64, 128) if not bigT and not bigR else (64, 64, 128)
    return (64 if bigT else 32, 128 if bigR else 64, 64)


def bwd_ntasks(T, R, gate):
    Ls = [T, R]
    nt = 0
    for m in range(2):
        if gate[m][0] or gate[m][1]:
            nt += (Ls[m] + 15) // 16
        if gate[0][m] or gate[1][m]:
            nt += (Ls[m] + 15) // 16
    return nt


def bwd_branch(T, R, dh, gate):
    """Which branch of launch_bwd (attention.hip:552-569) serves the launch: 'occ3' (three workgroups per CU, 4 waves), 'occ2' (two
    4-wave workgroups per CU) or 'occ2-1wg' (images so large that one workgroup holds the CU: up to 8 waves).  Returns (branch, waves)."""
    TP, RP, DHT = mfma_instance(T, R, dh)
    lds = 4 * (TP + RP) * 2 * DHT + 3 * (TP + RP) * 4 + 16
    nt = bwd_ntasks(T, R, gate)
    if DHT == 64 and 3 * lds <= LDS_LIMIT:
        return "occ3", 4
    if 2 * lds > LDS_LIMIT:
        return "occ2-1wg", min(8, max(4, nt))
    return "occ2", 4


Shape = namedtuple("Shape", "name B nh dh T R path")


def _mfma(nh, dh, T, R, B=3):
    TP, RP, DHT = mfma_instance(T, R, dh)
    return Shape("mfma%d_%d_%d-T%dR%d" % (TP, RP, DHT, T, R), B, nh, dh, T, R, "mfma<%d,%d,%d>" % (TP, RP, DHT))


def _gen(nh, dh, T, R, B=3, tag=""):
    return Shape("gen%s-d%d-T%dR%d" % (tag, dh, T, R), B, nh, dh, T, R, "generic")


SHAPES = (
    # head size 64 (12 heads), <32,64,64>: every tile edge of 16 / 32 text rows, 1 / 37 / 64 regions; backward branch occ3
    [_mfma(12, 64, T, R) for T in (1, 16, 17, 32) for R in (1, 37, 64)]
    # <64,64,64>: backward branch occ2 (two 4-wave workgroups per CU)
    + [_mfma(12, 64, T, R) for T in (33, 38, 64) for R in (37, 64)]
    # <32,128,64>: backward branch occ2-1wg
    + [_mfma(12, 64, 20, R) for R in (65, 101, 128)]
    # <64,128,64>: backward branch occ2-1wg, 8 waves (20+ tasks with every gate open)
    + [_mfma(12, 64, T, R) for T in (38, 64) for R in (101, 128)]
    # head size 128 (8 heads): <32,64,128> and <64,64,128> (vilbert_base's co-attention at T = 38); backward occ2-1wg
    + [_mfma(8, 128, 20, 37)] + [_mfma(8, 128, T, R) for T in (38, 64) for R in (37, 64)]
    # generic kernels: the other head sizes, the first lengths past the MFMA tiles, 128-wide heads whose backward does not fit the MFMA
    # LDS budget, and total keys per query row on either side of the NS = 3 / 5 thresholds (192, 320 keys) and of 128
    + [_gen(4, 32, 20, 37), _gen(4, 96, 38, 101), _gen(12, 64, 65, 37), _gen(12, 64, 20, 129), _gen(8, 128, 65, 37),
       _gen(8, 128, 20, 129), _gen(8, 128, 20, 65), _gen(4, 128, 33, 65),
       _gen(4, 64, 65, 63), _gen(4, 64, 65, 64), _gen(2, 64, 65, 127), _gen(2, 64, 65, 128), _gen(2, 64, 70, 250), _gen(2, 64, 70, 251)]
)


def dist_for(i, gname, train):
    """Input distribution of a case: cycled so that every path sees near-uniform, mid and peaked rows."""
    return ("uniform", "mid", "peaked")[(i + list(GATES).index(gname) + int(train)) % 3]


def largest_bwd_shape(lib_, dh, T=65):
    """Largest vision length R (gate 'all', text length T) whose generic backward vk_gated_attn_lds_bytes admits; found by search."""
    import ctypes as C
    from volta_amd import _lib as L
    aa = L.AttnArgs()
    aa.B, aa.nh, aa.dh, aa.scale = 1, 1, dh, 1.0 / math.sqrt(dh)
    for i in range(2):
        for j in range(2):
            aa.gate[i][j] = 1
    aa.L[0] = T
    best = None
    for R in range(129, 512 - T + 1):
        aa.L[1] = R
        if lib_.vk_gated_attn_lds_bytes(C.byref(aa), 1) > LDS_LIMIT:
            break
        best = R
    return best


Case = namedtuple("Case", "id shape gname p dist probs fwd_only")


def table_cases():
    """Every case of the GPU table that needs no library call to define (the largest-backward shapes are found at test time)."""
    out = []
    for i, sh in enumerate(SHAPES):
        for gname in GATES:
            for train in (False, True):
                out.append(Case("%s-%s-%s" % (sh.name, gname, "train" if train else "eval"), sh, gname, 0.1 if train else 0.0,
                                dist_for(i, gname, train), False, False))
    seen = set()
    for sh in SHAPES:                          # p = 0.5 once per path
        if sh.path not in seen:
            seen.add(sh.path)
            out.append(Case("%s-all-p0.5" % sh.name, sh, "all", 0.5, "mid", False, False))
    bench = Shape("bench-B256", 256, 12, 64, 20, 37, "mfma<32,64,64>")      # the bench workload's grid: 3072 workgroups
    out += [Case("bench-B256-%s" % g, bench, g, 0.1, "mid", False, False) for g in GATES]
    for sh in (Shape("B1", 1, 12, 64, 20, 37, "mfma<32,64,64>"), Shape("B1-gen", 1, 12, 64, 65, 129, "generic")):
        out += [Case("%s-%s" % (sh.name, g), sh, g, 0.1, "uniform", False, False) for g in ("all", "tv+vt")]
    # attention maps: an MFMA-sized shape (which then runs on the generic kernels, the writers of the maps) and a generic one
    for sh in (Shape("probs-T20R37", 3, 12, 64, 20, 37, "generic"), Shape("probs-T65R129", 2, 4, 64, 65, 129, "generic")):
        out += [Case("%s-%s" % (sh.name, g), sh, g, 0.1, "uniform", True, False) for g in GATES]
    # 512 keys per query row: the forward's limit (its backward does not fit the LDS)
    out.append(Case("fwd512-T80R432", Shape("fwd512", 2, 2, 64, 80, 432, "generic-fwd"), "all", 0.1, "uniform", True, True))
    return out


def largest_cases(lib_):
    out = []
    for dh in (64, 128):
        R = largest_bwd_shape(lib_, dh)
        sh = Shape("largest-bwd-d%d-T65R%d" % (dh, R), 2, 2, dh, 65, R, "generic")
        out += [Case(sh.name + "-" + g, sh, g, 0.1, d, False, False) for g, d in (("all", "uniform"), ("tt+tv", "peaked"))]
    return out


def case_path(T, R, dh, gate, probs=False):
    """The dispatch of attention.hip:588-598 (attn_mfma_ok) restated: 'mfma<TP,RP,DHT>' or 'generic'."""
    if probs:
        return "generic"                       # the generic kernels write the attention maps
    Ls = [T, R]
    for m in range(2):
        if (gate[m][0] or gate[m][1] or gate[0][m] or gate[1][m]) and Ls[m] > (64, 128)[m]:
            return "generic"
    if dh == 128:
        TP, RP = (64 if T > 32 else 32), (128 if R > 64 else 64)
        if 4 * (TP + RP) * 2 * dh + 3 * (TP + RP) * 4 + 16 > LDS_LIMIT:
            return "generic"
    elif dh != 64:
        return "generic"
    return "mfma<%d,%d,%d>" % mfma_instance(T, R, dh)


def case_seed(case):
    import zlib
    return zlib.crc32(case.id.encode()) & 0xFFFF
