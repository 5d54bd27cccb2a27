"""csrc/embed.hip through the C ABI against plain float64 torch: the embedding sum and its deterministic two-kernel backward (slots,
keys elected with atomicMin, a combine that walks slots in order), the box-location linear, add_dropout, colsum, rowgroup_sum, relu_bwd
and VL-BERT's region input and mask-embedding gradient.  Dropout masks are replayed with the oracle's Philox stream.

Gates used below (u = 2^-24, the fp32 unit roundoff):
  * a bf16 output is allowed one bf16 ulp of the float64 value (its own round-to-nearest is half of that) plus the fp32 error of what
    was computed before the rounding, written as eps where it is not negligible;
  * an fp32 sum of n + 1 terms (n rows onto a prefill) is allowed gamma_n * sum|terms|, gamma_n = n u / (1 - n u).  That is the bound of
    ANY summation tree whose longest root path has at most n additions (Higham, Accuracy and Stability of Numerical Algorithms, 4.2);
    every kernel here adds exact bf16 / fp32 inputs with plain fp32 adds (adding a zero is exact), so c = 1 needs no knowledge of how
    the kernel groups its slots, waves and workgroups.  A table row that no id reaches has n = 0: it must keep the prefill's bits."""
import ctypes as C

import pytest
import torch

from oracle import volta_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DEV = "cuda"


def _lib():
    from volta_amd import _lib as L
    return L


def _p(t):
    """Raw pointer of a device tensor.  Keep the tensor referenced until the launch: the pointer of a temporary (`_p(x.to(DEV))`)
    can be handed to the next allocation, and two arguments would then alias."""
    return None if t is None else C.c_void_p(t.data_ptr())


def _gamma(n):
    n = torch.as_tensor(n, dtype=torch.float64)
    return n * U / (1 - n * U)


def _bf16_ulp(x):
    """ulp of bf16 at |x| (float64 in, float64 out); 2^-133 at 0, so that a zero reference demands an exact zero."""
    _, e = torch.frexp(x.abs())
    e = torch.where(x == 0, torch.full_like(e, -125), e.clamp_min(-125))
    return torch.ldexp(torch.ones_like(x), e - 8)


def _bf16_close(got, ref, eps=0.0):
    """|got - ref| <= ulp_bf16(|ref| + eps) + eps, elementwise (a bool tensor)."""
    got, ref = got.double(), ref.double()
    eps = torch.as_tensor(eps, dtype=torch.float64, device=ref.device)
    return (got - ref).abs() <= _bf16_ulp(ref.abs() + eps) + eps


def _seed(value):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------------------------------------ embedding sum (forward)
@pytest.mark.parametrize("B,T,H,V", [(256, 20, 768, 30522), (3, 7, 64, 50), (5, 38, 1024, 3000), (4, 9, 100, 77)])
@pytest.mark.parametrize("explicit_pos,with_type,with_extra", [(False, False, False), (True, True, True), (False, True, False), (True, False, True)])
def test_embed_sum_fwd(B, T, H, V, explicit_pos, with_type, with_extra):
    L = _lib()
    g = torch.Generator().manual_seed(B * 1000 + H)
    M, P, NT = B * T, T + 5, 3
    word, pos, typ = torch.randn(V, H, generator=g), torch.randn(P, H, generator=g), torch.randn(NT, H, generator=g)
    ids = torch.randint(0, V, (M,), generator=g)
    ids[:3] = torch.tensor([-1, V, V + 7])                                   # clamped into [0, V)
    type_ids = torch.randint(0, NT, (M,), generator=g) if with_type else None
    if with_type:
        type_ids[:2] = torch.tensor([-2, NT + 1])
    pos_ids = torch.randint(0, P, (M,), generator=g) if explicit_pos else None
    if explicit_pos:
        pos_ids[:2] = torch.tensor([-5, P])
    extra = torch.randn(M, H, generator=g).bfloat16() if with_extra else None
    dv = {k: (None if v is None else v.to(DEV)) for k, v in dict(ids=ids, type_ids=type_ids, pos_ids=pos_ids, word=word, pos=pos, typ=typ, extra=extra).items()}
    z = torch.full((M, H), 7.0, dtype=torch.bfloat16, device=DEV)
    a = L.EmbedArgs(_p(dv["ids"]), _p(dv["type_ids"]), _p(dv["pos_ids"]), _p(dv["word"]), _p(dv["pos"]), _p(dv["typ"]), _p(dv["extra"]), _p(z),
                    M, T, H, V, P, NT)
    L.check(L.lib.vk_embed_sum_fwd(C.byref(a), L.stream_ptr()))
    torch.cuda.synchronize()
    got = z.cpu()
    pi = (pos_ids if explicit_pos else torch.arange(M) % T).clamp(0, P - 1)
    ti = type_ids.clamp(0, NT - 1) if with_type else torch.zeros(M, dtype=torch.long)
    terms = [word.double()[ids.clamp(0, V - 1)], pos.double()[pi], typ.double()[ti]] + ([extra.double()] if with_extra else [])
    ref, absum = sum(terms), sum(t.abs() for t in terms)
    # the fp32 sum of <= 4 terms carries <= 3 roundings of u * sum|terms| before the bf16 rounding
    eps = 4 * U * absum
    assert bool(_bf16_close(got, ref, eps).all()), float((got.double() - ref).abs().max())
    # sensitivity: the position row of the next sequence index is a plausible indexing slip, and the gate sees it
    wrong = ref - terms[1] + pos.double()[(pi + 1).clamp(max=P - 1)]
    assert not bool(_bf16_close(got, wrong, eps).all())


# ------------------------------------------------------------------------------------------------ embedding backward
def _concap_ids(B, T, V, g):
    """ConceptCap-like token ids: [CLS] at t = 0, [SEP] at the caption's end, [MASK] on ~15 %, pad (0) after it, some ids that occur
    once, out-of-range ids (clamped by the kernel), and a key that occurs only in the LAST slot (position-major index M - 1)."""
    lens = torch.randint(min(6, T), T + 1, (B,), generator=g)
    ids = torch.randint(min(1000, V // 2), V, (B, T), generator=g)
    ids[torch.rand(B, T, generator=g) < 0.15] = 103
    ids[torch.arange(T)[None] >= lens[:, None]] = 0
    ids[torch.arange(B), lens - 1] = 102
    ids[:, 0] = 101
    for k, b in enumerate(range(1, min(B, 6))):
        ids[b, 1] = 500 + k                                                    # rare ids: once each
    ids[min(2, B - 1), min(2, T - 1)] = -3
    ids[min(3, B - 1), min(3, T - 1)] = V
    ids[min(4, B - 1), min(4, T - 1)] = V + 7
    ids[B - 1, T - 1] = 998                                                    # slot S - 1 (or the last used slot): its only row
    return ids.view(-1)


def _table_ref(prefill, idx, dz64):
    """float64 reference of an accumulated table, the per-element sum|terms| and the per-row term count."""
    ref = prefill.double().index_add(0, idx, dz64)
    absum = prefill.double().abs().index_add(0, idx, dz64.abs())
    cnt = torch.zeros(prefill.shape[0], dtype=torch.float64).index_add(0, idx, torch.ones(idx.numel(), dtype=torch.float64))
    return ref, absum, cnt


def _sum_ok(got, ref, absum, cnt):
    """gamma_n * sum|terms| per element, n = the row's count (see the module docstring)."""
    return (got.double() - ref).abs() <= _gamma(cnt)[:, None] * absum


def _embed_bwd(L, dz, ids, type_ids, pos_ids, T, V, P, NT, dword0, dpos0, dtype0, ws_fill=0, dpos_null=False):
    """One vk_embed_sum_bwd call from the given (CPU) prefills; returns the three tables on the CPU (None where not passed)."""
    M, H = dz.shape
    dev = lambda t: None if t is None else t.to(DEV).contiguous()
    dz_d, ids_d, ty_d, ps_d = dev(dz), dev(ids), dev(type_ids), dev(pos_ids)
    dw, dp, dt = dev(dword0.clone()), None if dpos_null else dev(dpos0.clone()), None if dtype0 is None else dev(dtype0.clone())
    nbytes = L.lib.vk_embed_bwd_workspace_bytes(M, H, V, P, int(pos_ids is not None and dp is not None))
    work = torch.full((nbytes,), ws_fill, dtype=torch.uint8, device=DEV)
    a = L.EmbedBwdArgs(_p(dz_d), _p(ids_d), _p(ty_d), _p(ps_d), _p(dw), _p(dp), _p(dt), M, T, H, NT, V, P, _p(work))
    L.check(L.lib.vk_embed_sum_bwd(C.byref(a), L.stream_ptr()))
    torch.cuda.synchronize()
    return dw.cpu(), None if dp is None else dp.cpu(), None if dt is None else dt.cpu()


def _check_bwd(dz, ids, type_ids, pos_ids, T, V, P, NT, dword0, dpos0, dtype0, got):
    """Every table against float64 index_add_ of the bf16 rows; returns the word table's reference for further checks."""
    dw, dp, dt = got
    M = dz.shape[0]
    dz64 = dz.double()
    ref_w = _table_ref(dword0, ids.clamp(0, V - 1), dz64)
    ok = _sum_ok(dw, *ref_w)
    assert bool(ok.all()), ("dword", int((~ok).sum()), float((dw.double() - ref_w[0]).abs().max()))
    if dt is not None:
        ti = type_ids.clamp(0, NT - 1) if type_ids is not None else torch.zeros(M, dtype=torch.long)
        ref_t = _table_ref(dtype0, ti, dz64)
        assert bool(_sum_ok(dt, *ref_t).all()), ("dtype", float((dt.double() - ref_t[0]).abs().max()))
    if dp is not None:
        if pos_ids is not None:                                                # explicit positions: accumulated
            ref_p = _table_ref(dpos0, pos_ids.clamp(0, P - 1), dz64)
            assert bool(_sum_ok(dp, *ref_p).all()), ("dpos", float((dp.double() - ref_p[0]).abs().max()))
        else:                                                                  # implicit: rows [0, T) overwritten, the rest untouched
            zero = torch.zeros(T, dz.shape[1])
            ref_p = _table_ref(zero, torch.arange(M) % T, dz64)
            assert bool(_sum_ok(dp[:T], *ref_p).all()), ("dpos", float((dp[:T].double() - ref_p[0]).abs().max()))
            assert torch.equal(dp[T:], dpos0[T:])
    return ref_w


def _prefills(g, V, P, NT, H):
    return torch.randn(V, H, generator=g) * 0.5, torch.randn(P, H, generator=g) * 0.5, torch.randn(NT, H, generator=g) * 0.5


def test_embed_bwd_ctrl_vilbert_shape_with_contract_checks():
    """Case A: ctrl_vilbert's text call (B=256, T=20, V=30522, two types, implicit positions).  [CLS] fills slots of 8 workgroups,
    [MASK] and pad reach every workgroup (the combine's multi-wave, base += 256 loop).  Plus: accumulation onto a non-zero prefill,
    untouched rows keep their bits, a 0xFF-filled workspace gives the same bits as a zeroed one, two calls give the same bits, and the
    gate rejects a reference that lost one row of [CLS]."""
    L = _lib()
    B, T, V, P, NT, H = 256, 20, 30522, 512, 2, 768
    g = torch.Generator().manual_seed(11)
    ids = _concap_ids(B, T, V, g)
    type_ids = (torch.rand(B * T, generator=g) < 0.3).long()
    dz = torch.randn(B * T, H, generator=g).bfloat16()
    dword0, dpos0, dtype0 = _prefills(g, V, P, NT, H)
    got = _embed_bwd(L, dz, ids, type_ids, None, T, V, P, NT, dword0, dpos0, dtype0)
    ref, absum, cnt = _check_bwd(dz, ids, type_ids, None, T, V, P, NT, dword0, dpos0, dtype0, got)
    untouched = cnt == 0
    assert int(untouched.sum()) > 20000 and torch.equal(got[0][untouched], dword0[untouched])
    assert cnt[998] == 1 and cnt[101] == B and cnt[0] > 64 * 8
    # sensitivity: [CLS] (101) is one key in 8 slots; a reference without one of its rows must fail the gate
    lost = ref.clone()
    lost[101] -= dz[37 * T].double()
    assert not bool(_sum_ok(got[0][101:102], lost[101:102], absum[101:102], cnt[101:102]).all())
    again = _embed_bwd(L, dz, ids, type_ids, None, T, V, P, NT, dword0, dpos0, dtype0, ws_fill=0xFF)
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    third = _embed_bwd(L, dz, ids, type_ids, None, T, V, P, NT, dword0, dpos0, dtype0)
    for a, b in zip(got, third):
        assert torch.equal(a, b)


def test_embed_bwd_vlbert_visual_one_position_key():
    """Case B: VL-BERT's visual call: 256 samples x 100 regions, a 3-row word table, every row the same explicit position id and type 2
    of 3 -- one position key in 25 600 slots, one type key over every workgroup."""
    L = _lib()
    B, T, V, P, NT, H = 256, 100, 3, 512, 3, 768
    g = torch.Generator().manual_seed(12)
    ids = torch.where(torch.rand(B, T, generator=g) < 0.15, 2, 0)
    ids[:, -1] = 1
    ids = ids.view(-1)
    type_ids = torch.full((B * T,), 2, dtype=torch.long)
    pos_ids = torch.full((B * T,), 21, dtype=torch.long)
    dz = (torch.randn(B * T, H, generator=g) + 0.25).bfloat16()
    dword0, dpos0, dtype0 = _prefills(g, V, P, NT, H)
    got = _embed_bwd(L, dz, ids, type_ids, pos_ids, T, V, P, NT, dword0, dpos0, dtype0)
    _check_bwd(dz, ids, type_ids, pos_ids, T, V, P, NT, dword0, dpos0, dtype0, got)
    keep = torch.ones(P, dtype=torch.bool)
    keep[21] = False
    assert torch.equal(got[1][keep], dpos0[keep]) and torch.equal(got[2][:2], dtype0[:2])
    again = _embed_bwd(L, dz, ids, type_ids, pos_ids, T, V, P, NT, dword0, dpos0, dtype0, ws_fill=0xFF)
    for a, b in zip(got, again):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,T", [(37, 20), (3, 7), (32, 4)])
@pytest.mark.parametrize("explicit_pos", [False, True])
def test_embed_bwd_ragged_row_counts(B, T, explicit_pos):
    """Case C / D: M not a multiple of 32 (a partial last workgroup) and a key whose only row is in the last slot."""
    L = _lib()
    V, P, NT, H = 3000, 64, 2, 768
    g = torch.Generator().manual_seed(B * T)
    ids = _concap_ids(B, T, V, g)
    type_ids = torch.randint(0, NT, (B * T,), generator=g)
    pos_ids = torch.randint(-2, P + 3, (B * T,), generator=g) if explicit_pos else None
    dz = torch.randn(B * T, H, generator=g).bfloat16()
    dword0, dpos0, dtype0 = _prefills(g, V, P, NT, H)
    got = _embed_bwd(L, dz, ids, type_ids, pos_ids, T, V, P, NT, dword0, dpos0, dtype0)
    _check_bwd(dz, ids, type_ids, pos_ids, T, V, P, NT, dword0, dpos0, dtype0, got)
    # the last slot's key: exactly its one row on the prefill (fp32 add of one bf16 value: one rounding)
    assert torch.equal(got[0][998], (dword0[998] + dz[-1].float()))


@pytest.mark.parametrize("H", [64, 100, 260, 768, 1024])
def test_embed_bwd_hidden_sizes(H):
    """Case E: the four NCH instantiations (H <= 256, 512, 768, 1024) and partial 256-column chunks (100, 260)."""
    L = _lib()
    B, T, V, P, NT = 40, 12, 700, 32, 2
    g = torch.Generator().manual_seed(H)
    ids = _concap_ids(B, T, V, g)
    type_ids = torch.randint(0, NT, (B * T,), generator=g)
    pos_ids = torch.randint(0, P, (B * T,), generator=g)
    dz = torch.randn(B * T, H, generator=g).bfloat16()
    dword0, dpos0, dtype0 = _prefills(g, V, P, NT, H)
    for pids in (None, pos_ids):
        got = _embed_bwd(L, dz, ids, type_ids, pids, T, V, P, NT, dword0, dpos0, dtype0)
        _check_bwd(dz, ids, type_ids, pids, T, V, P, NT, dword0, dpos0, dtype0, got)


@pytest.mark.parametrize("NT", [1, 2, 3, 4])
@pytest.mark.parametrize("with_dtype", [True, False])
def test_embed_bwd_type_counts(NT, with_dtype):
    """Case F: one to four token types (out-of-range type ids clamped), and no type table at all (dtype NULL)."""
    L = _lib()
    B, T, V, P, H = 33, 9, 500, 16, 260
    g = torch.Generator().manual_seed(NT)
    ids = _concap_ids(B, T, V, g)
    type_ids = torch.randint(-1, NT + 2, (B * T,), generator=g)
    dz = torch.randn(B * T, H, generator=g).bfloat16()
    dword0, dpos0, dtype0 = _prefills(g, V, P, NT, H)
    got = _embed_bwd(L, dz, ids, type_ids, None, T, V, P, NT, dword0, dpos0, dtype0 if with_dtype else None)
    _check_bwd(dz, ids, type_ids, None, T, V, P, NT, dword0, dpos0, dtype0 if with_dtype else None, got)
    assert (got[2] is not None) == with_dtype


def test_embed_bwd_explicit_positions_without_dpos():
    """Case G: pos_ids set, dpos NULL (the header's workspace formula has no position part then): the word and type tables get exactly
    the bits of the call without position ids."""
    L = _lib()
    B, T, V, P, NT, H = 37, 20, 3000, 64, 2, 768
    g = torch.Generator().manual_seed(5)
    ids = _concap_ids(B, T, V, g)
    type_ids = torch.randint(0, NT, (B * T,), generator=g)
    pos_ids = torch.full((B * T,), 7, dtype=torch.long)
    dz = torch.randn(B * T, H, generator=g).bfloat16()
    dword0, dpos0, dtype0 = _prefills(g, V, P, NT, H)
    got = _embed_bwd(L, dz, ids, type_ids, pos_ids, T, V, P, NT, dword0, dpos0, dtype0, dpos_null=True)
    assert got[1] is None
    _check_bwd(dz, ids, type_ids, None, T, V, P, NT, dword0, dpos0, dtype0, got)
    plain = _embed_bwd(L, dz, ids, type_ids, None, T, V, P, NT, dword0, dpos0, dtype0, dpos_null=True)
    assert torch.equal(got[0], plain[0]) and torch.equal(got[2], plain[2])


# ------------------------------------------------------------------------------------------------ box-location linear
@pytest.mark.parametrize("M", [1, 31, 33, 9472])
@pytest.mark.parametrize("H", [64, 768, 1024])
@pytest.mark.parametrize("nloc", [5, 8])
def test_loc_linear_fwd_bwd(M, H, nloc):
    L = _lib()
    g = torch.Generator().manual_seed(M + H + nloc)
    loc, W, b = torch.rand(M, nloc, generator=g), torch.randn(H, nloc, generator=g) * 0.3, torch.randn(H, generator=g) * 0.1
    dz = torch.randn(M, H, generator=g).bfloat16()
    locd, Wd, bd, dzd = loc.to(DEV), W.to(DEV), b.to(DEV), dz.to(DEV)
    out = torch.full((M, H), 7.0, dtype=torch.bfloat16, device=DEV)
    partial = torch.zeros(L.lib.vk_rows32(M) * 9 * H, device=DEV)
    dW, db = torch.full((H, nloc), 7.0, device=DEV), torch.full((H,), 7.0, device=DEV)
    L.check(L.lib.vk_loc_linear_fwd(_p(locd), _p(Wd), _p(bd), _p(out), M, H, nloc, L.stream_ptr()))
    L.check(L.lib.vk_loc_linear_bwd(_p(dzd), _p(locd), _p(partial), _p(dW), _p(db), M, H, nloc, L.stream_ptr()))
    torch.cuda.synchronize()
    l64, W64, b64, dz64 = loc.double(), W.double(), b.double(), dz.double()
    ref = l64 @ W64.T + b64
    # nloc products and nloc adds in fp32 (fused or not): <= (nloc + 1) u * sum|terms| before the bf16 rounding
    eps = (nloc + 1) * U * (l64.abs() @ W64.abs().T + b64.abs())
    assert bool(_bf16_close(out.cpu(), ref, eps).all())
    # dW[n][k] = sum_m dz[m][n] loc[m][k]: M products (one rounding each) summed by a tree: gamma_{M+1}
    ref_dW, abs_dW = dz64.T @ l64, dz64.abs().T @ l64.abs()
    assert bool(((dW.cpu().double() - ref_dW).abs() <= _gamma(M + 1) * abs_dW).all())
    assert bool(((db.cpu().double() - dz64.sum(0)).abs() <= _gamma(M) * dz64.abs().sum(0)).all())
    # sensitivity: a bias gradient that skipped the last row is outside the gate
    if 1 < M <= 64:                                                            # (at M = 9472 the bound exceeds one row's size)
        assert not bool(((db.cpu().double() - dz64[:-1].sum(0)).abs() <= _gamma(M) * dz64.abs().sum(0)).all())


# ------------------------------------------------------------------------------------------------ add_dropout
@pytest.mark.parametrize("scale", [0.5, 1.0])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("backward", [0, 1])
def test_add_dropout(scale, p, backward):
    L = _lib()
    M, H = 37, 2048 + 260
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(M, H, generator=g).bfloat16(), torch.randn(M, H, generator=g).bfloat16()
    seed, site = 0x1234ABCD5678, 9
    seed_t = _seed(seed)
    y = torch.full((M, H), 7.0, dtype=torch.bfloat16, device=DEV)
    ad, bd = a.to(DEV), b.to(DEV)
    L.check(L.lib.vk_add_dropout(_p(ad), _p(bd), _p(y), M, H, scale, L.dropout_cfg(seed_t.data_ptr(), site, p), backward, L.stream_ptr()))
    torch.cuda.synchronize()
    keep = R.philox_keep_mask(seed, site, (M, H), p).double() / (1 - p) if p else torch.ones(M, H, dtype=torch.float64)
    x = a.double() if backward else a.double() + b.double()                   # the backward ignores b
    ref = x * scale * keep
    eps = 4 * U * (a.double().abs() + (0 if backward else b.double().abs())) * scale * keep
    got = y.cpu()
    assert bool(_bf16_close(got, ref, eps).all())
    if p:
        assert bool((got[keep == 0] == 0).all()) and 0.05 < float((keep == 0).double().mean()) < 0.15
        # sensitivity: the mask of the neighbouring site is not this one
        other = R.philox_keep_mask(seed, site + 1, (M, H), p).double() / (1 - p)
        assert not bool(_bf16_close(got, x * scale * other, eps).all())


# ------------------------------------------------------------------------------------------------ column / row-group sums, relu_bwd
@pytest.mark.parametrize("M", [1, 33, 9472])
@pytest.mark.parametrize("H", [64, 260, 1024])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_colsum(M, H, accumulate):
    L = _lib()
    g = torch.Generator().manual_seed(M * H)
    src, out0 = torch.randn(M, H, generator=g).bfloat16(), torch.randn(H, generator=g)
    out = out0.to(DEV)
    partial = torch.full((L.lib.vk_rows32(M) * H,), float("nan"), device=DEV)
    srcd = src.to(DEV)
    L.check(L.lib.vk_colsum_bf16(_p(srcd), _p(partial), _p(out), M, H, accumulate, L.stream_ptr()))
    torch.cuda.synchronize()
    s64 = src.double()
    ref = s64.sum(0) + (out0.double() if accumulate else 0)
    absum = s64.abs().sum(0) + (out0.double().abs() if accumulate else 0)
    assert bool(((out.cpu().double() - ref).abs() <= _gamma(M) * absum).all())


@pytest.mark.parametrize("T", [1, 20, 36])
@pytest.mark.parametrize("H", [64, 768, 1028])
def test_rowgroup_sum(T, H):
    L = _lib()
    B = 37
    g = torch.Generator().manual_seed(T * H)
    x = torch.randn(B * T, H, generator=g).bfloat16()
    out = torch.full((B, H), 7.0, dtype=torch.bfloat16, device=DEV)
    xd = x.to(DEV)
    L.check(L.lib.vk_rowgroup_sum_bf16(_p(xd), _p(out), B, T, H, L.stream_ptr()))
    torch.cuda.synchronize()
    x64 = x.double().view(B, T, H)
    ref, eps = x64.sum(1), _gamma(T) * x64.abs().sum(1)
    assert bool(_bf16_close(out.cpu(), ref, eps).all())
    if T > 1:                                                                  # sensitivity: a sum that missed the group's last row
        assert not bool(_bf16_close(out.cpu(), x64[:, :-1].sum(1), eps).all())


@pytest.mark.parametrize("n", [8, 8 * (4096 * 256 + 3)])
def test_relu_bwd_exact(n):
    """Bit-exact: dy passes where y > 0; +0, -0, negatives and NaN in y give +0.  The larger n exceeds the 4096-block grid (stride loop)."""
    L = _lib()
    g = torch.Generator().manual_seed(n % 1000)
    y = torch.randn(n, generator=g).bfloat16()
    dy = torch.randn(n, generator=g).bfloat16()
    y[:8] = torch.tensor([0.0, -0.0, 1.0, -1.0, float("nan"), 1e-30, -1e-30, float("inf")]).bfloat16()
    out = torch.full((n,), 7.0, dtype=torch.bfloat16, device=DEV)
    dyd, yd = dy.to(DEV), y.to(DEV)
    L.check(L.lib.vk_relu_bwd_bf16(_p(dyd), _p(yd), _p(out), n, L.stream_ptr()))
    torch.cuda.synchronize()
    want = torch.where(y.float() > 0, dy, torch.zeros_like(dy))
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))


# ------------------------------------------------------------------------------------------------ VL-BERT region input
@pytest.mark.parametrize("F,dim", [(2048, 16), (256, 8)])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_vlbert_prep_and_maskgrad(F, dim, p):
    """Rows [sin|cos box embedding | feature] with all-zero feature rows (-0.0 included) replaced by the mask embedding and flagged; the
    mask embedding's gradient sums the flagged rows' dropout-masked gradient from column col0 = 8 * dim on."""
    L = _lib()
    M = 73
    g = torch.Generator().manual_seed(F + dim)
    xy = torch.rand(M, 2, generator=g) * 0.6
    wh = torch.rand(M, 2, generator=g) * 0.4
    loc = torch.cat([xy, xy + wh, (wh[:, :1] * wh[:, 1:])], 1)               # x1 y1 x2 y2 area
    feat = torch.relu(torch.randn(M, F, generator=g))
    feat[[3, 40, 72]] = 0.0
    feat[41] = -0.0
    feat[5] = 0.0
    feat[5, F - 1] = 1e-3                                                      # one non-zero element: not a masked row
    mask_emb = torch.randn(F, generator=g)
    W = 8 * dim + F
    seed, site = 0x0DDBA11, 13
    seed_t = _seed(seed)
    drop = L.dropout_cfg(seed_t.data_ptr(), site, p)
    out = torch.full((M, W), 7.0, dtype=torch.bfloat16, device=DEV)
    flag = torch.full((M,), 7, dtype=torch.int32, device=DEV)
    locd, featd, embd = loc.to(DEV), feat.to(DEV), mask_emb.to(DEV)
    L.check(L.lib.vk_vlbert_prep_fwd(_p(locd), 5, _p(featd), _p(embd), _p(out), _p(flag), M, F, dim, drop, L.stream_ptr()))
    dx = torch.randn(M, W, generator=g).bfloat16()
    partial = torch.full((L.lib.vk_rows32(M) * F,), float("nan"), device=DEV)
    dmask = torch.full((F,), 7.0, device=DEV)
    dxd = dx.to(DEV)
    L.check(L.lib.vk_vlbert_maskgrad(_p(dxd), W, 8 * dim, _p(flag), _p(partial), _p(dmask), M, F, drop, L.stream_ptr()))
    torch.cuda.synchronize()
    zero = (feat == 0).all(1)
    assert zero.nonzero().view(-1).tolist() == [3, 40, 41, 72]
    assert torch.equal(flag.cpu(), zero.int())
    keep = R.philox_keep_mask(seed, site, (M, W), p).double() / (1 - p) if p else torch.ones(M, W, dtype=torch.float64)
    coord = R.coordinate_embeddings(loc[:, :4].double(), dim).reshape(M, 8 * dim)
    fsel = torch.where(zero[:, None], mask_emb.double(), feat.double())
    ref = torch.cat([coord, fsel], 1) * keep
    # the fp32 angle pos / 1000^(i/dim) carries a few roundings (|ang| <= 100): sin / cos move by <= 8 u |ang|, plus their own error
    pos = torch.stack([(loc[:, 0] + loc[:, 2]) / 2, (loc[:, 1] + loc[:, 3]) / 2, loc[:, 2] - loc[:, 0], loc[:, 3] - loc[:, 1]], 1).double() * 100
    ang = (pos[:, :, None] / 1000 ** (torch.arange(dim, dtype=torch.float64) / dim)).repeat(1, 1, 2).reshape(M, 8 * dim)
    eps = torch.cat([8 * U * ang + 2.0 ** -21, 4 * U * fsel.abs()], 1) * keep
    assert bool(_bf16_close(out.cpu(), ref, eps).all())
    # d(mask_emb) = sum over flagged rows of keep * dx[:, col0:]: the fp32 scale and the product round once each, a summation tree
    # over the n rows: gamma_{n+2}
    terms = (dx.double() * keep)[zero][:, 8 * dim:]
    n = int(zero.sum())
    got = dmask.cpu().double()
    assert bool(((got - terms.sum(0)).abs() <= _gamma(n + 2) * terms.abs().sum(0)).all())
    # sensitivity: the gradient of columns that start at 0 instead of col0 is a different vector
    wrong = (dx.double() * keep)[zero][:, :F].sum(0)
    assert not bool(((got - wrong).abs() <= _gamma(n + 2) * terms.abs().sum(0)).all())
