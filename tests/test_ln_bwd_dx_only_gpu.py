"""The LayerNorm backward without parameter gradients (vk_ln_bwd_args.partial NULL: gamma and beta frozen), against the full kernel.

The two instantiations share the row arithmetic, so the claim is equality of bits, not a tolerance: dz / dd of a job without `partial`
are torch.equal to the full kernel's on the same inputs (the full kernel itself is pinned by the float64 tests of
tests/test_ln_kernels_gpu.py).  Widths of one, three and four column chunks; a lone row, one row past a workgroup's block of 16, and the
tiny plan's 74 rows; dropout off and on, applied before (`post` 0) and after (`post` 1) the normalisation's input; dd and dz present or
NULL; and a mixed pair of different row counts, whose job with parameter gradients must give the dgamma / dbeta bits of a launch alone."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 0x5EED1234
CANARY = -7.5


def _inputs(M, H, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    dy, z = r(M, H).bfloat16().cuda(), (r(M, H) * 1.5 + 0.25).bfloat16().cuda()
    zf = z.float()
    mean = zf.mean(1).contiguous()
    rstd = (zf.var(1, unbiased=False) + 1e-12).rsqrt().contiguous()
    gamma = (1.0 + 0.1 * r(H)).cuda()
    return dy, z, mean, rstd, gamma


class Job:
    """One vk_ln_bwd_args over fresh output buffers; `params` False leaves partial / dgamma / dbeta NULL."""

    def __init__(self, inp, M, H, p, post, dd, dz, params, seed_t):
        from volta_amd import _lib as L, ops
        dy, z, mean, rstd, gamma = inp
        new = lambda on: torch.full((M, H), CANARY, dtype=torch.bfloat16, device="cuda") if on else None
        self.dz, self.dd = new(dz), new(dd)
        self.partial = torch.zeros(L.lib.vk_ln_bwd_partial_rows(M) * 2 * H, device="cuda") if params else None
        self.dgamma = torch.full((H,), CANARY, device="cuda") if params else None
        self.dbeta = torch.full((H,), CANARY, device="cuda") if params else None
        drop = L.dropout_cfg(seed_t.data_ptr(), 3, p)
        self.keep = (inp, seed_t)
        self.args = ops.ln_bwd_args(dy, z, mean, rstd, gamma, self.dz, self.dd, self.partial, self.dgamma, self.dbeta, M, H, drop=drop, post=post,
                                    out_scale=0.5)

    def run(self):
        import ctypes as C
        from volta_amd import _lib as L
        L.check(L.lib.vk_ln_bwd(C.byref(self.args), L.stream_ptr()))
        torch.cuda.synchronize()
        return self


@pytest.fixture(scope="module")
def seed_t():
    from volta_amd import ops
    t = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.set_seed(t, SEED)
    return t


@pytest.fixture(scope="module")
def reference(seed_t):
    """The full kernel's outputs per (M, H, p, post), computed once and shared by every case that needs them."""
    cache = {}

    def get(M, H, p, post):
        key = (M, H, p, post)
        if key not in cache:
            inp = _inputs(M, H, 1000 * M + H)
            cache[key] = (inp, Job(inp, M, H, p, post, True, True, True, seed_t).run())
        return cache[key]
    return get


@pytest.mark.parametrize("dz", [True, False])
@pytest.mark.parametrize("dd", [True, False])
@pytest.mark.parametrize("post", [0, 1])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("M", [1, 17, 74])
@pytest.mark.parametrize("H", [64, 768, 1024])
def test_dx_only_equals_full_kernel(reference, seed_t, H, M, p, post, dd, dz):
    inp, full = reference(M, H, p, post)
    assert not torch.any(full.dz == CANARY) and not torch.any(full.dd == CANARY) and not torch.any(full.dgamma == CANARY)
    job = Job(inp, M, H, p, post, dd, dz, False, seed_t).run()
    if dz:
        assert torch.equal(job.dz, full.dz)
    if dd:
        assert torch.equal(job.dd, full.dd)
    if p > 0 and post == 0:
        assert not torch.equal(full.dd, full.dz)          # the dropout really is applied: dd is the masked, rescaled dz


@pytest.mark.parametrize("H", [64, 768, 1024])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_full_kernel_without_dz(reference, seed_t, H, p):
    """`dz` NULL on the full instantiation too: dd and the parameter gradients are those of a launch that stores dz."""
    M = 74
    inp, full = reference(M, H, p, 0)
    job = Job(inp, M, H, p, 0, True, False, True, seed_t).run()
    assert torch.equal(job.dd, full.dd) and torch.equal(job.dgamma, full.dgamma) and torch.equal(job.dbeta, full.dbeta)


@pytest.mark.parametrize("H", [64, 768, 1024])
@pytest.mark.parametrize("order", ["params_first", "params_second"])
def test_mixed_pair(reference, seed_t, H, order):
    """One job with parameter gradients, one without, of different row counts, through vk_ln_bwd_pair: both jobs' dz / dd are the full
    kernel's, and the job with parameter gradients gets the dgamma / dbeta bits of a launch alone."""
    from volta_amd import ops
    Ma, Mb, p, post = 74, 17, 0.1, 1
    inp_a, full_a = reference(Ma, H, p, post)
    inp_b, full_b = reference(Mb, H, p, post)
    a = Job(inp_a, Ma, H, p, post, True, True, True, seed_t)
    b = Job(inp_b, Mb, H, p, post, True, True, False, seed_t)
    ops.ln_bwd_pair(*((a.args, b.args) if order == "params_first" else (b.args, a.args)))
    torch.cuda.synchronize()
    assert torch.equal(a.dz, full_a.dz) and torch.equal(a.dd, full_a.dd)
    assert torch.equal(a.dgamma, full_a.dgamma) and torch.equal(a.dbeta, full_a.dbeta)
    assert torch.equal(b.dz, full_b.dz) and torch.equal(b.dd, full_b.dd)


def test_pair_without_parameter_gradients(reference, seed_t):
    """Both jobs frozen: one launch of the instantiation without column sums."""
    from volta_amd import ops
    H, p, post = 768, 0.1, 0
    inp_a, full_a = reference(74, H, p, post)
    inp_b, full_b = reference(17, H, p, post)
    a = Job(inp_a, 74, H, p, post, True, False, False, seed_t)
    b = Job(inp_b, 17, H, p, post, True, True, False, seed_t)
    ops.ln_bwd_pair(a.args, b.args)
    torch.cuda.synchronize()
    assert torch.equal(a.dd, full_a.dd) and torch.equal(b.dd, full_b.dd) and torch.equal(b.dz, full_b.dz)


def test_finalize_without_records_is_an_error(reference, seed_t):
    import ctypes as C
    from volta_amd import _lib as L
    inp, _ = reference(17, 64, 0.0, 0)
    job = Job(inp, 17, 64, 0.0, 0, True, True, False, seed_t)
    assert L.lib.vk_ln_bwd_finalize(C.byref(job.args), L.stream_ptr()) != 0
    assert b"partial" in L.lib.vk_last_error()
