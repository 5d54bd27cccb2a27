// Fused LAMB over the flat fp32 arenas and tensors outside them, with the semantics of the apex FusedLAMB the reference tree vendors
// (apex/apex/optimizers/fused_lamb.py over apex/csrc/multi_tensor_lamb.cu).  LAMB needs two reductions per PARAMETER TENSOR (|p| and
// |update|), and tensor boundaries fall inside the arena's 1024-element chunks (the three biases of a fused Q|K|V slot share one), so the
// chunk-class scheme of adamw_kernel / radam_kernel cannot carry it.  The work is cut into pieces instead: at most 1024 consecutive
// elements of one tensor, one workgroup each, described by a piece table the host builds once (include/volta_hip.h, vk_lamb_step):
//   gsq     per piece: sum of g^2                    |  only when a group clips
//   gsum    per norm group: its pieces' sums, double |  (64 runs per group, then the runs in order)
//   cdiv    per norm group: the clip divisor c_n     |
//   stage 1 per piece: moments, sums of p^2 and u^2
//   finish  per tensor: its pieces' sums in double -> trust ratio
//   stage 2 per piece: u again from the m, v, p it reads (same element function, same bits), p -= ratio u, bf16 copy
// Every sum has a fixed order (lane, DPP tree, four waves; pieces in piece order): no atomics, equal inputs give equal bits, and a
// tensor's norms depend on its own data alone.
#include "common.h"
#include "../../include/volta_hip.h"
#include "util.h"

namespace vk {

struct LambDev {                // what the kernels take by value
    const vk_lamb_tensor* tensors;
    const vk_lamb_piece* pieces;
    const vk_lamb_group* groups;
    double* gpart;              // [ngroups][LAMB_SEGS]
    double* gsum;               // [ngroups]
    float* gsq;                 // [npieces]
    float* psq;                 // [npieces]
    float* usq;                 // [npieces]
    float* cdiv;                // [ngroups], NULL: no group clips
    float* table;               // [ntensors][4]
    const float* clip;
    int32_t ntensors, npieces, ngroups, flags;
    float cls_lr[VK_LAMB_CLASSES], cls_wd[VK_LAMB_CLASSES], cls_bc1[VK_LAMB_CLASSES], cls_bc2[VK_LAMB_CLASSES];
    float beta1, beta2, eps, grad_scale;
};

// The element functions, spelled with explicit fused multiply-adds and no further contraction: both stages, and the 16-byte and the
// element-wise paths, give the same bits for equal inputs.
__device__ __forceinline__ void lamb_moments(float& m, float& v, float g, float p, float gs, float c, float b1, float b2, float b3, float wd, bool adam_w) {
#pragma clang fp contract(off)
    float gc = (g * gs) / c;
    if (!adam_w && wd != 0.f) gc = __builtin_fmaf(wd, p, gc);
    m = __builtin_fmaf(b1, m, b3 * gc);
    v = __builtin_fmaf(b2, v, ((1.f - b2) * gc) * gc);
}
__device__ __forceinline__ float lamb_update(float m, float v, float p, float bc1, float bc2, float eps, float wd, bool adam_w) {
#pragma clang fp contract(off)
    const float r = (m / bc1) / (sqrtf(v / bc2) + eps);
    return (adam_w && wd != 0.f) ? __builtin_fmaf(wd, p, r) : r;
}

// sum over the workgroup's 256 lanes in a fixed order; valid in thread 0
__device__ __forceinline__ float block_sum(float s, float* sh) {
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__device__ __forceinline__ double block_sum(double s, double* sh) {
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// 16-byte accesses for a piece: the tensor's pointers allow them and the piece starts on a multiple of four elements
__device__ __forceinline__ bool piece_vec(const vk_lamb_tensor& t, const vk_lamb_piece& pc) {
    return !((((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v) & 15) | ((uintptr_t)t.shadow & 7) | (uintptr_t)(pc.offset & 3));
}

__global__ __launch_bounds__(256) void lamb_gsq_kernel(LambDev a) {
    __shared__ float sh[4];
    const vk_lamb_piece pc = a.pieces[blockIdx.x];
    const vk_lamb_tensor t = a.tensors[pc.tensor];
    const float* g = t.g + pc.offset;
    const int i = threadIdx.x * 4;
    float s = 0.f;
    {
#pragma clang fp contract(off)
        if (piece_vec(t, pc) && i + 4 <= pc.count) {
            const f32x4 x = __builtin_nontemporal_load((const f32x4*)(g + i));
            s = ((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + x[3] * x[3];
        } else {
            float x[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) x[r] = i + r < pc.count ? g[i + r] : 0.f;
            s = ((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + x[3] * x[3];
        }
    }
    s = block_sum(s, sh);
    if (threadIdx.x == 0) a.gsq[blockIdx.x] = s;
}

// a group's piece sums in two levels, both in a fixed order: LAMB_SEGS workgroups add contiguous runs of them in double, then one thread
// adds the runs' sums in run order (lamb_cdiv_kernel)
constexpr int LAMB_SEGS = 64;
__global__ __launch_bounds__(256) void lamb_gsum_kernel(LambDev a) {
    __shared__ double sh[4];
    const vk_lamb_group gr = a.groups[blockIdx.y];
    const int per = (gr.piece1 - gr.piece0 + LAMB_SEGS - 1) / LAMB_SEGS;
    const int lo = gr.piece0 + (int)blockIdx.x * per, hi = lo + per < gr.piece1 ? lo + per : gr.piece1;
    double s = 0.0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += 256) s += (double)a.gsq[i];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) a.gpart[(size_t)blockIdx.y * LAMB_SEGS + blockIdx.x] = s;
}

// ONE workgroup: every group's sum, then every group's divisor (with VK_LAMB_GLOBAL_NORM from the sum over all groups, in group order)
__global__ __launch_bounds__(256) void lamb_cdiv_kernel(LambDev a) {
    for (int n = threadIdx.x; n < a.ngroups; n += 256) {
        double S = 0.0;
        for (int k = 0; k < LAMB_SEGS; ++k) S += a.gpart[(size_t)n * LAMB_SEGS + k];
        a.gsum[n] = S;
    }
    __syncthreads();
    double all = 0.0;
    if (a.flags & VK_LAMB_GLOBAL_NORM)
        for (int h = 0; h < a.ngroups; ++h) all += a.gsum[h];
    const float gs = a.grad_scale * (a.clip ? a.clip[1] : 1.f);
    for (int n = threadIdx.x; n < a.ngroups; n += 256) {
        const double S = (a.flags & VK_LAMB_GLOBAL_NORM) ? all : a.gsum[n];
        const float norm = (float)sqrt(S) * fabsf(gs), mx = a.groups[n].max_grad_norm;
        a.cdiv[n] = (mx > 0.f && norm > mx) ? norm / mx : 1.f;
    }
}

__global__ __launch_bounds__(256) void lamb_stage1_kernel(LambDev a) {
    __shared__ float shp[4], shu[4];
    const vk_lamb_piece pc = a.pieces[blockIdx.x];
    const vk_lamb_tensor t = a.tensors[pc.tensor];
    const float wd = a.cls_wd[t.cls], bc1 = a.cls_bc1[t.cls], bc2 = a.cls_bc2[t.cls];
    const bool adam_w = a.flags & VK_LAMB_ADAM_W_MODE;
    const float b3 = (a.flags & VK_LAMB_GRAD_AVERAGING) ? 1.f - a.beta1 : 1.f;
    const float gs = a.grad_scale * (a.clip ? a.clip[1] : 1.f);
    const float c = a.cdiv ? a.cdiv[t.group] : 1.f;
    const float* gp = t.g + pc.offset;
    float *pp = t.p + pc.offset, *mp = t.m + pc.offset, *vp = t.v + pc.offset;
    const int i = threadIdx.x * 4;
    float p[4], u[4];
    if (piece_vec(t, pc) && i + 4 <= pc.count) {
        // g, m and v are one-pass streams of the step: non-temporal, like adamw_kernel, so that they do not displace the bf16 weights
        const f32x4 g = __builtin_nontemporal_load((const f32x4*)(gp + i)), p4 = __builtin_nontemporal_load((const f32x4*)(pp + i));
        f32x4 m = __builtin_nontemporal_load((const f32x4*)(mp + i)), v = __builtin_nontemporal_load((const f32x4*)(vp + i));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float mr = m[r], vr = v[r];
            lamb_moments(mr, vr, g[r], p4[r], gs, c, a.beta1, a.beta2, b3, wd, adam_w);
            m[r] = mr; v[r] = vr; p[r] = p4[r];
            u[r] = lamb_update(mr, vr, p4[r], bc1, bc2, a.eps, wd, adam_w);
        }
        __builtin_nontemporal_store(m, (f32x4*)(mp + i)); __builtin_nontemporal_store(v, (f32x4*)(vp + i));
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            p[r] = u[r] = 0.f;
            if (i + r < pc.count) {
                float mr = mp[i + r], vr = vp[i + r];
                p[r] = pp[i + r];
                lamb_moments(mr, vr, gp[i + r], p[r], gs, c, a.beta1, a.beta2, b3, wd, adam_w);
                mp[i + r] = mr; vp[i + r] = vr;
                u[r] = lamb_update(mr, vr, p[r], bc1, bc2, a.eps, wd, adam_w);
            }
        }
    }
    float sp, su;
    {
#pragma clang fp contract(off)
        sp = ((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]) + p[3] * p[3];
        su = ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) + u[3] * u[3];
    }
    sp = block_sum(sp, shp);
    su = block_sum(su, shu);
    if (threadIdx.x == 0) { a.psq[blockIdx.x] = sp; a.usq[blockIdx.x] = su; }
}

__global__ __launch_bounds__(256) void lamb_finish_kernel(LambDev a) {
    __shared__ double shp[4], shu[4];
    const vk_lamb_tensor t = a.tensors[blockIdx.x];
    double P = 0.0, Uu = 0.0;
    for (int i = t.piece0 + (int)threadIdx.x; i < t.piece0 + t.npieces; i += 256) { P += (double)a.psq[i]; Uu += (double)a.usq[i]; }
    P = block_sum(P, shp);
    Uu = block_sum(Uu, shu);
    if (threadIdx.x == 0) {
        const float pn = (float)sqrt(P), un = (float)sqrt(Uu), lr = a.cls_lr[t.cls];
        const bool both = pn != 0.f && un != 0.f;
        const float trust = both ? pn / un : 1.f;
        float* o = a.table + (size_t)blockIdx.x * 4;
        o[0] = both ? lr * trust : lr; o[1] = trust; o[2] = pn; o[3] = un;
    }
}

__global__ __launch_bounds__(256) void lamb_stage2_kernel(LambDev a) {
    const vk_lamb_piece pc = a.pieces[blockIdx.x];
    const vk_lamb_tensor t = a.tensors[pc.tensor];
    const float wd = a.cls_wd[t.cls], bc1 = a.cls_bc1[t.cls], bc2 = a.cls_bc2[t.cls];
    const bool adam_w = a.flags & VK_LAMB_ADAM_W_MODE;
    const float ratio = a.table[(size_t)pc.tensor * 4];
    float* pp = t.p + pc.offset;
    const float *mp = t.m + pc.offset, *vp = t.v + pc.offset;
    uint16_t* sp = t.shadow ? (uint16_t*)t.shadow + pc.offset : nullptr;
    const int i = threadIdx.x * 4;
    if (piece_vec(t, pc) && i + 4 <= pc.count) {
        f32x4 p = __builtin_nontemporal_load((const f32x4*)(pp + i));
        const f32x4 m = __builtin_nontemporal_load((const f32x4*)(mp + i)), v = __builtin_nontemporal_load((const f32x4*)(vp + i));
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] = __builtin_fmaf(-ratio, lamb_update(m[r], v[r], p[r], bc1, bc2, a.eps, wd, adam_w), p[r]);
        __builtin_nontemporal_store(p, (f32x4*)(pp + i));
        if (sp) *(u32x2*)(sp + i) = u32x2{pack2bf(p[0], p[1]), pack2bf(p[2], p[3])};      // what the next forward reads: a plain store
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (i + r < pc.count) {
                const float p0 = pp[i + r];
                const float p1 = __builtin_fmaf(-ratio, lamb_update(mp[i + r], vp[i + r], p0, bc1, bc2, a.eps, wd, adam_w), p0);
                pp[i + r] = p1;
                if (sp) sp[i + r] = f2bf(p1);
            }
        }
    }
}

// The host tables: every rule of the header.  *clips: some group has max_grad_norm > 0.
static int check_tables(const char* who, const vk_lamb_tensor* T, int nt, const vk_lamb_piece* P, int np, const vk_lamb_group* G, int ng, bool* clips) {
    if (nt < 0 || np < 0 || ng < 1 || ng > 65535) return set_error("%s: %d tensors, %d pieces, %d groups (1 .. 65535)", who, nt, np, ng);
    if ((nt && !T) || (np && !P) || !G) return set_error("%s: a table is missing", who);
    *clips = false;
    int next = 0;
    for (int n = 0; n < ng; ++n) {
        if (G[n].piece0 != next || G[n].piece1 < G[n].piece0 || G[n].piece1 > np)
            return set_error("%s: group %d covers pieces [%d, %d): the groups' ranges must follow each other from 0 to %d", who, n, G[n].piece0, G[n].piece1, np);
        next = G[n].piece1;
        if (G[n].max_grad_norm > 0.f) *clips = true;
    }
    if (next != np) return set_error("%s: the groups cover %d of %d pieces", who, next, np);
    next = 0;
    int group = 0;
    for (int t = 0; t < nt; ++t) {
        const vk_lamb_tensor& d = T[t];
        if (d.numel < 0) return set_error("%s: tensor %d has numel %lld", who, t, (long long)d.numel);
        if (!d.p || !d.g || !d.m || !d.v || (((uintptr_t)d.p | (uintptr_t)d.g | (uintptr_t)d.m | (uintptr_t)d.v) & 3) || ((uintptr_t)d.shadow & 1))
            return set_error("%s: tensor %d: p / g / m / v are required and need 4-byte, shadow 2-byte alignment", who, t);
        if (d.cls < 0 || d.cls >= VK_LAMB_CLASSES) return set_error("%s: tensor %d: class %d", who, t, d.cls);
        if (d.group < group || d.group >= ng) return set_error("%s: tensor %d: group %d (groups ascend, %d of them)", who, t, d.group, ng);
        group = d.group;
        if (d.piece0 != next || d.npieces < 0 || d.npieces > np - next)
            return set_error("%s: tensor %d: pieces [%d, +%d) do not follow the previous tensor's (%d of %d)", who, t, d.piece0, d.npieces, next, np);
        if (d.piece0 < G[group].piece0 || d.piece0 + d.npieces > G[group].piece1)
            return set_error("%s: tensor %d: its pieces lie outside its group's range", who, t);
        int64_t at = 0;
        for (int i = next; i < next + d.npieces; ++i) {
            if (P[i].tensor != t) return set_error("%s: piece %d belongs to tensor %d, expected %d", who, i, P[i].tensor, t);
            if (P[i].count < 1 || P[i].count > VK_LAMB_PIECE) return set_error("%s: piece %d: count %d (1 .. %d)", who, i, P[i].count, VK_LAMB_PIECE);
            if (P[i].offset != at) return set_error("%s: piece %d starts at element %lld, expected %lld (pieces tile their tensor in order)", who, i, (long long)P[i].offset, (long long)at);
            if (P[i].count > d.numel - at) return set_error("%s: piece %d ends past its tensor (%lld + %d > %lld)", who, i, (long long)at, P[i].count, (long long)d.numel);
            at += P[i].count;
        }
        if (at != d.numel) return set_error("%s: tensor %d: its pieces cover %lld of %lld elements", who, t, (long long)at, (long long)d.numel);
        next += d.npieces;
    }
    if (next != np) return set_error("%s: the tensors own %d of %d pieces", who, next, np);
    return 0;
}

static int64_t work_bytes(int np, int ng) { return 8 * (int64_t)ng * (LAMB_SEGS + 1) + 4 * (3 * (int64_t)np + ng); }

}  // namespace vk

using namespace vk;

extern "C" int64_t vk_lamb_work_bytes(const vk_lamb_tensor* tensors, int ntensors, const vk_lamb_piece* pieces, int npieces, const vk_lamb_group* groups, int ngroups) {
    bool clips;
    if (check_tables("vk_lamb_work_bytes", tensors, ntensors, pieces, npieces, groups, ngroups, &clips)) return -1;
    return work_bytes(npieces, ngroups);
}

// ev: NULL, or 7 events recorded around the six launches (a launch that is left out leaves an empty interval)
static int lamb_run(const vk_lamb_args* a, vk_stream_t s, hipEvent_t* ev, const char* who) {
    if (!a) return set_error("%s: no arguments", who);
    if (!(a->beta1 >= 0.f && a->beta1 < 1.f && a->beta2 >= 0.f && a->beta2 < 1.f && a->eps >= 0.f))
        return set_error("%s: betas (%g, %g) must lie in [0, 1), eps (%g) must be >= 0", who, (double)a->beta1, (double)a->beta2, (double)a->eps);
    bool clips;
    if (int rc = check_tables(who, a->tensors, a->ntensors, a->pieces, a->npieces, a->groups, a->ngroups, &clips)) return rc;
    if (a->ntensors == 0) return ev ? set_error("%s: nothing to time", who) : 0;
    if (!a->d_tensors || (a->npieces && !a->d_pieces) || !a->d_groups || !a->table) return set_error("%s: the device tables and the ratio table are required", who);
    if (!a->work || ((uintptr_t)a->work & 7) || a->work_bytes < work_bytes(a->npieces, a->ngroups))
        return set_error("%s: work needs 8-byte alignment and %lld bytes (got %lld)", who, (long long)work_bytes(a->npieces, a->ngroups), (long long)a->work_bytes);
    LambDev d;
    d.tensors = a->d_tensors; d.pieces = a->d_pieces; d.groups = a->d_groups;
    d.gpart = (double*)a->work;
    d.gsum = d.gpart + (size_t)a->ngroups * LAMB_SEGS;
    d.gsq = (float*)(d.gsum + a->ngroups);
    d.psq = d.gsq + a->npieces;
    d.usq = d.psq + a->npieces;
    d.cdiv = clips ? d.usq + a->npieces : nullptr;
    d.table = a->table; d.clip = a->clip;
    d.ntensors = a->ntensors; d.npieces = a->npieces; d.ngroups = a->ngroups; d.flags = a->flags;
    for (int k = 0; k < VK_LAMB_CLASSES; ++k) { d.cls_lr[k] = a->cls_lr[k]; d.cls_wd[k] = a->cls_wd[k]; d.cls_bc1[k] = a->cls_bc1[k]; d.cls_bc2[k] = a->cls_bc2[k]; }
    d.beta1 = a->beta1; d.beta2 = a->beta2; d.eps = a->eps; d.grad_scale = a->grad_scale;
    hipStream_t st = (hipStream_t)s;
    const dim3 np((unsigned)a->npieces), wg(256);
    const bool norm = a->npieces && clips;
    int e = 0;
    auto mark = [&]() { if (ev) (void)hipEventRecord(ev[e++], st); };
    mark();
    if (norm) hipLaunchKernelGGL(lamb_gsq_kernel, np, wg, 0, st, d);
    mark();
    if (norm) hipLaunchKernelGGL(lamb_gsum_kernel, dim3(LAMB_SEGS, (unsigned)a->ngroups), wg, 0, st, d);
    mark();
    if (norm) hipLaunchKernelGGL(lamb_cdiv_kernel, dim3(1), wg, 0, st, d);
    mark();
    if (a->npieces) hipLaunchKernelGGL(lamb_stage1_kernel, np, wg, 0, st, d);
    mark();
    hipLaunchKernelGGL(lamb_finish_kernel, dim3((unsigned)a->ntensors), wg, 0, st, d);
    mark();
    if (a->npieces) hipLaunchKernelGGL(lamb_stage2_kernel, np, wg, 0, st, d);
    mark();
    return check_launch(who);
}

extern "C" int vk_lamb_step(const vk_lamb_args* a, vk_stream_t s) { return lamb_run(a, s, nullptr, "vk_lamb_step"); }

extern "C" int vk_lamb_step_timed(const vk_lamb_args* a, vk_stream_t s, float* ms) {
    if (!ms) return set_error("vk_lamb_step_timed: no output");
    hipEvent_t ev[7];
    for (auto& x : ev)
        if (hipEventCreate(&x) != hipSuccess) return set_error("vk_lamb_step_timed: hipEventCreate failed");
    int rc = lamb_run(a, s, ev, "vk_lamb_step_timed");
    if (!rc && hipEventSynchronize(ev[6]) != hipSuccess) rc = set_error("vk_lamb_step_timed: hipEventSynchronize failed");
    for (int i = 0; i < 6 && !rc; ++i)
        if (hipEventElapsedTime(ms + i, ev[i], ev[i + 1]) != hipSuccess) rc = set_error("vk_lamb_step_timed: hipEventElapsedTime failed");
    for (auto& x : ev) (void)hipEventDestroy(x);
    return rc;
}
