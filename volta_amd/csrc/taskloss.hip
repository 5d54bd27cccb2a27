// Loss, score and arg-max of the fine-tuning step, read in place from the engine's fp32 logits (volta/task_utils.py:140-281,429-434):
//   * BCE-with-logits over [rows, C] label scores (VQA, GQA: x C; NLVR2, SNLI-VE: plain mean), score = target at the row's arg-max
//   * BCE-with-logits over the regions of an image (RefCOCO*), the logit in column 0 of every region row, padded regions at -10000
//   * cross-entropy over the options of a sample (retrieval, multiple choice), the logit in column 0 of every option row
// Forward: one launch writes one (loss, score, arg-max) per group, a second one-workgroup launch sums the groups in a fixed order --
// the result is the same bits on every run (no floating-point atomics, no hand-off inside a launch).  Per-element terms are fp32 with the
// accurate expf / log1pf; they are ACCUMULATED in double, so the sum is the correctly rounded sum of those terms whatever the order.
// Backward: d loss / d logits x the incoming gradient (a device scalar), fp32, rounded once to bf16, pad columns written as zero.
// Wide groups (n > 64) take one 256-thread workgroup each, narrow ones one wave each (four per workgroup).
#include "common.h"
#include "../../include/volta_hip.h"
#include "util.h"

namespace vk {

enum { TL_ROWS = 0, TL_REGIONS = 1, TL_OPTIONS = 2 };      // how a group is laid out: along a logits row | column 0 of n rows (BCE | CE)

struct TlMax { float v; int i; };
__device__ __forceinline__ TlMax tl_better(TlMax a, TlMax b) {      // the larger value; among equals the smaller index
    return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
template <int TPG>
__device__ __forceinline__ TlMax tl_group_max(TlMax m, TlMax* sh) {
#pragma unroll
    for (int o = 32; o; o >>= 1) m = tl_better(m, TlMax{__shfl_xor(m.v, o), __shfl_xor(m.i, o)});
    if (TPG == 256) {
        __syncthreads();
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
        __syncthreads();
        m = tl_better(tl_better(sh[0], sh[1]), tl_better(sh[2], sh[3]));
    }
    return m;
}
template <int TPG>
__device__ __forceinline__ double tl_group_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    if (TPG == 256) {
        __syncthreads();
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
        __syncthreads();
        v = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    }
    return v;
}

__device__ __forceinline__ float tl_bce(float x, float t) {        // max(x, 0) - x t + log(1 + exp(-|x|))
    return __builtin_fmaf(-x, t, fmaxf(x, 0.f)) + log1pf(expf(-fabsf(x)));
}
// sigmoid(x) - t without the cancellation of 1 - 1: ((1 - t) - t e) / (1 + e) for x >= 0, (e (1 - t) - t) / (1 + e) for x < 0, e = exp(-|x|).
// Where a soft target meets its own sigmoid the fp32 difference keeps too few bits for the bf16 result: that rare element is redone in double.
__device__ __forceinline__ float tl_bce_grad(float x, float t) {
    const float e = expf(-fabsf(x)), u = 1.f - t;
    const float num = x >= 0.f ? __builtin_fmaf(-t, e, u) : __builtin_fmaf(e, u, -t);
    float d = num / (1.f + e);
    if (fabsf(d) < 0x1p-10f && t > 0.f && t < 1.f) d = (float)(1.0 / (1.0 + exp(-(double)x)) - (double)t);
    return d;
}
__device__ __forceinline__ float tl_region_logit(const vk_task_loss_args& a, size_t r) {
    const float x = a.logits[r * (size_t)a.ld];
    return a.mask ? x + (1.f - (float)a.mask[r]) * -10000.f : x;
}

// One group per TPG threads.  work = double loss[groups] followed by float score[groups].
template <int LAYOUT, int TPG>
__global__ __launch_bounds__(256) void task_loss_fwd_kernel(vk_task_loss_args a) {
    __shared__ TlMax sh_m[4];
    __shared__ double sh_d[4];
    const int g = blockIdx.x * (256 / TPG) + (int)threadIdx.x / TPG, t = (int)threadIdx.x % TPG;
    if (g >= a.groups) return;                 // a whole workgroup (TPG 256) or a whole wave (TPG 64, which never meets a barrier)
    const int n = a.n;
    double acc = 0.0;
    TlMax m = {-INFINITY, 0x7fffffff};
    const float* tg = (const float*)a.target + (size_t)g * n;
    if (LAYOUT == TL_ROWS) {
        const float* x = a.logits + (size_t)g * a.ld;
        if (TPG == 256) {                      // rows are 256-byte aligned (ld is a multiple of 64): one float4 per lane; columns >= n are not used
            for (int j = t * 4; j < n; j += 1024) {
                const f32x4 xv = *(const f32x4*)(x + j);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (j + k < n) {
                        acc += (double)tl_bce(xv[k], tg[j + k]);
                        if (xv[k] > m.v) m = TlMax{xv[k], j + k};
                    }
            }
        } else if (t < n) {
            acc = (double)tl_bce(x[t], tg[t]);
            m = TlMax{x[t], t};
        }
    } else {
        for (int j = t; j < n; j += TPG) {
            const size_t r = (size_t)g * n + j;
            const float x = LAYOUT == TL_REGIONS ? tl_region_logit(a, r) : a.logits[r * (size_t)a.ld];
            if (LAYOUT == TL_REGIONS) acc += (double)tl_bce(x, tg[j]);
            if (x > m.v) m = TlMax{x, j};
        }
    }
    m = tl_group_max<TPG>(m, sh_m);
    if (m.i >= n) m.i = 0;                     // a group without a comparable value (all NaN): keep every later index in range
    double* wl = (double*)a.work;
    float* ws = (float*)(wl + a.groups);
    if (LAYOUT == TL_OPTIONS) {
        for (int j = t; j < n; j += TPG) acc += (double)expf(a.logits[((size_t)g * n + j) * (size_t)a.ld] - m.v);
        acc = tl_group_sum<TPG>(acc, sh_d);
        if (t == 0) {
            int64_t lab = ((const int64_t*)a.target)[g];
            lab = lab < 0 ? 0 : (lab >= n ? n - 1 : lab);
            wl[g] = ((double)m.v - (double)a.logits[((size_t)g * n + lab) * (size_t)a.ld]) + log(acc);
            ws[g] = m.i == (int)lab ? 1.f : 0.f;
            a.row_argmax[g] = m.i;
        }
    } else {
        acc = tl_group_sum<TPG>(acc, sh_d);
        if (t == 0) {
            wl[g] = acc;
            ws[g] = LAYOUT == TL_ROWS ? tg[m.i] : (tg[m.i] > 0.5f ? 1.f : 0.f);
            a.row_argmax[g] = m.i;
        }
    }
}

// out[0] = sum_g loss[g] / divisor (x n where the reference scales the mean back up), out[1] = sum_g score[g]: one workgroup, fixed order
__global__ __launch_bounds__(256) void task_loss_final_kernel(vk_task_loss_args a) {
    __shared__ double sl[256], ss[256];
    const double* wl = (const double*)a.work;
    const float* ws = (const float*)(wl + a.groups);
    double l = 0.0, s = 0.0;
    for (int g = threadIdx.x; g < a.groups; g += 256) { l += wl[g]; s += (double)ws[g]; }
    sl[threadIdx.x] = l;
    ss[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o; o >>= 1) {
        if ((int)threadIdx.x < o) { sl[threadIdx.x] += sl[threadIdx.x + o]; ss[threadIdx.x] += ss[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double div = a.kind == VK_TASK_BCE_MEAN ? (double)a.groups * (double)a.n : (double)a.groups;
        a.out[0] = (float)(sl[0] / div);
        a.out[1] = (float)ss[0];
    }
}

// BCE backward is element-wise: one thread per four columns of dlogits.  TL_ROWS: columns < n carry a gradient; TL_REGIONS: column 0 does.
template <int LAYOUT>
__global__ __launch_bounds__(256) void task_bce_bwd_kernel(vk_task_loss_args a, const float* gscale, uint16_t* dlogits, int rows) {
    const int q = a.ld >> 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)rows * q) return;
    const int r = (int)(idx / q), c = (int)(idx - (int64_t)r * q) * 4;
    const float coef = *gscale / (a.kind == VK_TASK_BCE_MEAN ? (float)a.groups * (float)a.n : (float)a.groups);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (LAYOUT == TL_ROWS) {
        if (c < a.n) {
            const f32x4 xv = *(const f32x4*)(a.logits + (size_t)r * a.ld + c);
            const float* tg = (const float*)a.target + (size_t)r * a.n;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c + k < a.n) v[k] = tl_bce_grad(xv[k], tg[c + k]) * coef;
        }
    } else if (c == 0) {
        v[0] = tl_bce_grad(tl_region_logit(a, (size_t)r), ((const float*)a.target)[r]) * coef;
    }
    u32x2 o = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
    *(u32x2*)(dlogits + (size_t)r * a.ld + c) = o;
}

// d/dx_j of mean_g (lse - x[target]) = (softmax_j - [j == target]) / groups; at the target it is -(sum of the OTHER exponentials) / sum, which
// keeps its bits when the target dominates.  The thread of option j writes that option's whole dlogits row (column 0, then zeros).
template <int TPG>
__global__ __launch_bounds__(256) void task_ce_bwd_kernel(vk_task_loss_args a, const float* gscale, uint16_t* dlogits) {
    __shared__ TlMax sh_m[4];
    __shared__ double sh_d[4];
    const int g = blockIdx.x * (256 / TPG) + (int)threadIdx.x / TPG, t = (int)threadIdx.x % TPG;
    if (g >= a.groups) return;
    const int n = a.n;
    int64_t lab64 = ((const int64_t*)a.target)[g];
    const int lab = (int)(lab64 < 0 ? 0 : (lab64 >= n ? n - 1 : lab64));
    TlMax m = {-INFINITY, 0x7fffffff};
    for (int j = t; j < n; j += TPG) {
        const float x = a.logits[((size_t)g * n + j) * (size_t)a.ld];
        if (x > m.v) m = TlMax{x, j};
    }
    m = tl_group_max<TPG>(m, sh_m);
    double all = 0.0, others = 0.0;
    for (int j = t; j < n; j += TPG) {
        const double e = (double)expf(a.logits[((size_t)g * n + j) * (size_t)a.ld] - m.v);
        all += e;
        if (j != lab) others += e;
    }
    all = tl_group_sum<TPG>(all, sh_d);
    others = tl_group_sum<TPG>(others, sh_d);
    const float coef = *gscale / (float)a.groups;
    for (int j = t; j < n; j += TPG) {
        const size_t r = (size_t)g * n + j;
        const float p = j == lab ? -(float)(others / all) : (float)((double)expf(a.logits[r * (size_t)a.ld] - m.v) / all);
        uint16_t* d = dlogits + r * (size_t)a.ld;
        const u32x4 z = {0u, 0u, 0u, 0u};
        for (int c = 0; c < a.ld; c += 8) *(u32x4*)(d + c) = z;
        d[0] = f2bf(p * coef);
    }
}

}  // namespace vk

using namespace vk;

static int check_task(const vk_task_loss_args* a, const char* who) {
    if (!a) return set_error("%s: null arguments", who);
    if (a->kind < VK_TASK_BCE_SCALED || a->kind > VK_TASK_CE_OPTIONS) return set_error("%s: unknown kind %d", who, a->kind);
    if (!a->logits || !a->target) return set_error("%s: missing logits / target", who);
    if (a->groups <= 0 || a->n <= 0) return set_error("%s: groups %d and n %d must be positive", who, a->groups, a->n);
    if (a->ld <= 0 || a->ld % 64) return set_error("%s: ld %d must be a positive multiple of 64", who, a->ld);
    if (a->kind <= VK_TASK_BCE_MEAN && a->n > a->ld) return set_error("%s: n %d exceeds ld %d", who, a->n, a->ld);
    if ((int64_t)a->groups * a->n > 0x7fffffffLL) return set_error("%s: groups x n overflows", who);
    return 0;
}

extern "C" int64_t vk_task_loss_work_bytes(int groups) { return groups > 0 ? (int64_t)groups * 12 + 4 : 0; }

template <int LAYOUT>
static void launch_task_fwd(const vk_task_loss_args* a, hipStream_t st) {
    if (a->n > 64) hipLaunchKernelGGL((task_loss_fwd_kernel<LAYOUT, 256>), dim3(a->groups), dim3(256), 0, st, *a);
    else hipLaunchKernelGGL((task_loss_fwd_kernel<LAYOUT, 64>), dim3((a->groups + 3) / 4), dim3(256), 0, st, *a);
}

extern "C" int vk_task_loss_fwd(const vk_task_loss_args* a, vk_stream_t s) {
    if (check_task(a, "vk_task_loss_fwd")) return -1;
    if (!a->work || !a->out || !a->row_argmax) return set_error("vk_task_loss_fwd: missing work / out / row_argmax");
    hipStream_t st = (hipStream_t)s;
    switch (a->kind) {
        case VK_TASK_BCE_REGIONS: launch_task_fwd<TL_REGIONS>(a, st); break;
        case VK_TASK_CE_OPTIONS: launch_task_fwd<TL_OPTIONS>(a, st); break;
        default: launch_task_fwd<TL_ROWS>(a, st); break;
    }
    if (check_launch("vk_task_loss_fwd")) return -1;
    hipLaunchKernelGGL(task_loss_final_kernel, dim3(1), dim3(256), 0, st, *a);
    return check_launch("vk_task_loss_fwd (final sum)");
}

extern "C" int vk_task_loss_bwd(const vk_task_loss_args* a, const float* gscale, void* dlogits, vk_stream_t s) {
    if (check_task(a, "vk_task_loss_bwd")) return -1;
    if (!gscale || !dlogits) return set_error("vk_task_loss_bwd: missing gscale / dlogits");
    hipStream_t st = (hipStream_t)s;
    uint16_t* d = (uint16_t*)dlogits;
    if (a->kind == VK_TASK_CE_OPTIONS) {
        if (a->n > 64) hipLaunchKernelGGL((task_ce_bwd_kernel<256>), dim3(a->groups), dim3(256), 0, st, *a, gscale, d);
        else hipLaunchKernelGGL((task_ce_bwd_kernel<64>), dim3((a->groups + 3) / 4), dim3(256), 0, st, *a, gscale, d);
    } else {
        const int rows = a->kind == VK_TASK_BCE_REGIONS ? a->groups * a->n : a->groups;
        const int64_t threads = (int64_t)rows * (a->ld / 4);
        const dim3 grid((unsigned)((threads + 255) / 256));
        if (a->kind == VK_TASK_BCE_REGIONS) hipLaunchKernelGGL((task_bce_bwd_kernel<TL_REGIONS>), grid, dim3(256), 0, st, *a, gscale, d, rows);
        else hipLaunchKernelGGL((task_bce_bwd_kernel<TL_ROWS>), grid, dim3(256), 0, st, *a, gscale, d, rows);
    }
    return check_launch("vk_task_loss_bwd");
}
