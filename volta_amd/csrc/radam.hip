// Fused RAdam over the flat fp32 arenas (volta/optimization.py:9-93 RAdam.step, :96-169 PlainRAdam.step; train_task.py:227-228):
// the reference's per-parameter Python loop as ONE HBM-bound launch over (p, g, m, v) that also refreshes the bf16 shadow copy of the
// weights, like adamw_kernel (optim.hip).  The step sizes, the rectification switch and the decay factor are host-side numbers: the
// reference's shared `buffer` bookkeeping (volta_amd/optimization.py, radam_plan) decides them per (group lr, weight decay, step count)
// class, and the kernel looks them up by the chunk's class byte.
#include "common.h"
#include "../../include/volta_hip.h"
#include "util.h"

namespace vk {

// One element, volta/optimization.py:48-91 in fp32, spelled with explicit fused multiply-adds and no further contraction (the arena and
// list kernels give the same bits for equal inputs):
//   v = b2 v + (1-b2) g g ; m = b1 m + (1-b1) g ; p -= decay p ; p -= step m / (sqrt(v) + eps)  (rectified) | p -= step m  (not)
// The (1 - beta) factors come from the host, rounded from double as the reference's `addcmul_(1 - beta2, ...)` / `add_(1 - beta1, ...)`
// round them: 1 - fp32(0.999) is 1.3e-5 away from fp32(0.001) relative.
__device__ __forceinline__ void radam_element(float& p, float& m, float& v, float g, const vk_radam_args& a, float decay, float step, bool rect, float gs) {
#pragma clang fp contract(off)
    const float gr = g * gs;
    v = __builtin_fmaf(a.beta2, v, (a.one_minus_beta2 * gr) * gr);
    m = __builtin_fmaf(a.beta1, m, a.one_minus_beta1 * gr);
    if (decay != 0.f) p = __builtin_fmaf(-decay, p, p);
    p = rect ? __builtin_fmaf(-step, m / (sqrtf(v) + a.eps), p) : __builtin_fmaf(-step, m, p);
}

__global__ __launch_bounds__(256) void radam_kernel(vk_radam_args a) {
    const size_t chunk = blockIdx.x;
    const int cls = a.chunk_class ? a.chunk_class[chunk] : 0;
    if (cls >= VK_RADAM_CLASSES) return;     // VK_CHUNK_SKIP (frozen / gradient-less parameters): weights, moments and the bf16 copy stay
    const float decay = a.cls_decay[cls], step = a.cls_step[cls];
    const bool rect = a.cls_rect[cls] != 0;
    const float gs = a.grad_scale * (a.clip ? a.clip[1] : 1.f);
    const size_t i = chunk * 1024 + threadIdx.x * 4;
    // one pass over 7 GB that nothing reads again before the next step's optimizer: non-temporal, as in adamw_kernel (the bf16 copies
    // are what the next forward reads)
    const f32x4 g = __builtin_nontemporal_load((const f32x4*)(a.g + i));
    f32x4 p = __builtin_nontemporal_load((const f32x4*)(a.p + i)), m = __builtin_nontemporal_load((const f32x4*)(a.m + i)), v = __builtin_nontemporal_load((const f32x4*)(a.v + i));
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float pr = p[r], mr = m[r], vr = v[r];
        radam_element(pr, mr, vr, g[r], a, decay, step, rect, gs);
        p[r] = pr; m[r] = mr; v[r] = vr;
    }
    __builtin_nontemporal_store(p, (f32x4*)(a.p + i)); __builtin_nontemporal_store(m, (f32x4*)(a.m + i)); __builtin_nontemporal_store(v, (f32x4*)(a.v + i));
    if (a.shadow) *(u32x2*)((uint16_t*)a.shadow + i) = u32x2{pack2bf(p[0], p[1]), pack2bf(p[2], p[3])};
}

// Tensors outside the arena: blockIdx.y = descriptor, blockIdx.x strides over its elements, four per thread (16-byte accesses where the
// tensor's four pointers allow it, element by element at a ragged end).  No bf16 copy to refresh.
__global__ __launch_bounds__(256) void radam_list_kernel(vk_radam_args a, const vk_adamw_tensor* list) {
    const vk_adamw_tensor t = list[blockIdx.y];
    if (t.cls < 0 || t.cls >= VK_RADAM_CLASSES) return;
    const float decay = a.cls_decay[t.cls], step = a.cls_step[t.cls];
    const bool rect = a.cls_rect[t.cls] != 0;
    const float gs = a.grad_scale * (a.clip ? a.clip[1] : 1.f);
    const bool vec = !(((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v) & 15);
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < t.numel; i += (int64_t)gridDim.x * 1024) {
        if (vec && i + 4 <= t.numel) {
            const f32x4 g = *(const f32x4*)(t.g + i);
            f32x4 p = *(const f32x4*)(t.p + i), m = *(const f32x4*)(t.m + i), v = *(const f32x4*)(t.v + i);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float pr = p[r], mr = m[r], vr = v[r];
                radam_element(pr, mr, vr, g[r], a, decay, step, rect, gs);
                p[r] = pr; m[r] = mr; v[r] = vr;
            }
            *(f32x4*)(t.p + i) = p; *(f32x4*)(t.m + i) = m; *(f32x4*)(t.v + i) = v;
        } else {
            for (int64_t k = i; k < i + 4 && k < t.numel; ++k) {
                float pr = t.p[k], mr = t.m[k], vr = t.v[k];
                radam_element(pr, mr, vr, t.g[k], a, decay, step, rect, gs);
                t.p[k] = pr; t.m[k] = mr; t.v[k] = vr;
            }
        }
    }
}

static int check_args(const vk_radam_args* a, const char* who) {
    if (!a) return set_error("%s: no arguments", who);
    if (!(a->beta1 >= 0.f && a->beta1 < 1.f && a->beta2 >= 0.f && a->beta2 < 1.f && a->eps >= 0.f && a->one_minus_beta1 > 0.f && a->one_minus_beta1 <= 1.f &&
          a->one_minus_beta2 > 0.f && a->one_minus_beta2 <= 1.f))
        return set_error("%s: betas (%g, %g) must lie in [0, 1), their complements in (0, 1], eps (%g) must be >= 0", who, (double)a->beta1,
                         (double)a->beta2, (double)a->eps);
    return 0;
}

}  // namespace vk

using namespace vk;

extern "C" int vk_radam_step(const vk_radam_args* a, vk_stream_t s) {
    if (int rc = check_args(a, "vk_radam_step")) return rc;
    if (a->n < 0 || a->n % 1024) return set_error("vk_radam_step: arena length %lld must be a non-negative multiple of 1024 elements", (long long)a->n);
    if (a->n == 0) return 0;
    if (!a->p || !a->g || !a->m || !a->v) return set_error("vk_radam_step: p, g, m and v are required");
    if ((((uintptr_t)a->p | (uintptr_t)a->g | (uintptr_t)a->m | (uintptr_t)a->v) & 15) || ((uintptr_t)a->shadow & 7))
        return set_error("vk_radam_step: p / g / m / v need 16-byte and shadow 8-byte alignment");
    hipLaunchKernelGGL(radam_kernel, dim3((unsigned)(a->n / 1024)), dim3(256), 0, (hipStream_t)s, *a);
    return check_launch("vk_radam_step");
}

extern "C" int vk_radam_step_list(const vk_radam_args* a, const vk_adamw_tensor* list, int n, int64_t max_numel, vk_stream_t s) {
    if (int rc = check_args(a, "vk_radam_step_list")) return rc;
    if (n < 0 || n > 65535 || max_numel < 0) return set_error("vk_radam_step_list: %d tensors, max numel %lld", n, (long long)max_numel);
    if (n == 0 || max_numel == 0) return 0;
    if (!list) return set_error("vk_radam_step_list: no descriptor list");
    int64_t b = (max_numel + 1023) / 1024;
    b = b < 1 ? 1 : b > 1024 ? 1024 : b;
    hipLaunchKernelGGL(radam_list_kernel, dim3((unsigned)b, (unsigned)n), dim3(256), 0, (hipStream_t)s, *a, list);
    return check_launch("vk_radam_step_list");
}
