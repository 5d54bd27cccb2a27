// Gradient seeds of the standalone BertModel (volta_amd/modeling.py): the hidden states and pooled vectors leave the engine as fp32 torch
// tensors, and their gradients re-enter it here, written or added into the engine's bf16 [rows, H] gradient buffers.  Memory-bound: eight
// elements per thread (two 16-byte loads, one 16-byte store), grid-stride.
#include "common.h"
#include "../../include/volta_hip.h"
#include "util.h"

namespace vk {

__global__ __launch_bounds__(256) void grad_seed_kernel(const vk_grad_seed_args a) {
    const int64_t per_row = a.H / 8, total = (int64_t)a.B * a.L * per_row;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / per_row;
        const int h = (int)(i - r * per_row) * 8;
        const int64_t b = r / a.L, l = r - b * a.L;
        float x[8];
        if (a.src) {
            const float* s = a.src + b * a.stride_b + l * a.stride_l + h;
            const f32x4 lo = *(const f32x4*)s, hi = *(const f32x4*)(s + 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) { x[k] = lo[k]; x[k + 4] = hi[k]; }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) x[k] = 0.f;
        }
        if (a.y) {
            const u32x4 yv = *(const u32x4*)((const uint16_t*)a.y + r * a.ldy + h);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!(bf2f((uint16_t)(yv[k] & 0xFFFFu)) > 0.f)) x[2 * k] = 0.f;
                if (!(bf2f((uint16_t)(yv[k] >> 16)) > 0.f)) x[2 * k + 1] = 0.f;
            }
        }
        uint16_t* d = (uint16_t*)a.dst + (a.row0 + r) * a.ld + h;
        if (a.accumulate) {
            const u32x4 dv = *(const u32x4*)d;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                x[2 * k] += bf2f((uint16_t)(dv[k] & 0xFFFFu));
                x[2 * k + 1] += bf2f((uint16_t)(dv[k] >> 16));
            }
        }
        *(u32x4*)d = u32x4{pack2bf(x[0], x[1]), pack2bf(x[2], x[3]), pack2bf(x[4], x[5]), pack2bf(x[6], x[7])};
    }
}

}  // namespace vk

using namespace vk;

extern "C" int vk_grad_seed(const vk_grad_seed_args* a, vk_stream_t s) {
    if (a->B <= 0 || a->L <= 0 || a->H <= 0) return set_error("vk_grad_seed: empty shape %d x %d x %d", a->B, a->L, a->H);
    if (a->H % 8 || a->ld % 8 || a->row0 < 0 || a->ld < a->H || (a->y && (a->ldy % 8 || a->ldy < a->H)))
        return set_error("vk_grad_seed: H, ld and ldy must be multiples of 8 (H %d, ld %d, ldy %d)", a->H, a->ld, a->ldy);
    if (!a->dst || ((uintptr_t)a->dst & 15) || ((uintptr_t)a->y & 15)) return set_error("vk_grad_seed: dst and y need 16-byte alignment");
    if (!a->src && a->accumulate) return 0;                 // an absent gradient adds nothing
    if (a->src && (((uintptr_t)a->src & 15) || (a->stride_b & 3) || (a->stride_l & 3)))
        return set_error("vk_grad_seed: src needs 16-byte alignment and strides that are multiples of 4 (copy it contiguous)");
    const int64_t total = (int64_t)a->B * a->L * (a->H / 8);
    int64_t blocks = (total + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(grad_seed_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, *a);
    return check_launch("vk_grad_seed");
}
