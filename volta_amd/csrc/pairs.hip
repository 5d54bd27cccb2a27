// Pair gather of the retrieval scorer (volta_amd/retrieval.py).  The caption and image prefixes are computed once per item; this kernel
// builds the per-pair inputs of the mixing suffix from them: for every pair and every segment, one row block of the pair's caption or
// image is copied into the pair's slot.  Memory-bound and read-heavy on a few rows: a caption block is read ni times within one launch and
// the image blocks of a chunk are read again by the next caption's launch, and the suffix's first GEMM reads what is written here -- plain
// (temporal) 16-byte loads and stores, so those rows stay in L2.  A block whose source or destination is not 16-byte aligned (int64 mask
// rows of an odd length) takes the 4-byte path.
#include "common.h"
#include "../../include/volta_hip.h"
#include "util.h"

namespace vk {

__global__ __launch_bounds__(256) void pair_gather_kernel(const vk_pair_gather_args a) {
    const int p = blockIdx.x, k = blockIdx.y, t = threadIdx.x;
    const int side = a.side[k];
    int64_t item;
    if (a.cap_idx) item = side ? a.img_idx[p] : a.cap_idx[p];
    else item = side ? (int64_t)a.i0 + p % a.ni : (int64_t)a.c0 + p / a.ni;
    const bool ok = item >= 0 && item < a.n_items[side];           // an explicit index out of range zero-fills its block, reads nothing
    const int64_t nb = a.bytes[k];
    const char* __restrict__ src = (const char*)a.src[k] + (ok ? item : 0) * nb;
    char* __restrict__ dst = (char*)a.dst[k] + (int64_t)p * nb;
    int64_t done = 0;
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
        const u32x4* __restrict__ s4 = (const u32x4*)src;
        u32x4* __restrict__ d4 = (u32x4*)dst;
        const int64_t n16 = nb >> 4;
        const u32x4 z = {0u, 0u, 0u, 0u};
        int64_t j = t;
        for (; j + 3 * 256 < n16; j += 4 * 256) {                  // four loads in flight per lane before the stores
            const u32x4 v0 = ok ? s4[j] : z, v1 = ok ? s4[j + 256] : z, v2 = ok ? s4[j + 512] : z, v3 = ok ? s4[j + 768] : z;
            d4[j] = v0;
            d4[j + 256] = v1;
            d4[j + 512] = v2;
            d4[j + 768] = v3;
        }
        for (; j < n16; j += 256) d4[j] = ok ? s4[j] : z;
        done = n16 << 2;                                            // in 4-byte words
    }
    const uint32_t* __restrict__ s1 = (const uint32_t*)src;
    uint32_t* __restrict__ d1 = (uint32_t*)dst;
    for (int64_t j = done + t; j < (nb >> 2); j += 256) d1[j] = ok ? s1[j] : 0u;
}

}  // namespace vk

using namespace vk;

extern "C" int vk_pair_gather(const vk_pair_gather_args* a, vk_stream_t s) {
    if (a->nseg < 1 || a->nseg > VK_PAIR_MAX_SEGS || a->npairs < 0) return set_error("vk_pair_gather: %d segments (1..%d), %d pairs", a->nseg, VK_PAIR_MAX_SEGS, a->npairs);
    if (!a->cap_idx != !a->img_idx) return set_error("vk_pair_gather: cap_idx and img_idx are given together or not at all");
    if (a->n_items[0] < 0 || a->n_items[1] < 0) return set_error("vk_pair_gather: negative item count");
    if (!a->cap_idx && a->npairs > 0) {
        if (a->nc <= 0 || a->ni <= 0 || (int64_t)a->nc * a->ni != a->npairs || a->c0 < 0 || a->i0 < 0 ||
            (int64_t)a->c0 + a->nc > a->n_items[0] || (int64_t)a->i0 + a->ni > a->n_items[1])
            return set_error("vk_pair_gather: cross product captions [%d, +%d) x images [%d, +%d) does not fit %d pairs of %lld x %lld items", a->c0, a->nc,
                             a->i0, a->ni, a->npairs, (long long)a->n_items[0], (long long)a->n_items[1]);
    }
    for (int k = 0; k < a->nseg; ++k) {
        if (!a->src[k] || !a->dst[k] || a->bytes[k] <= 0 || (a->bytes[k] & 3) || (a->side[k] != 0 && a->side[k] != 1) ||
            ((uintptr_t)a->src[k] & 3) || ((uintptr_t)a->dst[k] & 3))
            return set_error("vk_pair_gather: segment %d (bytes %lld, side %d): buffers 4-byte aligned, bytes a positive multiple of 4, side 0 | 1", k,
                             (long long)a->bytes[k], a->side[k]);
        if (a->n_items[a->side[k]] <= 0) return set_error("vk_pair_gather: segment %d reads side %d, which has no items", k, a->side[k]);
    }
    if (a->npairs == 0) return 0;
    hipLaunchKernelGGL(pair_gather_kernel, dim3((unsigned)a->npairs, (unsigned)a->nseg), dim3(256), 0, (hipStream_t)s, *a);
    return check_launch("vk_pair_gather");
}
