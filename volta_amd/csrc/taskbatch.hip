// Batch assembler of the fine-tuning loader (volta_amd/datasets.py TaskLoader): the per-sample padding, box normalisation, global feature,
// image mask and target that the reference's task datasets build in Python (volta/datasets/vqa_dataset.py:241-282, nlvr2_dataset.py:184-223,
// retrieval_dataset.py:157-254, refer_expression_dataset.py:21-58,222-269) from the staged images of a batch, in two launches:
//
//   task_mean_kernel    (only with a global row) mean[s][f] = (((x[0][f] + x[1][f]) + x[2][f]) + ...) / n: the rows are added one after the
//                       other in fp32, which is what np.sum(features, axis=0) does over the outer axis of a C-contiguous array, then one
//                       correctly rounded division by float(n) (_image_features_reader.py:105)
//   task_batch_kernel   one workgroup per (output block, group of VK_TASK_ROWS rows): copies the feature rows its segments name, writes zeros
//                       where no segment reaches, the normalised boxes, the mask and the IoU target; the workgroups of grid row N write the
//                       scattered soft target.  Every output element is written exactly once: no memset in front.
//
// Pure streaming: a VQA batch writes 256 x 101 x 2048 x 4 B = 212 MB that is read once afterwards (by the cast in front of the image
// projection GEMM), so rows move as 16-byte pieces, consecutive lanes on consecutive pieces, and the feature stores are non-temporal
// (DESIGN.md 3.1).  The staged rows are read once as well (non-temporal loads); the mean rows are re-read by every block that places a
// global row and stay temporal.
//
// This file is built with -ffp-contract=off (Makefile): x / w, the area product, and the sums, products and quotient of the IoU are each one
// rounded fp32 operation, as in the reference's numpy / torch code -- the tests ask for equal bits.
//
// The segment lists live in device memory and are not trusted: a slot outside [0, S), a source row outside the image's logical row list or a
// destination row outside the block is skipped, n is clamped to Rcap, so no segment content can make the kernel read or write out of bounds.
//
// Both kernels are templates on the argument struct, which decides where image slot s comes from (the way ranks.hip templates on SHARD):
//   vk_task_batch_args   dense staging arrays feat [S, Rcap, F] / boxes [S, Rcap, 4] and the mean workspace [S, F]
//   vk_task_pool_args    two byte regions (the loader's resident pool, this batch's scratch) and per-slot byte offsets: features [n, F],
//                        boxes [n, 4] and the stored global row [F] of an image.  The slot tables are not trusted either: slot_rows() gives
//                        -1 for a slot whose `where`, alignment or ranges are off; such a slot feeds no row and nothing of it is read.
// The segment walk, the arithmetic and the stores are one copy of the code.  With the pool, the global row is computed once, when the image is
// filled (vk_task_pool_means: the same mean kernel, the same order of additions), stored beside the image, and only read by the batch launch.
#include "common.h"
#include "../../include/volta_hip.h"
#include "util.h"

namespace vk {

// ---- where image slot s lives: its rows (-1 = the slot is refused), feature row q, box row q, global row
__device__ __forceinline__ int slot_rows(const vk_task_batch_args& a, int s) { return min(max(a.n[s], 0), a.Rcap); }
__device__ __forceinline__ const float* feat_row(const vk_task_batch_args& a, int s, int q) { return a.feat + ((size_t)s * a.Rcap + q) * a.F; }
__device__ __forceinline__ const float* box_row(const vk_task_batch_args& a, int s, int q) { return a.boxes + ((size_t)s * a.Rcap + q) * 4; }
__device__ __forceinline__ float* mean_row(const vk_task_batch_args& a, int s) { return a.mean + (size_t)s * a.F; }

__device__ __forceinline__ bool pool_range_ok(uint64_t off, uint64_t len, uint64_t bytes) { return !(off & 15) && off <= bytes && len <= bytes - off; }
__device__ __forceinline__ int slot_rows(const vk_task_pool_args& a, int s) {
    const int w = a.where[s], n = a.n[s];
    if ((w != 0 && w != 1) || n < 0) return -1;
    const uint64_t bytes = a.bytes[w], row = (uint64_t)a.F * 4;
    if (!pool_range_ok(a.feat_off[s], (uint64_t)n * row, bytes) || !pool_range_ok(a.box_off[s], (uint64_t)n * 16, bytes)) return -1;
    if (a.add_global && !pool_range_ok(a.mean_off[s], row, bytes)) return -1;
    return n;
}
__device__ __forceinline__ const float* feat_row(const vk_task_pool_args& a, int s, int q) {
    return (const float*)(a.base[a.where[s]] + a.feat_off[s]) + (size_t)q * a.F;
}
__device__ __forceinline__ const float* box_row(const vk_task_pool_args& a, int s, int q) {
    return (const float*)(a.base[a.where[s]] + a.box_off[s]) + (size_t)q * 4;
}
__device__ __forceinline__ float* mean_row(const vk_task_pool_args& a, int s) { return (float*)(a.base[a.where[s]] + a.mean_off[s]); }

// the mean launch of the dense path takes every slot; the pool's takes the slots a device list names (the newly filled ones)
struct TaskDenseMeans {
    vk_task_batch_args a;
};
struct TaskPoolMeans {
    vk_task_pool_args a;
    const int32_t* slots;
};
__device__ __forceinline__ int mean_slot(const TaskDenseMeans&, int y) { return y; }
__device__ __forceinline__ int mean_slot(const TaskPoolMeans& m, int y) {
    const int s = m.slots[y];
    return s >= 0 && s < m.a.S ? s : -1;
}

template <class M>
__global__ __launch_bounds__(256) void task_mean_kernel(const M m) {
    const int s = mean_slot(m, blockIdx.y);
    const int c4 = blockIdx.x * 256 + threadIdx.x;                  // 16-byte piece of the row
    if (s < 0 || c4 * 4 >= m.a.F) return;
    const int n = slot_rows(m.a, s);
    if (n < 0) return;                                              // a refused pool slot: nothing read, nothing written
    const f32x4* __restrict__ src = (const f32x4*)feat_row(m.a, s, 0) + c4;
    const int ld4 = m.a.F >> 2;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (n > 0) acc = src[0];
    for (int i = 1; i < n; ++i) acc += src[(size_t)i * ld4];        // rows in order: ((x0 + x1) + x2) + ...
    const float fn = (float)n;
    f32x4 r;
    for (int k = 0; k < 4; ++k) r[k] = __fdiv_rn(acc[k], fn);       // n == 0: 0 / 0 = NaN, as numpy gives; no block can place that row
    ((f32x4*)mean_row(m.a, s))[c4] = r;
}

// the image slot, its row count and the logical source row that feed row r of block o, or slot -1.  The later segment wins where two overlap
// (retrieval option 3 lays the new image over the head of the old one).
template <class A>
__device__ __forceinline__ void task_source(const A& a, int o, int r, int& slot, int& row, int& n) {
    slot = -1;
    row = n = 0;
    for (int k = VK_TASK_MAX_SEGS - 1; k >= 0; --k) {
        const int32_t* sg = a.segs + ((size_t)o * VK_TASK_MAX_SEGS + k) * 4;
        const int s = sg[0], from = sg[1], to = sg[2], cnt = sg[3];
        if (cnt <= 0 || s < 0 || s >= a.S || from < 0 || r < to || r - to >= cnt) continue;
        const int ns = slot_rows(a, s);
        if (ns < 0) continue;
        const int nl = ns + (a.add_global ? 1 : 0);
        const int q = from + (r - to);
        if (q >= nl) continue;
        slot = s;
        row = q;
        n = ns;
        return;
    }
}

template <class A>
__global__ __launch_bounds__(256) void task_batch_kernel(const A a) {
    const int t = threadIdx.x;
    if ((int)blockIdx.y == a.N) {                                   // the scattered soft target [B, num_labels]
        const int64_t total = (int64_t)a.B * a.num_labels;
        for (int64_t e = (int64_t)blockIdx.x * 256 + t; e < total; e += (int64_t)gridDim.x * 256) {
            const int b = (int)(e / a.num_labels), j = (int)(e % a.num_labels);
            float v = 0.f;
            for (int p = a.csr[b]; p < a.csr[b + 1]; ++p)
                if (a.labels[p] == j) v = a.scores[p];
            a.target[e] = v;
        }
        return;
    }
    const int o = blockIdx.y, r0 = blockIdx.x * VK_TASK_ROWS;
    const int ld4 = a.F >> 2;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < VK_TASK_ROWS; ++i) {
        const int r = r0 + i;
        if (r >= a.R) break;
        int slot, row, n;
        task_source(a, o, r, slot, row, n);                         // uniform over the workgroup
        f32x4* __restrict__ dst = (f32x4*)(a.features + ((size_t)o * a.R + r) * a.F);
        if (slot < 0) {
            for (int j = t; j < ld4; j += 256) __builtin_nontemporal_store(z, dst + j);
            continue;
        }
        const bool global_row = a.add_global == 1 ? row == 0 : (a.add_global == 2 && row == n);
        if (global_row) {
            const f32x4* __restrict__ src = (const f32x4*)mean_row(a, slot);
            for (int j = t; j < ld4; j += 256) __builtin_nontemporal_store(src[j], dst + j);
        } else {
            const int q = row - (a.add_global == 1 ? 1 : 0);
            const f32x4* __restrict__ src = (const f32x4*)feat_row(a, slot, q);
            int j = t;
            for (; j + 256 < ld4; j += 512) {                       // two loads in flight per lane before the stores
                const f32x4 v0 = __builtin_nontemporal_load(src + j), v1 = __builtin_nontemporal_load(src + j + 256);
                __builtin_nontemporal_store(v0, dst + j);
                __builtin_nontemporal_store(v1, dst + j + 256);
            }
            for (; j < ld4; j += 256) __builtin_nontemporal_store(__builtin_nontemporal_load(src + j), dst + j);
        }
    }
    // boxes, mask and IoU target: one lane per row of the group
    if (t < VK_TASK_ROWS && r0 + t < a.R) {
        const int r = r0 + t;
        int slot, row, n;
        task_source(a, o, r, slot, row, n);
        float loc[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, iou = 0.f;
        if (slot >= 0) {
            const float w = (float)a.wh[2 * slot], h = (float)a.wh[2 * slot + 1];
            const bool global_row = a.add_global == 1 ? row == 0 : (a.add_global == 2 && row == n);
            float x1 = 0.f, y1 = 0.f, x2 = w, y2 = h;              // the whole-image box in pixels
            if (global_row) {
                loc[2] = loc[3] = loc[4] = 1.f;
            } else {
                const float* bx = box_row(a, slot, row - (a.add_global == 1 ? 1 : 0));
                x1 = bx[0], y1 = bx[1], x2 = bx[2], y2 = bx[3];
                loc[4] = __fdiv_rn(__fmul_rn(__fsub_rn(y2, y1), __fsub_rn(x2, x1)), __fmul_rn(w, h));
                loc[0] = __fdiv_rn(x1, w);
                loc[1] = __fdiv_rn(y1, h);
                loc[2] = __fdiv_rn(x2, w);
                loc[3] = __fdiv_rn(y2, h);
            }
            if (a.target_kind == VK_TASK_TARGET_IOU) {
                const float* g = a.ref_box + (size_t)o * 4;
                const float ga = __fmul_rn(__fadd_rn(__fsub_rn(g[2], g[0]), 1.f), __fadd_rn(__fsub_rn(g[3], g[1]), 1.f));
                const float aa = __fmul_rn(__fadd_rn(__fsub_rn(x2, x1), 1.f), __fadd_rn(__fsub_rn(y2, y1), 1.f));
                float iw = __fadd_rn(__fsub_rn(fminf(x2, g[2]), fmaxf(x1, g[0])), 1.f);
                float ih = __fadd_rn(__fsub_rn(fminf(y2, g[3]), fmaxf(y1, g[1])), 1.f);
                if (iw < 0.f) iw = 0.f;
                if (ih < 0.f) ih = 0.f;
                const float inter = __fmul_rn(iw, ih);
                iou = __fdiv_rn(inter, __fsub_rn(__fadd_rn(aa, ga), inter));
            }
        }
        float* sp = a.spatials + ((size_t)o * a.R + r) * a.num_locs;
        for (int k = 0; k < a.num_locs; ++k) sp[k] = loc[k];
        a.image_mask[(size_t)o * a.R + r] = r < a.mask_count[o] ? 1 : 0;
        if (a.target_kind == VK_TASK_TARGET_IOU) a.target[(size_t)o * a.R + r] = iou;
    }
}

// the checks the two entry points share: counts, codes and the buffers every launch needs
template <class A>
static int task_common_checks(const char* who, const A* a) {
    if (a->S < 0 || a->N < 0 || a->B < 0 || a->R <= 0 || a->F <= 0 || (a->F & 3))
        return set_error("%s: S=%d N=%d B=%d R=%d F=%d: counts >= 0, R > 0, F a positive multiple of 4", who, a->S, a->N, a->B, a->R, a->F);
    if (a->num_locs != 4 && a->num_locs != 5) return set_error("%s: num_locs = %d (4 | 5)", who, a->num_locs);
    if (a->add_global < 0 || a->add_global > 2) return set_error("%s: add_global = %d (0 none | 1 first | 2 last)", who, a->add_global);
    if (a->target_kind != VK_TASK_TARGET_NONE && a->target_kind != VK_TASK_TARGET_SCATTER && a->target_kind != VK_TASK_TARGET_IOU)
        return set_error("%s: target kind %d", who, a->target_kind);
    if (a->N > 65534) return set_error("%s: at most 65534 output blocks per launch (got %d)", who, a->N);
    if (a->N > 0 && (!a->n || !a->wh || !a->segs || !a->mask_count || !a->features || !a->spatials || !a->image_mask)) return set_error("%s: null buffer", who);
    if ((uintptr_t)a->features & 15) return set_error("%s: features must be 16-byte aligned", who);
    if (a->target_kind == VK_TASK_TARGET_SCATTER && (a->num_labels <= 0 || (a->B > 0 && (!a->csr || !a->target))))
        return set_error("%s: the scatter target needs csr [B + 1], target [B, num_labels] (labels / scores may be empty) and num_labels > 0", who);
    if (a->target_kind == VK_TASK_TARGET_IOU && a->N > 0 && (!a->ref_box || !a->target)) return set_error("%s: the IoU target needs ref_box [N, 4] and target [N, R]", who);
    return 0;
}

template <class A>
static int task_batch_launch(const char* who, const A* a, hipStream_t st) {
    const bool scatter = a->target_kind == VK_TASK_TARGET_SCATTER && a->B > 0;
    if (a->N == 0 && !scatter) return 0;
    const unsigned gx = (unsigned)((a->R + VK_TASK_ROWS - 1) / VK_TASK_ROWS);
    // without a scatter target there is no grid row N: blockIdx.y == N never happens
    hipLaunchKernelGGL(task_batch_kernel<A>, dim3(gx, (unsigned)a->N + (scatter ? 1u : 0u)), dim3(256), 0, st, *a);
    return check_launch(who);
}

static int task_pool_checks(const char* who, const vk_task_pool_args* a) {
    if (!a) return set_error("%s: null argument", who);
    if (int rc = task_common_checks(who, a)) return rc;
    if (a->S > 0 && (!a->where || !a->feat_off || !a->box_off || !a->n || (a->add_global && !a->mean_off))) return set_error("%s: null slot table", who);
    for (int w = 0; w < 2; ++w) {
        if (a->bytes[w] && !a->base[w]) return set_error("%s: region %d has %llu bytes and no base", who, w, (unsigned long long)a->bytes[w]);
        if ((uintptr_t)a->base[w] & 15) return set_error("%s: region bases must be 16-byte aligned", who);
    }
    return 0;
}

}  // namespace vk

using namespace vk;

extern "C" int vk_task_batch(const vk_task_batch_args* a, vk_stream_t s) {
    if (!a) return set_error("vk_task_batch: null argument");
    if (a->S < 0 || a->N < 0 || a->B < 0 || a->R <= 0 || a->Rcap <= 0 || a->F <= 0 || (a->F & 3))
        return set_error("vk_task_batch: S=%d N=%d B=%d R=%d Rcap=%d F=%d: counts >= 0, R, Rcap > 0, F a positive multiple of 4", a->S, a->N, a->B, a->R, a->Rcap, a->F);
    if (int rc = task_common_checks("vk_task_batch", a)) return rc;
    if (a->N > 0 && (!a->feat || !a->boxes)) return set_error("vk_task_batch: null buffer");
    if (a->add_global && a->S > 0 && !a->mean) return set_error("vk_task_batch: a global row needs the mean workspace [S, F]");
    if (((uintptr_t)a->feat | (uintptr_t)a->mean) & 15) return set_error("vk_task_batch: feat, features and mean must be 16-byte aligned");
    hipStream_t st = (hipStream_t)s;
    if (a->add_global && a->S > 0) {
        const TaskDenseMeans m = {*a};
        hipLaunchKernelGGL(task_mean_kernel<TaskDenseMeans>, dim3((unsigned)((a->F / 4 + 255) / 256), (unsigned)a->S), dim3(256), 0, st, m);
        if (int rc = check_launch("vk_task_batch (mean)")) return rc;
    }
    return task_batch_launch("vk_task_batch", a, st);
}

extern "C" int vk_task_batch_pool(const vk_task_pool_args* a, vk_stream_t s) {
    if (int rc = task_pool_checks("vk_task_batch_pool", a)) return rc;
    return task_batch_launch("vk_task_batch_pool", a, (hipStream_t)s);
}

extern "C" int vk_task_pool_means(const vk_task_pool_args* a, const int32_t* slots, int nslots, vk_stream_t s) {
    if (int rc = task_pool_checks("vk_task_pool_means", a)) return rc;
    if (nslots < 0 || nslots > 65535) return set_error("vk_task_pool_means: nslots = %d (0 ... 65535)", nslots);
    if (nslots == 0 || a->S == 0) return 0;
    if (!slots || !a->mean_off) return set_error("vk_task_pool_means: null slot list or mean offsets");
    TaskPoolMeans m = {*a, slots};
    m.a.add_global = 1;                                             // the mean range is part of the slot check here whatever the batch places
    hipLaunchKernelGGL(task_mean_kernel<TaskPoolMeans>, dim3((unsigned)((a->F / 4 + 255) / 256), (unsigned)nslots), dim3(256), 0, (hipStream_t)s, m);
    return check_launch("vk_task_pool_means");
}
