// Retrieval ranks (volta_amd/retrieval.py:evaluate_retrieval): what eval_retrieval.py:200-263 computes with one np.argsort per row and per
// column of the caption x image score matrix, by counting instead of sorting.
//
// One total order: the key of (score s, index j) is sortable(s) << 32 | (0xFFFFFFFF - j); sortable maps fp32 to uint32 monotonically with
// -0.0 == +0.0 and every NaN lowest.  A larger key ranks earlier, so an element's position in np.argsort(-s, kind="stable") is the number of
// keys above its own, and the top-K are K rounds of "largest key below the previous winner": ties and NaN need no special case.
//
//   ranks_row_kernel   one workgroup per caption row.  The row is read from HBM once with 16-byte loads (a 4-byte head up to the first
//                      16-byte boundary and a 4-byte tail, so any row start and any ld qualify), counted against the target's key and kept
//                      as sortable words in LDS when it has at most RANK_RESIDENT elements; longer rows are re-read (from L2) by each
//                      top-K round.  Writes rank_ir, topk_ir and the target's sortable word for the column pass.
//   ranks_col_kernel   one workgroup per (64 adjacent columns, COL_ROWS rows): lane = column, the four waves interleave the rows, every
//                      wave-load is one 256-byte row segment.  The captions of a column's image come from the CSR in register chunks of
//                      COL_CHUNK targets; per-wave counts meet in LDS and leave as one integer atomicAdd per (target, workgroup).
//   ranks_min_kernel   per image the minimum of its captions' counts, -1 without a caption.
// Counts and minima are integers: the result does not depend on the order in which workgroups finish.
//
// Sharded over captions (vk_retrieval_ranks_shard_rows / _shard_cols / _finish): a shard holds the rows [row0, row0 + nrows) of the matrix.
// The row pass is row-local and writes at the rows' global positions; the column pass counts the shard's rows against the targets of ALL
// captions, with the global row index row0 + r in the tie rule, so the shards' count arrays add up to the unsharded one bit for bit
// (integers, any order); the minimum is taken over the sum.  Both kernels are the unsharded ones instantiated with SHARD = true.
#include "common.h"
#include "../../include/volta_hip.h"
#include "util.h"

namespace vk {

constexpr int RANK_THREADS = 256;
constexpr int RANK_RESIDENT = 8192;       // elements of a row kept in LDS (32 KiB)
constexpr int COL_BLOCK = 64;             // columns per workgroup: one per lane
constexpr int COL_ROWS = 256;             // rows per workgroup
constexpr int COL_CHUNK = 8;              // targets per column held in registers at a time

__device__ __forceinline__ uint32_t sortable(float s) {
    const uint32_t u = __float_as_uint(s), mag = u & 0x7FFFFFFFu;
    if (mag > 0x7F800000u) return 0u;                               // NaN: below -inf (0x007FFFFF)
    if (mag == 0u) return 0x80000000u;                              // -0.0 == +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint64_t rank_key(uint32_t sk, int j) { return ((uint64_t)sk << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)j); }

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint64_t o = __shfl_xor((unsigned long long)v, m, 64);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// f(j, S[j]) for every j in [0, n), thread t of RANK_THREADS: 4-byte head up to the first 16-byte boundary, 16-byte body, 4-byte tail
template <class F>
__device__ __forceinline__ void row_foreach(const float* __restrict__ row, int n, int t, F f) {
    const int to_boundary = (int)(((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u) >> 2);
    const int head = to_boundary < n ? to_boundary : n;
    if (t < head) f(t, row[t]);
    const int n4 = (n - head) >> 2;
    const f32x4* __restrict__ r4 = (const f32x4*)(row + head);
    for (int q = t; q < n4; q += RANK_THREADS) {
        const f32x4 v = r4[q];
        const int j = head + 4 * q;
        f(j, v[0]);
        f(j + 1, v[1]);
        f(j + 2, v[2]);
        f(j + 3, v[3]);
    }
    const int done = head + 4 * n4;
    if (t < n - done) f(done + t, row[done + t]);
}

// what the three kernels read: vk_retrieval_ranks_args, and for a shard the rows [row0, row0 + nrows) that S holds
struct ranks_params {
    vk_retrieval_ranks_args a;
    int32_t row0, nrows;
};

// SHARD: S holds the rows [row0, row0 + nrows) only; outputs and caption_image are indexed by the global row
template <bool SHARD>
__global__ __launch_bounds__(RANK_THREADS) void ranks_row_kernel(const ranks_params p, const int resident) {
    const vk_retrieval_ranks_args& a = p.a;
    extern __shared__ __attribute__((aligned(16))) uint32_t row_keys[];       // [Ni] when resident
    __shared__ uint64_t best_slot[2][RANK_THREADS / 64];
    __shared__ int count_slot[RANK_THREADS / 64];
    const int c = (SHARD ? p.row0 : 0) + (int)blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6, Ni = a.Ni;
    const float* __restrict__ row = a.S + (int64_t)blockIdx.x * a.ld;
    const int tj = a.caption_image[c];
    const bool valid = (uint32_t)tj < (uint32_t)Ni;                            // the guarded read: an image index outside the row reads nothing
    const uint32_t tsk = valid ? sortable(row[tj]) : 0u;
    const uint64_t tkey = valid ? rank_key(tsk, tj) : ~0ull;
    int above = 0;
    row_foreach(row, Ni, t, [&](int j, float s) {
        const uint32_t sk = sortable(s);
        if (resident) row_keys[j] = sk;
        above += rank_key(sk, j) > tkey;
    });
    above = wave_sum_i32(above);
    if (lane == 0) count_slot[w] = above;
    __syncthreads();                                                           // also: row_keys complete
    if (t == 0) {
        a.rank_ir[c] = valid ? count_slot[0] + count_slot[1] + count_slot[2] + count_slot[3] : -1;
        a.target_key[c] = tsk;
    }
    uint64_t prev = ~0ull;
    for (int r = 0; r < a.K; ++r) {                                            // round r: the largest key below round r - 1's winner
        uint64_t best = 0;                                                     // no key is 0: its low word is 0xFFFFFFFF - j with j < 2^31
        if (resident) {
            for (int j = t; j < Ni; j += RANK_THREADS) {
                const uint64_t k = rank_key(row_keys[j], j);
                best = (k < prev && k > best) ? k : best;
            }
        } else {
            row_foreach(row, Ni, t, [&](int j, float s) {
                const uint64_t k = rank_key(sortable(s), j);
                best = (k < prev && k > best) ? k : best;
            });
        }
        best = wave_max_u64(best);
        if (lane == 0) best_slot[r & 1][w] = best;
        __syncthreads();                                                       // one barrier per round: the slots alternate
#pragma unroll
        for (int i = 0; i < RANK_THREADS / 64; ++i) best = best_slot[r & 1][i] > best ? best_slot[r & 1][i] : best;
        if (t == 0) a.topk_ir[(int64_t)c * a.K + r] = best ? (int32_t)(0xFFFFFFFFu - (uint32_t)best) : -1;
        prev = best;                                                           // 0 once the row is exhausted: every later round finds nothing
    }
}

// SHARD: the rows r of S are the captions row0 + r; targets are all Nc captions, the tie rule compares global caption indices
template <bool SHARD>
__global__ __launch_bounds__(RANK_THREADS) void ranks_col_kernel(const ranks_params p) {
    const vk_retrieval_ranks_args& a = p.a;
    __shared__ int part[RANK_THREADS / 64][COL_CHUNK][COL_BLOCK];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, Nc = a.Nc, Ni = a.Ni;
    const int col0 = blockIdx.x * COL_BLOCK, col = col0 + lane;
    const bool live = col < Ni;
    const int row0 = SHARD ? p.row0 : 0;
    const int r0 = blockIdx.y * COL_ROWS, r1 = min(SHARD ? p.nrows : Nc, r0 + COL_ROWS);
    const int e0 = live ? min(max(a.image_ptr[col], 0), Nc) : 0, e1 = live ? min(max(a.image_ptr[col + 1], 0), Nc) : 0;
    int most = e1 - e0;                                                        // lane -> column is the same in all four waves, so is this maximum
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) most = max(most, __shfl_xor(most, m, 64));
    const float* __restrict__ src = a.S + col;
    for (int base = 0; base < most; base += COL_CHUNK) {                       // an image may own more captions than one register chunk
        uint32_t tk[COL_CHUNK], tc[COL_CHUNK];
        int above[COL_CHUNK];
#pragma unroll
        for (int k = 0; k < COL_CHUNK; ++k) {
            const int e = e0 + base + k;
            const int cc = e < e1 ? a.image_captions[e] : -1;
            const bool ok = (uint32_t)cc < (uint32_t)Nc;
            tk[k] = ok ? a.target_key[cc] : 0xFFFFFFFFu;                       // above every sortable word (+inf is 0xFF800000): counts nothing
            tc[k] = ok ? (uint32_t)cc : 0u;
            above[k] = 0;
        }
#pragma unroll 4
        for (int r = r0 + w; r < r1; r += RANK_THREADS / 64) {
            const uint32_t sk = live ? sortable(src[(int64_t)r * a.ld]) : 0u;
#pragma unroll
            for (int k = 0; k < COL_CHUNK; ++k) above[k] += (int)((sk > tk[k]) | ((sk == tk[k]) & ((uint32_t)(row0 + r) < tc[k])));
        }
#pragma unroll
        for (int k = 0; k < COL_CHUNK; ++k) part[w][k][lane] = above[k];
        __syncthreads();
        for (int idx = t; idx < COL_CHUNK * COL_BLOCK; idx += RANK_THREADS) {
            const int k = idx >> 6, l = idx & 63, cl = col0 + l;
            const int sum = part[0][k][l] + part[1][k][l] + part[2][k][l] + part[3][k][l];
            if (cl < Ni && sum) {
                const int e = min(max(a.image_ptr[cl], 0), Nc) + base + k;
                if (e < min(a.image_ptr[cl + 1], Nc)) atomicAdd(&a.count[e], sum);
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(RANK_THREADS) void ranks_min_kernel(const ranks_params p) {
    const vk_retrieval_ranks_args& a = p.a;
    const int i = blockIdx.x * RANK_THREADS + threadIdx.x;
    if (i >= a.Ni) return;
    const int e0 = min(max(a.image_ptr[i], 0), a.Nc), e1 = min(max(a.image_ptr[i + 1], 0), a.Nc);
    int best = -1;
    for (int e = e0; e < e1; ++e) {
        const int v = a.count[e];
        best = (best < 0 || v < best) ? v : best;
    }
    a.rank_tr[i] = best;
}

}  // namespace vk

using namespace vk;

extern "C" int vk_retrieval_ranks(const vk_retrieval_ranks_args* a, vk_stream_t s) {
    if (!a) return set_error("vk_retrieval_ranks: null argument struct");
    if (a->Nc <= 0 || a->Ni <= 0) return set_error("vk_retrieval_ranks: %d captions x %d images; both must be positive", a->Nc, a->Ni);
    if (a->K < 0 || a->K > VK_RANKS_MAX_TOPK) return set_error("vk_retrieval_ranks: top-k of %d, expected 0..%d", a->K, VK_RANKS_MAX_TOPK);
    if (a->ld < a->Ni) return set_error("vk_retrieval_ranks: leading dimension %lld is shorter than a row of %d scores", (long long)a->ld, a->Ni);
    if (!a->S || !a->caption_image || !a->image_ptr || !a->image_captions || !a->rank_ir || !a->rank_tr || !a->target_key || !a->count || (a->K > 0 && !a->topk_ir))
        return set_error("vk_retrieval_ranks: null pointer (S, caption_image, image_ptr, image_captions, rank_ir, rank_tr, target_key, count%s)", a->K > 0 ? ", topk_ir" : "");
    if ((uintptr_t)a->S & 3) return set_error("vk_retrieval_ranks: S is not 4-byte aligned");
    const unsigned cb = (unsigned)((a->Ni + COL_BLOCK - 1) / COL_BLOCK), rb = (unsigned)((a->Nc + COL_ROWS - 1) / COL_ROWS);
    if (rb > 65535u) return set_error("vk_retrieval_ranks: %d captions exceed the column pass's %d row blocks of %d", a->Nc, 65535, COL_ROWS);
    hipStream_t st = (hipStream_t)s;
    if (hipMemsetAsync(a->count, 0, sizeof(int32_t) * (size_t)a->Nc, st) != hipSuccess) return set_error("vk_retrieval_ranks: clearing the counts failed");
    const int resident = a->Ni <= RANK_RESIDENT;
    const size_t lds = resident ? (((size_t)a->Ni * 4 + 15) & ~(size_t)15) : 0;
    const ranks_params p{*a, 0, a->Nc};
    hipLaunchKernelGGL(ranks_row_kernel<false>, dim3((unsigned)a->Nc), dim3(RANK_THREADS), lds, st, p, resident);
    if (check_launch("vk_retrieval_ranks (rows)")) return -1;
    hipLaunchKernelGGL(ranks_col_kernel<false>, dim3(cb, rb), dim3(RANK_THREADS), 0, st, p);
    if (check_launch("vk_retrieval_ranks (columns)")) return -1;
    hipLaunchKernelGGL(ranks_min_kernel, dim3((unsigned)((a->Ni + RANK_THREADS - 1) / RANK_THREADS)), dim3(RANK_THREADS), 0, st, p);
    return check_launch("vk_retrieval_ranks (minima)");
}

// what the three shard calls check alike; `what` names the call
static int shard_check(const vk_retrieval_ranks_shard_args* a, const char* what) {
    if (!a) return set_error("%s: null argument struct", what);
    if (a->Nc <= 0 || a->Ni <= 0) return set_error("%s: %d captions x %d images; both must be positive", what, a->Nc, a->Ni);
    if (a->row0 < 0 || a->nrows < 0 || (int64_t)a->row0 + a->nrows > a->Nc)
        return set_error("%s: rows [%d, %lld) are not inside the %d captions", what, a->row0, (long long)a->row0 + a->nrows, a->Nc);
    if (a->ld < a->Ni) return set_error("%s: leading dimension %lld is shorter than a row of %d scores", what, (long long)a->ld, a->Ni);
    if ((uintptr_t)a->S & 3) return set_error("%s: S is not 4-byte aligned", what);
    return 0;
}

static ranks_params shard_params(const vk_retrieval_ranks_shard_args* a) {
    ranks_params p{};
    p.a.S = a->S, p.a.caption_image = a->caption_image, p.a.image_ptr = a->image_ptr, p.a.image_captions = a->image_captions;
    p.a.rank_ir = a->rank_ir, p.a.topk_ir = a->topk_ir, p.a.rank_tr = a->rank_tr, p.a.target_key = a->target_key, p.a.count = a->count;
    p.a.ld = a->ld, p.a.Nc = a->Nc, p.a.Ni = a->Ni, p.a.K = a->K;
    p.row0 = a->row0, p.nrows = a->nrows;
    return p;
}

extern "C" int vk_retrieval_ranks_shard_rows(const vk_retrieval_ranks_shard_args* a, vk_stream_t s) {
    if (shard_check(a, "vk_retrieval_ranks_shard_rows")) return -1;
    if (a->K < 0 || a->K > VK_RANKS_MAX_TOPK) return set_error("vk_retrieval_ranks_shard_rows: top-k of %d, expected 0..%d", a->K, VK_RANKS_MAX_TOPK);
    if ((a->nrows > 0 && !a->S) || !a->caption_image || !a->rank_ir || !a->target_key || (a->K > 0 && !a->topk_ir))
        return set_error("vk_retrieval_ranks_shard_rows: null pointer (S, caption_image, rank_ir, target_key%s)", a->K > 0 ? ", topk_ir" : "");
    if (a->nrows == 0) return 0;                                               // an empty shard: nothing to write
    const int resident = a->Ni <= RANK_RESIDENT;
    const size_t lds = resident ? (((size_t)a->Ni * 4 + 15) & ~(size_t)15) : 0;
    hipLaunchKernelGGL(ranks_row_kernel<true>, dim3((unsigned)a->nrows), dim3(RANK_THREADS), lds, (hipStream_t)s, shard_params(a), resident);
    return check_launch("vk_retrieval_ranks_shard_rows");
}

extern "C" int vk_retrieval_ranks_shard_cols(const vk_retrieval_ranks_shard_args* a, vk_stream_t s) {
    if (shard_check(a, "vk_retrieval_ranks_shard_cols")) return -1;
    if (a->flags & ~VK_RANKS_ACCUMULATE) return set_error("vk_retrieval_ranks_shard_cols: unknown flags 0x%x", (unsigned)a->flags);
    if ((a->nrows > 0 && !a->S) || !a->image_ptr || !a->image_captions || !a->target_key || !a->count)
        return set_error("vk_retrieval_ranks_shard_cols: null pointer (S, image_ptr, image_captions, target_key, count)");
    const unsigned cb = (unsigned)((a->Ni + COL_BLOCK - 1) / COL_BLOCK), rb = (unsigned)((a->nrows + COL_ROWS - 1) / COL_ROWS);
    if (rb > 65535u) return set_error("vk_retrieval_ranks_shard_cols: %d rows exceed the column pass's %d row blocks of %d", a->nrows, 65535, COL_ROWS);
    hipStream_t st = (hipStream_t)s;
    if (!(a->flags & VK_RANKS_ACCUMULATE) && hipMemsetAsync(a->count, 0, sizeof(int32_t) * (size_t)a->Nc, st) != hipSuccess)
        return set_error("vk_retrieval_ranks_shard_cols: clearing the counts failed");
    if (a->nrows == 0) return 0;                                               // an empty shard counts nothing
    hipLaunchKernelGGL(ranks_col_kernel<true>, dim3(cb, rb), dim3(RANK_THREADS), 0, st, shard_params(a));
    return check_launch("vk_retrieval_ranks_shard_cols");
}

extern "C" int vk_retrieval_ranks_finish(const vk_retrieval_ranks_shard_args* a, vk_stream_t s) {
    if (!a) return set_error("vk_retrieval_ranks_finish: null argument struct");
    if (a->Nc <= 0 || a->Ni <= 0) return set_error("vk_retrieval_ranks_finish: %d captions x %d images; both must be positive", a->Nc, a->Ni);
    if (!a->image_ptr || !a->count || !a->rank_tr) return set_error("vk_retrieval_ranks_finish: null pointer (image_ptr, count, rank_tr)");
    hipLaunchKernelGGL(ranks_min_kernel, dim3((unsigned)((a->Ni + RANK_THREADS - 1) / RANK_THREADS)), dim3(RANK_THREADS), 0, (hipStream_t)s, shard_params(a));
    return check_launch("vk_retrieval_ranks_finish");
}
