// Hard-negative pool of the retrieval task (volta_amd/retrieval.py:generate_hard_pool): per image the mean of its region features, and per
// mean vector its k nearest vectors under Euclidean distance, exact in float64.
//
//   image_means_kernel  mean[s][f] = (((x[0][f] + x[1][f]) + x[2][f]) + ...) / n: numpy's np.sum(features, 0) / n in fp32, bit for bit.
//
// vk_knn_pool, for X fp32 [N, D]: row i of the result holds the first k candidates j under the total order (d2(i, j), j), with
// d2(i, j) = sum_k (double(x_ik) - double(x_jk))^2 from wave_dist2 below (one fixed order).  Three stages on one stream:
//   knn_norm_kernel     n_j = |x_j|^2 in float64, its fp32 rounding, and the largest n_j.
//   knn_screen_kernel   one workgroup per KNN_BQ query rows, sweeping all candidates in tiles of KNN_BC: st_ij = fl(fl(n_j) - 2 dot_ij) with the
//                       dot product on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32, a k-ordered fmaf chain).  Selection is fused into the
//                       sweep: a row keeps a threshold tau (+inf at first); an element below it is appended to the row's buffer (cap = M + 2
//                       KNN_BC keys of sortable(st) << 32 | j); a row whose buffer could overflow in the next tile is compacted by one wave
//                       to its M smallest keys (rank by counting in LDS) and tau drops to the M-th.  Every candidate left out screened at
//                       or above the final M-th value.
//   knn_refine_kernel   one workgroup per row: exact d2 of the M members, sorted by (d2, j); the row is certified when the k-th member's
//                       exact s = d2 - n_i lies strictly below st_max - E_i (E_i bounds |st - s| for the whole row); otherwise its index
//                       goes to the fallback list (device counter, no host read).
//   knn_fallback_kernel exact d2 to all N candidates for the listed rows and k rounds of "smallest (d2, j) above the previous one".
// Integer outputs and a fixed summation order: the result does not depend on how the workgroups are scheduled.
#include "common.h"
#include "../../include/volta_hip.h"
#include "util.h"

namespace vk {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int KNN_THREADS = 256;
constexpr int KNN_BQ = 128;                  // query rows per workgroup
constexpr int KNN_BC = 128;                  // candidates per tile
constexpr int KNN_BK = 16;                   // k extent of one LDS slab
constexpr int KNN_LD = KNN_BQ + 4;           // slab row pitch in floats
constexpr int KNN_CAP_EXTRA = 2 * KNN_BC;    // buffer capacity above M: one tile of head room before and after the compaction mark
constexpr int KNN_CAP_MAX = VK_KNN_MAX_SHORTLIST + KNN_CAP_EXTRA;
constexpr int KNN_KEYS_PER_LANE = KNN_CAP_MAX / 64;
constexpr int KNN_LAUNCH_BLOCKS = 256;       // query blocks per screen launch (one per CU)
constexpr int KNN_FB_BLOCKS = 128;           // workgroups (and distance rows of workspace) of one fallback launch
constexpr int KNN_FB_SLOTS = 4096;           // fallback rows one launch may take
constexpr uint64_t KNN_EMPTY = ~0ull;

__device__ __forceinline__ uint32_t knn_sortable(float s) {         // fp32 -> uint32, ascending with s (s is never NaN or -0.0 here)
    const uint32_t u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float knn_unsortable(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

__device__ __forceinline__ uint64_t key_load(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void key_store(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// sum_k (double(a_k) - double(b_k))^2 by one wave: lane l adds k = l, l + 64, ... in order, the 64 partial sums meet in a fixed xor tree.
// The only distance in this file: equal vectors get equal values whichever kernel asks.
__device__ __forceinline__ double wave_dist2(const float* __restrict__ a, const float* __restrict__ b, int D, int lane) {
    double acc = 0.0;
    for (int k = lane; k < D; k += 64) {
        const double d = (double)a[k] - (double)b[k];
        acc += d * d;
    }
    return wave_sum_f64(acc);
}

__global__ __launch_bounds__(256) void image_means_kernel(const vk_image_means_args a) {
    const int s = blockIdx.y;
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= a.F) return;
    const int n = min(max(a.n[s], 0), a.Rcap);
    const float* __restrict__ src = a.feat + (size_t)s * a.Rcap * a.F + f;
    float acc = 0.f;
    if (n > 0) acc = src[0];
    for (int i = 1; i < n; ++i) acc += src[(size_t)i * a.F];        // rows in order: ((x0 + x1) + x2) + ...
    a.mean[(size_t)s * a.F + f] = __fdiv_rn(acc, (float)n);         // n == 0: 0 / 0 = NaN, as numpy gives
}

struct KnnWork {                              // the carve-up of vk_knn_pool_args.work
    float* nrm32;                             // [N]
    double* nrm64;                            // [N]
    unsigned long long* max_n;                // bits of the largest n_j (a non-negative double orders as its bits)
    int32_t* fb_rows;                         // [N]
    uint64_t* shortlist;                      // [N, M]
    uint64_t* buf;                            // [launch rows, M + KNN_CAP_EXTRA]
    double* fb_dist;                          // [KNN_FB_BLOCKS, N]
    size_t bytes;
};

static size_t launch_rows(int N) {
    const size_t blocks = ((size_t)N + KNN_BQ - 1) / KNN_BQ;
    return (blocks < (size_t)KNN_LAUNCH_BLOCKS ? blocks : (size_t)KNN_LAUNCH_BLOCKS) * KNN_BQ;
}

static KnnWork carve(void* base, int N, int M) {
    KnnWork w;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        char* p = (char*)base + at;
        at += (bytes + 255) & ~(size_t)255;
        return (void*)p;
    };
    w.nrm32 = (float*)take(sizeof(float) * (size_t)N);
    w.nrm64 = (double*)take(sizeof(double) * (size_t)N);
    w.max_n = (unsigned long long*)take(sizeof(unsigned long long));
    w.fb_rows = (int32_t*)take(sizeof(int32_t) * (size_t)N);
    w.shortlist = (uint64_t*)take(sizeof(uint64_t) * (size_t)N * (size_t)M);
    w.buf = (uint64_t*)take(sizeof(uint64_t) * launch_rows(N) * (size_t)(M + KNN_CAP_EXTRA));
    const size_t fb = (size_t)N < (size_t)KNN_FB_BLOCKS ? (size_t)N : (size_t)KNN_FB_BLOCKS;
    w.fb_dist = (double*)take(sizeof(double) * fb * (size_t)N);
    w.bytes = at;
    return w;
}

__global__ __launch_bounds__(KNN_THREADS) void knn_norm_kernel(const float* __restrict__ X, int N, int D, KnnWork w) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * (KNN_THREADS / 64) + (threadIdx.x >> 6);
    if (j >= N) return;
    const float* __restrict__ x = X + (size_t)j * D;
    double acc = 0.0;
    for (int k = lane; k < D; k += 64) {
        const double v = (double)x[k];
        acc += v * v;
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) {
        w.nrm64[j] = acc;
        w.nrm32[j] = (float)acc;
        atomicMax(w.max_n, (unsigned long long)__double_as_longlong(acc));
    }
}

// the M smallest of the `cnt` keys of `src`, in order, to dst[0 .. min(cnt, M)); returns (to every lane) the M-th key, or KNN_EMPTY when
// cnt < M.  One wave; `scratch` is this wave's KNN_CAP_MAX keys of LDS.  The keys of a row are distinct (distinct j), so the ranks are a
// permutation.
__device__ __forceinline__ uint64_t compact_row(const uint64_t* src, int cnt, int M, uint64_t* dst, uint64_t* scratch, int lane) {
    uint64_t mine[KNN_KEYS_PER_LANE];
    int rank[KNN_KEYS_PER_LANE];
#pragma unroll
    for (int q = 0; q < KNN_KEYS_PER_LANE; ++q) {
        const int e = lane + 64 * q;
        mine[q] = e < cnt ? key_load(src + e) : KNN_EMPTY;
        rank[q] = 0;
        if (e < cnt) scratch[e] = mine[q];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int e = 0; e < cnt; ++e) {
        const uint64_t other = scratch[e];
#pragma unroll
        for (int q = 0; q < KNN_KEYS_PER_LANE; ++q) rank[q] += other < mine[q];
    }
    uint64_t mth = KNN_EMPTY;
#pragma unroll
    for (int q = 0; q < KNN_KEYS_PER_LANE; ++q) {
        const int e = lane + 64 * q;
        if (e < cnt && rank[q] < M) key_store(dst + rank[q], mine[q]);
        if (e < cnt && rank[q] == M - 1) mth = mine[q];
    }
    // at most one lane holds the M-th key: the minimum over the wave hands it to all
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint64_t o = __shfl_xor((unsigned long long)mth, m, 64);
        mth = o < mth ? o : mth;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();                                 // the next row reuses the scratch
    return mth;
}

// 16 bytes of row `row` of X from column k (k a multiple of 4): zero beyond N rows or D columns; scalar loads unless the rows are 16-byte
// aligned (vec)
__device__ __forceinline__ f32x4 load_piece(const float* __restrict__ X, int row, int k, int N, int D, bool vec) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row >= N || k >= D) return v;
    const float* __restrict__ p = X + (size_t)row * D + k;
    if (vec && k + 4 <= D) return *(const f32x4*)p;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (k + c < D) v[c] = p[c];
    return v;
}

__global__ __launch_bounds__(KNN_THREADS) void knn_screen_kernel(const float* __restrict__ X, int N, int D, int M, int row_base, int vec, KnnWork w) {
    __shared__ float sA[KNN_BK][KNN_LD];                              // [k][query row]
    __shared__ float sB[KNN_BK][KNN_LD];                              // [k][candidate]
    __shared__ float tau_s[KNN_BQ];
    __shared__ int cnt_s[KNN_BQ];
    __shared__ uint64_t scratch_s[KNN_THREADS / 64][KNN_CAP_MAX];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv >> 1, wn = wv & 1;
    const int row0 = row_base + blockIdx.x * KNN_BQ;                  // first query row of this workgroup
    const int cap = M + KNN_CAP_EXTRA, mark = M + KNN_BC;             // a row above `mark` keys is compacted before the next tile
    uint64_t* buf = w.buf + (size_t)blockIdx.x * KNN_BQ * cap;
    if (t < KNN_BQ) {
        tau_s[t] = row0 + t < N ? __builtin_inff() : -__builtin_inff();   // rows past N take nothing
        cnt_s[t] = 0;
    }
    const int lr = t >> 2, lk = (t & 3) * 4;                          // staging: rows lr and lr + 64, columns lk .. lk + 3 of the slab
    const int hl = lane >> 5, cl = lane & 31;
    const int ntiles = (N + KNN_BC - 1) / KNN_BC;
    for (int ct = 0; ct < ntiles; ++ct) {
        const int c0 = ct * KNN_BC;
        f32x16 acc[2][2];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
        f32x4 pa0 = load_piece(X, row0 + lr, lk, N, D, vec), pa1 = load_piece(X, row0 + lr + 64, lk, N, D, vec);
        f32x4 pb0 = load_piece(X, c0 + lr, lk, N, D, vec), pb1 = load_piece(X, c0 + lr + 64, lk, N, D, vec);
        for (int k0 = 0; k0 < D; k0 += KNN_BK) {
            __syncthreads();                                          // the slab's readers are done (first pass: tau / cnt are written)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                sA[lk + c][lr] = pa0[c];
                sA[lk + c][lr + 64] = pa1[c];
                sB[lk + c][lr] = pb0[c];
                sB[lk + c][lr + 64] = pb1[c];
            }
            __syncthreads();
            const int kn = k0 + KNN_BK + lk;                          // next slab, in flight under the MFMAs (zero past D)
            pa0 = load_piece(X, row0 + lr, kn, N, D, vec);
            pa1 = load_piece(X, row0 + lr + 64, kn, N, D, vec);
            pb0 = load_piece(X, c0 + lr, kn, N, D, vec);
            pb1 = load_piece(X, c0 + lr + 64, kn, N, D, vec);
#pragma unroll
            for (int kk = 0; kk < KNN_BK; kk += 2) {                  // lane l: A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]
                const float a0 = sA[kk + hl][wm * 64 + cl], a1 = sA[kk + hl][wm * 64 + 32 + cl];
                const float b0 = sB[kk + hl][wn * 64 + cl], b1 = sB[kk + hl][wn * 64 + 32 + cl];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
        // C layout: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int j = c0 + wn * 64 + ni * 32 + cl;
            const float nj = j < N ? w.nrm32[j] : 0.f;
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * hl;
                    const float st = __builtin_fmaf(-2.f, acc[mi][ni][r], nj) + 0.f;      // + 0: -0.0 becomes +0.0
                    if (j < N && st < tau_s[row]) {                                          // NaN (inf - inf) takes no slot
                        const int slot = atomicAdd(&cnt_s[row], 1);                          // < cap: at most `mark` before the tile, KNN_BC in it
                        key_store(buf + (size_t)row * cap + slot, ((uint64_t)knn_sortable(st) << 32) | (uint32_t)j);
                    }
                }
            }
        }
        __syncthreads();                                              // the tile's keys and counts are complete
        const bool last = ct + 1 == ntiles;
        for (int row = wv * (KNN_BQ / 4); row < (wv + 1) * (KNN_BQ / 4); ++row) {
            const int cnt = cnt_s[row];
            if (row0 + row >= N) continue;
            uint64_t* keys = buf + (size_t)row * cap;
            uint64_t* fin = w.shortlist + (size_t)(row0 + row) * M;
            if (cnt > (last ? M : mark)) {
                const uint64_t mth = compact_row(keys, cnt, M, last ? fin : keys, scratch_s[wv], lane);
                if (lane == 0) {
                    tau_s[row] = knn_unsortable((uint32_t)(mth >> 32));
                    cnt_s[row] = M;
                }
            } else if (last) {                                        // at most M keys, in arrival order; the refinement sorts
                for (int e = lane; e < M; e += 64) fin[e] = e < cnt ? key_load(keys + e) : KNN_EMPTY;
            }
        }
        // the next tile's first barrier orders these writes before its appends
    }
}

__global__ __launch_bounds__(KNN_THREADS) void knn_refine_kernel(const float* __restrict__ X, int N, int D, int k, int M, KnnWork w,
                                                                 int32_t* __restrict__ out, int32_t* __restrict__ stats) {
    __shared__ double d2_s[VK_KNN_MAX_SHORTLIST], sd_s[VK_KNN_MAX_SHORTLIST];
    __shared__ int j_s[VK_KNN_MAX_SHORTLIST], sj_s[VK_KNN_MAX_SHORTLIST];
    __shared__ float st_s[VK_KNN_MAX_SHORTLIST];
    __shared__ int ok_s;
    const int i = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const float* __restrict__ xi = X + (size_t)i * D;
    const uint64_t* __restrict__ keys = w.shortlist + (size_t)i * M;
    for (int c = wv; c < M; c += KNN_THREADS / 64) {
        const uint64_t key = keys[c];
        const uint32_t j = (uint32_t)key;
        const bool valid = key != KNN_EMPTY && j < (uint32_t)N;     // wave-uniform
        const double d = valid ? wave_dist2(xi, X + (size_t)j * D, D, lane) : __builtin_inf();
        if (lane == 0) {
            d2_s[c] = d;
            j_s[c] = valid ? (int)j : 0x7FFFFFFF - c;                // distinct, past every index
            st_s[c] = valid ? knn_unsortable((uint32_t)(key >> 32)) : __builtin_inff();
        }
    }
    __syncthreads();
    if (t < M) {
        const double d = d2_s[t];
        const int j = j_s[t];
        int rank = 0;
        for (int c = 0; c < M; ++c) rank += (d2_s[c] < d) | ((d2_s[c] == d) & (j_s[c] < j));
        sd_s[rank] = d;
        sj_s[rank] = j;
    }
    __syncthreads();
    if (t == 0) {
        bool valid = true;
        float st_max = -__builtin_inff();
        for (int c = 0; c < M; ++c) {
            valid = valid && j_s[c] < N;
            st_max = fmaxf(st_max, st_s[c]);
        }
        // E_i >= |st_ij - s_ij| for every j: u = 2^-24, gamma = D u / (1 - D u), a = |x_i|, B = max_j |x_j|
        const double u = 5.9604644775390625e-08, gam = (double)D * u / (1.0 - (double)D * u);
        const double ni = w.nrm64[i], B2 = __longlong_as_double((long long)*w.max_n), a = sqrt(ni), B = sqrt(B2);
        const double E = 1.01 * (2.0 * u * B2 + 2.0 * (gam + u) * a * B) + (double)(D + 4) * 4.5e-16 * (a + B) * (a + B) + (double)(D + 2) * 1.5e-45;
        const bool in_range = B2 < 1e37 && (double)D * u < 0.01;    // no fp32 overflow anywhere in the screen
        const bool sure = M == N || (in_range && (sd_s[k - 1] - ni) < (double)st_max - E);
        ok_s = valid && sure;
        if (ok_s) atomicAdd(&stats[0], 1);
        else w.fb_rows[atomicAdd(&stats[1], 1)] = i;
    }
    __syncthreads();
    if (ok_s && t < k) out[(size_t)i * k + t] = sj_s[t];
}

__global__ __launch_bounds__(KNN_THREADS) void knn_fallback_kernel(const float* __restrict__ X, int N, int D, int k, int slot0, KnnWork w,
                                                                   int32_t* __restrict__ out, const int32_t* __restrict__ stats) {
    __shared__ double best_d[2][KNN_THREADS / 64];
    __shared__ int best_j[2][KNN_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int total = min(stats[1], N), end = min(total, slot0 + KNN_FB_SLOTS);
    double* __restrict__ dist = w.fb_dist + (size_t)blockIdx.x * N;
    for (int slot = slot0 + blockIdx.x; slot < end; slot += gridDim.x) {
        const int i = w.fb_rows[slot];
        const float* __restrict__ xi = X + (size_t)i * D;
        for (int c = wv; c < N; c += KNN_THREADS / 64) {
            const double d = wave_dist2(xi, X + (size_t)c * D, D, lane);
            if (lane == 0) dist[c] = d;
        }
        __syncthreads();
        double pd = -1.0;                                             // below every distance
        int pj = -1;
        for (int r = 0; r < k; ++r) {                                 // round r: the smallest (d2, j) above round r - 1's
            double bd = __builtin_inf();
            int bj = 0x7FFFFFFF;
            for (int c = t; c < N; c += KNN_THREADS) {
                const double d = dist[c];
                const bool above = (d > pd) | ((d == pd) & (c > pj));
                const bool better = (d < bd) | ((d == bd) & (c < bj));
                if (above && better) { bd = d; bj = c; }
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const double od = __shfl_xor(bd, m, 64);
                const int oj = __shfl_xor(bj, m, 64);
                if ((od < bd) | ((od == bd) & (oj < bj))) { bd = od; bj = oj; }
            }
            if (lane == 0) { best_d[r & 1][wv] = bd; best_j[r & 1][wv] = bj; }
            __syncthreads();                                          // one barrier per round: the slots alternate
#pragma unroll
            for (int q = 0; q < KNN_THREADS / 64; ++q) {
                const double od = best_d[r & 1][q];
                const int oj = best_j[r & 1][q];
                if ((od < bd) | ((od == bd) & (oj < bj))) { bd = od; bj = oj; }
            }
            if (t == 0) out[(size_t)i * k + r] = bj;
            pd = bd;
            pj = bj;
        }
        __syncthreads();                                              // the next row overwrites dist
    }
}

}  // namespace vk

using namespace vk;

extern "C" int vk_image_means(const vk_image_means_args* a, vk_stream_t s) {
    if (!a) return set_error("vk_image_means: null argument struct");
    if (a->S < 0 || a->Rcap <= 0 || a->F <= 0) return set_error("vk_image_means: S = %d images of Rcap = %d rows and F = %d columns; S >= 0, Rcap and F positive", a->S, a->Rcap, a->F);
    if (a->S == 0) return 0;
    if (!a->feat || !a->n || !a->mean) return set_error("vk_image_means: null pointer (feat, n, mean)");
    if (((uintptr_t)a->feat | (uintptr_t)a->n | (uintptr_t)a->mean) & 3) return set_error("vk_image_means: feat, n and mean must be 4-byte aligned");
    if (a->S > 65535) return set_error("vk_image_means: S = %d images exceed the 65535 of one launch", a->S);
    hipLaunchKernelGGL(image_means_kernel, dim3((unsigned)((a->F + 255) / 256), (unsigned)a->S), dim3(256), 0, (hipStream_t)s, *a);
    return check_launch("vk_image_means");
}

static const char* knn_shape_error(int N, int D, int k, int M) {
    if (N <= 0 || D <= 0) { set_error("vk_knn_pool: X is %d x %d; N and D must be positive", N, D); return error_buffer(); }
    if (k <= 0 || k > N) { set_error("vk_knn_pool: k = %d neighbours of N = %d vectors; expected 1..N", k, N); return error_buffer(); }
    if (M < k || M > VK_KNN_MAX_SHORTLIST || M > N) {
        set_error("vk_knn_pool: shortlist M = %d; expected k = %d <= M <= min(N = %d, %d)", M, k, N, VK_KNN_MAX_SHORTLIST);
        return error_buffer();
    }
    if ((int64_t)N * D > ((int64_t)1 << 40)) { set_error("vk_knn_pool: X of %d x %d is beyond 2^40 elements", N, D); return error_buffer(); }
    return nullptr;
}

extern "C" int64_t vk_knn_pool_work_bytes(int N, int D, int k, int M) {
    if (knn_shape_error(N, D, k, M)) return -1;
    return (int64_t)carve(nullptr, N, M).bytes;
}

extern "C" int vk_knn_pool(const vk_knn_pool_args* a, vk_stream_t s) {
    if (!a) return set_error("vk_knn_pool: null argument struct");
    if (knn_shape_error(a->N, a->D, a->k, a->M)) return -1;
    if (a->flags & ~VK_KNN_SCREEN_ONLY) return set_error("vk_knn_pool: unknown flags 0x%x", a->flags);
    if (!a->X || !a->out || !a->work || !a->stats) return set_error("vk_knn_pool: null pointer (X, out, work, stats)");
    if (((uintptr_t)a->X | (uintptr_t)a->out | (uintptr_t)a->stats) & 3) return set_error("vk_knn_pool: X, out and stats must be 4-byte aligned");
    if ((uintptr_t)a->work & 255) return set_error("vk_knn_pool: work is not 256-byte aligned");
    const int N = a->N, D = a->D, k = a->k, M = a->M;
    const KnnWork w = carve(a->work, N, M);
    if (a->work_bytes < (int64_t)w.bytes) return set_error("vk_knn_pool: work_bytes = %lld, vk_knn_pool_work_bytes gives %lld", (long long)a->work_bytes, (long long)w.bytes);
    hipStream_t st = (hipStream_t)s;
    if (hipMemsetAsync(a->stats, 0, 2 * sizeof(int32_t), st) != hipSuccess || hipMemsetAsync(w.max_n, 0, sizeof(unsigned long long), st) != hipSuccess)
        return set_error("vk_knn_pool: clearing the counters failed");
    hipLaunchKernelGGL(knn_norm_kernel, dim3((unsigned)((N + 3) / 4)), dim3(KNN_THREADS), 0, st, a->X, N, D, w);
    if (check_launch("vk_knn_pool (norms)")) return -1;
    const int vec = (D % 4 == 0) && (((uintptr_t)a->X & 15) == 0);
    const int rows = (int)launch_rows(N);
    for (int64_t base = 0; base < N; base += rows) {                  // a bounded block of query rows per launch
        const int64_t left = (int64_t)N - base;
        const unsigned blocks = (unsigned)(((left < rows ? left : rows) + KNN_BQ - 1) / KNN_BQ);
        hipLaunchKernelGGL(knn_screen_kernel, dim3(blocks), dim3(KNN_THREADS), 0, st, a->X, N, D, M, (int)base, vec, w);
        if (check_launch("vk_knn_pool (screen)")) return -1;
    }
    if (a->flags & VK_KNN_SCREEN_ONLY) return 0;
    hipLaunchKernelGGL(knn_refine_kernel, dim3((unsigned)N), dim3(KNN_THREADS), 0, st, a->X, N, D, k, M, w, a->out, a->stats);
    if (check_launch("vk_knn_pool (refine)")) return -1;
    const unsigned fb = (unsigned)(N < KNN_FB_BLOCKS ? N : KNN_FB_BLOCKS);
    for (int64_t slot0 = 0; slot0 < N; slot0 += KNN_FB_SLOTS) {       // every launch reads the device counter and takes its slice: no host read
        hipLaunchKernelGGL(knn_fallback_kernel, dim3(fb), dim3(KNN_THREADS), 0, st, a->X, N, D, k, (int)slot0, w, a->out, a->stats);
        if (check_launch("vk_knn_pool (fallback)")) return -1;
    }
    return 0;
}
