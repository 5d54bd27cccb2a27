// Low-rank adapters (include/volta_hip.h): on the fused Q|K|V projection (vk_lora_fwd / vk_lora_bwd: K and N up to 1024) and on the
// attention-output and feed-forward projections (vk_lora_proj_fwd / vk_lora_proj_bwd: K or N up to 4096, the GELU, a saved gelu').
// ONE family of kernels and ONE pair of host builders serves both: the Q|K|V entry points are the whole-projection ones without the
// optional ends, with their own cap and their own schedule of the row product (see Family).
//
// One problem is one adapter (A [r, K], B [N, r], both bf16 from the shadow arena) on the rows of one stream.  Every product here has one
// dimension of r <= 32, so none of them fills an MFMA tile of the grouped GEMM; they are passes over X, Y, dY and dX, written as
// vector FMA / packed-bf16 dot loops over 16-byte loads (profiles/lora.md: their times against the bytes they move).  The rounding
// points are those of the header:
//   forward   T = bf16(X A^T)                       rowdot      a wave per four rows, the panel A in LDS, v_dot2c_f32_bf16
//             Y = bf16(f(Y + s T B^T))              expand      8 columns x 4 rows per lane, reads the bf16 T just stored
//   backward  dT = bf16(s dY B)                     rowdot      the panel B^T in LDS
//             dB = s dY^T T, dA = dT^T X            colpartial  per block of VK_LORA_ROW_BLOCK rows into the workspace, then
//                                                   reduce      the blocks summed in index order (no float atomics: same bits every run)
//             dX = bf16(dX + rho sum_c dT_c A_c)    expand      every adapter of a stream in ONE read-modify-write of dX
// Two launches forward, four backward, each over all (<= 6) problems of the call.
// rowdot has two schedules over one inner product (stage_panel, rowdot_accumulate, rowdot_store):
//   lora_rowdot_kernel           the whole panel in LDS (r * Kc * 2 bytes: Kc <= 1024), 64 rows per workgroup, few registers (Q|K|V)
//   lora_rowdot_chunked_kernel   the panel in stages of PROJ_CHUNK columns, the accumulators of every row of the workgroup kept in
//                                registers across the stages (whole projections: Kc up to 4096)
// expand has two optional ends, both NULL for Q|K|V: G (f = the GEMM epilogue's gelu_both, gelu' stored to G: the FFN-up adapter, whose
// term belongs inside the GELU) and rho (a saved gelu' on the adapter's share of dX: the FFN-down adapter, whose input is the GELU's
// output); without them f is the identity and rho is 1.  A launch without either runs the instantiation compiled without them.
// LoRA dropout (vk_lora_*_drop): the same launches with a Philox keep mask on the adapter's input X where it is read -- the rowdot of T,
// the colpartial of dA, the expand of dX -- and 1 / (1 - p) where a scale was 1 (rowdot's, reduce's member, expand's member).  The
// unmasked kernels are untouched instantiations: see keep_mask8.
#include "common.h"
#include "../../include/volta_hip.h"
#include "util.h"
#include <stdio.h>

namespace vk {

constexpr int LORA_MAXP = VK_LORA_MAX_PROBLEMS;
constexpr int LORA_RB = VK_LORA_ROW_BLOCK;      // rows per partial record of dA / dB: fixed, so a gradient's bits do not depend on the other problems
constexpr int ROWDOT_ROWS = 64;                 // rows per workgroup of rowdot (4 waves x 16 rows): amortises the panel's LDS fill
constexpr int ROWDOT_RW = 4;                    // rows a wave of rowdot takes at a time
constexpr int EXPAND_RPT = 4;                   // rows per lane of expand: a panel fragment in registers serves 4 rows
constexpr int COLP_COLS = 64;                   // columns per workgroup of colpartial
constexpr int PROJ_CHUNK = 1024;                // panel columns per LDS stage of the chunked rowdot
constexpr int QKV_MAX_DIM = 1024;               // the un-chunked rowdot stages a whole panel
constexpr int PROJ_MAX_DIM = 4096;

__device__ __forceinline__ int rows_of(int M, const int32_t* dyn) {
    if (!dyn) return M;
    const int d = *dyn;
    return d < 0 ? 0 : (d < M ? d : M);
}

__device__ __forceinline__ void unpack8(const u32x4 v, float* f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[2 * i] = __uint_as_float(v[i] << 16); f[2 * i + 1] = __uint_as_float(v[i] & 0xFFFF0000u); }
}

// JC consecutive bf16 (JC = 4: 8 bytes, JC = 8: 16 bytes) -> floats
template <int JC>
__device__ __forceinline__ void load_bf(const uint16_t* p, float* f) {
    if constexpr (JC == 8) {
        unpack8(*(const u32x4*)p, f);
    } else {
        const u32x2 v = *(const u32x2*)p;
        f[0] = __uint_as_float(v[0] << 16); f[1] = __uint_as_float(v[0] & 0xFFFF0000u);
        f[2] = __uint_as_float(v[1] << 16); f[3] = __uint_as_float(v[1] & 0xFFFF0000u);
    }
}

// ---- LoRA dropout (vk_lora_*_drop): the keep decisions of the 8 elements (row, k .. k + 7), k a multiple of 8, of the site `d` -- two
// Philox calls -- as a mask on the packed bf16 pairs of a 16-byte load: 0xFFFF over a kept element's half, 0 over a dropped one's.
// A masked kernel is the instantiation with one more argument (the sites of its jobs) of the kernel the unmasked entry points launch:
// kernel<R> is the code it was without the mask, kernel<R, RowdotDrop> the masked form.
__device__ __forceinline__ u32x4 keep_mask8(const DropCfg& d, uint64_t seed, uint32_t row, uint32_t k) {
    const u32x4 w0 = drop_words(d, seed, row, k >> 2), w1 = drop_words(d, seed, row, (k >> 2) + 1);
    u32x4 m;
    m[0] = (w0[0] >= d.thr ? 0xFFFFu : 0u) | (w0[1] >= d.thr ? 0xFFFF0000u : 0u);
    m[1] = (w0[2] >= d.thr ? 0xFFFFu : 0u) | (w0[3] >= d.thr ? 0xFFFF0000u : 0u);
    m[2] = (w1[0] >= d.thr ? 0xFFFFu : 0u) | (w1[1] >= d.thr ? 0xFFFF0000u : 0u);
    m[3] = (w1[2] >= d.thr ? 0xFFFFu : 0u) | (w1[3] >= d.thr ? 0xFFFF0000u : 0u);
    return m;
}
template <typename T> __device__ __forceinline__ const T& the_drop(const T& d) { return d; }

// ---------------------------------------------------------------------------------------------- rowdot
// out[m, j] = bf16(scale * sum_k P[m, k] * Q(j, k)), j < R, k < Kc;  Q(j, k) = Q[j * qs_j + k * qs_k]
struct RowdotJob {
    const uint16_t* P; const uint16_t* Q; uint16_t* out; const int32_t* dyn;
    int M, Kc, ldp, qs_j, qs_k; float scale;
};
struct RowdotArgs { RowdotJob job[LORA_MAXP]; int start[LORA_MAXP + 1]; int n; };
struct RowdotDrop { DropCfg d[LORA_MAXP]; };                 // per job; thr = 0: the job is not masked (seed is not read)

// Sums V values per lane over the 64 lanes of a wave so that every sum ends up in ONE lane: at each step a lane keeps one half of its
// values, picked by one bit of its lane number, and adds the other lane's copy of that half (V -> V / 2 values per step, V - 1 exchanges
// in all instead of 6 V for V full wave sums).  Afterwards vals[0 .. max(1, V / 64)) hold the sums of the original values
// idx .. idx + max(1, V / 64), in a fixed order of additions.
template <int N, int MASK>
__device__ __forceinline__ void lane_scatter_sum(float* vals, int lane, int& idx) {
    if constexpr (MASK >= 1) {
        if constexpr (N > 1) {
            constexpr int H = N / 2;
            const bool up = (lane & MASK) != 0;
#pragma unroll
            for (int v = 0; v < H; ++v) {
                const float keep = up ? vals[v + H] : vals[v], send = up ? vals[v] : vals[v + H];
                vals[v] = keep + __shfl_xor(send, MASK);
            }
            if (up) idx += H;
            lane_scatter_sum<H, MASK / 2>(vals, lane, idx);
        } else {
            vals[0] += __shfl_xor(vals[0], MASK);          // fewer values than lanes: the lanes that differ in this bit share one sum
            lane_scatter_sum<1, MASK / 2>(vals, lane, idx);
        }
    }
}

typedef __attribute__((ext_vector_type(2))) __bf16 bf16pair;
__device__ __forceinline__ float dot2(uint32_t a, uint32_t b, float c) {       // c + a.lo * b.lo + a.hi * b.hi on packed bf16: v_dot2c_f32_bf16
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16pair, a), __builtin_bit_cast(bf16pair, b), c, false);
}

// The three pieces both schedules are made of.  A wave takes 4 rows at a time: a lane holds 8 elements of each row, reads the panel's
// 8 elements per j from LDS once for the four rows and feeds packed bf16 pairs to v_dot2c_f32_bf16 (no unpacking); the 4 R lane sums
// are then combined across the wave.

// the panel's columns c0 .. c0 + len of every j into LDS, `stride` elements per j
template <int R>
__device__ __forceinline__ void stage_panel(uint16_t* Qs, const RowdotJob& jb, int c0, int len, int stride) {
    for (int i = threadIdx.x; i < R * len; i += 256) {
        const int j = i / len, k = i - j * len;
        Qs[j * stride + k] = jb.Q[(size_t)j * jb.qs_j + (size_t)(c0 + k) * jb.qs_k];
    }
}

// acc[i * R + j] += sum over the lane's 8-element slices k of c0 .. c0 + len (a multiple of 8: a slice lies inside the row) of
// P[m0 + i, k] * panel(j, k).  DROP: P is the adapter's input, its packed pairs are ANDed with the keep mask in front of the dots
// (1 / (1 - p) is the job's `scale`).
template <int R, bool DROP>
__device__ __forceinline__ void rowdot_accumulate(float* acc, const RowdotJob& jb, const uint16_t* Qs, int stride, int m0, int rows, int c0, int len,
                                                  int lane, const DropCfg& dc, uint64_t seed) {
    constexpr int RW = ROWDOT_RW;
    const uint16_t* prow[RW];
#pragma unroll
    for (int i = 0; i < RW; ++i) prow[i] = jb.P + (size_t)(m0 + i < rows ? m0 + i : rows - 1) * jb.ldp + c0;      // a row past the end: a valid row read, its sums not stored
    for (int k0 = lane * 8; k0 < len; k0 += 512) {
        u32x4 x[RW];
#pragma unroll
        for (int i = 0; i < RW; ++i) x[i] = *(const u32x4*)(prow[i] + k0);
        if constexpr (DROP) {
            if (dc.thr) {
#pragma unroll
                for (int i = 0; i < RW; ++i) x[i] &= keep_mask8(dc, seed, uniform32((uint32_t)(m0 + i)), (uint32_t)(c0 + k0));
            }
        }
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const u32x4 q = *(const u32x4*)(Qs + j * stride + k0);
#pragma unroll
            for (int i = 0; i < RW; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i * R + j] = dot2(x[i][e], q[e], acc[i * R + j]);
        }
    }
}

// the lane sums of the four rows from m0 across the wave, scaled, to the dense out
template <int R>
__device__ __forceinline__ void rowdot_store(float* acc, const RowdotJob& jb, int m0, int rows, int lane) {
    constexpr int V = ROWDOT_RW * R, OWN = V / 64 > 1 ? V / 64 : 1;
    int idx = 0;
    lane_scatter_sum<V, 32>(acc, lane, idx);
    // value v of this lane is element idx + v of the four rows' [4][R] block, which is contiguous in the dense out
    const bool owner = V >= 64 || (lane & (64 / V - 1)) == 0;
    if (owner) {
#pragma unroll
        for (int v = 0; v < OWN; ++v)
            if (m0 + (idx + v) / R < rows) jb.out[(size_t)m0 * R + idx + v] = f2bf(acc[v] * jb.scale);
    }
}

// the whole panel in LDS; a wave walks the workgroup's 64 rows four at a time
template <int R, typename... D>
__global__ __launch_bounds__(256) void lora_rowdot_kernel(const RowdotArgs a, const D... d) {
    constexpr bool DROP = sizeof...(D) == 1;
    constexpr int RW = ROWDOT_RW, V = RW * R;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint16_t* Qs = (uint16_t*)smem;                  // [R][Kc]
    int p = 0;
    while (p + 1 < a.n && (int)blockIdx.x >= a.start[p + 1]) ++p;
    const RowdotJob& jb = a.job[p];
    const int Kc = jb.Kc, rows = rows_of(jb.M, jb.dyn);
    const int row0 = ((int)blockIdx.x - a.start[p]) * ROWDOT_ROWS;
    if (row0 >= rows) return;
    DropCfg dc = {};
    uint64_t seed = 0;
    if constexpr (DROP) {
        dc = the_drop(d...).d[p];
        if (dc.thr) seed = *dc.seed;
    }
    stage_panel<R>(Qs, jb, 0, Kc, Kc);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row_end = row0 + ROWDOT_ROWS < rows ? row0 + ROWDOT_ROWS : rows;
    for (int m0 = row0 + wave * RW; m0 < row_end; m0 += 4 * RW) {
        float acc[V];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = 0.f;
        rowdot_accumulate<R, DROP>(acc, jb, Qs, Kc, m0, rows, 0, Kc, lane, dc, seed);
        rowdot_store<R>(acc, jb, m0, rows, lane);
    }
}

// Row groups of 4 rows per wave whose accumulators stay in registers: IT * 4 * R <= 128 floats per lane
template <int R> struct ProjRowdot { static constexpr int IT = 32 / R > 4 ? 4 : 32 / R; static constexpr int ROWS = 16 * IT; };

// the panel in stages of PROJ_CHUNK columns (r * 1024 * 2 bytes <= 64 KB of LDS at r = 32); every row group of the workgroup takes
// each stage before the next one replaces it
template <int R, typename... D>
__global__ __launch_bounds__(256) void lora_rowdot_chunked_kernel(const RowdotArgs a, const D... d) {
    constexpr bool DROP = sizeof...(D) == 1;
    constexpr int RW = ROWDOT_RW, V = RW * R, IT = ProjRowdot<R>::IT, ROWS = ProjRowdot<R>::ROWS;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint16_t* Qs = (uint16_t*)smem;                  // [R][CH]
    int p = 0;
    while (p + 1 < a.n && (int)blockIdx.x >= a.start[p + 1]) ++p;
    const RowdotJob& jb = a.job[p];
    const int Kc = jb.Kc, rows = rows_of(jb.M, jb.dyn);
    const int row0 = ((int)blockIdx.x - a.start[p]) * ROWS;
    if (row0 >= rows) return;                        // the whole workgroup: no barrier is left waiting
    const int CH = Kc < PROJ_CHUNK ? Kc : PROJ_CHUNK;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    DropCfg dc = {};
    uint64_t seed = 0;
    if constexpr (DROP) {
        dc = the_drop(d...).d[p];
        if (dc.thr) seed = *dc.seed;
    }
    float acc[IT][V];
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
        for (int v = 0; v < V; ++v) acc[it][v] = 0.f;
    for (int c0 = 0; c0 < Kc; c0 += CH) {
        const int len = Kc - c0 < CH ? Kc - c0 : CH;          // a multiple of 64, like Kc
        if (c0) __syncthreads();                              // every wave has read the previous chunk
        stage_panel<R>(Qs, jb, c0, len, CH);
        __syncthreads();
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int m0 = row0 + (it * 4 + wave) * RW;
            if (m0 < rows) rowdot_accumulate<R, DROP>(acc[it], jb, Qs, CH, m0, rows, c0, len, lane, dc, seed);          // the same for every lane of a wave
        }
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int m0 = row0 + (it * 4 + wave) * RW;
        if (m0 < rows) rowdot_store<R>(acc[it], jb, m0, rows, lane);
    }
}

// ---------------------------------------------------------------------------------------------- expand
// out[m, x] = bf16(f(float(out[m, x]) + rho[m, x] * sum_c scale_c * sum_j T_c[m, j] * W_c(j, x))), x < ncols, over the nmem members of a
// job.  mode 0: W(j, x) = W[x * R + j] (B [N, r]);  mode 1: W(j, x) = W[j * ncols + x] (A [r, K]).  The two optional ends, uniform per
// job: rho = 1 without `rho`; f = identity, or with `G` the GELU, whose derivative at the same argument goes to G[m, x].  ENDS = false
// is the same body for a launch none of whose jobs has an end (every Q|K|V launch): testing for them at run time cost the forward
// expand 0.7 us of 24.6 at r = 8 (profiles/lora.md).
struct ExpandMember { const uint16_t* T; const uint16_t* W; float scale; int mode; };
struct ExpandJob {
    uint16_t* out; const int32_t* dyn; const uint16_t* rho; uint16_t* G; int M, ncols, ldo, ldr, ldg, nmem;
    ExpandMember mem[3];
};
struct ExpandArgs { ExpandJob job[LORA_MAXP]; int start[LORA_MAXP + 1]; int n; };

struct ExpandDrop { DropCfg d[LORA_MAXP][3]; };              // per job and member; thr = 0: the member is not masked

// DROP (the input gradient): member c's sum over j is zeroed where its site dropped element (m, x) of the input; 1 / (1 - p) is the
// member's `scale`.
template <int R, bool ENDS, typename... D>
__global__ __launch_bounds__(256) void lora_expand_kernel(const ExpandArgs a, const D... d) {
    constexpr bool DROP = sizeof...(D) == 1;
    constexpr int JC = R < 8 ? R : 8;
    int p = 0;
    while (p + 1 < a.n && (int)blockIdx.x >= a.start[p + 1]) ++p;
    const ExpandJob& jb = a.job[p];
    const int rows = rows_of(jb.M, jb.dyn), chunks = jb.ncols >> 3;
    const long long item = (long long)((int)blockIdx.x - a.start[p]) * 256 + threadIdx.x;
    const int rg = (int)(item / chunks), x = ((int)(item - (long long)rg * chunks)) << 3;
    const int m0 = rg * EXPAND_RPT;
    if (m0 >= rows) return;
    const int nr = rows - m0 < EXPAND_RPT ? rows - m0 : EXPAND_RPT;
    float acc[EXPAND_RPT][8];
#pragma unroll
    for (int i = 0; i < EXPAND_RPT; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[i][e] = 0.f;
    for (int c = 0; c < jb.nmem; ++c) {
        const ExpandMember& mb = jb.mem[c];
        float part[EXPAND_RPT][8];
#pragma unroll
        for (int i = 0; i < EXPAND_RPT; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) part[i][e] = 0.f;
        for (int jc = 0; jc < R; jc += JC) {
            float w[JC][8];
            if (mb.mode == 0) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float t[JC];
                    load_bf<JC>(mb.W + (size_t)(x + e) * R + jc, t);
#pragma unroll
                    for (int jj = 0; jj < JC; ++jj) w[jj][e] = t[jj];
                }
            } else {
#pragma unroll
                for (int jj = 0; jj < JC; ++jj) unpack8(*(const u32x4*)(mb.W + (size_t)(jc + jj) * jb.ncols + x), w[jj]);
            }
#pragma unroll
            for (int i = 0; i < EXPAND_RPT; ++i) {
                if (i < nr) {
                    float t[JC];
                    load_bf<JC>(mb.T + (size_t)(m0 + i) * R + jc, t);
#pragma unroll
                    for (int jj = 0; jj < JC; ++jj)
#pragma unroll
                        for (int e = 0; e < 8; ++e) part[i][e] = __builtin_fmaf(t[jj], w[jj][e], part[i][e]);
                }
            }
        }
        if constexpr (DROP) {
            const DropCfg dc = the_drop(d...).d[p][c];
            if (dc.thr) {
                const uint64_t seed = *dc.seed;
#pragma unroll
                for (int i = 0; i < EXPAND_RPT; ++i) {
                    if (i < nr) {
                        const u32x4 km = keep_mask8(dc, seed, (uint32_t)(m0 + i), (uint32_t)x);
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            if (!(km[e >> 1] & (e & 1 ? 0x10000u : 1u))) part[i][e] = 0.f;
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < EXPAND_RPT; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[i][e] = __builtin_fmaf(part[i][e], mb.scale, acc[i][e]);
    }
#pragma unroll
    for (int i = 0; i < EXPAND_RPT; ++i) {
        if (i < nr) {
            uint16_t* o = jb.out + (size_t)(m0 + i) * jb.ldo + x;
            float y[8], v[8];
            unpack8(*(const u32x4*)o, y);
            if (ENDS && jb.rho) {
                float rho[8];
                unpack8(*(const u32x4*)(jb.rho + (size_t)(m0 + i) * jb.ldr + x), rho);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = __builtin_fmaf(rho[e], acc[i][e], y[e]);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = y[e] + acc[i][e];
            }
            if (ENDS && jb.G) {
                float d[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) { const float u = v[e]; gelu_both(u, v[e], d[e]); }
                // gelu'(v) is read again only by the backward pass: non-temporal, as the GEMM epilogue stores its C2
                __builtin_nontemporal_store(u32x4{pack2bf(d[0], d[1]), pack2bf(d[2], d[3]), pack2bf(d[4], d[5]), pack2bf(d[6], d[7])},
                                            (u32x4*)(jb.G + (size_t)(m0 + i) * jb.ldg + x));
            }
            *(u32x4*)o = u32x4{pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])};
        }
    }
}

// ---------------------------------------------------------------------------------------------- colpartial
// part[blk][x * xs + j * js] = sum over the rows m of block blk of P[m, x] * T[m, j]: x < ncols, j < R.  A workgroup owns 64 columns of one
// row block; its 256 lanes are NS row slices x (8 column chunks x R/4 groups of four j), each lane sums its slice's rows, and the slices
// are added in index order through LDS.
struct ColpJob {
    const uint16_t* P; const uint16_t* T; float* part; const int32_t* dyn;
    int M, ncols, ldp, xs, js, nblk;
};
struct ColpArgs { ColpJob job[2 * LORA_MAXP]; int start[2 * LORA_MAXP + 1]; int n; };

struct ColpDrop { DropCfg d[2 * LORA_MAXP]; };               // per job; thr = 0 (every dB job: T carries the mask already): not masked

// DROP (a dA job): P is the adapter's input, masked like the forward's; 1 / (1 - p) is applied by reduce.
template <int R, typename... D>
__global__ __launch_bounds__(256) void lora_colpartial_kernel(const ColpArgs a, const D... d) {
    constexpr bool DROP = sizeof...(D) == 1;
    constexpr int JG = R / 4, TPS = 8 * JG, NS = 256 / TPS;
    __shared__ float red[256 * 33];                 // [lane][32 (+1: the slices of one output sit 32 * TPS words apart)]
    int p = 0;
    while (p + 1 < a.n && (int)blockIdx.x >= a.start[p + 1]) ++p;
    const ColpJob& jb = a.job[p];
    const int tiles = jb.ncols / COLP_COLS;
    const int local = (int)blockIdx.x - a.start[p];
    const int blk = local / tiles, tile = local - blk * tiles;
    const int rows = rows_of(jb.M, jb.dyn);
    const int slice = threadIdx.x / TPS, t = threadIdx.x - slice * TPS;
    const int chunk = t & 7, jg = t >> 3;
    const int x0 = tile * COLP_COLS + chunk * 8;
    const int row_lo = blk * LORA_RB, row_hi = row_lo + LORA_RB < rows ? row_lo + LORA_RB : rows;
    DropCfg dc = {};
    uint64_t seed = 0;
    if constexpr (DROP) {
        dc = the_drop(d...).d[p];
        if (dc.thr) seed = *dc.seed;
    }
    float acc[4][8];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[jj][e] = 0.f;
    for (int m = row_lo + slice; m < row_hi; m += NS) {
        float x[8], tv[4];
        u32x4 xp = *(const u32x4*)(jb.P + (size_t)m * jb.ldp + x0);
        if constexpr (DROP) {
            if (dc.thr) xp &= keep_mask8(dc, seed, (uint32_t)m, (uint32_t)x0);
        }
        unpack8(xp, x);
        load_bf<4>(jb.T + (size_t)m * R + jg * 4, tv);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[jj][e] = __builtin_fmaf(x[e], tv[jj], acc[jj][e]);
    }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int e = 0; e < 8; ++e) red[threadIdx.x * 33 + jj * 8 + e] = acc[jj][e];
    __syncthreads();
    float* out = jb.part + (size_t)blk * jb.ncols * R;
    for (int o = threadIdx.x; o < TPS * 32; o += 256) {        // output o = (lane-in-slice t2, value v) of this tile
        const int t2 = o >> 5, v = o & 31;
        float s = 0.f;
        for (int sl = 0; sl < NS; ++sl) s += red[(sl * TPS + t2) * 33 + v];
        const int xcol = tile * COLP_COLS + (t2 & 7) * 8 + (v & 7), j = (t2 >> 3) * 4 + (v >> 3);
        out[(size_t)xcol * jb.xs + (size_t)j * jb.js] = s;
    }
}

// ---------------------------------------------------------------------------------------------- reduce
// dst[e] = (accumulate ? dst[e] : 0) + sum over members (scale * sum over blocks, in index order), e < n
struct ReduceMember { const float* part; int nblk; float scale; };
struct ReduceJob { float* dst; int n, nmem, accumulate; ReduceMember mem[2]; };
struct ReduceArgs { ReduceJob job[2 * LORA_MAXP]; int start[2 * LORA_MAXP + 1]; int n; };

__global__ __launch_bounds__(256) void lora_reduce_kernel(const ReduceArgs a) {
    int p = 0;
    while (p + 1 < a.n && (int)blockIdx.x >= a.start[p + 1]) ++p;
    const ReduceJob& jb = a.job[p];
    const int e = ((int)blockIdx.x - a.start[p]) * 256 + threadIdx.x;
    if (e >= jb.n) return;
    float total = jb.accumulate ? jb.dst[e] : 0.f;
    for (int c = 0; c < jb.nmem; ++c) {
        const ReduceMember& mb = jb.mem[c];
        float s = 0.f;
#pragma unroll 8
        for (int b = 0; b < mb.nblk; ++b) s += mb.part[(size_t)b * jb.n + e];          // unrolled: eight loads in flight, the additions stay in block order
        total += s * mb.scale;
    }
    jb.dst[e] = total;
}

}  // namespace vk

// ================================================================================================ host
namespace {

int nblk_of(int M) { return M > 0 ? (M + VK_LORA_ROW_BLOCK - 1) / VK_LORA_ROW_BLOCK : 0; }
// bytes of a problem's partial records: dB [nblk][N][r], then dA [nblk][r][K]
int64_t record_bytes(int M, int K, int N, int r) { return ((int64_t)nblk_of(M) * r * ((int64_t)K + N) * 4 + 255) & ~(int64_t)255; }

template <typename P>
int64_t work_bytes(const P* p, int n) {
    if (!p || n < 1 || n > VK_LORA_MAX_PROBLEMS) return -1;
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        if (p[i].M < 0 || p[i].K <= 0 || p[i].N <= 0 || p[i].r <= 0) return -1;
        total += record_bytes(p[i].M, p[i].K, p[i].N, p[i].r);
    }
    return total > 0 ? total : 256;
}

template <typename K4, typename K8, typename K16, typename K32, typename... Args>
void launch_by_r(int r, K4 k4, K8 k8, K16 k16, K32 k32, int blocks, size_t lds, hipStream_t st, const Args&... a) {
    switch (r) {
        case 4: hipLaunchKernelGGL(k4, dim3(blocks), dim3(256), lds, st, a...); break;
        case 8: hipLaunchKernelGGL(k8, dim3(blocks), dim3(256), lds, st, a...); break;
        case 16: hipLaunchKernelGGL(k16, dim3(blocks), dim3(256), lds, st, a...); break;
        default: hipLaunchKernelGGL(k32, dim3(blocks), dim3(256), lds, st, a...);
    }
}

// the dynamic-LDS limit of the four ranks of a kernel template: a panel of `cols` bf16 columns per j
template <typename K>
bool allow_panel(K k4, K k8, K k16, K k32, int cols) {
    const K k[4] = {k4, k8, k16, k32};
    for (int i = 0; i < 4; ++i) (void)hipFuncSetAttribute((const void*)k[i], hipFuncAttributeMaxDynamicSharedMemorySize, (4 << i) * cols * 2);
    return true;
}

// LoRA dropout: entry i of a _drop call's vk_dropout array as the kernels take it; threshold 0 = not masked, scale 1
vk::DropCfg drop_cfg(const vk_dropout* drop, int i) {
    if (!drop || !drop[i].threshold) return vk::DropCfg{nullptr, 0u, 0u, 1.0f};
    return vk::DropCfg{drop[i].seed, drop[i].site, drop[i].threshold, drop[i].scale};
}
int check_count(const char* fn, const void* p, int n) {
    if (!p || n < 1 || n > VK_LORA_MAX_PROBLEMS) return vk::set_error("%s: %d problems (1 .. %d)", fn, n, VK_LORA_MAX_PROBLEMS);
    return 0;
}
// what a _drop entry point checks in front of its builder
int check_drop(const char* fn, const void* p, const vk_dropout* drop, int n) {
    if (check_count(fn, p, n)) return -1;
    if (!drop) return vk::set_error("%s: NULL dropout array (one vk_dropout per problem)", fn);
    for (int i = 0; i < n; ++i) {
        if (drop[i].threshold && !drop[i].seed) return vk::set_error("%s: problem %d: threshold %u with a NULL seed", fn, i, drop[i].threshold);
        if (drop[i].threshold && ((uintptr_t)drop[i].seed & 7)) return vk::set_error("%s: problem %d: the seed is not 8-byte aligned", fn, i);
        if (drop[i].threshold && !(drop[i].scale > 0.f)) return vk::set_error("%s: problem %d: scale %g (1 / (1 - p))", fn, i, (double)drop[i].scale);
    }
    return 0;
}
bool any_drop(const vk_dropout* drop, int n) {
    for (int i = 0; drop && i < n; ++i)
        if (drop[i].threshold) return true;
    return false;
}

// ---- launchers: the blocks of every job, then the instantiation of the call's rank, with the sites (d) when a problem is masked
int rowdot_blocks(vk::RowdotArgs& a, int per) {
    int blocks = 0;
    for (int i = 0; i < a.n; ++i) { a.start[i] = blocks; blocks += (a.job[i].M + per - 1) / per; }
    return a.start[a.n] = blocks;
}

template <typename... D>
void run_rowdot(int r, int blocks, int maxK, hipStream_t st, const vk::RowdotArgs& a, const D&... d) {
    static const bool limit = allow_panel(vk::lora_rowdot_kernel<4, D...>, vk::lora_rowdot_kernel<8, D...>, vk::lora_rowdot_kernel<16, D...>,
                                          vk::lora_rowdot_kernel<32, D...>, vk::QKV_MAX_DIM);
    (void)limit;
    launch_by_r(r, vk::lora_rowdot_kernel<4, D...>, vk::lora_rowdot_kernel<8, D...>, vk::lora_rowdot_kernel<16, D...>, vk::lora_rowdot_kernel<32, D...>,
                blocks, (size_t)r * maxK * 2, st, a, d...);
}
int launch_rowdot(const char* fn, int r, vk::RowdotArgs& a, int maxK, hipStream_t st, const vk::RowdotDrop* d) {
    const int blocks = rowdot_blocks(a, vk::ROWDOT_ROWS);
    if (!blocks) return 0;
    if (d) run_rowdot(r, blocks, maxK, st, a, *d);
    else run_rowdot(r, blocks, maxK, st, a);
    return vk::check_launch(fn);
}

template <typename... D>
void run_rowdot_chunked(int r, int blocks, int maxK, hipStream_t st, const vk::RowdotArgs& a, const D&... d) {
    static const bool limit = allow_panel(vk::lora_rowdot_chunked_kernel<4, D...>, vk::lora_rowdot_chunked_kernel<8, D...>,
                                          vk::lora_rowdot_chunked_kernel<16, D...>, vk::lora_rowdot_chunked_kernel<32, D...>, vk::PROJ_CHUNK);
    (void)limit;
    const int ch = maxK < vk::PROJ_CHUNK ? maxK : vk::PROJ_CHUNK;          // every job's chunk stride is min(its Kc, PROJ_CHUNK) <= this
    launch_by_r(r, vk::lora_rowdot_chunked_kernel<4, D...>, vk::lora_rowdot_chunked_kernel<8, D...>, vk::lora_rowdot_chunked_kernel<16, D...>,
                vk::lora_rowdot_chunked_kernel<32, D...>, blocks, (size_t)r * ch * 2, st, a, d...);
}
int launch_rowdot_chunked(const char* fn, int r, vk::RowdotArgs& a, int maxK, hipStream_t st, const vk::RowdotDrop* d) {
    const int blocks = rowdot_blocks(a, r == 4 ? vk::ProjRowdot<4>::ROWS : r == 8 ? vk::ProjRowdot<8>::ROWS : r == 16 ? vk::ProjRowdot<16>::ROWS : vk::ProjRowdot<32>::ROWS);
    if (!blocks) return 0;
    if (d) run_rowdot_chunked(r, blocks, maxK, st, a, *d);
    else run_rowdot_chunked(r, blocks, maxK, st, a);
    return vk::check_launch(fn);
}

template <typename... D>
void run_expand(int r, int blocks, hipStream_t st, const vk::ExpandArgs& a, const D&... d) {
    bool ends = false;
    for (int i = 0; i < a.n; ++i) ends = ends || a.job[i].rho || a.job[i].G;
    if (ends)
        launch_by_r(r, vk::lora_expand_kernel<4, true, D...>, vk::lora_expand_kernel<8, true, D...>, vk::lora_expand_kernel<16, true, D...>,
                    vk::lora_expand_kernel<32, true, D...>, blocks, 0, st, a, d...);
    else
        launch_by_r(r, vk::lora_expand_kernel<4, false, D...>, vk::lora_expand_kernel<8, false, D...>, vk::lora_expand_kernel<16, false, D...>,
                    vk::lora_expand_kernel<32, false, D...>, blocks, 0, st, a, d...);
}
int launch_expand(const char* fn, int r, vk::ExpandArgs& a, hipStream_t st, const vk::ExpandDrop* d = nullptr) {
    int64_t blocks = 0;
    for (int i = 0; i < a.n; ++i) {
        a.start[i] = (int)blocks;
        const int64_t items = (int64_t)((a.job[i].M + vk::EXPAND_RPT - 1) / vk::EXPAND_RPT) * (a.job[i].ncols / 8);
        blocks += (items + 255) / 256;
    }
    a.start[a.n] = (int)blocks;
    if (!blocks) return 0;
    if (blocks > 0x7FFFFFFF) return vk::set_error("%s: too many rows", fn);
    if (d) run_expand(r, (int)blocks, st, a, *d);
    else run_expand(r, (int)blocks, st, a);
    return vk::check_launch(fn);
}

template <typename... D>
void run_colpartial(int r, int blocks, hipStream_t st, const vk::ColpArgs& a, const D&... d) {
    launch_by_r(r, vk::lora_colpartial_kernel<4, D...>, vk::lora_colpartial_kernel<8, D...>, vk::lora_colpartial_kernel<16, D...>,
                vk::lora_colpartial_kernel<32, D...>, blocks, 0, st, a, d...);
}
int launch_colpartial(const char* fn, int r, vk::ColpArgs& cp, hipStream_t st, const vk::ColpDrop* d) {
    int blocks = 0;
    for (int i = 0; i < cp.n; ++i) { cp.start[i] = blocks; blocks += cp.job[i].nblk * (cp.job[i].ncols / vk::COLP_COLS); }
    cp.start[cp.n] = blocks;
    if (!blocks) return 0;
    if (d) run_colpartial(r, blocks, st, cp, *d);
    else run_colpartial(r, blocks, st, cp);
    return vk::check_launch(fn);
}

int launch_reduce(const char* fn, vk::ReduceArgs& re, hipStream_t st) {
    int blocks = 0;
    for (int i = 0; i < re.n; ++i) { re.start[i] = blocks; blocks += (re.job[i].n + 255) / 256; }
    re.start[re.n] = blocks;
    if (!blocks) return 0;
    hipLaunchKernelGGL(vk::lora_reduce_kernel, dim3(blocks), dim3(256), 0, st, re);
    return vk::check_launch(fn);
}

// ---- the two families of entry points: what differs between them.  The builders below take the whole-projection problems; the Q|K|V
// entry points hand them theirs in that form (widen), without G, act and R.
struct Family {
    const char* fwd; const char* bwd;            // the unmasked entry points: the names in a failed launch's message
    const char* fwd_writes;                      // ... and in the forward's aliasing refusal
    int cap;                                     // K and N at most
    int (*rowdot)(const char*, int, vk::RowdotArgs&, int, hipStream_t, const vk::RowdotDrop*);
};
const Family QKV = {"vk_lora_fwd", "vk_lora_bwd", "T or Y", vk::QKV_MAX_DIM, launch_rowdot};            // a whole panel in LDS: not beyond 1024
const Family PROJ = {"vk_lora_proj_fwd", "vk_lora_proj_bwd", "T, Y or G", vk::PROJ_MAX_DIM, launch_rowdot_chunked};

struct Label {                                   // "vk_lora_fwd (T)"
    char s[64];
    Label(const char* fn, const char* what) { snprintf(s, sizeof(s), "%s (%s)", fn, what); }
    operator const char*() const { return s; }
};

const vk_lora_proj_problem* widen(const vk_lora_problem* p, int n, vk_lora_proj_problem* w) {
    for (int i = 0; i < n; ++i) {
        const vk_lora_problem& q = p[i];
        w[i] = vk_lora_proj_problem{q.X, q.A, q.B, q.T, q.Y, nullptr, q.dyn, q.M, q.K, q.N, q.r, q.ldx, q.ldy, 0, q.scale, 0};
    }
    return w;
}
const vk_lora_proj_bwd_problem* widen(const vk_lora_bwd_problem* p, int n, vk_lora_proj_bwd_problem* w) {
    for (int i = 0; i < n; ++i) {
        const vk_lora_bwd_problem& q = p[i];
        w[i] = vk_lora_proj_bwd_problem{q.X, q.A, q.B, q.T, q.dY, q.dT, q.dX, q.dA, q.dB, nullptr, q.dyn, q.M, q.K, q.N, q.r, q.ldx, q.ldy, q.lddx, 0,
                                        q.accumulate, q.scale};
    }
    return w;
}

int check_common(const char* fn, int cap, int i, int M, int K, int N, int r, int ldx, int ldy, const void* const* ptrs, int nptr) {
    if (r != 4 && r != 8 && r != 16 && r != 32) return vk::set_error("%s: problem %d: r = %d (4, 8, 16 or 32)", fn, i, r);
    if (M < 0) return vk::set_error("%s: problem %d: M = %d", fn, i, M);
    if (K <= 0 || N <= 0 || K % 64 || N % 64 || K > cap || N > cap)
        return vk::set_error("%s: problem %d: K = %d, N = %d (multiples of 64, at most %d)", fn, i, K, N, cap);
    if (ldx < K || ldy < N || ldx % 8 || ldy % 8) return vk::set_error("%s: problem %d: leading dimensions %d / %d (multiples of 8, >= K / N)", fn, i, ldx, ldy);
    for (int k = 0; k < nptr; ++k) {
        if (!ptrs[k]) return vk::set_error("%s: problem %d: NULL operand %d", fn, i, k);
        if ((uintptr_t)ptrs[k] & 15) return vk::set_error("%s: problem %d: operand %d is not 16-byte aligned", fn, i, k);
    }
    return 0;
}

// The forward of `fn` (an entry point of the family, masked or not; drop NULL: not masked).  The masked kernels run only when a
// problem has a threshold.
int lora_fwd(const Family& fam, const char* fn, const vk_lora_proj_problem* p, const vk_dropout* drop, int n, vk_stream_t s) {
    vk::RowdotArgs rd = {};
    vk::RowdotDrop rdd = {};
    vk::ExpandArgs ex = {};
    int maxK = 0;
    for (int i = 0; i < n; ++i) {
        const vk_lora_proj_problem& q = p[i];
        const void* ptrs[5] = {q.X, q.A, q.B, q.T, q.Y};
        if (check_common(fn, fam.cap, i, q.M, q.K, q.N, q.r, q.ldx, q.ldy, ptrs, 5)) return -1;
        if (q.r != p[0].r) return vk::set_error("%s: problem %d: r = %d, problem 0 has %d (one rank per call)", fn, i, q.r, p[0].r);
        if (q.act != 0 && q.act != 1) return vk::set_error("%s: problem %d: act = %d (0 or 1)", fn, i, q.act);
        if (q.act == 0 && q.G) return vk::set_error("%s: problem %d: act = 0 takes no G", fn, i);
        if (q.act == 1 && (!q.G || ((uintptr_t)q.G & 15) || q.ldg < q.N || q.ldg % 8))
            return vk::set_error("%s: problem %d: act = 1 needs G (16-byte aligned, ldg %d a multiple of 8, >= N)", fn, i, q.ldg);
        for (int k = 0; k < i; ++k)
            if (p[k].Y == q.Y || p[k].T == q.T || (q.G && p[k].G == q.G))
                return vk::set_error("%s: problems %d and %d write the same %s", fn, k, i, fam.fwd_writes);
        rdd.d[i] = drop_cfg(drop, i);
        rd.job[i] = vk::RowdotJob{(const uint16_t*)q.X, (const uint16_t*)q.A, (uint16_t*)q.T, q.dyn, q.M, q.K, q.ldx, q.K, 1, rdd.d[i].scale};
        vk::ExpandJob& e = ex.job[i];
        e.out = (uint16_t*)q.Y; e.dyn = q.dyn; e.rho = nullptr; e.G = (uint16_t*)q.G; e.M = q.M; e.ncols = q.N; e.ldo = q.ldy; e.ldr = 0; e.ldg = q.ldg;
        e.nmem = 1;
        e.mem[0] = vk::ExpandMember{(const uint16_t*)q.T, (const uint16_t*)q.B, q.scale, 0};
        if (q.K > maxK) maxK = q.K;
    }
    rd.n = ex.n = n;
    if (fam.rowdot(Label(fam.fwd, "T"), p[0].r, rd, maxK, (hipStream_t)s, any_drop(drop, n) ? &rdd : nullptr)) return -1;
    return launch_expand(Label(fam.fwd, "expand"), p[0].r, ex, (hipStream_t)s);
}

int lora_bwd(const Family& fam, const char* fn, const vk_lora_proj_bwd_problem* p, const vk_dropout* drop, int n, void* work, vk_stream_t s) {
    if (!work || ((uintptr_t)work & 15)) return vk::set_error("%s: the workspace must be a 16-byte aligned buffer of %s_work_bytes()", fn, fam.bwd);
    hipStream_t st = (hipStream_t)s;
    vk::RowdotArgs rd = {};
    vk::ColpArgs cp = {};
    vk::ColpDrop cpd = {};
    vk::ReduceArgs re = {};
    vk::ExpandArgs ex = {};
    vk::ExpandDrop exd = {};
    const bool masked = any_drop(drop, n);
    const int r = p[0].r;
    int maxN = 0;
    char* w = (char*)work;
    for (int i = 0; i < n; ++i) {
        const vk_lora_proj_bwd_problem& q = p[i];
        const void* ptrs[6] = {q.X, q.A, q.B, q.T, q.dY, q.dT};
        if (check_common(fn, fam.cap, i, q.M, q.K, q.N, q.r, q.ldx, q.ldy, ptrs, 6)) return -1;
        if (!q.dA != !q.dB || ((uintptr_t)q.dA & 15) || ((uintptr_t)q.dB & 15))
            return vk::set_error("%s: problem %d: dA and dB are both set (16-byte aligned) or both NULL (a frozen adapter)", fn, i);
        if (!q.dA && !q.dX) return vk::set_error("%s: problem %d has no output (dA, dB and dX are NULL)", fn, i);
        if (q.r != r) return vk::set_error("%s: problem %d: r = %d, problem 0 has %d (one rank per call)", fn, i, q.r, r);
        if (q.dX && (((uintptr_t)q.dX & 15) || q.lddx < q.K || q.lddx % 8)) return vk::set_error("%s: problem %d: dX alignment / lddx %d", fn, i, q.lddx);
        if (q.R && (((uintptr_t)q.R & 15) || q.ldr < q.K || q.ldr % 8)) return vk::set_error("%s: problem %d: R alignment / ldr %d", fn, i, q.ldr);
        for (int k = 0; k < i; ++k)
            if (p[k].dT == q.dT) return vk::set_error("%s: problems %d and %d write the same dT", fn, k, i);
        rd.job[i] = vk::RowdotJob{(const uint16_t*)q.dY, (const uint16_t*)q.B, (uint16_t*)q.dT, q.dyn, q.M, q.N, q.ldy, 1, q.r, q.scale};
        if (q.N > maxN) maxN = q.N;
        // partial records: dB [nblk][N][r], then dA [nblk][r][K]
        const int nblk = nblk_of(q.M);
        float* partB = (float*)w;
        float* partA = partB + (size_t)nblk * q.N * q.r;
        w += record_bytes(q.M, q.K, q.N, q.r);
        const vk::DropCfg dc = drop_cfg(drop, i);
        if (q.dA) {
            cp.job[cp.n++] = vk::ColpJob{(const uint16_t*)q.dY, (const uint16_t*)q.T, partB, q.dyn, q.M, q.N, q.ldy, q.r, 1, nblk};
            cpd.d[cp.n] = dc;                // the dA job that follows: X is masked as the forward masked it
            cp.job[cp.n++] = vk::ColpJob{(const uint16_t*)q.X, (const uint16_t*)q.dT, partA, q.dyn, q.M, q.K, q.ldx, 1, q.K, nblk};
            // gradient jobs: the problems of one adapter (a shared sub-layer's two streams) are summed by ONE job, in list order
            int g = -1;
            for (int k = 0; k < re.n; k += 2)
                if (re.job[k].dst == q.dB) g = k;
            if (g < 0) {
                g = re.n;
                re.n += 2;
                re.job[g].dst = q.dB; re.job[g].n = q.N * q.r; re.job[g].accumulate = q.accumulate != 0;
                re.job[g + 1].dst = q.dA; re.job[g + 1].n = q.r * q.K; re.job[g + 1].accumulate = q.accumulate != 0;
            } else {
                if (!q.accumulate) return vk::set_error("%s: problem %d writes the gradients of an earlier problem without `accumulate`", fn, i);
                if (re.job[g + 1].dst != q.dA || re.job[g].n != q.N * q.r || re.job[g + 1].n != q.r * q.K || re.job[g].nmem >= 2)
                    return vk::set_error("%s: problem %d: a shared adapter has one dA, one dB and at most two sources", fn, i);
            }
            re.job[g].mem[re.job[g].nmem++] = vk::ReduceMember{partB, nblk, q.scale};
            re.job[g + 1].mem[re.job[g + 1].nmem++] = vk::ReduceMember{partA, nblk, dc.scale};      // 1 / (1 - p) on this problem's finished sum
        }
        if (q.dX) {
            int e = -1;
            for (int k = 0; k < ex.n; ++k)
                if (ex.job[k].out == (uint16_t*)q.dX) e = k;
            if (e < 0) {
                e = ex.n++;
                vk::ExpandJob& j = ex.job[e];
                j.out = (uint16_t*)q.dX; j.dyn = q.dyn; j.rho = (const uint16_t*)q.R; j.G = nullptr; j.M = q.M; j.ncols = q.K; j.ldo = q.lddx;
                j.ldr = q.R ? q.ldr : 0; j.ldg = 0; j.nmem = 0;
            }
            vk::ExpandJob& j = ex.job[e];
            if (j.rho != (const uint16_t*)q.R || (q.R && j.ldr != q.ldr))
                return vk::set_error("%s: problem %d: the adapters that add into one dX name one R (and ldr)", fn, i);
            if (j.M != q.M || j.ncols != q.K || j.ldo != q.lddx || j.dyn != q.dyn || j.nmem >= 3)
                return vk::set_error("%s: problem %d: the (at most 3) adapters that add into one dX share its shape", fn, i);
            exd.d[e][j.nmem] = dc;
            j.mem[j.nmem++] = vk::ExpandMember{(const uint16_t*)q.dT, (const uint16_t*)q.A, dc.scale, 1};
        }
    }
    for (int i = 0; i < n; ++i)          // no gradient may alias another job's: dA of one adapter is nobody's dB
        for (int k = 0; k < n; ++k)
            if (p[i].dA && p[i].dA == p[k].dB) return vk::set_error("%s: dA of problem %d is dB of problem %d", fn, i, k);
    rd.n = n;
    if (fam.rowdot(Label(fam.bwd, "dT"), r, rd, maxN, st, nullptr)) return -1;
    if (launch_colpartial(Label(fam.bwd, "partials"), r, cp, st, masked ? &cpd : nullptr)) return -1;
    if (launch_reduce(Label(fam.bwd, "reduce"), re, st)) return -1;
    if (ex.n) return launch_expand(Label(fam.bwd, "dX"), r, ex, st, masked ? &exd : nullptr);
    return 0;
}

}  // namespace

// ---- the entry points: the count (and a _drop call's array) checked, a Q|K|V call's problems widened on the stack, then the builder
extern "C" int vk_lora_fwd(const vk_lora_problem* p, int n, vk_stream_t s) {
    vk_lora_proj_problem w[VK_LORA_MAX_PROBLEMS];
    if (check_count("vk_lora_fwd", p, n)) return -1;
    return lora_fwd(QKV, "vk_lora_fwd", widen(p, n, w), nullptr, n, s);
}
extern "C" int vk_lora_fwd_drop(const vk_lora_problem* p, const vk_dropout* drop, int n, vk_stream_t s) {
    vk_lora_proj_problem w[VK_LORA_MAX_PROBLEMS];
    if (check_drop("vk_lora_fwd_drop", p, drop, n)) return -1;
    return lora_fwd(QKV, "vk_lora_fwd_drop", widen(p, n, w), drop, n, s);
}
extern "C" int vk_lora_proj_fwd(const vk_lora_proj_problem* p, int n, vk_stream_t s) {
    if (check_count("vk_lora_proj_fwd", p, n)) return -1;
    return lora_fwd(PROJ, "vk_lora_proj_fwd", p, nullptr, n, s);
}
extern "C" int vk_lora_proj_fwd_drop(const vk_lora_proj_problem* p, const vk_dropout* drop, int n, vk_stream_t s) {
    if (check_drop("vk_lora_proj_fwd_drop", p, drop, n)) return -1;
    return lora_fwd(PROJ, "vk_lora_proj_fwd_drop", p, drop, n, s);
}

extern "C" int64_t vk_lora_bwd_work_bytes(const vk_lora_bwd_problem* p, int n) { return work_bytes(p, n); }
extern "C" int64_t vk_lora_proj_bwd_work_bytes(const vk_lora_proj_bwd_problem* p, int n) { return work_bytes(p, n); }

extern "C" int vk_lora_bwd(const vk_lora_bwd_problem* p, int n, void* work, vk_stream_t s) {
    vk_lora_proj_bwd_problem w[VK_LORA_MAX_PROBLEMS];
    if (check_count("vk_lora_bwd", p, n)) return -1;
    return lora_bwd(QKV, "vk_lora_bwd", widen(p, n, w), nullptr, n, work, s);
}
extern "C" int vk_lora_bwd_drop(const vk_lora_bwd_problem* p, const vk_dropout* drop, int n, void* work, vk_stream_t s) {
    vk_lora_proj_bwd_problem w[VK_LORA_MAX_PROBLEMS];
    if (check_drop("vk_lora_bwd_drop", p, drop, n)) return -1;
    return lora_bwd(QKV, "vk_lora_bwd_drop", widen(p, n, w), drop, n, work, s);
}
extern "C" int vk_lora_proj_bwd(const vk_lora_proj_bwd_problem* p, int n, void* work, vk_stream_t s) {
    if (check_count("vk_lora_proj_bwd", p, n)) return -1;
    return lora_bwd(PROJ, "vk_lora_proj_bwd", p, nullptr, n, work, s);
}
extern "C" int vk_lora_proj_bwd_drop(const vk_lora_proj_bwd_problem* p, const vk_dropout* drop, int n, void* work, vk_stream_t s) {
    if (check_drop("vk_lora_proj_bwd_drop", p, drop, n)) return -1;
    return lora_bwd(PROJ, "vk_lora_proj_bwd_drop", p, drop, n, work, s);
}
