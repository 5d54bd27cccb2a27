// Device-side base64 decoder of the fine-tuning loader (volta_amd/datasets.py TaskLoader with resident_bytes > 0): every `features` / `boxes`
// text field of a batch, ragged lengths included, from a device copy of the text straight to its destination (the resident pool or the
// batch's scratch), so the first epoch decodes on no host thread.  The contract is in include/volta_hip.h (vk_b64_decode_device).
//
//   b64_status_init_kernel   status[j] = 0xFFFFFFFF for a job the table check accepts, 0xFFFFFFFE for one it refuses
//   b64_decode_kernel        the ONE decoding launch: grid (chunk, job), a workgroup early-exits where its chunk lies past the job's text.
//                            A lane takes 64 characters -> 48 bytes: four 16-byte non-temporal loads (the text is read once), three 16-byte
//                            stores; consecutive lanes take consecutive units.  The lane that holds the ragged end of a job (fewer than 64
//                            characters) walks it byte by byte, so nothing is read past `nsig` or written past `want_bytes`.  An offending
//                            byte is reported with an integer atomicMin of 1 + its offset, so the smallest offset wins.
//   b64_status_finish_kernel 0xFFFFFFFF -> 0 (decoded)
//
// Characters are classified with compares and adds on the bytes of the packed 32-bit words a lane holds in registers: there is no lookup
// table (a 256-entry LDS table would be read with random bank patterns).  The job table lives in device memory and is not trusted: every
// workgroup re-checks its job's ranges against text_bytes / dst_bytes before it forms an address, so no table content can make the kernel
// read or write out of bounds.
#include "common.h"
#include "../../include/volta_hip.h"
#include "util.h"

namespace vk {

constexpr uint32_t B64_LANE_CHARS = 64, B64_LANE_BYTES = 48, B64_CHUNK_CHARS = 256 * B64_LANE_CHARS;
constexpr uint32_t B64_OK_PENDING = 0xFFFFFFFFu, B64_REFUSED = 0xFFFFFFFEu, B64_MAX_NSIG = 0x7FFFFFFFu;

struct B64Launch {
    const uint8_t* text;
    uint8_t* dst;
    const vk_b64_job* jobs;
    uint32_t* status;
    uint64_t text_bytes, dst_bytes;
    uint32_t max_nsig;
    int njobs;
};

// the table check every kernel of this file applies: ranges inside the regions, lengths that agree, aligned offsets
__device__ __forceinline__ bool b64_job_ok(const B64Launch& a, const vk_b64_job& j) {
    if (j.nsig > a.max_nsig || j.nsig > B64_MAX_NSIG) return false;
    if ((j.want_bytes & 3u) || (uint64_t)j.want_bytes != ((uint64_t)j.nsig * 3) >> 2) return false;
    if ((j.text_off | j.dst_off) & 15u) return false;
    if (j.text_off > a.text_bytes || (uint64_t)j.nsig > a.text_bytes - j.text_off) return false;
    if (j.dst_off > a.dst_bytes || (uint64_t)j.want_bytes > a.dst_bytes - j.dst_off) return false;
    return true;
}

// one character -> its 6-bit value, or a value >= 64 for a byte outside both alphabets ('=' and line breaks included)
__device__ __forceinline__ uint32_t b64_value(uint32_t c) {
    const uint32_t up = c - 'A', lo = c - 'a', dg = c - '0';
    uint32_t v = 64u;
    v = (c == '+' || c == '-') ? 62u : v;
    v = (c == '/' || c == '_') ? 63u : v;
    v = dg < 10u ? dg + 52u : v;
    v = lo < 26u ? lo + 26u : v;
    v = up < 26u ? up : v;
    return v;
}

// four characters packed in one word (first character in the low byte) -> 24 bits, the first output byte on top; `bad` collects bit 6
__device__ __forceinline__ uint32_t b64_quad(uint32_t w, uint32_t& bad) {
    const uint32_t a = b64_value(w & 0xFFu), b = b64_value((w >> 8) & 0xFFu), c = b64_value((w >> 16) & 0xFFu), d = b64_value(w >> 24);
    bad |= a | b | c | d;
    return ((a & 63u) << 18) | ((b & 63u) << 12) | ((c & 63u) << 6) | (d & 63u);
}

// 16 characters -> 12 bytes as three little-endian words
__device__ __forceinline__ void b64_sixteen(const u32x4 t, uint32_t* o, uint32_t& bad) {
    uint32_t q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = __builtin_bswap32(b64_quad(t[k], bad) << 8);   // bytes 0..2 of the triple in the low 24 bits
    o[0] = q[0] | (q[1] << 24);
    o[1] = (q[1] >> 8) | (q[2] << 16);
    o[2] = (q[2] >> 16) | (q[3] << 8);
}

__global__ __launch_bounds__(256) void b64_status_init_kernel(const B64Launch a) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < a.njobs) a.status[j] = b64_job_ok(a, a.jobs[j]) ? B64_OK_PENDING : B64_REFUSED;
}

__global__ __launch_bounds__(256) void b64_status_finish_kernel(const B64Launch a) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < a.njobs && a.status[j] == B64_OK_PENDING) a.status[j] = 0u;
}

__global__ __launch_bounds__(256) void b64_decode_kernel(const B64Launch a) {
    const vk_b64_job j = a.jobs[blockIdx.y];
    if ((uint64_t)blockIdx.x * B64_CHUNK_CHARS >= j.nsig) return;                  // ragged jobs: most of a boxes job's grid row leaves here
    if (!b64_job_ok(a, j)) return;                                                 // nsig <= B64_MAX_NSIG below: 32-bit offsets do not wrap
    const uint32_t u = blockIdx.x * 256u + threadIdx.x, c0 = u * B64_LANE_CHARS;
    if (c0 >= j.nsig) return;
    const uint8_t* __restrict__ src = a.text + j.text_off + c0;
    uint8_t* __restrict__ dst = a.dst + j.dst_off + (uint64_t)u * B64_LANE_BYTES;
    uint32_t first_bad = 0xFFFFFFFFu;
    if (j.nsig - c0 >= B64_LANE_CHARS) {
        const u32x4* __restrict__ s4 = (const u32x4*)src;
        const u32x4 t0 = __builtin_nontemporal_load(s4), t1 = __builtin_nontemporal_load(s4 + 1), t2 = __builtin_nontemporal_load(s4 + 2),
                    t3 = __builtin_nontemporal_load(s4 + 3);
        uint32_t o[12], bad = 0u;
        b64_sixteen(t0, o, bad);
        b64_sixteen(t1, o + 3, bad);
        b64_sixteen(t2, o + 6, bad);
        b64_sixteen(t3, o + 9, bad);
        u32x4* __restrict__ d4 = (u32x4*)dst;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const u32x4 v = {o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]};
            d4[k] = v;
        }
        if (bad & 64u) {                                                           // rare: walk the unit again for its first offender
            for (uint32_t i = 0; i < B64_LANE_CHARS; ++i) {
                if (b64_value(src[i]) >= 64u) {
                    first_bad = c0 + i;
                    break;
                }
            }
        }
    } else {                                                                       // the ragged end of the job: at most 63 characters
        const uint32_t chars = j.nsig - c0, room = j.want_bytes - u * B64_LANE_BYTES;
        uint32_t acc = 0u, bits = 0u, at = 0u;
        for (uint32_t i = 0; i < chars; ++i) {
            const uint32_t v = b64_value(src[i]);
            if (v >= 64u) {
                first_bad = c0 + i;
                break;
            }
            acc = (acc << 6) | v;
            bits += 6u;
            if (bits >= 8u) {
                bits -= 8u;
                if (at < room) dst[at++] = (uint8_t)(acc >> bits);                 // the unused low bits of the last character fall away
            }
        }
    }
    if (first_bad != 0xFFFFFFFFu) atomicMin(a.status + blockIdx.y, first_bad + 1u);
}

}  // namespace vk

using namespace vk;

extern "C" int vk_b64_decode_device(const uint8_t* text, uint64_t text_bytes, uint8_t* dst, uint64_t dst_bytes, const vk_b64_job* jobs, int njobs,
                                    uint32_t max_nsig, uint32_t* status, vk_stream_t s) {
    if (njobs < 0) return set_error("vk_b64_decode_device: njobs = %d", njobs);
    if (njobs == 0) return 0;
    if (!jobs || !status) return set_error("vk_b64_decode_device: null job table or status");
    if (njobs > 65535) return set_error("vk_b64_decode_device: at most 65535 jobs per launch (got %d)", njobs);
    if (max_nsig > B64_MAX_NSIG) return set_error("vk_b64_decode_device: max_nsig = %u (at most 2^31 - 1 characters per job)", max_nsig);
    if ((text_bytes && !text) || (dst_bytes && !dst)) return set_error("vk_b64_decode_device: null text or destination");
    if (((uintptr_t)text | (uintptr_t)dst) & 15) return set_error("vk_b64_decode_device: text and dst must be 16-byte aligned");
    if (((uintptr_t)jobs & 7) || ((uintptr_t)status & 3)) return set_error("vk_b64_decode_device: misaligned job table or status");
    hipStream_t st = (hipStream_t)s;
    const B64Launch a = {text, dst, jobs, status, text_bytes, dst_bytes, max_nsig, njobs};
    const unsigned gj = (unsigned)((njobs + 255) / 256);
    hipLaunchKernelGGL(b64_status_init_kernel, dim3(gj), dim3(256), 0, st, a);
    if (int rc = check_launch("vk_b64_decode_device (status)")) return rc;
    if (max_nsig > 0) {
        const unsigned gx = (unsigned)(((uint64_t)max_nsig + B64_CHUNK_CHARS - 1) / B64_CHUNK_CHARS);
        hipLaunchKernelGGL(b64_decode_kernel, dim3(gx, (unsigned)njobs), dim3(256), 0, st, a);
        if (int rc = check_launch("vk_b64_decode_device")) return rc;
    }
    hipLaunchKernelGGL(b64_status_finish_kernel, dim3(gj), dim3(256), 0, st, a);
    return check_launch("vk_b64_decode_device (finish)");
}
