// hybrid_kernel.hip -- device-side glue of the hybrid SC / SC-list decoder (pl_hybrid_decode) and of
// pl_crc_status, for gfx950 (wave64).
//
// Hybrid decoding [Cammerer_Hybrid_SCL] (the decoder my_sn/fec/polar/dec.py:187 names and never
// implemented): SC-decode every row, list-decode only the rows whose CRC fails.  The decoders are
// the library's own (pl_sc_decode, launch_scl); this file is what lies between them:
//   crc_flag          valid[b] = the k decoded bits of row b pass the CRC
//   compact_failed    the failing row indices, ascending, and their number
//   gather_rows_idx   the failing rows' channel LLRs, packed for the list decoder
//   scatter_bits_idx  the list decoder's answers back into their rows
// All four move a few bytes per element and compute next to nothing: they are bound by launch and
// memory latency, so each is one pass with coalesced row accesses and no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/polar_mi355x.h"
#include "hybrid.h"
#include "plan.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxK = 2048;

// XOR of v over the 16 lanes of each DPP row, in every lane (row_ror:8, 4, 2, 1).
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_xor(uint32_t v) {
    return v ^ (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
// XOR of v over the wave, wave-uniform.  All 64 lanes must be active.
__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
    v = dpp_xor<0x128>(v);
    v = dpp_xor<0x124>(v);
    v = dpp_xor<0x122>(v);
    v = dpp_xor<0x121>(v);
    return (uint32_t)(__builtin_amdgcn_readlane((int)v, 0) ^ __builtin_amdgcn_readlane((int)v, 16) ^
                      __builtin_amdgcn_readlane((int)v, 32) ^ __builtin_amdgcn_readlane((int)v, 48));
}

// The CRC register of the SCL kernels (scl_kernel.hip: fb = msb ^ bit; reg <<= 1; if fb reg ^= g)
// is linear in the bits: after k bits it holds sum_m bit[m] * x^(deg + k-1-m) mod G, G = x^deg + g.
// So one row costs k/64 table look-ups per lane and one wave XOR.  The table rem[j] = x^(deg+j)
// mod G, j < k, is built per block in LDS: the first 64 entries by stepping (lane j: j times x),
// then by doubling, rem[j] = rem[j-c] * x^c with x^c = rem[c - deg] read back from the table.
template <typename T>
__global__ __launch_bounds__(kThreads) void crc_flag(const T* __restrict__ bits, int64_t bs, int k, int deg, uint32_t g,
                                                     const int32_t* __restrict__ idx, uint8_t* __restrict__ valid) {
    __shared__ uint32_t s_rem[kMaxK];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t mask = deg >= 32 ? 0xffffffffu : (1u << deg) - 1u;
    const int top = deg - 1;
    g &= mask;
    auto times_x = [&](uint32_t a) { return ((a << 1) & mask) ^ (((a >> top) & 1u) ? g : 0u); };
    if (tid < 64) {
        uint32_t v = g;  // x^deg mod G
        for (int i = 0; i < 63; ++i)
            if (i < tid) v = times_x(v);
        if (tid < k) s_rem[tid] = v;
    }
    __syncthreads();
    for (int c = 64; c < k; c <<= 1) {
        const uint32_t xc = s_rem[c - deg];  // x^c mod G (deg <= 32 < c)
        const int end = 2 * c < k ? 2 * c : k;
        for (int j = c + tid; j < end; j += kThreads) {
            const uint32_t a = s_rem[j - c];
            uint32_t r = 0u;
            for (int i = top; i >= 0; --i) {
                r = times_x(r);
                if ((xc >> i) & 1u) r ^= a;
            }
            s_rem[j] = r;
        }
        __syncthreads();
    }
    // one wave per row, lane l the bits l, l + 64, ... (coalesced), rows by grid stride
    for (int64_t b = (int64_t)blockIdx.x * kWaves + (tid >> 6); b < bs; b += (int64_t)gridDim.x * kWaves) {
        const T* x = bits + b * k;
        uint32_t acc = 0u;
        for (int m = lane; m < k; m += 64)
            if (x[m] != (T)0) acc ^= s_rem[k - 1 - m];
        acc = wave_xor(acc);
        if (lane == 0) valid[idx ? (int64_t)idx[b] : b] = acc == 0u ? 1 : 0;
    }
}

// compact_failed, two launches, stable: block q owns rows [q * span, (q+1) * span); it counts its
// failing rows (count), then every block sums the counts before it and writes its own indices in
// order (write): wave ballot + popcount for the place in the wave, LDS for the waves of the block.
__global__ __launch_bounds__(kThreads) void compact_failed_count(const uint8_t* __restrict__ valid, int64_t bs,
                                                                 int64_t span, int32_t* __restrict__ counts) {
    __shared__ int s_w[kWaves];
    const int tid = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.x * span, b1 = b0 + span < bs ? b0 + span : bs;
    int w = 0;
    for (int64_t base = b0; base < b1; base += kThreads) {  // uniform trip count: every lane ballots
        const int64_t r = base + tid;
        const bool fail = r < b1 && valid[r] == 0;
        w += __popcll(__ballot(fail));
    }
    if ((tid & 63) == 0) s_w[tid >> 6] = w;
    __syncthreads();
    if (tid == 0) {
        int c = 0;
        for (int i = 0; i < kWaves; ++i) c += s_w[i];
        counts[blockIdx.x] = c;
    }
}

__global__ __launch_bounds__(kThreads) void compact_failed_write(const uint8_t* __restrict__ valid, int64_t bs,
                                                                 int64_t span, const int32_t* __restrict__ counts,
                                                                 int32_t* __restrict__ rows,
                                                                 int64_t* __restrict__ n_fail) {
    __shared__ int s_w[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // rows that fail in the blocks before this one (at most kCompactMaxBlocks counts)
    int part = 0;
    for (int i = tid; i < (int)blockIdx.x; i += kThreads) part += counts[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off, 64);
    if (lane == 0) s_w[wave] = part;
    __syncthreads();
    int64_t offset = 0;
    for (int i = 0; i < kWaves; ++i) offset += s_w[i];
    __syncthreads();
    const int64_t b0 = (int64_t)blockIdx.x * span, b1 = b0 + span < bs ? b0 + span : bs;
    for (int64_t base = b0; base < b1; base += kThreads) {
        const int64_t r = base + tid;
        const bool fail = r < b1 && valid[r] == 0;
        const unsigned long long bal = __ballot(fail);
        if (lane == 0) s_w[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
        for (int i = 0; i < kWaves; ++i) {
            if (i < wave) before += s_w[i];
            total += s_w[i];
        }
        if (fail) rows[offset + before + __popcll(bal & ((1ull << lane) - 1ull))] = (int32_t)r;
        offset += total;
        __syncthreads();
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) *n_fail = offset;
}

// Rows of `units` elements of U, 2^log_lpr lanes per row (64 >> log_lpr rows per wave).
// SCATTER: dst[idx[j]] = src[j]; else dst[j] = src[idx[j]].
template <typename U, bool SCATTER>
__device__ __forceinline__ void copy_rows_idx(const U* __restrict__ src, U* __restrict__ dst,
                                              const int32_t* __restrict__ idx, int64_t cnt, int units, int log_lpr) {
    const int lane = threadIdx.x & 63, lpr = 1 << log_lpr;
    const int64_t wave = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const int64_t j = (wave << (6 - log_lpr)) + (lane >> log_lpr);
    if (j >= cnt) return;
    const int64_t r = idx[j];
    const U* s = src + (SCATTER ? j : r) * units;
    U* d = dst + (SCATTER ? r : j) * units;
    for (int i = lane & (lpr - 1); i < units; i += lpr) d[i] = s[i];
}

template <typename U>
__global__ __launch_bounds__(kThreads) void gather_rows_idx(const U* __restrict__ src, U* __restrict__ dst,
                                                            const int32_t* __restrict__ idx, int64_t cnt, int units,
                                                            int log_lpr) {
    copy_rows_idx<U, false>(src, dst, idx, cnt, units, log_lpr);
}

template <typename U>
__global__ __launch_bounds__(kThreads) void scatter_bits_idx(const U* __restrict__ src, U* __restrict__ dst,
                                                             const int32_t* __restrict__ idx, int64_t cnt, int units,
                                                             int log_lpr) {
    copy_rows_idx<U, true>(src, dst, idx, cnt, units, log_lpr);
}

// The widest unit (16, 4 or 1 bytes) that divides the row and both base addresses.
int unit_bytes(const void* a, const void* b, size_t row_bytes) {
    const uintptr_t m = (uintptr_t)a | (uintptr_t)b | (uintptr_t)row_bytes;
    return (m & 15u) == 0 ? 16 : (m & 3u) == 0 ? 4 : 1;
}

template <bool SCATTER>
int launch_copy_rows(const void* src, void* dst, const int32_t* idx, int64_t cnt, size_t row_bytes, hipStream_t st,
                     const char* what) {
    if (cnt == 0 || row_bytes == 0) return PL_OK;
    const int ub = unit_bytes(src, dst, row_bytes);
    const int units = (int)(row_bytes / ub);
    int log_lpr = 0;
    while (log_lpr < 6 && (1 << log_lpr) < units) ++log_lpr;
    const int64_t rows_per_block = (int64_t)kWaves << (6 - log_lpr);
    const int64_t blocks = (cnt + rows_per_block - 1) / rows_per_block;
    if (blocks > 0x7fffffffLL) {
        pl::set_error(std::string(what) + ": too many rows");
        return PL_EINVAL;
    }
    const dim3 grid((unsigned)blocks), block(kThreads);
#define PL_COPY(U)                                                                                                  \
    if (SCATTER)                                                                                                    \
        hipLaunchKernelGGL(scatter_bits_idx<U>, grid, block, 0, st, static_cast<const U*>(src), static_cast<U*>(dst), \
                           idx, cnt, units, log_lpr);                                                               \
    else                                                                                                            \
        hipLaunchKernelGGL(gather_rows_idx<U>, grid, block, 0, st, static_cast<const U*>(src), static_cast<U*>(dst),  \
                           idx, cnt, units, log_lpr);
    if (ub == 16) {
        PL_COPY(uint4)
    } else if (ub == 4) {
        PL_COPY(uint32_t)
    } else {
        PL_COPY(uint8_t)
    }
#undef PL_COPY
    return pl::check_hip(hipGetLastError(), what);
}

}  // namespace

namespace pl {

int launch_crc_flag(const void* bits, int kind, int64_t bs, int k, int deg, uint32_t g, const int32_t* idx,
                    uint8_t* valid, hipStream_t st) {
    if (deg < 1 || deg > 32 || k < deg || k > kMaxK) {
        set_error("CRC flag: needs 1 <= degree <= 32 and degree <= k <= 2048");
        return PL_EINVAL;
    }
    if (bs == 0) return PL_OK;
    // two rows per wave where the batch allows, so the table built per block serves eight rows
    int64_t blocks = (bs + 2 * kWaves - 1) / (2 * kWaves);
    if (blocks > 2048) blocks = 2048;
    const dim3 grid((unsigned)blocks), block(kThreads);
    if (kind == PL_OUT_F32)
        hipLaunchKernelGGL(crc_flag<float>, grid, block, 0, st, static_cast<const float*>(bits), bs, k, deg, g, idx,
                           valid);
    else
        hipLaunchKernelGGL(crc_flag<uint8_t>, grid, block, 0, st, static_cast<const uint8_t*>(bits), bs, k, deg, g,
                           idx, valid);
    return check_hip(hipGetLastError(), "CRC flag launch");
}

int launch_compact_failed(const uint8_t* valid, int64_t bs, int32_t* block_counts, int32_t* rows, int64_t* n_fail,
                          hipStream_t st) {
    if (bs <= 0 || bs > 0x7fffffffLL) {
        set_error("compact: the batch must have 1 ... 2^31 - 1 rows (int32 row indices)");
        return PL_EINVAL;
    }
    // at most kCompactMaxBlocks blocks, each over a multiple of the block size
    int64_t span = (bs + kCompactMaxBlocks - 1) / kCompactMaxBlocks;
    span = (span + kThreads - 1) / kThreads * kThreads;
    const int64_t blocks = (bs + span - 1) / span;
    hipLaunchKernelGGL(compact_failed_count, dim3((unsigned)blocks), dim3(kThreads), 0, st, valid, bs, span,
                       block_counts);
    hipLaunchKernelGGL(compact_failed_write, dim3((unsigned)blocks), dim3(kThreads), 0, st, valid, bs, span,
                       static_cast<const int32_t*>(block_counts), rows, n_fail);
    return check_hip(hipGetLastError(), "compact launch");
}

int launch_gather_rows_idx(const float* src, const int32_t* idx, int64_t cnt, int n, float* dst, hipStream_t st) {
    return launch_copy_rows<false>(src, dst, idx, cnt, (size_t)n * sizeof(float), st, "gather launch");
}

int launch_scatter_bits_idx(const void* src, const int32_t* idx, int64_t cnt, int k, int kind, void* dst,
                            hipStream_t st) {
    const size_t elem = kind == PL_OUT_F32 ? sizeof(float) : sizeof(uint8_t);
    return launch_copy_rows<true>(src, dst, idx, cnt, (size_t)k * elem, st, "scatter launch");
}

}  // namespace pl
