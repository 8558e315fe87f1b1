// genie_kernel.hip -- genie-aided SC for frozen-set design on gfx950 (pl_genie_count,
// include/polar_mi355x.h): the leaf LLR of every position when all earlier bits are fed back
// correctly, and per-position counts of the leaves whose hard decision misses the true bit.
//
// With the true u known, every partial sum is known before decoding starts: the partial sums SC
// feeds into g at stage s are the encoder butterfly (butterfly.h) of u stopped after s - 1 stages.
// So the n leaves are a log2 n-stage butterfly of (f, g) pairs over a = -logits, top stage first,
//     x = a[p], y = a[p + h], a[p] = f(x, y), a[p + h] = g(x, y, beta_{s-1}[p]),  h = 2^(s-1),
// for every p whose index bit s - 1 is 0, with no serial dependency inside a stage and no
// data-dependent control flow.  f and g are the SC decoder's fop / gop (sc_tree.h).
//
// Layout: a codeword is held by G = max(1, n / 32) lanes, element p in lane p % G, slot p / G, E =
// min(n, 32) slots a lane; a wave holds C = 64 / G codewords.  Stages with h >= G pair two slots of
// one lane; the log2 G stages below exchange with lane ^ h (DPP for h = 1, 2, 8, ds_swizzle for 4 and
// 16, ds_bpermute for 32) and both lanes evaluate f and g of the pair, each keeping its own.  The
// partial sums are one packed word per lane and stage (bit j = slot j), built bottom-up from u with
// one shift-xor or one lane exchange a stage.
//
// A wave walks its rows with a grid stride and keeps the E error counts of its lane in registers.
// At the end every lane adds them into an n-entry LDS array (integer atomics: the groups of a wave
// and the waves of a block meet there), and the block adds each nonzero entry to counts[] with one
// 64-bit atomic.  Integer sums: counts[] does not depend on the schedule.
//
// Bounds: rows past bs are clamped to row bs - 1 for the loads and masked out of the counts and
// stores; slot j < E and lane-in-group < G give p = j G + lig < n; u word indices are p / 32 <
// ceil(n / 32).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/polar_mi355x.h"
#include "exactf.h"
#include "plan.h"
#include "sc_tree.h"

namespace {

constexpr int kWaves = 4;        // waves per block
constexpr int kMinWaves = 2;     // waves per SIMD the register allocation must allow: at 3 or 4 the n >= 64 kernels spill
constexpr int kMaxBlocks = 1024;  // grid cap: 256 CUs x 2 waves per SIMD x 4 SIMDs / 4 waves a block, twice over

using pl::tree::fop;
using pl::tree::gop;

// the value of lane ^ H
template <int H>
__device__ __forceinline__ uint32_t xor_lane(uint32_t v) {
    if constexpr (H == 1)
        return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false);  // quad_perm [1,0,3,2]
    else if constexpr (H == 2)
        return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, false);  // quad_perm [2,3,0,1]
    else if constexpr (H == 8)
        return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x128, 0xF, 0xF, false);  // row_ror:8
    else if constexpr (H == 4 || H == 16)
        return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (H << 10) | 0x1F);  // bit mode: and 0x1f, xor H
    else
        return (uint32_t)__shfl_xor((int)v, H, 64);
}

// slots j of a lane whose bit log2(HS) is 0
template <int HS>
constexpr uint32_t low_mask() {
    return HS == 1 ? 0x55555555u : HS == 2 ? 0x33333333u : HS == 4 ? 0x0F0F0F0Fu : HS == 8 ? 0x00FF00FFu : 0x0000FFFFu;
}

// beta[s] = the butterfly of u stopped after s stages, s = 0 .. LOG_N - 1 (beta[0] set by the caller)
template <int LOG_N, int LOG_G, int s>
__device__ __forceinline__ void build_beta(uint32_t (&beta)[LOG_N], int lig) {
    if constexpr (s < LOG_N) {
        constexpr int H = 1 << (s - 1);
        const uint32_t b = beta[s - 1];
        if constexpr (H < (1 << LOG_G)) {
            const uint32_t o = xor_lane<H>(b);
            beta[s] = (lig & H) ? b : (b ^ o);
        } else {
            constexpr int HS = H >> LOG_G;
            beta[s] = b ^ ((b >> HS) & low_mask<HS>());
        }
        build_beta<LOG_N, LOG_G, s + 1>(beta, lig);
    }
}

// stages s, s - 1, ..., 1 of the transform
template <int LOG_N, int LOG_G, int E, int FM, int s>
__device__ __forceinline__ void stages(float (&a)[E], const uint32_t (&beta)[LOG_N], int lig, float lmax) {
    if constexpr (s >= 1) {
        constexpr int H = 1 << (s - 1);
        const uint32_t bw = beta[s - 1];
        if constexpr (H >= (1 << LOG_G)) {
            constexpr int HS = H >> LOG_G;
#pragma unroll
            for (int j = 0; j < E; ++j)
                if ((j & HS) == 0) {
                    const float x = a[j], y = a[j + HS];
                    a[j] = fop<FM>(x, y, lmax);
                    a[j + HS] = gop(x, y, (bw >> j) & 1u);
                }
        } else {
            const bool hi = (lig & H) != 0;
            const uint32_t bo = xor_lane<H>(bw);  // exchanged by every lane: never inside the select
            const uint32_t bl = hi ? bo : bw;     // the low lane's partial sums
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const float mine = a[j];
                const float o = __uint_as_float(xor_lane<H>(__float_as_uint(mine)));
                const float x = hi ? o : mine, y = hi ? mine : o;
                const float f = fop<FM>(x, y, lmax);
                const float g = gop(x, y, (bl >> j) & 1u);
                a[j] = hi ? g : f;
            }
        }
        stages<LOG_N, LOG_G, E, FM, s - 1>(a, beta, lig, lmax);
    }
}

template <int LOG_N, int FM>
__global__ __launch_bounds__(64 * kWaves, kMinWaves) void genie_kernel(const float* __restrict__ llr,
                                                               const uint32_t* __restrict__ ubits, int64_t bs,
                                                               unsigned long long* __restrict__ counts,
                                                               float* __restrict__ leaf, float lmax) {
    constexpr int LOG_E = LOG_N < 5 ? LOG_N : 5, LOG_G = LOG_N - LOG_E;
    constexpr int N = 1 << LOG_N, E = 1 << LOG_E, G = 1 << LOG_G, C = 64 / G;
    constexpr int NW = (N + 31) / 32;  // u words a row
    __shared__ uint32_t s_cnt[N];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lig = lane & (G - 1), grp = lane >> LOG_G;
    for (int i = tid; i < N; i += 64 * kWaves) s_cnt[i] = 0u;
    if constexpr (FM == 1)
        plx::load_tables(tid, 64 * kWaves);  // ends with a barrier
    else
        __syncthreads();

    uint32_t cnt[E];
#pragma unroll
    for (int j = 0; j < E; ++j) cnt[j] = 0u;

    const int64_t iters = (bs + C - 1) / C;  // C rows per wave and iteration
    for (int64_t it = (int64_t)blockIdx.x * kWaves + wave; it < iters; it += (int64_t)gridDim.x * kWaves) {
        const int64_t cw = it * C + grp;
        const bool valid = cw < bs;
        const int64_t row = valid ? cw : bs - 1;
        const float* x = llr + row * N;
        const uint32_t* urow = ubits + row * NW;

        float a[E];
#pragma unroll
        for (int j = 0; j < E; ++j) a[j] = -x[j * G + lig];

        uint32_t beta[LOG_N];
        uint32_t b0 = 0u;
        if constexpr (G >= 32) {
#pragma unroll
            for (int j = 0; j < E; ++j) b0 |= ((urow[j * (G / 32) + (lig >> 5)] >> (lig & 31)) & 1u) << j;
        } else {  // G divides 32: slot j sits in word j G / 32 at bit (j G) % 32 + lig
            uint32_t w[NW];
#pragma unroll
            for (int i = 0; i < NW; ++i) w[i] = urow[i];
#pragma unroll
            for (int j = 0; j < E; ++j) b0 |= ((w[(j * G) >> 5] >> (((j * G) & 31) + lig)) & 1u) << j;
        }
        beta[0] = b0;
        build_beta<LOG_N, LOG_G, 1>(beta, lig);

        stages<LOG_N, LOG_G, E, FM, LOG_N>(a, beta, lig, lmax);

        const uint32_t v = valid ? 1u : 0u;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const uint32_t hd = (a[j] > 0.0f) ? 0u : 1u;
            cnt[j] += (hd ^ ((b0 >> j) & 1u)) & v;
        }
        if (leaf != nullptr && valid) {
            float* o = leaf + cw * N;
#pragma unroll
            for (int j = 0; j < E; ++j) o[j * G + lig] = a[j];
        }
    }

    if (counts != nullptr) {  // uniform over the grid
#pragma unroll
        for (int j = 0; j < E; ++j)
            if (cnt[j] != 0u) atomicAdd(&s_cnt[j * G + lig], cnt[j]);
        __syncthreads();
        for (int i = tid; i < N; i += 64 * kWaves) {
            const uint32_t c = s_cnt[i];
            if (c != 0u) atomicAdd(&counts[i], (unsigned long long)c);
        }
    }
}

template <int LOG_N>
void launch_n(int f_mode, const float* llr, const uint32_t* ubits, int64_t bs, int64_t* counts, float* leaf,
              float lmax, hipStream_t st) {
    constexpr int LOG_E = LOG_N < 5 ? LOG_N : 5, C = 64 >> (LOG_N - LOG_E);
    const int64_t per_block = (int64_t)kWaves * C;
    int64_t blocks = (bs + per_block - 1) / per_block;
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    unsigned long long* c = reinterpret_cast<unsigned long long*>(counts);
    if (f_mode == PL_F_MINSUM)
        hipLaunchKernelGGL((genie_kernel<LOG_N, 0>), dim3((unsigned)blocks), dim3(64 * kWaves), 0, st, llr, ubits, bs, c,
                           leaf, lmax);
    else
        hipLaunchKernelGGL((genie_kernel<LOG_N, 1>), dim3((unsigned)blocks), dim3(64 * kWaves), 0, st, llr, ubits, bs, c,
                           leaf, lmax);
}

int einval(const char* msg) {
    pl::set_error(std::string("pl_genie_count: ") + msg);
    return PL_EINVAL;
}

}  // namespace

extern "C" {

int pl_genie_count(int32_t n, int32_t f_mode, float llr_max, const float* llr_logits, const uint32_t* u_bits,
                   int64_t bs, int64_t* counts, float* leaf_out, void* hip_stream) {
    int log_n = 0;
    while ((1 << log_n) < n && log_n < 12) ++log_n;
    if (n < 2 || n > 2048 || (1 << log_n) != n) return einval("n must be a power of two in [2, 2048]");
    if (f_mode != PL_F_MINSUM && f_mode != PL_F_EXACT) return einval("f_mode must be PL_F_MINSUM or PL_F_EXACT");
    if (!(llr_max > 0.0f)) return einval("llr_max must be positive");
    if (bs < 0) return einval("bs must be >= 0");
    if (bs > ((int64_t)1 << 40)) return einval("bs must be <= 2^40");
    if (!counts && !leaf_out) return einval("counts and leaf_out are both NULL: nothing to compute");
    if (bs == 0) return PL_OK;
    if (!llr_logits) return einval("llr_logits is NULL");
    if (!u_bits) return einval("u_bits is NULL");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    switch (log_n) {
        case 1: launch_n<1>(f_mode, llr_logits, u_bits, bs, counts, leaf_out, llr_max, st); break;
        case 2: launch_n<2>(f_mode, llr_logits, u_bits, bs, counts, leaf_out, llr_max, st); break;
        case 3: launch_n<3>(f_mode, llr_logits, u_bits, bs, counts, leaf_out, llr_max, st); break;
        case 4: launch_n<4>(f_mode, llr_logits, u_bits, bs, counts, leaf_out, llr_max, st); break;
        case 5: launch_n<5>(f_mode, llr_logits, u_bits, bs, counts, leaf_out, llr_max, st); break;
        case 6: launch_n<6>(f_mode, llr_logits, u_bits, bs, counts, leaf_out, llr_max, st); break;
        case 7: launch_n<7>(f_mode, llr_logits, u_bits, bs, counts, leaf_out, llr_max, st); break;
        case 8: launch_n<8>(f_mode, llr_logits, u_bits, bs, counts, leaf_out, llr_max, st); break;
        case 9: launch_n<9>(f_mode, llr_logits, u_bits, bs, counts, leaf_out, llr_max, st); break;
        case 10: launch_n<10>(f_mode, llr_logits, u_bits, bs, counts, leaf_out, llr_max, st); break;
        default: launch_n<11>(f_mode, llr_logits, u_bits, bs, counts, leaf_out, llr_max, st); break;
    }
    return pl::check_hip(hipGetLastError(), "pl_genie_count launch");
}

}  // extern "C"
