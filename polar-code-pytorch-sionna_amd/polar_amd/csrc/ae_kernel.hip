// ae_kernel.hip -- automorphism-ensemble SC decoding (pl_ae_decode, include/polar_mi355x.h) for gfx950
// (wave64).
//
// AED (Geiselhart, Elkelesh, Ebada, Cammerer, ten Brink 2021): decode M permuted copies of the received
// word with plain SC, un-permute the M candidate codewords and keep the one closest to the received word.
// One wave (= one work-group) per row; the C = 64/G lane groups of the wave each run a whole register-tree
// SC decode (sc_tree.h) of the same row, every group through another permutation:
//
//   1. a = -logits of the row goes to LDS once (s_a).
//   2. ceil(M / C) passes.  Group `slot` of pass `base` decodes candidate t = base + slot: its root LLRs
//      are a'[i] = s_a[pi_t(i)], gathered where the tree asks for them (the two top stages are recomputed,
//      so a position is gathered up to four times a decode).  pi_t is read from global memory through the
//      cache (at most 128 KiB of tables for the whole grid); every entry is masked with n - 1, so a bad
//      table cannot index outside the row.  Groups with t >= M decode candidate M - 1 again and carry the
//      key ~0: the tree's control flow depends on the frozen set alone and stays uniform over the wave.
//   3. Metric, from the root partial sums x' before the encoder butterfly and the same gathered a':
//      m = sum |a'_i| [x'_i != HD(a'_i)], fp32, per lane over its slots in ascending order, then over the
//      group's lanes by DPP.  Key (bits of m) << 32 | t: the wave minimum is the smallest metric, the
//      lowest t among equal ones (metrics are non-negative).
//   4. A running best key over the passes (strictly smaller replaces: earlier passes hold the lower t).
//      When a pass improves it, the winning group scatters its x' to s_x[pi_t(i)]: the candidate
//      codeword in natural order.
//   5. After the last pass: u = x G_n by the encoder butterfly on s_x in LDS (log2 n stages of byte XORs).
//   6. out[m] = s_x[info_pos[m]]; lane 0 stores best_idx and best_metric.
//
// Bounds: row < bs; tree positions j G + lig < n; table rows min(t, M - 1) < M and entries & (n - 1) < n;
// info_pos[m] < n for m < k (the plan's own table).  LDS: 4 n + max(n, 4) bytes, and the exact f's tables.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/polar_mi355x.h"
#include "ae.h"
#include "exactf.h"
#include "plan.h"
#include "sc_tree.h"

namespace {

using namespace pl::tree;

constexpr int kMaxBlocks = 4096;  // grid cap, as the flip kernel: 16 waves for each of 256 CUs

// Root LLRs of one candidate: the row's a[] in LDS read through its permutation
template <int N>
struct PermRoot {
    const float* s_a;
    const uint16_t* __restrict__ pi;
    __device__ __forceinline__ int src(int i) const { return pi[i] & (N - 1); }
    __device__ __forceinline__ float at(int i) const { return s_a[src(i)]; }
};

// Sum over the G <= 8 lanes of a group, the same bits in every lane (each step adds two equal-shaped
// partial sums, and fp32 addition commutes)
template <int G>
__device__ __forceinline__ float grp_sum(float v) {
    static_assert(G <= 8, "group wider than the DPP steps below");
    if constexpr (G >= 2) v += dppf<0xB1>(v);   // quad_perm [1,0,3,2]
    if constexpr (G >= 4) v += dppf<0x4E>(v);   // quad_perm [2,3,0,1]
    if constexpr (G >= 8) v += dppf<0x141>(v);  // row_half_mirror
    return v;
}

template <int LOG_N, int FM>
__global__ __launch_bounds__(64) void ae_kernel(const float* __restrict__ llr, int64_t bs,
                                                const uint16_t* __restrict__ perms, int num_perms, void* out,
                                                int out_kind, int32_t* best_idx, float* best_metric,
                                                const uint32_t* __restrict__ frozen_words,
                                                const uint32_t* __restrict__ type_words,
                                                const int32_t* __restrict__ info_pos, int k, float lmax) {
    constexpr int LOG_G = (LOG_N > 7) ? (LOG_N - 7) : 0;
    constexpr int N = 1 << LOG_N, G = 1 << LOG_G, C = 64 / G;
    constexpr int NSL = N / G;          // slots per lane (<= 128)
    constexpr int WPC = (N + 31) / 32;  // frozen words
    __shared__ float s_a[N];
    __shared__ uint8_t s_x[N < 4 ? 4 : N];

    const int lane = threadIdx.x;
    Ctx c;
    c.vfrozen = lane < WPC ? frozen_words[lane] : 0u;
    c.vr0 = type_words[lane];  // plane 0 of the node type flags: rate-0
    c.lane = lane;
    c.lig = lane & (G - 1);
    c.flip = -1;
    c.lmax = lmax;
    if constexpr (FM == 1) plx::load_tables(lane, 64);  // the exact f's exp / log tables

    const int slot = lane >> LOG_G;
    for (int64_t row = blockIdx.x; row < bs; row += gridDim.x) {
        const float* ch = llr + row * N;
        for (int i = lane; i < N; i += 64) s_a[i] = -ch[i];
        __syncthreads();

        uint64_t best = ~0ull;
        for (int base = 0; base < num_perms; base += C) {
            const int t = base + slot;
            const bool live = t < num_perms;
            const PermRoot<N> root{s_a, perms + (size_t)(live ? t : num_perms - 1) * N};
            uint64_t lo, hi;
            decode_x<LOG_N, LOG_G, FM>(root, c, lo, hi);

            float m = 0.0f;
#pragma unroll 8
            for (int j = 0; j < NSL; ++j) {
                const float a = root.at(j * G + c.lig);
                const uint32_t bit = j < 64 ? bitof(lo, j) : bitof(hi, j - 64);
                m += bit != hd(a) ? fabsf(a) : 0.0f;
            }
            m = grp_sum<G>(m);
            uint64_t key = live ? ((uint64_t)__float_as_uint(m) << 32) | (uint32_t)t : ~0ull;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const uint64_t o = (uint64_t)__shfl_xor((long long)key, off, 64);
                key = o < key ? o : key;
            }
            if (key < best) {  // uniform: the pass's winner replaces the codeword kept so far
                best = key;
                if (t == (int)(uint32_t)key) {
#pragma unroll 8
                    for (int j = 0; j < NSL; ++j) {
                        const uint32_t bit = j < 64 ? bitof(lo, j) : bitof(hi, j - 64);
                        s_x[root.src(j * G + c.lig)] = (uint8_t)bit;
                    }
                }
                __syncthreads();
            }
        }

        // u = x G_n on the winner's codeword
        for (int s = 1; s <= LOG_N; ++s) {
            const int h = 1 << (s - 1);
            for (int idx = lane; idx < N / 2; idx += 64) {
                const int p = low_pos(idx, h);
                s_x[p] ^= s_x[p + h];
            }
            __syncthreads();
        }
        for (int m = lane; m < k; m += 64) {
            const uint32_t bit = s_x[info_pos[m]];
            if (out_kind == PL_OUT_F32)
                static_cast<float*>(out)[row * k + m] = bit ? 1.0f : 0.0f;
            else
                static_cast<uint8_t*>(out)[row * k + m] = (uint8_t)bit;
        }
        if (lane == 0) {
            if (best_idx) best_idx[row] = (int32_t)(uint32_t)best;
            if (best_metric) best_metric[row] = __uint_as_float((uint32_t)(best >> 32));
        }
        __syncthreads();  // s_a and s_x are reused by the next row
    }
}

template <int LOG_N>
void launch_n(const pl_plan* p, const float* llr, int64_t bs, const uint16_t* perms, int num_perms, void* out,
              int out_kind, int32_t* best_idx, float* best_metric, hipStream_t st) {
    const unsigned blocks = (unsigned)(bs < kMaxBlocks ? bs : kMaxBlocks);
    if (p->f_mode == PL_F_MINSUM)
        hipLaunchKernelGGL((ae_kernel<LOG_N, 0>), dim3(blocks), dim3(64), 0, st, llr, bs, perms, num_perms, out,
                           out_kind, best_idx, best_metric, p->d_frozen_words, p->d_type_words, p->d_info_pos, p->k,
                           p->llr_max);
    else
        hipLaunchKernelGGL((ae_kernel<LOG_N, 1>), dim3(blocks), dim3(64), 0, st, llr, bs, perms, num_perms, out,
                           out_kind, best_idx, best_metric, p->d_frozen_words, p->d_type_words, p->d_info_pos, p->k,
                           p->llr_max);
}

}  // namespace

namespace pl {

int launch_ae(const pl_plan* p, const float* llr, int64_t bs, const uint16_t* perms, int num_perms, void* out,
              int out_kind, int32_t* best_idx, float* best_metric, hipStream_t st) {
    if (bs == 0) return PL_OK;
    if (num_perms < 1 || num_perms > kAeMaxPerms) {
        set_error("automorphism-ensemble decoding: needs 1 <= num_perms <= 64");
        return PL_EINVAL;
    }
#define PL_AE_CASE(LN) \
    case LN: launch_n<LN>(p, llr, bs, perms, num_perms, out, out_kind, best_idx, best_metric, st); break;
    switch (p->log_n) {
        PL_AE_CASE(1) PL_AE_CASE(2) PL_AE_CASE(3) PL_AE_CASE(4) PL_AE_CASE(5)
        PL_AE_CASE(6) PL_AE_CASE(7) PL_AE_CASE(8) PL_AE_CASE(9) PL_AE_CASE(10)
        default: set_error("automorphism-ensemble decoding: n must be a power of two in [2, 1024]"); return PL_ENOTSUP;
    }
#undef PL_AE_CASE
    return check_hip(hipGetLastError(), "automorphism-ensemble launch");
}

}  // namespace pl
