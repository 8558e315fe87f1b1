// bp_kernel.hip -- iterative belief-propagation polar decoding with soft output on gfx950
// (pl_bp_decode, include/polar_mi355x.h; the "BP" decoder my_sn/fec/polar/dec.py names).
//
// The factor graph is the encoder butterfly (butterfly.h): S = log2 n stages of n / 2 units; the unit
// of stage s at p (index bit s - 1 of p clear, h = 2^(s-1)) joins (s-1, p), (s-1, p+h), (s, p), (s, p+h).
// L[s][i] runs towards the u side, R[s][i] towards the channel side; L[S] is the clipped channel row,
// R[0] is +llr_max at frozen positions and 0 elsewhere.  One iteration is an R pass over s = 1 .. S and
// an L pass over s = S .. 1; inside a stage every message is written once and reads only the
// neighbouring stage, so the schedule below (one unit a thread, a barrier a stage) computes exactly the
// values the header states.
//
// Layout: a codeword is held by its n / 2 unit threads and (2 S + 1) n fp32 of LDS -- L[0 .. S], then
// R[1 .. S], row s at s n -- never by HBM; R[0] is two registers (the frozen bits of the thread's
// stage-1 unit).  A work-group has max(256, n / 2) threads and holds C = threads / (n / 2) codewords
// (256 at n = 2, 1 at n >= 512); for n <= 32, where several codewords share a 32-lane half, the codeword
// stride is padded by one float so that they start on different banks.  Thread t of a codeword owns unit
// t of every stage, p = ((t >> (s-1)) << s) | (t & (h-1)), and positions t and t + n/2 for the loads, the
// early-stop bits and the stores.  ds_read_b32 banks are (address / 4) % 32 per 32-lane half: stages
// with h >= 32 read consecutive floats, the stages below read two runs that share banks (2-way).
//
// Early stop: the hard decisions u^ (frozen positions 0) and x^ = !(L[S] + R[S] > 0) are packed with
// wave ballots; n <= 64 runs the butterfly on one 64-bit word in every lane, n >= 128 on n / 32 words
// in the first wave of the codeword (pl::polar_butterfly).  A stopped codeword leaves its messages as
// they are and only keeps meeting the barriers; the work-group leaves the loop when none is active.
//
// Bounds: row = group * C + c is clamped to bs - 1 for the loads and masked out of the iterations and
// the stores; p + h < n by construction (bit s - 1 of p is clear); positions t, t + n/2 < n; frozen and
// packed words are indexed by position / 32 < ceil(n / 32); info_rank[i] < k.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/polar_mi355x.h"
#include "butterfly.h"
#include "exactf.h"
#include "plan.h"

namespace {

constexpr int kMaxBlocks = 1024;  // grid cap; a work-group walks the rows with a grid stride

using plx::clip_l;

template <int FM>
__device__ __forceinline__ float fop(float x, float y, float lmax, float scale) {
    if constexpr (FM == 0) {  // genie_kernel.hip fop<0>, the magnitude scaled (one rounding) before the sign goes on
        const float m = fminf(fminf(fabsf(x), fabsf(y)), lmax) * scale;
        const uint32_t sg = (__float_as_uint(x) ^ __float_as_uint(y)) & 0x80000000u;
        return __uint_as_float(__float_as_uint(m) | sg);
    } else {
        return plx::f_exact(x, y, lmax);
    }
}

// positions of a 64-bit word whose index bit log2(h) is 0
__device__ __forceinline__ unsigned long long span_mask64(int h) {
    return h == 32 ? 0x00000000FFFFFFFFull : (unsigned long long)pl::span_mask(h) * 0x0000000100000001ull;
}

template <int LOG_N>
struct Geo {
    static constexpr int S = LOG_N, N = 1 << LOG_N, TPC = N / 2;  // threads per codeword: one per unit
    static constexpr int T = TPC > 256 ? TPC : 256;               // threads per work-group
    static constexpr int C = T / TPC;                             // codewords per work-group
    static constexpr int STRIDE = (2 * S + 1) * N + (N <= 32 ? 1 : 0);
    static constexpr int NW = N >= 128 ? N / 32 : 1;  // packed words of a codeword (the n >= 128 early stop)
};

template <int LOG_N>
struct Shared {
    using G = Geo<LOG_N>;
    float m[G::C][G::STRIDE];
    uint32_t uw[G::C][G::NW], xw[G::C][G::NW];  // n >= 128: the packed u^ and x^
    uint32_t stop[G::C];
    uint32_t alive;
};

template <int LOG_N, int FM>
__global__ __launch_bounds__(Geo<LOG_N>::T) void bp_kernel(const float* __restrict__ llr,
                                                           const uint32_t* __restrict__ frozen_words,
                                                           const int32_t* __restrict__ info_rank, int64_t bs, int k,
                                                           int num_iter, float scale, int early_stop, float lmax,
                                                           void* __restrict__ out_bits, int out_kind,
                                                           float* __restrict__ soft_u, float* __restrict__ ext_x,
                                                           int32_t* __restrict__ iters) {
    using G = Geo<LOG_N>;
    constexpr int S = G::S, N = G::N, TPC = G::TPC, T = G::T, C = G::C, NW = G::NW;
    __shared__ Shared<LOG_N> sm;

    const int tid = threadIdx.x, lane = tid & 63;
    const int c = tid / TPC, t = tid % TPC;
    if constexpr (FM == 1) plx::load_tables(tid, T);  // ends with a barrier

    // the thread's two positions (loads, early stop, stores) and the R[0] of its stage-1 unit
    const int i0 = t, i1 = t + TPC;
    const int rank0 = info_rank[i0], rank1 = info_rank[i1];
    const uint32_t fw = frozen_words[(2 * t) >> 5] >> ((2 * t) & 31);
    const float r0a = (fw & 1u) ? lmax : 0.0f, r0b = (fw & 2u) ? lmax : 0.0f;

    float* const M = sm.m[c];
    float* const Ls = M;                // L[s][p] = Ls[s N + p], s = 0 .. S
    float* const Rs = M + (S + 1) * N;  // R[s][p] = Rs[(s - 1) N + p], s = 1 .. S

    const int64_t groups = (bs + C - 1) / C;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t cw = g * C + c;
        const bool valid = cw < bs;
        const float* x = llr + (valid ? cw : bs - 1) * N;
        Ls[S * N + i0] = clip_l(-x[i0], lmax);
        Ls[S * N + i1] = clip_l(-x[i1], lmax);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            Ls[s * N + i0] = 0.0f;
            Ls[s * N + i1] = 0.0f;
        }
        __syncthreads();

        bool act = valid;
        int done = num_iter;
        for (int it = 0; it < num_iter; ++it) {
            for (int s = 1; s <= S; ++s) {  // R pass
                if (act) {
                    const int h = 1 << (s - 1), p = ((t >> (s - 1)) << s) | (t & (h - 1));
                    const float ra = s == 1 ? r0a : Rs[(s - 2) * N + p], rb = s == 1 ? r0b : Rs[(s - 2) * N + p + h];
                    const float la = Ls[s * N + p], lb = Ls[s * N + p + h];
                    Rs[(s - 1) * N + p] = clip_l(fop<FM>(ra, lb + rb, lmax, scale), lmax);
                    Rs[(s - 1) * N + p + h] = clip_l(fop<FM>(ra, la, lmax, scale) + rb, lmax);
                }
                __syncthreads();
            }
            for (int s = S; s >= 1; --s) {  // L pass
                if (act) {
                    const int h = 1 << (s - 1), p = ((t >> (s - 1)) << s) | (t & (h - 1));
                    const float ra = s == 1 ? r0a : Rs[(s - 2) * N + p], rb = s == 1 ? r0b : Rs[(s - 2) * N + p + h];
                    const float la = Ls[s * N + p], lb = Ls[s * N + p + h];
                    Ls[(s - 1) * N + p] = clip_l(fop<FM>(la, lb + rb, lmax, scale), lmax);
                    Ls[(s - 1) * N + p + h] = clip_l(fop<FM>(la, ra, lmax, scale) + lb, lmax);
                }
                __syncthreads();
            }
            if (early_stop) {  // uniform over the grid
                const bool u0 = rank0 >= 0 && !(Ls[i0] > 0.0f), u1 = rank1 >= 0 && !(Ls[i1] > 0.0f);
                const bool x0 = !(Ls[S * N + i0] + Rs[(S - 1) * N + i0] > 0.0f);
                const bool x1 = !(Ls[S * N + i1] + Rs[(S - 1) * N + i1] > 0.0f);
                const unsigned long long bu0 = __ballot(u0), bu1 = __ballot(u1);
                const unsigned long long bx0 = __ballot(x0), bx1 = __ballot(x1);
                bool stop = false;
                if (tid == 0) sm.alive = 0u;
                if constexpr (N >= 128) {  // a wave holds positions 64 w .. 64 w + 63 and n/2 + the same
                    if (lane == 0) {
                        const int w0 = (t >> 6) * 2, w1 = (TPC >> 5) + w0;
                        sm.uw[c][w0] = (uint32_t)bu0, sm.uw[c][w0 + 1] = (uint32_t)(bu0 >> 32);
                        sm.uw[c][w1] = (uint32_t)bu1, sm.uw[c][w1 + 1] = (uint32_t)(bu1 >> 32);
                        sm.xw[c][w0] = (uint32_t)bx0, sm.xw[c][w0 + 1] = (uint32_t)(bx0 >> 32);
                        sm.xw[c][w1] = (uint32_t)bx1, sm.xw[c][w1 + 1] = (uint32_t)(bx1 >> 32);
                    }
                    __syncthreads();
                    if (t < 64) {  // the codeword's first wave, whole
                        const bool mine = t < NW;
                        const uint32_t e = pl::polar_butterfly(mine ? sm.uw[c][mine ? t : 0] : 0u, 32, NW, t);
                        stop = __ballot(mine && e != sm.xw[c][mine ? t : 0]) == 0ull;
                        if (t == 0) sm.stop[c] = stop ? 1u : 0u;
                    }
                } else {  // the codeword's n / 2 lanes sit at lane - t of the ballots
                    constexpr unsigned long long mask = (1ull << TPC) - 1ull;
                    const int sh = lane - t;
                    unsigned long long e = ((bu0 >> sh) & mask) | (((bu1 >> sh) & mask) << TPC);
                    const unsigned long long xh = ((bx0 >> sh) & mask) | (((bx1 >> sh) & mask) << TPC);
#pragma unroll
                    for (int h = 1; h < N; h <<= 1) e ^= (e >> h) & span_mask64(h);
                    stop = e == xh;
                    __syncthreads();
                }
                if (t == 0 && act && !stop) sm.alive = 1u;
                __syncthreads();
                if constexpr (N >= 128) stop = sm.stop[c] != 0u;
                if (act && stop) {
                    act = false;
                    done = it + 1;
                }
                if (sm.alive == 0u) break;
            }
        }

        if (valid) {
            const float l0 = Ls[i0], l1 = Ls[i1];
            if (out_bits != nullptr) {
                if (out_kind == PL_OUT_F32) {
                    float* o = static_cast<float*>(out_bits) + cw * k;
                    if (rank0 >= 0) o[rank0] = (l0 > 0.0f) ? 0.0f : 1.0f;
                    if (rank1 >= 0) o[rank1] = (l1 > 0.0f) ? 0.0f : 1.0f;
                } else {
                    uint8_t* o = static_cast<uint8_t*>(out_bits) + cw * k;
                    if (rank0 >= 0) o[rank0] = (l0 > 0.0f) ? 0 : 1;
                    if (rank1 >= 0) o[rank1] = (l1 > 0.0f) ? 0 : 1;
                }
            }
            if (soft_u != nullptr) {
                float* o = soft_u + cw * k;
                if (rank0 >= 0) o[rank0] = -l0;
                if (rank1 >= 0) o[rank1] = -l1;
            }
            if (ext_x != nullptr) {
                float* o = ext_x + cw * N;
                o[i0] = -Rs[(S - 1) * N + i0];
                o[i1] = -Rs[(S - 1) * N + i1];
            }
            if (iters != nullptr && t == 0) iters[cw] = done;
        }
        __syncthreads();  // the next row's loads overwrite the messages
    }
}

template <int LOG_N>
void launch_n(const pl_plan* p, const float* llr, int64_t bs, int num_iter, float scale, int early_stop, void* out_bits,
              int out_kind, float* soft_u, float* ext_x, int32_t* iters, hipStream_t st) {
    using G = Geo<LOG_N>;
    int64_t blocks = (bs + G::C - 1) / G::C;
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    if (p->f_mode == PL_F_MINSUM)
        hipLaunchKernelGGL((bp_kernel<LOG_N, 0>), dim3((unsigned)blocks), dim3(G::T), 0, st, llr, p->d_frozen_words,
                           p->d_info_rank, bs, p->k, num_iter, scale, early_stop, p->llr_max, out_bits, out_kind, soft_u,
                           ext_x, iters);
    else
        hipLaunchKernelGGL((bp_kernel<LOG_N, 1>), dim3((unsigned)blocks), dim3(G::T), 0, st, llr, p->d_frozen_words,
                           p->d_info_rank, bs, p->k, num_iter, scale, early_stop, p->llr_max, out_bits, out_kind, soft_u,
                           ext_x, iters);
}

}  // namespace

namespace pl {

// the arguments are checked by pl_bp_decode (capi.cpp): an SC plan with n <= 1024, bs > 0, some output
int launch_bp(const pl_plan* p, const float* llr, int64_t bs, int num_iter, float scale, int early_stop, void* out_bits,
              int out_kind, float* soft_u, float* ext_x, int32_t* iters, hipStream_t st) {
    switch (p->log_n) {
        case 1: launch_n<1>(p, llr, bs, num_iter, scale, early_stop, out_bits, out_kind, soft_u, ext_x, iters, st); break;
        case 2: launch_n<2>(p, llr, bs, num_iter, scale, early_stop, out_bits, out_kind, soft_u, ext_x, iters, st); break;
        case 3: launch_n<3>(p, llr, bs, num_iter, scale, early_stop, out_bits, out_kind, soft_u, ext_x, iters, st); break;
        case 4: launch_n<4>(p, llr, bs, num_iter, scale, early_stop, out_bits, out_kind, soft_u, ext_x, iters, st); break;
        case 5: launch_n<5>(p, llr, bs, num_iter, scale, early_stop, out_bits, out_kind, soft_u, ext_x, iters, st); break;
        case 6: launch_n<6>(p, llr, bs, num_iter, scale, early_stop, out_bits, out_kind, soft_u, ext_x, iters, st); break;
        case 7: launch_n<7>(p, llr, bs, num_iter, scale, early_stop, out_bits, out_kind, soft_u, ext_x, iters, st); break;
        case 8: launch_n<8>(p, llr, bs, num_iter, scale, early_stop, out_bits, out_kind, soft_u, ext_x, iters, st); break;
        case 9: launch_n<9>(p, llr, bs, num_iter, scale, early_stop, out_bits, out_kind, soft_u, ext_x, iters, st); break;
        case 10: launch_n<10>(p, llr, bs, num_iter, scale, early_stop, out_bits, out_kind, soft_u, ext_x, iters, st); break;
        default:
            set_error("pl_bp_decode: n must be a power of two in [2, 1024]");
            return PL_ENOTSUP;
    }
    return check_hip(hipGetLastError(), "pl_bp_decode launch");
}

}  // namespace pl
