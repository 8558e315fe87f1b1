// scan_kernel.hip -- soft-cancellation (SCAN) polar decoding with soft output on gfx950
// (pl_scan_decode, include/polar_mi355x.h; Fayyaz and Barry 2014).
//
// The factor graph, the four unit equations, the initial values and the outputs are pl_bp_decode's
// (bp_kernel.hip); the schedule is the SC tree walk: node(s, b), h = 2^(s-1), computes L[s-1] of its left
// half (phase 1), visits the left child, computes L[s-1] of its right half from the R the left child just
// wrote (phase 2), visits the right child and then writes R[s] of both halves (phase 3).
//
// Register block: the lowest SB = min(S, 6) stages of the tree live in registers, one position a lane:
// lane p of a block holds L[0 .. SB][p] and R[0 .. SB][p], the partner p ^ h of a unit is a DPP move
// (h = 1, 2: one quad_perm; h = 4, 8: two), a ds_swizzle (h = 16) or a ds_bpermute (h = 32), never an LDS
// round trip.  The 63 nodes of a block are unrolled; every lane executes every phase and a select keeps
// the lanes outside the node (control flow depends on n only and is uniform over the wave).
//   n <= 64: the block is the codeword.  A wave holds 64 / n codewords side by side (lane = c n + p: the
//     xor partners stay inside a codeword), a work-group of 256 threads 256 / n; no message touches LDS,
//     R persists in registers across the iterations and there is no barrier.  A stopped codeword keeps its
//     registers (the select) and the wave leaves the loop when none of its codewords is active.
//   n >= 128: a work-group is one wave and one codeword.  Stages 7 .. S (h >= 64) run over LDS, 64
//     consecutive floats an access (no bank conflict), h / 64 accesses a phase; the walk is a loop over the
//     n / 64 blocks: before block q the phases 1 / 2 of the ancestors it enters, after it the phases 3 of
//     the ancestors it completes (trailing zeros / ones of q).  The work-group is a single wave, so
//     __syncthreads() orders the LDS accesses of its lanes and no wave ever waits for another.
//
// LDS of n >= 128, in floats (tests/test_scan_resources.py asserts the bytes):
//   L path   L[S] (n), then L[s], s = S-1 .. 6, the current node only (2^s):            2 n - 64
//   R        R[s][n], s = 6 .. S:                                                       (S - 5) n
//   P        R[t] of the right children inside the blocks, t = 1 .. 5, the lanes whose
//            index bit t is set, packed (32 floats a stage and block):                  5 n / 2
//   L0       L[0][n], the leaf messages (outputs, early stop):                          n
//   total (S + 1/2) n - 64 floats, plus 2 n / 32 words of packed u^ / x^ and, with the exact f, the 6 KiB
//   tables: 93,952 + 512 B at n = 2048 against (2 S + 1) n floats of the BP kernel.
//
// Bounds: row = group * C + c is clamped to bs - 1 for the loads and masked for the stores; a path buffer
// L[s] is indexed by li, li + h < 2^s; R[s] by b + li + h < n (b a multiple of 2 h); P by
// (q 5 + t - 1) 32 + packed lane < 5 n / 2; frozen bits by (64 q + lane) / 32 < n / 32; info_rank[i] < k.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/polar_mi355x.h"
#include "butterfly.h"
#include "exactf.h"
#include "plan.h"

namespace {

// Grid: a work-group walks the rows with a grid stride.  n <= 64 (256 threads, 256 / n codewords): 1024 work-groups
// at most, as the BP kernel.  n >= 128 (one wave, one codeword): as many work-groups as the device holds at once --
// compute units times what LDS and registers let onto one -- so that every SIMD has as many waves as fit to hide the
// latency of each other's dependent chains, and every work-group decodes the same number of rows (+- 1).
constexpr int kMaxBlocks = 1024;
constexpr int kMaxDevices = 64;

using plx::clip_l;

template <int FM>
__device__ __forceinline__ float fop(float x, float y, float lmax, float scale) {
    if constexpr (FM == 0) {  // bp_kernel.hip fop<0>
        const float m = fminf(fminf(fabsf(x), fabsf(y)), lmax) * scale;
        const uint32_t sg = (__float_as_uint(x) ^ __float_as_uint(y)) & 0x80000000u;
        return __uint_as_float(__float_as_uint(m) | sg);
    } else {
        return plx::f_exact(x, y, lmax);
    }
}

template <int CTRL>
__device__ __forceinline__ float dppf(float v) {
    const int i = (int)__float_as_uint(v);
    return __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(i, i, CTRL, 0xF, 0xF, false));
}

// the value of lane ^ H; every lane of the wave calls
template <int H>
__device__ __forceinline__ float xlane(float v) {
    if constexpr (H == 1) return dppf<0xB1>(v);                    // quad_perm [1,0,3,2]
    else if constexpr (H == 2) return dppf<0x4E>(v);               // quad_perm [2,3,0,1]
    else if constexpr (H == 4) return dppf<0x141>(dppf<0x1B>(v));  // quad_perm [3,2,1,0], row_half_mirror: ^3 ^7
    else if constexpr (H == 8) return dppf<0x141>(dppf<0x140>(v)); // row_mirror, row_half_mirror: ^15 ^7
    else if constexpr (H == 16)                                     // bit mode: and 0x1f, or 0, xor 0x10
        return __uint_as_float((uint32_t)__builtin_amdgcn_ds_swizzle((int)__float_as_uint(v), 0x401F));
    else return __shfl_xor(v, 32, 64);
}

// positions of a 64-bit word whose index bit log2(h) is 0
__device__ __forceinline__ unsigned long long span_mask64(int h) {
    return h == 32 ? 0x00000000FFFFFFFFull : (unsigned long long)pl::span_mask(h) * 0x0000000100000001ull;
}

// node(s, b) of the register block: p = the lane's position in the block, act = its codeword iterates
template <int FM, int s, int b>
__device__ __forceinline__ void node_reg(float (&L)[7], float (&R)[7], int p, bool act, float lmax, float scale) {
    if constexpr (s > 0) {
        constexpr int h = 1 << (s - 1);
        const int q = p & ~(h - 1);
        const bool lo = act && q == b, hi = act && q == b + h;
        {
            const float t = xlane<h>(L[s] + R[s - 1]);
            const float v = clip_l(fop<FM>(L[s], t, lmax, scale), lmax);
            L[s - 1] = lo ? v : L[s - 1];
        }
        node_reg<FM, s - 1, b>(L, R, p, act, lmax, scale);
        const float a = xlane<h>(L[s]), r = xlane<h>(R[s - 1]);  // in the upper half: L[s][i], R[s-1][i]
        {
            const float v = clip_l(fop<FM>(a, r, lmax, scale) + L[s], lmax);
            L[s - 1] = hi ? v : L[s - 1];
        }
        node_reg<FM, s - 1, b + h>(L, R, p, act, lmax, scale);
        {
            const float t = xlane<h>(L[s] + R[s - 1]);
            const float fv = fop<FM>(lo ? R[s - 1] : r, lo ? t : a, lmax, scale);
            const float v = clip_l(lo ? fv : fv + R[s - 1], lmax);
            R[s] = (lo || hi) ? v : R[s];
        }
    }
}

template <int LOG_N>
struct Geo {
    static constexpr int S = LOG_N, N = 1 << LOG_N;
    static constexpr bool REG = N <= 64;      // the codeword is one register block
    static constexpr int T = REG ? 256 : 64;  // threads per work-group
    static constexpr int C = REG ? T / N : 1; // codewords per work-group
    static constexpr int NBLK = REG ? 1 : N / 64, NW = N / 32;
    // LDS floats (n >= 128)
    static constexpr int OFF_R = 2 * N - 64, OFF_P = OFF_R + (S - 5) * N, OFF_L0 = OFF_P + 5 * (N / 2);
    static constexpr int FLOATS = OFF_L0 + N;
};

template <int LOG_N>
struct Shared {
    using G = Geo<LOG_N>;
    float m[G::FLOATS];
    uint32_t uw[G::NW], xw[G::NW];  // the packed u^ and x^
};

__device__ __forceinline__ void store_row(int64_t cw, int i, int rank, int k, int n, float l0, float rs, void* out_bits,
                                          int out_kind, float* soft_u, float* ext_x) {
    if (rank >= 0) {
        if (out_bits != nullptr) {
            if (out_kind == PL_OUT_F32)
                static_cast<float*>(out_bits)[cw * k + rank] = (l0 > 0.0f) ? 0.0f : 1.0f;
            else
                static_cast<uint8_t*>(out_bits)[cw * k + rank] = (l0 > 0.0f) ? 0 : 1;
        }
        if (soft_u != nullptr) soft_u[cw * k + rank] = -l0;
    }
    if (ext_x != nullptr) ext_x[cw * n + i] = -rs;
}

// n <= 64: codewords side by side in the wave, everything in registers
template <int LOG_N, int FM>
__device__ __forceinline__ void scan_reg(const float* __restrict__ llr, const uint32_t* __restrict__ frozen_words,
                                         const int32_t* __restrict__ info_rank, int64_t bs, int k, int num_iter,
                                         float scale, int early_stop, float lmax, void* __restrict__ out_bits,
                                         int out_kind, float* __restrict__ soft_u, float* __restrict__ ext_x,
                                         int32_t* __restrict__ iters) {
    using G = Geo<LOG_N>;
    constexpr int S = G::S, N = G::N, C = G::C;
    const int tid = threadIdx.x, lane = tid & 63;
    const int c = tid / N, p = tid % N;
    const int rank = info_rank[p];
    const bool frozen = (frozen_words[p >> 5] >> (p & 31)) & 1u;

    const int64_t groups = (bs + C - 1) / C;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t cw = g * C + c;
        const bool valid = cw < bs;
        float L[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, R[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        L[S] = clip_l(-llr[(valid ? cw : bs - 1) * N + p], lmax);
        R[0] = frozen ? lmax : 0.0f;

        bool act = valid;
        int done = num_iter;
        for (int it = 0; it < num_iter; ++it) {
            node_reg<FM, S, 0>(L, R, p, act, lmax, scale);
            if (early_stop) {  // uniform over the grid
                unsigned long long e = __ballot(rank >= 0 && !(L[0] > 0.0f));
                const unsigned long long xh = __ballot(!(L[S] + R[S] > 0.0f));
#pragma unroll
                for (int h = 1; h < N; h <<= 1) e ^= (e >> h) & span_mask64(h);  // spans stay inside a codeword
                constexpr unsigned long long mask = N == 64 ? ~0ull : (1ull << N) - 1ull;
                const bool stop = (((e ^ xh) >> (lane - p)) & mask) == 0ull;
                if (act && stop) {
                    act = false;
                    done = it + 1;
                }
                if (__ballot(act) == 0ull) break;
            }
        }
        if (valid) {
            store_row(cw, p, rank, k, N, L[0], R[S], out_bits, out_kind, soft_u, ext_x);
            if (iters != nullptr && p == 0) iters[cw] = done;
        }
    }
}

// n >= 128: one wave, one codeword; stages 7 .. S over LDS, the blocks in registers
template <int LOG_N, int FM>
__device__ __forceinline__ void scan_lds(const float* __restrict__ llr, const uint32_t* __restrict__ frozen_words,
                                         const int32_t* __restrict__ info_rank, int64_t bs, int k, int num_iter,
                                         float scale, int early_stop, float lmax, void* __restrict__ out_bits,
                                         int out_kind, float* __restrict__ soft_u, float* __restrict__ ext_x,
                                         int32_t* __restrict__ iters) {
    using G = Geo<LOG_N>;
    constexpr int S = G::S, N = G::N, NBLK = G::NBLK, NW = G::NW;
    __shared__ Shared<LOG_N> sm;
    float* const M = sm.m;
    float* const P = M + G::OFF_P;
    float* const L0 = M + G::OFF_L0;
    const int lane = threadIdx.x;

    // bit q of fz: position 64 q + lane is frozen
    uint32_t fz = 0u;
#pragma unroll
    for (int q = 0; q < NBLK; ++q) fz |= ((frozen_words[2 * q + (lane >> 5)] >> (lane & 31)) & 1u) << q;
    // the lane's slot in the packed row of stage t (index bit t removed)
    int slot[6];
#pragma unroll
    for (int t = 1; t <= 5; ++t) slot[t] = ((lane >> (t + 1)) << t) | (lane & ((1 << t) - 1));

    const auto off_l = [](int s) { return 2 * N - (2 << s); };             // L[s], s = 6 .. S: the current node
    const auto off_r = [](int s) { return G::OFF_R + (s - 6) * N; };      // R[s][n], s = 6 .. S

    for (int64_t cw = blockIdx.x; cw < bs; cw += gridDim.x) {
        const float* x = llr + cw * N;
#pragma unroll
        for (int j = 0; j < NBLK; ++j) M[j * 64 + lane] = clip_l(-x[j * 64 + lane], lmax);
        for (int i = G::OFF_R + lane; i < G::OFF_L0; i += 64) M[i] = 0.0f;  // R[6 .. S] and P
        __syncthreads();

        int done = num_iter;
        for (int it = 0; it < num_iter; ++it) {
            for (int q = 0; q < NBLK; ++q) {
                // phases 1 / 2 of the ancestors this block enters
                const int z = q == 0 ? S - 6 : __builtin_ctz(q);
                for (int s = (z + 7 < S ? z + 7 : S); s >= 7; --s) {
                    const int h = 1 << (s - 1), b = (q >> (s - 6)) << s;
                    const bool right = (q >> (s - 7)) & 1;
                    const float* Ls = M + off_l(s);
                    const float* Rc = M + off_r(s - 1) + b;
                    float* Lc = M + off_l(s - 1);
                    for (int li = lane; li < h; li += 64) {
                        const float la = Ls[li], lb = Ls[li + h];
                        Lc[li] = right ? clip_l(fop<FM>(la, Rc[li], lmax, scale) + lb, lmax)
                                       : clip_l(fop<FM>(la, lb + Rc[li + h], lmax, scale), lmax);
                    }
                    __syncthreads();
                }
                // the block
                float L[7], R[7];
                L[6] = M[off_l(6) + lane];
                R[0] = ((fz >> q) & 1u) ? lmax : 0.0f;
#pragma unroll
                for (int t = 1; t <= 5; ++t) {
                    L[t] = 0.0f;
                    // every lane loads its packed slot: a lane whose bit t is set receives its own R[t] of the
                    // previous iteration; a lane whose bit t is clear receives its partner's stale value (not 0),
                    // which the left child of the stage-(t+1) node overwrites before anything reads it
                    R[t] = P[(q * 5 + t - 1) * 32 + slot[t]];
                }
                L[0] = 0.0f, R[6] = 0.0f;
                node_reg<FM, 6, 0>(L, R, lane, true, lmax, scale);
#pragma unroll
                for (int t = 1; t <= 5; ++t)
                    if ((lane >> t) & 1) P[(q * 5 + t - 1) * 32 + slot[t]] = R[t];
                M[off_r(6) + q * 64 + lane] = R[6];
                L0[q * 64 + lane] = L[0];
                __syncthreads();
                // phases 3 of the ancestors this block completes
                const int o = __builtin_ctz(~q);
                for (int s = 7; s <= (o + 6 < S ? o + 6 : S); ++s) {
                    const int h = 1 << (s - 1), b = (q >> (s - 6)) << s;
                    const float* Ls = M + off_l(s);
                    const float* Rc = M + off_r(s - 1) + b;
                    float* Rs = M + off_r(s) + b;
                    for (int li = lane; li < h; li += 64) {
                        const float la = Ls[li], lb = Ls[li + h], ra = Rc[li], rb = Rc[li + h];
                        Rs[li] = clip_l(fop<FM>(ra, lb + rb, lmax, scale), lmax);
                        Rs[li + h] = clip_l(fop<FM>(ra, la, lmax, scale) + rb, lmax);
                    }
                    __syncthreads();
                }
            }
            if (early_stop) {  // uniform over the grid
                const float* Rs = M + off_r(S);
#pragma unroll
                for (int j = 0; j < NBLK; ++j) {
                    const int i = j * 64 + lane;
                    const unsigned long long bu = __ballot(!((fz >> j) & 1u) && !(L0[i] > 0.0f));
                    const unsigned long long bx = __ballot(!(M[i] + Rs[i] > 0.0f));
                    if (lane == 0) {
                        sm.uw[2 * j] = (uint32_t)bu, sm.uw[2 * j + 1] = (uint32_t)(bu >> 32);
                        sm.xw[2 * j] = (uint32_t)bx, sm.xw[2 * j + 1] = (uint32_t)(bx >> 32);
                    }
                }
                __syncthreads();
                const bool mine = lane < NW;
                const uint32_t e = pl::polar_butterfly(mine ? sm.uw[mine ? lane : 0] : 0u, 32, NW, lane);
                const bool stop = __ballot(mine && e != sm.xw[mine ? lane : 0]) == 0ull;
                __syncthreads();
                if (stop) {
                    done = it + 1;
                    break;
                }
            }
        }

        const float* Rs = M + off_r(S);
#pragma unroll
        for (int j = 0; j < NBLK; ++j) {
            const int i = j * 64 + lane;
            store_row(cw, i, info_rank[i], k, N, L0[i], Rs[i], out_bits, out_kind, soft_u, ext_x);
        }
        if (iters != nullptr && lane == 0) iters[cw] = done;
        __syncthreads();  // the next row's loads overwrite the messages
    }
}

template <int LOG_N, int FM>
__global__ __launch_bounds__(Geo<LOG_N>::T) void scan_kernel(const float* __restrict__ llr,
                                                             const uint32_t* __restrict__ frozen_words,
                                                             const int32_t* __restrict__ info_rank, int64_t bs, int k,
                                                             int num_iter, float scale, int early_stop, float lmax,
                                                             void* __restrict__ out_bits, int out_kind,
                                                             float* __restrict__ soft_u, float* __restrict__ ext_x,
                                                             int32_t* __restrict__ iters) {
    if constexpr (FM == 1) plx::load_tables(threadIdx.x, Geo<LOG_N>::T);  // ends with a barrier
    if constexpr (Geo<LOG_N>::REG)
        scan_reg<LOG_N, FM>(llr, frozen_words, info_rank, bs, k, num_iter, scale, early_stop, lmax, out_bits, out_kind,
                            soft_u, ext_x, iters);
    else
        scan_lds<LOG_N, FM>(llr, frozen_words, info_rank, bs, k, num_iter, scale, early_stop, lmax, out_bits, out_kind,
                            soft_u, ext_x, iters);
}

// work-groups of scan_kernel<LOG_N, FM> the plan's device holds at once (asked once a device and instantiation;
// 0: the query failed, the caller falls back to kMaxBlocks)
template <int LOG_N, int FM>
int resident_groups(int device) {
    static int cache[kMaxDevices] = {};
    const bool cached = device >= 0 && device < kMaxDevices;
    if (cached && cache[device] > 0) return cache[device];
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, scan_kernel<LOG_N, FM>, Geo<LOG_N>::T, 0) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || per_cu < 1 || cus < 1) {
        (void)hipGetLastError();
        return 0;
    }
    if (cached) cache[device] = per_cu * cus;  // racing callers store the same value
    return per_cu * cus;
}

template <int LOG_N>
void launch_n(const pl_plan* p, const float* llr, int64_t bs, int num_iter, float scale, int early_stop, void* out_bits,
              int out_kind, float* soft_u, float* ext_x, int32_t* iters, hipStream_t st) {
    using G = Geo<LOG_N>;
    int64_t blocks = (bs + G::C - 1) / G::C, cap = kMaxBlocks;
    if constexpr (!G::REG) {
        const int r = p->f_mode == PL_F_MINSUM ? resident_groups<LOG_N, 0>(p->device) : resident_groups<LOG_N, 1>(p->device);
        if (r > 0) cap = r;
    }
    if (blocks > cap) blocks = cap;
    if (p->f_mode == PL_F_MINSUM)
        hipLaunchKernelGGL((scan_kernel<LOG_N, 0>), dim3((unsigned)blocks), dim3(G::T), 0, st, llr, p->d_frozen_words,
                           p->d_info_rank, bs, p->k, num_iter, scale, early_stop, p->llr_max, out_bits, out_kind,
                           soft_u, ext_x, iters);
    else
        hipLaunchKernelGGL((scan_kernel<LOG_N, 1>), dim3((unsigned)blocks), dim3(G::T), 0, st, llr, p->d_frozen_words,
                           p->d_info_rank, bs, p->k, num_iter, scale, early_stop, p->llr_max, out_bits, out_kind,
                           soft_u, ext_x, iters);
}

}  // namespace

namespace pl {

// the arguments are checked by pl_scan_decode (capi.cpp): an SC plan with n <= 2048, bs > 0, some output
int launch_scan(const pl_plan* p, const float* llr, int64_t bs, int num_iter, float scale, int early_stop,
                void* out_bits, int out_kind, float* soft_u, float* ext_x, int32_t* iters, hipStream_t st) {
#define PL_SCAN_CASE(LN) \
    case LN: launch_n<LN>(p, llr, bs, num_iter, scale, early_stop, out_bits, out_kind, soft_u, ext_x, iters, st); break;
    switch (p->log_n) {
        PL_SCAN_CASE(1) PL_SCAN_CASE(2) PL_SCAN_CASE(3) PL_SCAN_CASE(4) PL_SCAN_CASE(5) PL_SCAN_CASE(6)
        PL_SCAN_CASE(7) PL_SCAN_CASE(8) PL_SCAN_CASE(9) PL_SCAN_CASE(10) PL_SCAN_CASE(11)
        default:
            set_error("pl_scan_decode: n must be a power of two in [2, 2048]");
            return PL_ENOTSUP;
    }
#undef PL_SCAN_CASE
    return check_hip(hipGetLastError(), "pl_scan_decode launch");
}

}  // namespace pl
