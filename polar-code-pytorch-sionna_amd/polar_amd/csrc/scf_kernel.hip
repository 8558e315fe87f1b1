// scf_kernel.hip -- second stage of the CRC-aided SC-Flip decoder (pl_scf_decode,
// include/polar_mi355x.h) for gfx950 (wave64).
//
// SC-Flip (Afisiadis, Balatsoukas-Stimming, Burg 2014): SC first; a row whose SC result fails the
// CRC is decoded again, up to T times, each time with one more of its least reliable decisions
// inverted, until the CRC passes.  The first stage is the library's own (pl_sc_decode, crc_flag,
// compact_failed; capi.cpp sequences them).  This file is what a failing row needs after that, in
// one kernel, one wave (= one work-group) per failing row:
//
//   1. Reliabilities.  With SC's own decisions u^0 fed back, the leaf LLRs SC decided on are the
//      genie butterfly of genie_kernel.hip: log2 n stages of (f, g) pairs over a = -logits, the
//      partial sums of stage s being the encoder butterfly of u^0 stopped after s - 1 stages.  The
//      row's a[] and partial sums sit in LDS; the partial sums are transformed up to stage
//      log2 n - 1 first and one stage is undone after each (f, g) stage (a stage is an involution).
//   2. Candidates.  Key of information position i: (bits of |alpha_i|) << 32 | i, a total order
//      that is (|alpha|, i) ascending (+0 and -0 share the magnitude bits).  Each lane holds the
//      keys of positions lane, lane + 64, ...; round t takes the smallest key above the last one
//      taken (a wave minimum), T' = min(T, k) rounds.
//   3. Flip decodes.  sc_kernel.hip's register tree (sc_tree.h) -- G = max(1, n/128) lanes per decode, element
//      i in lane i mod G, slot i / G, the two top stages recomputed from the channel -- without the
//      repetition and SPC shortcuts (rate-0 skipping stays: frozen leaves decide 0 whatever their
//      LLR), and with the decision at one position inverted.  The C = 64/G lane groups of the wave
//      decode C candidates of the same row at once, so the channel row is read once per pass;
//      passes of C candidates until one passes the CRC or T' are spent.  The CRC of a group is the
//      XOR of the remainder table over its 1 bits (crc_flag's table, built per work-group); a
//      ballot picks the lowest passing t, and the wave stores that group's row.
//
// The grid is fixed (capi.cpp never reads the count back): work-groups stride over the failing
// rows, whose number they read from device memory.  Bounds: rows[r] < bs for r < *n_fail <= bs
// (compact_failed); positions j G + lig < n; info_rank is read at positions < n and only the
// ranks m >= 0 index the remainder table at k - 1 - m < k <= 1024; candidate t < T' <= 64.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/polar_mi355x.h"
#include "exactf.h"
#include "plan.h"
#include "sc_tree.h"
#include "scf.h"

namespace {

using namespace pl::tree;  // the register tree: Ctx, decode, fop, gop, grp_xor, low_pos

constexpr int kMaxBlocks = 4096;  // fixed grid of the flip kernel: 16 waves for each of 256 CUs
constexpr int kInitThreads = 256;

// XOR over the table entries of the 1 bits of w (slot base + j of lane lig is position (base + j) G + lig)
template <int LOG_G>
__device__ __forceinline__ uint32_t crc_of_slots(uint64_t w, int base, int lig, const int32_t* __restrict__ info_rank,
                                                 const uint32_t* s_rem, int k) {
    uint32_t acc = 0u;
    while (w) {
        const int j = __builtin_ctzll(w);
        w &= w - 1;
        const int m = info_rank[((base + j) << LOG_G) + lig];
        if (m >= 0) acc ^= s_rem[k - 1 - m];
    }
    return acc;
}

template <int LOG_N, int FM>
__global__ __launch_bounds__(64) void scf_flip_kernel(
    const float* __restrict__ llr, void* out, int out_kind, const int32_t* __restrict__ rows,
    const int64_t* __restrict__ n_fail, int tp, const uint32_t* __restrict__ frozen_words,
    const uint32_t* __restrict__ type_words, const int32_t* __restrict__ info_pos,
    const int32_t* __restrict__ info_rank, int k, int deg, uint32_t g, float lmax, uint8_t* crc_ok,
    int32_t* flip_pos, int32_t* attempts) {
    constexpr int LOG_G = (LOG_N > 7) ? (LOG_N - 7) : 0;
    constexpr int N = 1 << LOG_N, G = 1 << LOG_G, C = 64 / G;
    constexpr int NSL = N / G;            // slots per lane (<= 128)
    constexpr int WPL = (NSL + 31) / 32;  // u words per lane
    constexpr int WPC = (N + 31) / 32;    // frozen words
    constexpr int KPL = N > 64 ? N / 64 : 1;  // candidate keys per lane
    __shared__ float s_a[N];
    __shared__ uint32_t s_rem[pl::kScfMaxK];
    __shared__ uint32_t s_u[64 * WPL];
    __shared__ int32_t s_cand[pl::kScfMaxFlips];
    __shared__ uint8_t s_b[N < 4 ? 4 : N];

    const int lane = threadIdx.x;
    const int64_t nf = *n_fail;
    if ((int64_t)blockIdx.x >= nf) return;  // uniform over the work-group

    Ctx c;
    c.vfrozen = lane < WPC ? frozen_words[lane] : 0u;
    c.vr0 = type_words[lane];  // plane 0 of the node type flags: rate-0
    c.lane = lane;
    c.lig = lane & (G - 1);
    c.flip = -1;
    c.lmax = lmax;
    if constexpr (FM == 1) plx::load_tables(lane, 64);  // the exact f's exp / log tables

    // rem[j] = x^(deg + j) mod (x^deg + g), j < k: hybrid_kernel.hip crc_flag's table
    {
        const uint32_t mask = (1u << deg) - 1u;  // deg <= 31 (pl_plan_set_crc)
        const int top = deg - 1;
        g &= mask;
        auto times_x = [&](uint32_t a) { return ((a << 1) & mask) ^ (((a >> top) & 1u) ? g : 0u); };
        uint32_t v = g;
        for (int i = 0; i < 63; ++i)
            if (i < lane) v = times_x(v);
        if (lane < k) s_rem[lane] = v;
        __syncthreads();
        for (int cc = 64; cc < k; cc <<= 1) {
            const uint32_t xc = s_rem[cc - deg];  // x^cc mod G (deg < 64 <= cc)
            const int end = 2 * cc < k ? 2 * cc : k;
            for (int j = cc + lane; j < end; j += 64) {
                const uint32_t a = s_rem[j - cc];
                uint32_t r = 0u;
                for (int i = top; i >= 0; --i) {
                    r = times_x(r);
                    if ((xc >> i) & 1u) r ^= a;
                }
                s_rem[j] = r;
            }
            __syncthreads();
        }
    }

    for (int64_t r = blockIdx.x; r < nf; r += gridDim.x) {
        const int64_t row = rows[r];
        const float* ch = llr + row * N;

        // ---- 1. the leaf LLRs attempt 0 decided on ----
        for (int i = lane; i < N; i += 64) {
            s_b[i] = 0;
            s_a[i] = -ch[i];
        }
        __syncthreads();
        for (int m = lane; m < k; m += 64) {
            const bool one = out_kind == PL_OUT_F32 ? static_cast<const float*>(out)[row * k + m] != 0.0f
                                                    : static_cast<const uint8_t*>(out)[row * k + m] != 0;
            s_b[info_pos[m]] = one ? 1 : 0;
        }
        __syncthreads();
        for (int s = 1; s < LOG_N; ++s) {  // partial sums up to stage LOG_N - 1
            const int h = 1 << (s - 1);
            for (int idx = lane; idx < N / 2; idx += 64) {
                const int p = low_pos(idx, h);
                s_b[p] ^= s_b[p + h];
            }
            __syncthreads();
        }
        for (int s = LOG_N; s >= 1; --s) {
            const int h = 1 << (s - 1);
            for (int idx = lane; idx < N / 2; idx += 64) {
                const int p = low_pos(idx, h);
                const float x = s_a[p], y = s_a[p + h];
                s_a[p] = fop<FM>(x, y, lmax);
                s_a[p + h] = gop(x, y, s_b[p]);
            }
            __syncthreads();
            if (s >= 2) {  // undo stage s - 1 of the partial sums
                const int h2 = 1 << (s - 2);
                for (int idx = lane; idx < N / 2; idx += 64) {
                    const int p = low_pos(idx, h2);
                    s_b[p] ^= s_b[p + h2];
                }
                __syncthreads();
            }
        }

        // ---- 2. the tp smallest (|alpha|, i) among the information positions ----
        uint64_t key[KPL];
#pragma unroll
        for (int j = 0; j < KPL; ++j) {
            const int i = lane + 64 * j;
            const bool info = i < N && info_rank[i < N ? i : 0] >= 0;
            const uint32_t mag = __float_as_uint(s_a[i < N ? i : 0]) & 0x7fffffffu;
            key[j] = info ? ((uint64_t)mag << 32) | (uint32_t)i : ~0ull;
        }
        uint64_t last = 0;
        for (int t = 0; t < tp; ++t) {
            uint64_t best = ~0ull;
#pragma unroll
            for (int j = 0; j < KPL; ++j)
                if ((t == 0 || key[j] > last) && key[j] < best) best = key[j];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const uint64_t o = (uint64_t)__shfl_xor((long long)best, off, 64);
                best = o < best ? o : best;
            }
            last = best;
            if (lane == 0) s_cand[t] = (int32_t)(uint32_t)best;
        }
        __syncthreads();

        // ---- 3. flip decodes, C candidates a pass ----
        const int slot = lane >> LOG_G;
        for (int base = 0; base < tp; base += C) {
            const int t = base + slot;
            c.flip = t < tp ? s_cand[t] : -1;
            uint64_t lo, hi;
            decode<LOG_N, LOG_G, FM>(ChannelRoot{ch}, c, lo, hi);
            uint32_t acc = crc_of_slots<LOG_G>(lo, 0, c.lig, info_rank, s_rem, k);
            if constexpr (NSL > 64) acc ^= crc_of_slots<LOG_G>(hi, 64, c.lig, info_rank, s_rem, k);
            acc = grp_xor<G>(acc);
            const unsigned long long bal = __ballot(t < tp && acc == 0u);
            if (bal != 0ull) {  // uniform: the lowest passing t stores the row
                const int wslot = __builtin_ctzll(bal) >> LOG_G;
                uint32_t* mine = s_u + lane * WPL;
                mine[0] = (uint32_t)lo;
                if constexpr (WPL > 1) mine[1] = (uint32_t)(lo >> 32);
                if constexpr (WPL > 2) {
                    mine[2] = (uint32_t)hi;
                    mine[3] = (uint32_t)(hi >> 32);
                }
                __syncthreads();
                for (int m = lane; m < k; m += 64) {
                    const int pos = info_pos[m];
                    const int l = pos & (G - 1), sl = pos >> LOG_G;
                    const uint32_t bit = (s_u[(wslot * G + l) * WPL + (sl >> 5)] >> (sl & 31)) & 1u;
                    if (out_kind == PL_OUT_F32)
                        static_cast<float*>(out)[row * k + m] = bit ? 1.0f : 0.0f;
                    else
                        static_cast<uint8_t*>(out)[row * k + m] = (uint8_t)bit;
                }
                if (lane == 0) {
                    const int wt = base + wslot;
                    if (crc_ok) crc_ok[row] = 1;
                    if (flip_pos) flip_pos[row] = s_cand[wt];
                    if (attempts) attempts[row] = wt + 2;  // attempt 0 and attempts 1 .. wt + 1
                }
                break;
            }
        }
        __syncthreads();  // s_a, s_b, s_cand and s_u are reused by the next row
    }
}

// flip_pos = -1 everywhere; attempts = 1 where attempt 0 passes, else 1 + tp (the flip kernel overwrites
// both for the rows it rescues)
__global__ __launch_bounds__(kInitThreads) void scf_init_kernel(const uint8_t* __restrict__ valid, int64_t bs, int tp,
                                                                 int32_t* __restrict__ flip_pos,
                                                                 int32_t* __restrict__ attempts) {
    for (int64_t b = (int64_t)blockIdx.x * kInitThreads + threadIdx.x; b < bs; b += (int64_t)gridDim.x * kInitThreads) {
        if (flip_pos) flip_pos[b] = -1;
        if (attempts) attempts[b] = valid[b] ? 1 : 1 + tp;
    }
}

template <int LOG_N>
void launch_n(const pl_plan* p, const float* llr, int64_t bs, void* out, int out_kind, const int32_t* rows,
              const int64_t* n_fail, int tp, uint8_t* crc_ok, int32_t* flip_pos, int32_t* attempts, hipStream_t st) {
    const unsigned blocks = (unsigned)(bs < kMaxBlocks ? bs : kMaxBlocks);
    if (p->f_mode == PL_F_MINSUM)
        hipLaunchKernelGGL((scf_flip_kernel<LOG_N, 0>), dim3(blocks), dim3(64), 0, st, llr, out, out_kind, rows, n_fail,
                           tp, p->d_frozen_words, p->d_type_words, p->d_info_pos, p->d_info_rank, p->k, p->crc_deg,
                           p->crc_g, p->llr_max, crc_ok, flip_pos, attempts);
    else
        hipLaunchKernelGGL((scf_flip_kernel<LOG_N, 1>), dim3(blocks), dim3(64), 0, st, llr, out, out_kind, rows, n_fail,
                           tp, p->d_frozen_words, p->d_type_words, p->d_info_pos, p->d_info_rank, p->k, p->crc_deg,
                           p->crc_g, p->llr_max, crc_ok, flip_pos, attempts);
}

}  // namespace

namespace pl {

int launch_scf_init(const uint8_t* valid, int64_t bs, int tp, int32_t* flip_pos, int32_t* attempts, hipStream_t st) {
    if (bs == 0 || (!flip_pos && !attempts)) return PL_OK;
    int64_t blocks = (bs + kInitThreads - 1) / kInitThreads;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(scf_init_kernel, dim3((unsigned)blocks), dim3(kInitThreads), 0, st, valid, bs, tp, flip_pos,
                       attempts);
    return check_hip(hipGetLastError(), "SC-Flip init launch");
}

int launch_scf_flip(const pl_plan* p, const float* llr, int64_t bs, void* out, int out_kind, const int32_t* rows,
                    const int64_t* n_fail, int tp, uint8_t* crc_ok, int32_t* flip_pos, int32_t* attempts,
                    hipStream_t st) {
    if (bs == 0 || tp == 0) return PL_OK;
    if (tp < 0 || tp > kScfMaxFlips || tp > p->k || p->k > kScfMaxK || p->crc_deg < 1 || p->crc_deg > 31) {
        set_error("SC-Flip: needs 1 <= flips <= min(64, k), k <= 1024 and a CRC of degree 1 ... 31");
        return PL_EINVAL;
    }
#define PL_SCF_CASE(LN) \
    case LN: launch_n<LN>(p, llr, bs, out, out_kind, rows, n_fail, tp, crc_ok, flip_pos, attempts, st); break;
    switch (p->log_n) {
        PL_SCF_CASE(1) PL_SCF_CASE(2) PL_SCF_CASE(3) PL_SCF_CASE(4) PL_SCF_CASE(5)
        PL_SCF_CASE(6) PL_SCF_CASE(7) PL_SCF_CASE(8) PL_SCF_CASE(9) PL_SCF_CASE(10)
        default: set_error("SC-Flip: n must be a power of two in [2, 1024]"); return PL_ENOTSUP;
    }
#undef PL_SCF_CASE
    return check_hip(hipGetLastError(), "SC-Flip launch");
}

}  // namespace pl
