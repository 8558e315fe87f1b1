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
//   3. Flip decodes.  sc_kernel.hip's register tree -- G = max(1, n/128) lanes per decode, element
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

#include <type_traits>

#include "../../../include/polar_mi355x.h"
#include "exactf.h"
#include "plan.h"
#include "scf.h"

namespace {

constexpr int kRootChunk = 8;  // root f/g outputs per scheduling chunk (bounds loads in flight)
constexpr int kLoopDepth = 3;  // nodes with >= 2^depth elements per lane run their children in a loop
constexpr int kMaxBlocks = 4096;  // fixed grid of the flip kernel: 16 waves for each of 256 CUs
constexpr int kInitThreads = 256;

template <int E>
using BetaT = typename std::conditional<(E <= 32), uint32_t, uint64_t>::type;

struct Ctx {
    uint32_t vfrozen;  // lane l: frozen-mask word l
    uint32_t vr0;      // lane l: word l of the rate-0 node flags
    int lane, lig;     // lane in wave, lane in decode group
    int flip;          // position whose decision this lane's group inverts (-1: none)
    float lmax;
};

__device__ __forceinline__ uint32_t rl(uint32_t v, int idx) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, idx);
}

template <int FM>
__device__ __forceinline__ float fop(float x, float y, float lmax) {
    if constexpr (FM == 0) {  // sc_kernel.hip fop<0> (polar_sc.py:46)
        const float m = fminf(fminf(fabsf(x), fabsf(y)), lmax);
        const uint32_t sg = (__float_as_uint(x) ^ __float_as_uint(y)) & 0x80000000u;
        return __uint_as_float(__float_as_uint(m) | sg);
    } else {
        return plx::f_exact(x, y, lmax);
    }
}
// sc_kernel.hip gop (polar_sc.py:49-53): (u ? -x : x) + y, one rounding
__device__ __forceinline__ float gop(float x, float y, uint32_t bit) {
    return __uint_as_float(__float_as_uint(x) ^ (bit << 31)) + y;
}
template <typename T>
__device__ __forceinline__ uint32_t bitof(T w, int j) {
    return (uint32_t)(w >> j) & 1u;
}
__device__ __forceinline__ uint32_t hd(float x) { return (x > 0.0f) ? 0u : 1u; }

// stage-s node at position p (wave-uniform) all frozen?  Flag bit OFF(s) + (p >> s), OFF(s) = n - (n >> (s-1)).
template <int LOG_N, int s>
__device__ __forceinline__ bool is_r0(const Ctx& c, int p) {
    constexpr int off = (1 << LOG_N) - ((1 << LOG_N) >> (s - 1));
    const int idx = off + (p >> s);
    return (rl(c.vr0, idx >> 5) >> (idx & 31)) & 1u;
}

template <int CTRL>
__device__ __forceinline__ uint32_t dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ float dppf(float v) {
    return __uint_as_float(dpp<CTRL>(__float_as_uint(v)));
}
// XOR over the G <= 8 lanes of a group, in every lane (groups never straddle a 16-lane DPP row)
template <int G>
__device__ __forceinline__ uint32_t grp_xor(uint32_t v) {
    static_assert(G <= 8, "group wider than the DPP steps below");
    if constexpr (G >= 2) v ^= dpp<0xB1>(v);   // quad_perm [1,0,3,2]
    if constexpr (G >= 4) v ^= dpp<0x4E>(v);   // quad_perm [2,3,0,1]
    if constexpr (G >= 8) v ^= dpp<0x141>(v);  // row_half_mirror
    return v;
}

// In-lane SC decode, leaf by leaf, of a 2^t-leaf subtree whose LLRs are all in v (bit q of fw = frozen
// flag of subtree leaf q; fq = the flipped leaf, relative to the subtree).  Returns the partial sums.
template <int t, int q, int FM>
__device__ __forceinline__ uint32_t inl(const float (&v)[1 << t], uint32_t fw, float lmax, int fq) {
    if constexpr (t == 0) {
        return ((fw >> q) & 1u) ? 0u : (hd(v[0]) ^ (uint32_t)(fq == q));
    } else {
        constexpr int H = 1 << (t - 1);
        constexpr uint32_t M = (t == 5) ? 0xffffffffu : ((1u << (1 << t)) - 1u);
        if (((fw >> q) & M) == M) return 0u;
        float x[H];
        uint32_t bl = 0u;
        constexpr uint32_t MH = (1u << H) - 1u;
        if (((fw >> q) & MH) != MH) {
#pragma unroll
            for (int j = 0; j < H; ++j) x[j] = fop<FM>(v[j], v[j + H], lmax);
            bl = inl<t - 1, q, FM>(x, fw, lmax, fq);
        }
#pragma unroll
        for (int j = 0; j < H; ++j) x[j] = gop(v[j], v[j + H], bitof(bl, j));
        const uint32_t br = inl<t - 1, q + H, FM>(x, fw, lmax, fq);
        return (bl ^ br) | (br << H);
    }
}

// v[j] = LLR held by lane j of this lane's group (all G of them, in every lane); sc_kernel.hip gather
template <int G>
__device__ __forceinline__ void gather(float a, const Ctx& c, float (&v)[G]) {
    static_assert(G == 2 || G == 4 || G == 8, "n <= 1024: groups of at most 8 lanes");
    if constexpr (G == 2) {
        v[0] = dppf<0xA0>(a);  // quad_perm [0,0,2,2]
        v[1] = dppf<0xF5>(a);  // quad_perm [1,1,3,3]
    } else if constexpr (G == 4) {
        v[0] = dppf<0x00>(a);
        v[1] = dppf<0x55>(a);
        v[2] = dppf<0xAA>(a);
        v[3] = dppf<0xFF>(a);
    } else {
        const bool hi = (c.lig & 4) != 0;
        float t[4];
        t[0] = dppf<0x00>(a);  // quad lane j: a_j (low quad) / a_{4+j} (high)
        t[1] = dppf<0x55>(a);
        t[2] = dppf<0xAA>(a);
        t[3] = dppf<0xFF>(a);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float down = dppf<0x114>(t[j]);  // row_shr:4 -> high quad sees low quad
            const float up = dppf<0x104>(t[j]);    // row_shl:4 -> low quad sees high quad
            v[j] = hi ? down : t[j];
            v[4 + j] = hi ? t[j] : up;
        }
    }
}

// Node of size G at position p (one LLR per lane).  Returns this lane's partial-sum bit.
template <int LOG_N, int LOG_G, int FM>
__device__ __forceinline__ uint32_t bottom(float a, int p, const Ctx& c) {
    constexpr int G = 1 << LOG_G;
    if constexpr (G == 1) {
        return ((rl(c.vfrozen, p >> 5) >> (p & 31)) & 1u) ? 0u : (hd(a) ^ (uint32_t)(c.flip == p));
    } else {
        if (is_r0<LOG_N, LOG_G>(c, p)) return 0u;
        constexpr uint32_t GM = (1u << G) - 1u;
        const uint32_t fw = (rl(c.vfrozen, p >> 5) >> (p & 31)) & GM;
        float v[G];
        gather<G>(a, c, v);
        const uint32_t beta = inl<LOG_G, 0, FM>(v, fw, c.lmax, c.flip - p);
        return bitof(beta, c.lig);
    }
}

template <int LOG_N, int LOG_G, int s, int FM>
__device__ BetaT<(1 << (s - LOG_G))> node(const float (&a)[1 << (s - LOG_G)], int p, const Ctx& c);

template <int LOG_N, int LOG_G, int s, int FM>
__device__ __forceinline__ BetaT<(1 << (s - LOG_G))> child(const float (&x)[1 << (s - LOG_G)], int p, const Ctx& c) {
    if constexpr (s == LOG_G) {
        return bottom<LOG_N, LOG_G, FM>(x[0], p, c);
    } else {
        return node<LOG_N, LOG_G, s, FM>(x, p, c);
    }
}

// Left child all-frozen?  (then its f pass is skipped; leaves of G = 1 codes use the frozen mask)
template <int LOG_N, int s>
__device__ __forceinline__ bool child_r0(const Ctx& c, int p) {
    if constexpr (s == 0) {
        return (rl(c.vfrozen, p >> 5) >> (p & 31)) & 1u;
    } else {
        return is_r0<LOG_N, s>(c, p);
    }
}

// Node at stage s (size 2^s) starting at position p: polar_sc.py:54-89 on registers.
template <int LOG_N, int LOG_G, int s, int FM>
__device__ __forceinline__ BetaT<(1 << (s - LOG_G))> node(const float (&a)[1 << (s - LOG_G)], int p, const Ctx& c) {
    constexpr int E = 1 << (s - LOG_G), H = E / 2, h = 1 << (s - 1);
    using BT = BetaT<E>;
    using BH = BetaT<H>;
    if (is_r0<LOG_N, s>(c, p)) return (BT)0;
    float x[H];
    BH bl = 0, br = 0;
    const bool left_r0 = child_r0<LOG_N, s - 1>(c, p);
    if constexpr (E >= (1 << kLoopDepth)) {
#pragma unroll 1
        for (int side = left_r0 ? 1 : 0; side < 2; ++side) {
            if (side == 0) {
#pragma unroll
                for (int j = 0; j < H; ++j) x[j] = fop<FM>(a[j], a[j + H], c.lmax);
            } else {
#pragma unroll
                for (int j = 0; j < H; ++j) x[j] = gop(a[j], a[j + H], bitof(bl, j));
            }
            const BH b = child<LOG_N, LOG_G, s - 1, FM>(x, p + side * h, c);
            if (side == 0) bl = b; else br = b;
        }
    } else {
        if (!left_r0) {
#pragma unroll
            for (int j = 0; j < H; ++j) x[j] = fop<FM>(a[j], a[j + H], c.lmax);
            bl = child<LOG_N, LOG_G, s - 1, FM>(x, p, c);
        }
#pragma unroll
        for (int j = 0; j < H; ++j) x[j] = gop(a[j], a[j + H], bitof(bl, j));
        br = child<LOG_N, LOG_G, s - 1, FM>(x, p + h, c);
    }
    return (BT)(bl ^ br) | ((BT)br << H);
}

// u = x * G_n on this lane's packed slots (sc_kernel.hip butterfly): slot j of lane l is position
// j G + l; spans >= G are in-lane, < G cross-lane.
template <int G>
__device__ __forceinline__ void butterfly(uint64_t& lo, uint64_t& hi, int nslots, int lig) {
    constexpr uint64_t M[6] = {0x5555555555555555ull, 0x3333333333333333ull, 0x0f0f0f0f0f0f0f0full,
                               0x00ff00ff00ff00ffull, 0x0000ffff0000ffffull, 0x00000000ffffffffull};
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const int hs = 1 << t;
        if (hs < nslots) {
            lo ^= (lo >> hs) & M[t];
            hi ^= (hi >> hs) & M[t];
        }
    }
    if (nslots > 64) lo ^= hi;
#pragma unroll
    for (int h = 1; h < G; h <<= 1) {
        const uint64_t olo = (uint64_t)__shfl_xor((long long)lo, h, 64);
        const uint64_t ohi = (uint64_t)__shfl_xor((long long)hi, h, 64);
        if ((lig & h) == 0) {
            lo ^= olo;
            hi ^= ohi;
        }
    }
}

// Root, as sc_kernel.hip: stage LOG_N is the negated channel, read from memory; stage LOG_N - 1 is
// recomputed from two channel values where the stage-(LOG_N-1) node needs it.
template <int LOG_N, int LOG_G, int FM>
__device__ __forceinline__ float root_alpha(const float* __restrict__ chl, const Ctx& c, int side, uint64_t bl_root,
                                            int j) {
    constexpr int N = 1 << LOG_N, G = 1 << LOG_G;
    const float x = -chl[j * G + c.lig], y = -chl[j * G + c.lig + N / 2];
    return side == 0 ? fop<FM>(x, y, c.lmax) : gop(x, y, bitof(bl_root, j));
}

template <int LOG_N, int LOG_G, int FM>
__device__ __forceinline__ BetaT<((1 << LOG_N) >> LOG_G) / 2> half_node(const float* __restrict__ ch, const Ctx& c,
                                                                        int side, uint64_t bl_root) {
    constexpr int s = LOG_N - 1, E = (1 << s) >> LOG_G, H = E / 2, h = 1 << (s - 1);
    using BT = BetaT<E>;
    using BH = BetaT<H>;
    const int p = side * (1 << s);
    if (is_r0<LOG_N, s>(c, p)) return (BT)0;
    float x[H];
    BH bl = 0, br = 0;
    const bool left_r0 = child_r0<LOG_N, s - 1>(c, p);
    constexpr int CH = kRootChunk < H ? kRootChunk : H;
#pragma unroll 1
    for (int sd = left_r0 ? 1 : 0; sd < 2; ++sd) {
#pragma unroll
        for (int j0 = 0; j0 < H; j0 += CH) {
#pragma unroll
            for (int j = j0; j < j0 + CH; ++j) {
                const float a0 = root_alpha<LOG_N, LOG_G, FM>(ch, c, side, bl_root, j);
                const float a1 = root_alpha<LOG_N, LOG_G, FM>(ch, c, side, bl_root, j + H);
                x[j] = sd == 0 ? fop<FM>(a0, a1, c.lmax) : gop(a0, a1, bitof(bl, j));
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        const BH b = child<LOG_N, LOG_G, s - 1, FM>(x, p + sd * h, c);
        if (sd == 0) bl = b; else br = b;
    }
    return (BT)(bl ^ br) | ((BT)br << H);
}

// One whole decode of this lane's group: the packed slots of u = x G_n, x the root's partial sums.
template <int LOG_N, int LOG_G, int FM>
__device__ __forceinline__ void decode(const float* __restrict__ ch, const Ctx& c, uint64_t& lo, uint64_t& hi) {
    constexpr int N = 1 << LOG_N, G = 1 << LOG_G, H = (N / G) / 2;
    using BH = BetaT<H>;
    BH bl = 0, br = 0;
    if constexpr (LOG_N - 1 == LOG_G) {
        // n = 2 G: the halves are bottoms, fed straight from the channel
        const float x = -ch[c.lig], y = -ch[c.lig + N / 2];
        bl = bottom<LOG_N, LOG_G, FM>(fop<FM>(x, y, c.lmax), 0, c);
        br = bottom<LOG_N, LOG_G, FM>(gop(x, y, bl), N / 2, c);
    } else {
#pragma unroll 1
        for (int side = 0; side < 2; ++side) {
            const BH b = half_node<LOG_N, LOG_G, FM>(ch, c, side, (uint64_t)bl);
            if (side == 0) bl = b; else br = b;
        }
    }
    if constexpr (H >= 64) {
        lo = (uint64_t)(bl ^ br);
        hi = (uint64_t)br;
    } else {
        lo = (uint64_t)(bl ^ br) | ((uint64_t)br << H);
        hi = 0;
    }
    butterfly<G>(lo, hi, N / G, c.lig);
}

// pair index idx < n/2 of a butterfly stage with half-span h -> its low position (index bit log2 h is 0)
__device__ __forceinline__ int low_pos(int idx, int h) { return ((idx & ~(h - 1)) << 1) | (idx & (h - 1)); }

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
            decode<LOG_N, LOG_G, FM>(ch, c, lo, hi);
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
