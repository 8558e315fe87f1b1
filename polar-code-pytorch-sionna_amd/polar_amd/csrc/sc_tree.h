// sc_tree.h -- the register-tree SC decode of one lane group, shared by scf_kernel.hip (one inverted
// decision per group) and ae_kernel.hip (one position permutation per group).  gfx950, wave64.
// genie_kernel.hip takes fop / gop from here.  sc_kernel.hip and scq_kernel.hip still carry their own copies
// of this walk.
//
// sc_kernel.hip's register tree -- G = max(1, n/128) lanes per decode, element i in lane i mod G, slot
// i / G, the two top stages recomputed from the root LLRs -- without the repetition and SPC shortcuts
// (rate-0 skipping stays: frozen leaves decide 0 whatever their LLR), and with the decision at one
// position (Ctx::flip, -1: none) inverted.  The C = 64/G lane groups of a wave run C decodes side by side;
// the tree's control flow depends on the frozen set alone, so it is uniform over the wave.
//
// The one point of variation is where the root LLRs come from: a Root type whose at(i) returns the LLR
// a_i (positive favours 0) at position i < n.  The tree calls it up to four times per position and decode.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "exactf.h"

namespace pl {
namespace tree {

constexpr int kRootChunk = 8;  // root f/g outputs per scheduling chunk (bounds loads in flight)
constexpr int kLoopDepth = 3;  // nodes with >= 2^depth elements per lane run their children in a loop

template <int E>
using BetaT = typename std::conditional<(E <= 32), uint32_t, uint64_t>::type;

struct Ctx {
    uint32_t vfrozen;  // lane l: frozen-mask word l
    uint32_t vr0;      // lane l: word l of the rate-0 node flags
    int lane, lig;     // lane in wave, lane in decode group
    int flip;          // position whose decision this lane's group inverts (-1: none)
    float lmax;
};

// Root LLRs straight from a row of channel logits: a = -logit
struct ChannelRoot {
    const float* __restrict__ ch;
    __device__ __forceinline__ float at(int i) const { return -ch[i]; }
};

__device__ __forceinline__ uint32_t rl(uint32_t v, int idx) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, idx);
}

template <int FM>
__device__ __forceinline__ float fop(float x, float y, float lmax) {
    if constexpr (FM == 0) {  // min-sum, clipped at lmax (polar_sc.py:46)
        const float m = fminf(fminf(fabsf(x), fabsf(y)), lmax);
        const uint32_t sg = (__float_as_uint(x) ^ __float_as_uint(y)) & 0x80000000u;
        return __uint_as_float(__float_as_uint(m) | sg);
    } else {
        return plx::f_exact(x, y, lmax);
    }
}
// g (polar_sc.py:49-53): (u ? -x : x) + y, one rounding.  fop / gop are also genie_kernel.hip's; sc_kernel.hip
// holds the same pair of its own
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

// Root, as sc_kernel.hip: stage LOG_N is the root's LLRs, read through Root::at; stage LOG_N - 1 is
// recomputed from two of them where the stage-(LOG_N-1) node needs it.
template <int LOG_N, int LOG_G, int FM, typename Root>
__device__ __forceinline__ float root_alpha(const Root& root, const Ctx& c, int side, uint64_t bl_root, int j) {
    constexpr int N = 1 << LOG_N, G = 1 << LOG_G;
    const float x = root.at(j * G + c.lig), y = root.at(j * G + c.lig + N / 2);
    return side == 0 ? fop<FM>(x, y, c.lmax) : gop(x, y, bitof(bl_root, j));
}

template <int LOG_N, int LOG_G, int FM, typename Root>
__device__ __forceinline__ BetaT<((1 << LOG_N) >> LOG_G) / 2> half_node(const Root& root, const Ctx& c, int side,
                                                                        uint64_t bl_root) {
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
                const float a0 = root_alpha<LOG_N, LOG_G, FM>(root, c, side, bl_root, j);
                const float a1 = root_alpha<LOG_N, LOG_G, FM>(root, c, side, bl_root, j + H);
                x[j] = sd == 0 ? fop<FM>(a0, a1, c.lmax) : gop(a0, a1, bitof(bl, j));
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        const BH b = child<LOG_N, LOG_G, s - 1, FM>(x, p + sd * h, c);
        if (sd == 0) bl = b; else br = b;
    }
    return (BT)(bl ^ br) | ((BT)br << H);
}

// One whole decode of this lane's group: the packed slots of the root's partial sums x (slot j of lane
// lig is position j G + lig; slots 0 ... 63 in lo, 64 ... 127 in hi).
template <int LOG_N, int LOG_G, int FM, typename Root>
__device__ __forceinline__ void decode_x(const Root& root, const Ctx& c, uint64_t& lo, uint64_t& hi) {
    constexpr int N = 1 << LOG_N, G = 1 << LOG_G, H = (N / G) / 2;
    using BH = BetaT<H>;
    BH bl = 0, br = 0;
    if constexpr (LOG_N - 1 == LOG_G) {
        // n = 2 G: the halves are bottoms, fed straight from the root
        const float x = root.at(c.lig), y = root.at(c.lig + N / 2);
        bl = bottom<LOG_N, LOG_G, FM>(fop<FM>(x, y, c.lmax), 0, c);
        br = bottom<LOG_N, LOG_G, FM>(gop(x, y, bl), N / 2, c);
    } else {
#pragma unroll 1
        for (int side = 0; side < 2; ++side) {
            const BH b = half_node<LOG_N, LOG_G, FM>(root, c, side, (uint64_t)bl);
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
}

// decode_x and the encoder butterfly: the packed slots of u = x G_n.
template <int LOG_N, int LOG_G, int FM, typename Root>
__device__ __forceinline__ void decode(const Root& root, const Ctx& c, uint64_t& lo, uint64_t& hi) {
    constexpr int N = 1 << LOG_N, G = 1 << LOG_G;
    decode_x<LOG_N, LOG_G, FM>(root, c, lo, hi);
    butterfly<G>(lo, hi, N / G, c.lig);
}

// pair index idx < n/2 of a butterfly stage with half-span h -> its low position (index bit log2 h is 0)
__device__ __forceinline__ int low_pos(int idx, int h) { return ((idx & ~(h - 1)) << 1) | (idx & (h - 1)); }

}  // namespace tree
}  // namespace pl
