// scq_kernel.hip -- fixed-point successive-cancellation decoding on int8 LLRs, and the LLR quantiser
// that feeds it, for gfx950 (MI355X).  pl_scq_decode / pl_llr_quantize; the contract is stated in
// include/polar_mi355x.h and restated in numpy in tests/golden/scq_ref.py.  The reference has no such decoder.
//
// All values are integers of magnitude <= Imax = 2^(q_internal-1) - 1 <= 127:
//   load  a = -clamp(q, -Imax, Imax)                   f(x, y) = sgn(x) sgn(y) min(|x|, |y|), sgn(0) = 0
//   g(x, y, b) = clamp(y + (1 - 2b) x, -Imax, Imax)    leaf: frozen -> 0, else HD(a) = !(a > 0)
// The carrier in registers is fp32: adds and mins of integers below 2^24 are exact, f is the sign-xor bit
// trick of sc_kernel.hip (a zero operand gives +-0, and -0 behaves as 0 everywhere: HD(-0) = 1, -0 + y = y,
// the clamp keeps it), g is one add and one v_med3_f32.
//
// Layout: sc_kernel.hip's register tree.  A wave64 decodes C = 64/G codewords, G = max(1, n/128) lanes per
// codeword; element i of a stage lives in lane (i mod G), slot i/G, so every stage of size >= 2G runs in VGPRs
// and the last log2(G) stages run on DPP.  The channel row is read with 16-byte loads, 16 LLRs a load: lane l
// of a group reads chunks l, G + l, 2G + l, ... and a log2(G)-step exchange inside the group (v_perm_b32 and
// DPP on the packed bytes, below) leaves every lane with the bytes of its own residue class, which are then
// unpacked once into n/G floats: from there on the register budget is the float kernel's.
//
// Shortcuts: rate-0 subtrees only (beta = 0, and the f pass of a rate-0 left child is skipped), which is
// exact for every integer input.  Repetition, rate-1 and SPC shortcuts are not compiled.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../../include/polar_mi355x.h"
#include "plan.h"

namespace {

// waves per SIMD the register allocation must allow: 2 (256 registers) up to n = 1024.  At n = 2048 the
// 16-lane bottom nodes (16 gathered LLRs decoded in-lane) need some 20 registers more, so that instantiation is
// given the whole file instead of scratch
constexpr int min_waves(int log_n) { return log_n <= 10 ? 2 : 1; }
constexpr int kRootChunk = 8;   // root f/g outputs per scheduling chunk
constexpr int kLoopDepth = 3;   // nodes with >= 2^depth elements per lane run their children in a loop
constexpr int kWavesPerBlock = 4;

template <int E>
using BetaT = typename std::conditional<(E <= 32), uint32_t, uint64_t>::type;

struct Ctx {
    uint32_t vfrozen;  // lane l: frozen-mask word l
    uint32_t vr0;      // lane l: word l of the rate-0 node flags
    int lane, lig;     // lane in wave, lane in codeword group
    float imax;
};

__device__ __forceinline__ uint32_t rl(uint32_t v, int idx) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, idx);
}
// f: |result| <= Imax already, so no clip; a zero operand gives a (signed) zero.  min(|x|, |y|) is written as
// med3(|x|, |y|, 0), one v_med3_f32 with abs modifiers: fminf would first canonicalise both operands (two
// v_max_f32 more for every f), which no integer-valued operand needs.
__device__ __forceinline__ float fop(float x, float y) {
    const float m = __builtin_amdgcn_fmed3f(fabsf(x), fabsf(y), 0.0f);
    const uint32_t sg = (__float_as_uint(x) ^ __float_as_uint(y)) & 0x80000000u;
    return __uint_as_float(__float_as_uint(m) | sg);
}
// g: the sum of two integers of magnitude <= 127 is exact; the clamp is one v_med3_f32
__device__ __forceinline__ float gop(float x, float y, uint32_t bit, float imax) {
    const float s = __uint_as_float(__float_as_uint(x) ^ (bit << 31)) + y;
    return __builtin_amdgcn_fmed3f(s, -imax, imax);
}
template <typename T>
__device__ __forceinline__ uint32_t bitof(T w, int j) {
    return (uint32_t)(w >> j) & 1u;
}
__device__ __forceinline__ uint32_t hd(float x) { return (x > 0.0f) ? 0u : 1u; }

// Rate-0 flag of the stage-s node at position p (p wave-uniform): bit OFF(s) + (p >> s), OFF(s) = n - (n >> (s-1)).
template <int LOG_N, int s>
__device__ __forceinline__ bool is_r0(const Ctx& c, int p) {
    constexpr int off = (1 << LOG_N) - ((1 << LOG_N) >> (s - 1));
    const int idx = off + (p >> s);
    return (rl(c.vr0, idx >> 5) >> (idx & 31)) & 1u;
}

// ---- cross-lane moves inside a G-lane group, on DPP (as sc_kernel.hip) ----
// dpp_ctrl: quad_perm 0x00-0xFF, row_shl:k 0x100+k, row_shr:k 0x110+k, row_ror:k 0x120+k.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ float dppf(float v) {
    return __uint_as_float(dpp<CTRL>(__float_as_uint(v)));
}
// the value of lane (l ^ 2^t) of the 16-lane row
template <int t>
__device__ __forceinline__ uint32_t from_xor(uint32_t v) {
    static_assert(t >= 0 && t <= 3, "partner outside the DPP row");
    if constexpr (t == 0) return dpp<0xB1>(v);        // quad_perm [1,0,3,2]
    else if constexpr (t == 1) return dpp<0x4E>(v);   // quad_perm [2,3,0,1]
    else if constexpr (t == 3) return dpp<0x128>(v);  // row_ror:8
    else {
        // banks 0 and 2 (lanes 0-3, 8-11) read lane + 4 (row_shl:4), banks 1 and 3 read lane - 4 (row_shr:4)
        int r = __builtin_amdgcn_update_dpp((int)v, (int)v, 0x104, 0xF, 0x5, false);
        r = __builtin_amdgcn_update_dpp(r, (int)v, 0x114, 0xF, 0xA, false);
        return (uint32_t)r;
    }
}

// ---- channel row: 16-byte loads and the in-group byte transposition ----
// One exchange step on the 16 bytes w[0..3] (byte position pos = 4 * word + byte) a lane holds of one load.
// Step t swaps "bit t of the position" with "bit t of the lane": a lane whose lig has bit t = b keeps the
// bytes at positions with bit t = b and replaces the others by its partner's (lig ^ 2^t) bytes at positions
// with bit t = b.  After steps 0 .. LOG_G - 1 the byte at position pos came from lane (pos mod G) of the
// group, where it stood at position (pos - pos mod G) + lig: element 16 * chunk + that position, which is
// congruent to lig mod G.
template <int t>
__device__ __forceinline__ void xchg(uint32_t (&w)[4], uint32_t b) {
    if constexpr (t < 2) {
        // v_perm_b32 D = perm(S0, S1, sel): selector 0-3 takes a byte of S1, 4-7 of S0
        constexpr uint32_t sel0 = t == 0 ? 0x06020400u : 0x05040100u;  // b = 0: [w0 r0 w2 r2] / [w0 w1 r0 r1]
        constexpr uint32_t sel1 = t == 0 ? 0x03070105u : 0x03020706u;  // b = 1: [r1 w1 r3 w3] / [r2 r3 w2 w3]
        const uint32_t sel = b ? sel1 : sel0;
#pragma unroll
        for (int d = 0; d < 4; ++d) w[d] = __builtin_amdgcn_perm(from_xor<t>(w[d]), w[d], sel);
    } else {
        constexpr int st = t == 2 ? 1 : 2;  // word-index bit of position bit t
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            if (d & st) continue;
            const uint32_t r = from_xor<t>(b ? w[d] : w[d + st]);
            if (b) w[d] = r; else w[d + st] = r;
        }
    }
}

// The packed row of this lane: NW = max(1, n / G / 4) words.  Slot j (element j * G + lig) is byte
// slot_byte(j) of word slot_word(j).
template <int LOG_N, int LOG_G>
struct Row {
    static constexpr int N = 1 << LOG_N, G = 1 << LOG_G, NSL = N / G;
    static constexpr int NW = NSL >= 4 ? NSL / 4 : 1;
    uint32_t w[NW];

    // slot j = 16 m + r, r = l' * (16 / G) + e_hi: loaded by lane l' of the group as byte (e_hi * G + lig) of
    // its m-th chunk, and left by the exchange at position e_hi * G + l'
    static constexpr int pos_of(int j) {
        if (NSL < 16) return j;
        const int m = j / 16, r = j % 16, per = 16 / G;
        return m * 16 + (((r % per) << LOG_G) | (r / per));
    }

    __device__ __forceinline__ void load(const int8_t* __restrict__ row, const Ctx& c) {
        if constexpr (NSL < 16) {  // n = 2, 4, 8 (G = 1): byte loads
#pragma unroll
            for (int d = 0; d < NW; ++d) w[d] = 0;
#pragma unroll
            for (int j = 0; j < NSL; ++j) w[j >> 2] |= (uint32_t)(uint8_t)row[j] << (8 * (j & 3));
        } else {
            const uint4* src = reinterpret_cast<const uint4*>(row);
#pragma unroll
            for (int m = 0; m < NSL / 16; ++m) {
                const uint4 v = src[m * G + c.lig];
                uint32_t x[4] = {v.x, v.y, v.z, v.w};
                if constexpr (LOG_G >= 1) xchg<0>(x, c.lig & 1);
                if constexpr (LOG_G >= 2) xchg<1>(x, (c.lig >> 1) & 1);
                if constexpr (LOG_G >= 3) xchg<2>(x, (c.lig >> 2) & 1);
                if constexpr (LOG_G >= 4) xchg<3>(x, (c.lig >> 3) & 1);
#pragma unroll
                for (int d = 0; d < 4; ++d) w[4 * m + d] = x[d];
            }
        }
    }
    // a[j] = -clamp(q, -Imax, Imax) of slot j, every slot once: from here on the row is fp32 in registers
    __device__ __forceinline__ void unpack(float imax, float (&a)[NSL]) const {
#pragma unroll
        for (int j = 0; j < NSL; ++j) {
            const int pos = pos_of(j);
            const int q = (int)(int8_t)(w[pos >> 2] >> (8 * (pos & 3)));
            a[j] = __builtin_amdgcn_fmed3f(-(float)q, -imax, imax);
        }
    }
};

// In-lane SC decode of a 2^t-leaf subtree whose LLRs are all in v (bit q of fw = frozen flag of leaf q).
template <int t, int q>
__device__ __forceinline__ uint32_t inl(const float (&v)[1 << t], uint32_t fw, float imax) {
    if constexpr (t == 0) {
        return ((fw >> q) & 1u) ? 0u : hd(v[0]);
    } else {
        constexpr int H = 1 << (t - 1);
        constexpr uint32_t M = (t == 5) ? 0xffffffffu : ((1u << (1 << t)) - 1u);
        if (((fw >> q) & M) == M) return 0u;
        float x[H];
        uint32_t bl = 0u;
        constexpr uint32_t MH = (1u << H) - 1u;
        if (((fw >> q) & MH) != MH) {
#pragma unroll
            for (int j = 0; j < H; ++j) x[j] = fop(v[j], v[j + H]);
            bl = inl<t - 1, q>(x, fw, imax);
        }
#pragma unroll
        for (int j = 0; j < H; ++j) x[j] = gop(v[j], v[j + H], bitof(bl, j), imax);
        const uint32_t br = inl<t - 1, q + H>(x, fw, imax);
        return (bl ^ br) | (br << H);
    }
}

// v[j] = LLR held by lane j of this lane's group (all G of them, in every lane).
template <int G>
__device__ __forceinline__ void gather(float a, const Ctx& c, float (&v)[G]) {
    if constexpr (G == 2) {
        v[0] = dppf<0xA0>(a);  // quad_perm [0,0,2,2]
        v[1] = dppf<0xF5>(a);  // quad_perm [1,1,3,3]
        return;
    } else if constexpr (G == 4) {
        v[0] = dppf<0x00>(a);
        v[1] = dppf<0x55>(a);
        v[2] = dppf<0xAA>(a);
        v[3] = dppf<0xFF>(a);
        return;
    } else if constexpr (G == 8) {
        const bool hi = (c.lig & 4) != 0;
        float t[4];
        t[0] = dppf<0x00>(a);
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
        return;
    }
    const int base = c.lane & ~(G - 1);
#pragma unroll
    for (int j = 0; j < G; ++j) v[j] = __shfl(a, base + j, 64);
}

// Node of size G at position p (one LLR per lane).  Returns this lane's partial-sum bit.
template <int LOG_N, int LOG_G>
__device__ __forceinline__ uint32_t bottom(float a, int p, const Ctx& c) {
    constexpr int G = 1 << LOG_G;
    if constexpr (G == 1) {
        return ((rl(c.vfrozen, p >> 5) >> (p & 31)) & 1u) ? 0u : hd(a);
    } else {
        if (is_r0<LOG_N, LOG_G>(c, p)) return 0u;
        constexpr uint32_t GM = (1u << G) - 1u;
        const uint32_t fw = (rl(c.vfrozen, p >> 5) >> (p & 31)) & GM;
        float v[G];
        gather<G>(a, c, v);
        const uint32_t beta = inl<LOG_G, 0>(v, fw, c.imax);
        return bitof(beta, c.lig);
    }
}

template <int LOG_N, int LOG_G, int s>
__device__ BetaT<(1 << (s - LOG_G))> node(const float (&a)[1 << (s - LOG_G)], int p, const Ctx& c);

template <int LOG_N, int LOG_G, int s>
__device__ __forceinline__ BetaT<(1 << (s - LOG_G))> child(const float (&x)[1 << (s - LOG_G)], int p, const Ctx& c) {
    if constexpr (s == LOG_G) {
        return bottom<LOG_N, LOG_G>(x[0], p, c);
    } else {
        return node<LOG_N, LOG_G, s>(x, p, c);
    }
}

template <int LOG_N, int s>
__device__ __forceinline__ bool child_r0(const Ctx& c, int p) {
    if constexpr (s == 0) {
        return (rl(c.vfrozen, p >> 5) >> (p & 31)) & 1u;
    } else {
        return is_r0<LOG_N, s>(c, p);
    }
}

// Node at stage s (size 2^s) starting at position p: left child on f, right child on g with the left
// child's partial sums.
template <int LOG_N, int LOG_G, int s>
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
                for (int j = 0; j < H; ++j) x[j] = fop(a[j], a[j + H]);
            } else {
#pragma unroll
                for (int j = 0; j < H; ++j) x[j] = gop(a[j], a[j + H], bitof(bl, j), c.imax);
            }
            const BH b = child<LOG_N, LOG_G, s - 1>(x, p + side * h, c);
            if (side == 0) bl = b; else br = b;
        }
    } else {
        if (!left_r0) {
#pragma unroll
            for (int j = 0; j < H; ++j) x[j] = fop(a[j], a[j + H]);
            bl = child<LOG_N, LOG_G, s - 1>(x, p, c);
        }
#pragma unroll
        for (int j = 0; j < H; ++j) x[j] = gop(a[j], a[j + H], bitof(bl, j), c.imax);
        br = child<LOG_N, LOG_G, s - 1>(x, p + h, c);
    }
    return (BT)(bl ^ br) | ((BT)br << H);
}

// u = x * G_n on this lane's packed slots (as sc_kernel.hip): spans >= G in-lane, < G cross-lane.
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

// Root.  Stage LOG_N is the unpacked row ch[] (n/G floats a lane, as the float kernel holds its channel);
// stage LOG_N - 1 is not held: each of its values is recomputed from two row values when the
// stage-(LOG_N - 1) node needs it (sc_kernel.hip's virtual root).
template <int NSL>
__device__ __forceinline__ float root_alpha(const float (&ch)[NSL], const Ctx& c, int side, uint64_t bl_root, int j) {
    const float x = ch[j], y = ch[j + NSL / 2];
    return side == 0 ? fop(x, y) : gop(x, y, bitof(bl_root, j), c.imax);
}

template <int LOG_N, int LOG_G>
__device__ __forceinline__ BetaT<((1 << LOG_N) >> LOG_G) / 2> half_node(
    float (&ch)[(1 << LOG_N) >> LOG_G], const Ctx& c, int side, uint64_t bl_root) {
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
        // The stage-(LOG_N - 1) values do not depend on sd (and the f ones not on side): without this the
        // compiler computes them ahead of the loops and holds them, n/G more registers than there are.  The
        // empty asm emits nothing; it only makes the row's registers opaque once per pass.  The same for the
        // root's partial sums, whose n/2G sign masks (bit << 31) it would otherwise hold as well.
#pragma unroll
        for (int j = 0; j < 2 * E; ++j) asm volatile("" : "+v"(ch[j]));
        asm volatile("" : "+v"(bl_root));
#pragma unroll
        for (int j0 = 0; j0 < H; j0 += CH) {  // in chunks, so the scheduler cannot compute every a0, a1 first
#pragma unroll
            for (int j = j0; j < j0 + CH; ++j) {
                const float a0 = root_alpha(ch, c, side, bl_root, j);
                const float a1 = root_alpha(ch, c, side, bl_root, j + H);
                x[j] = sd == 0 ? fop(a0, a1) : gop(a0, a1, bitof(bl, j), c.imax);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        const BH b = child<LOG_N, LOG_G, s - 1>(x, p + sd * h, c);
        if (sd == 0) bl = b; else br = b;
    }
    return (BT)(bl ^ br) | ((BT)br << H);
}

// Returns the packed re-encoded codeword slots of this lane (x = u * G_n).
template <int LOG_N, int LOG_G>
__device__ __forceinline__ void root(float (&ch)[(1 << LOG_N) >> LOG_G], const Ctx& c, uint64_t& lo, uint64_t& hi) {
    constexpr int N = 1 << LOG_N, G = 1 << LOG_G, H = (N / G) / 2;
    using BH = BetaT<H>;
    BH bl = 0, br = 0;
    if constexpr (LOG_N - 1 == LOG_G) {
        // n = 2: the halves are leaves, fed straight from the row
        const float x = ch[0], y = ch[1];
        bl = bottom<LOG_N, LOG_G>(fop(x, y), 0, c);
        br = bottom<LOG_N, LOG_G>(gop(x, y, bl, c.imax), N / 2, c);
    } else {
#pragma unroll 1
        for (int side = 0; side < 2; ++side) {
            const BH b = half_node<LOG_N, LOG_G>(ch, c, side, (uint64_t)bl);
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

template <int LOG_N, int OUTK>
__global__ __launch_bounds__(64 * kWavesPerBlock, min_waves(LOG_N)) void scq_decode_kernel(
    const int8_t* __restrict__ llr_q, int64_t bs, void* __restrict__ out, const uint32_t* __restrict__ frozen_words,
    const uint32_t* __restrict__ r0_words, const int32_t* __restrict__ info_pos, int k, float imax) {
    constexpr int LOG_G = (LOG_N > 7) ? (LOG_N - 7) : 0;
    constexpr int N = 1 << LOG_N, G = 1 << LOG_G, C = 64 / G;
    constexpr int NSL = N / G;            // slots per lane (<= 128)
    constexpr int WPL = (NSL + 31) / 32;  // u words per lane
    constexpr int WPC = (N + 31) / 32;    // frozen words
    __shared__ uint32_t ulds[kWavesPerBlock * 64 * WPL];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane >> LOG_G;
    const int64_t cw0 = ((int64_t)blockIdx.x * kWavesPerBlock + wave) * C;
    const int64_t cw = cw0 + grp;

    Ctx c;
    c.vfrozen = lane < WPC ? frozen_words[lane] : 0u;
    c.vr0 = r0_words[lane];
    c.lane = lane;
    c.lig = lane & (G - 1);
    c.imax = imax;

    // rows past the batch decode the last row again (no store): every lane stays in the cross-lane steps
    Row<LOG_N, LOG_G> row;
    row.load(llr_q + (size_t)(cw < bs ? cw : bs - 1) * N, c);

    float ch[NSL];
    row.unpack(imax, ch);

    uint64_t lo, hi;
    root<LOG_N, LOG_G>(ch, c, lo, hi);
    butterfly<G>(lo, hi, NSL, c.lig);

    uint32_t* mine = ulds + (wave * 64 + lane) * WPL;
    mine[0] = (uint32_t)lo;
    if constexpr (WPL > 1) mine[1] = (uint32_t)(lo >> 32);
    if constexpr (WPL > 2) {
        mine[2] = (uint32_t)hi;
        mine[3] = (uint32_t)(hi >> 32);
    }
    __syncthreads();

    // Gather the k information bits (info_pos ascending) -> coalesced rows.
    const uint32_t* ubase = ulds + wave * 64 * WPL;
    for (int g = 0; g < C; ++g) {
        const int64_t r = cw0 + g;
        if (r >= bs) break;
        for (int m = lane; m < k; m += 64) {
            const int pos = info_pos[m];
            const int l = pos & (G - 1), slot = pos >> LOG_G;
            const uint32_t bit = (ubase[(g * G + l) * WPL + (slot >> 5)] >> (slot & 31)) & 1u;
            if constexpr (OUTK == PL_OUT_F32) {
                static_cast<float*>(out)[r * k + m] = bit ? 1.0f : 0.0f;
            } else {
                static_cast<uint8_t*>(out)[r * k + m] = (uint8_t)bit;
            }
        }
    }
}

template <int LOG_N>
void launch_one(const pl_plan* p, const int8_t* llr_q, int64_t bs, float imax, void* out, int out_kind, hipStream_t st) {
    constexpr int LOG_G = (LOG_N > 7) ? (LOG_N - 7) : 0;
    constexpr int C = 64 >> LOG_G;
    const int64_t per_block = (int64_t)kWavesPerBlock * C;
    const int64_t blocks = (bs + per_block - 1) / per_block;
    if (out_kind == PL_OUT_F32) {
        hipLaunchKernelGGL((scq_decode_kernel<LOG_N, PL_OUT_F32>), dim3((unsigned)blocks), dim3(64 * kWavesPerBlock), 0,
                           st, llr_q, bs, out, p->d_frozen_words, p->d_type_words, p->d_info_pos, p->k, imax);
    } else {
        hipLaunchKernelGGL((scq_decode_kernel<LOG_N, PL_OUT_U8>), dim3((unsigned)blocks), dim3(64 * kWavesPerBlock), 0,
                           st, llr_q, bs, out, p->d_frozen_words, p->d_type_words, p->d_info_pos, p->k, imax);
    }
}

// ---- quantiser ----
// q = rint(med3(logit * inv_step, -Cmax, Cmax)), ties to even (v_rndne_f32); +-Inf saturates through the med3.
__device__ __forceinline__ uint32_t quant1(float x, float inv_step, float cmax) {
    const float t = x * inv_step;
    return (uint32_t)(int)rintf(__builtin_amdgcn_fmed3f(t, -cmax, cmax)) & 0xffu;
}

constexpr int kQuantThreads = 256;
constexpr int kQuantMaxBlocks = 4096;

// Grid-stride over groups of four elements: one 16-byte load, one packed 4-byte store.  The count % 4
// elements of the tail, and the whole array when a pointer is not aligned for that (vec == 0), go one by one.
__global__ __launch_bounds__(kQuantThreads) void llr_quantize_kernel(const float* __restrict__ in, int64_t count,
                                                                     float inv_step, float cmax,
                                                                     int8_t* __restrict__ out, int vec) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t quads = vec ? count / 4 : 0;
    const float4* in4 = reinterpret_cast<const float4*>(in);
    uint32_t* out4 = reinterpret_cast<uint32_t*>(out);
    for (int64_t i = tid; i < quads; i += stride) {
        const float4 v = in4[i];
        out4[i] = quant1(v.x, inv_step, cmax) | (quant1(v.y, inv_step, cmax) << 8) |
                  (quant1(v.z, inv_step, cmax) << 16) | (quant1(v.w, inv_step, cmax) << 24);
    }
    for (int64_t i = quads * 4 + tid; i < count; i += stride) out[i] = (int8_t)quant1(in[i], inv_step, cmax);
}

}  // namespace

namespace pl {
int launch_scq(const pl_plan* p, const int8_t* llr_q, int64_t bs, int q_internal, void* out, int out_kind,
               hipStream_t st) {
    if (bs == 0 || p->k == 0) return PL_OK;
    const float imax = (float)((1 << (q_internal - 1)) - 1);
    switch (p->log_n) {
        case 1: launch_one<1>(p, llr_q, bs, imax, out, out_kind, st); break;
        case 2: launch_one<2>(p, llr_q, bs, imax, out, out_kind, st); break;
        case 3: launch_one<3>(p, llr_q, bs, imax, out, out_kind, st); break;
        case 4: launch_one<4>(p, llr_q, bs, imax, out, out_kind, st); break;
        case 5: launch_one<5>(p, llr_q, bs, imax, out, out_kind, st); break;
        case 6: launch_one<6>(p, llr_q, bs, imax, out, out_kind, st); break;
        case 7: launch_one<7>(p, llr_q, bs, imax, out, out_kind, st); break;
        case 8: launch_one<8>(p, llr_q, bs, imax, out, out_kind, st); break;
        case 9: launch_one<9>(p, llr_q, bs, imax, out, out_kind, st); break;
        case 10: launch_one<10>(p, llr_q, bs, imax, out, out_kind, st); break;
        case 11: launch_one<11>(p, llr_q, bs, imax, out, out_kind, st); break;
        default: set_error("pl_scq_decode: n must be a power of two in [2, 2048]"); return PL_ENOTSUP;
    }
    return check_hip(hipGetLastError(), "SCQ decode launch");
}

int launch_llr_quantize(const float* in, int64_t count, float inv_step, int q_channel, int8_t* out, hipStream_t st) {
    if (count == 0) return PL_OK;
    const float cmax = (float)((1 << (q_channel - 1)) - 1);
    const int vec = ((reinterpret_cast<uintptr_t>(in) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0) ? 1 : 0;
    const int64_t items = vec ? (count + 3) / 4 : count;
    int64_t blocks = (items + kQuantThreads - 1) / kQuantThreads;
    if (blocks > kQuantMaxBlocks) blocks = kQuantMaxBlocks;
    hipLaunchKernelGGL(llr_quantize_kernel, dim3((unsigned)blocks), dim3(kQuantThreads), 0, st, in, count, inv_step, cmax,
                       out, vec);
    return check_hip(hipGetLastError(), "LLR quantise launch");
}
}  // namespace pl
