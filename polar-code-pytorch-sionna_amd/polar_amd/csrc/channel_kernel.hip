// channel_kernel.hip -- the Monte-Carlo caller side of the decoder, fused for gfx950:
//
//   awgn_llr_kernel   System_AWGN_model.forward up to the decoder call (x_run_sn_polar/
//                     z_sys_model/awgn_model.py:33-41): random information bits
//                     (BinarySource, my_sn/trans/binary_source.py:18-19), polar encoding
//                     (x_run enc.py:30-43), QPSK Gray mapping (my_sn/trans/mapping.py:136-149),
//                     AWGN of variance no (my_sn/trans/channel/awgn.py:19-29), exact demapping to
//                     logits log P(b=1)/P(b=0) (mapping.py:151-241) -- one launch instead of ~15
//                     torch kernels over [bs, n/2] complex tensors.
//   count_errors_kernel  count_errors + count_block_errors (my_sn/sim.py:7-18) in one pass.
//
// Randomness: Philox4x32-10 (Salmon et al., SC'11; the Random123 reference rounds), keyed by the
// 64-bit seed, counter (row, iteration, domain|block).  The reference draws from torch's CPU
// generator; no GPU stream can reproduce that, so parity here is statistical (the decoder input
// has the reference's distribution), and the bit placement is pinned against a numpy Philox in
// the tests.  Info bit r of a row is bit (r mod 32) of stream word r/32 = component (r/32) mod 4
// of Philox block r/128 (domain 0); the noise of positions 4c .. 4c+3 is Philox block c of domain 1
// (Box-Muller on its four uniforms).
//
// Demapping: for Gray QPSK the reference's logsumexp over the constellation reduces exactly
// (mathematically) to logit_j = -2*sqrt(2)*y_j/no on the real/imaginary component y_j carrying
// code bit j (the terms of the other component cancel); computed in fp32 here, the reference's
// fp32 logsumexp rounds differently at the last ulp -- immaterial next to the noise draw.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../../include/polar_mi355x.h"
#include "butterfly.h"
#include "plan.h"

namespace {

struct U4 {
    uint32_t x, y, z, w;
};

// Philox4x32-10 (Random123 philox4x32_R(10, ...)): 10 rounds, key bumped between rounds.
__device__ __forceinline__ U4 philox(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        // the 64-bit products: one v_mad_u64_u32 each (2.2 ns) instead of v_mul_lo + v_mul_hi (4.0 ns,
        // tools/micro/mul_cost.hip)
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.x, p1 = (uint64_t)0xCD9E8D57u * c.z;
        const uint32_t lo0 = (uint32_t)p0, hi0 = (uint32_t)(p0 >> 32);
        const uint32_t lo1 = (uint32_t)p1, hi1 = (uint32_t)(p1 >> 32);
        c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// Parallel bit deposit: bit i of x goes to the position of the i-th set bit of m (Hacker's
// Delight 7-5, "expand"), five log-steps instead of a loop over the set bits (no divergence).
__device__ __forceinline__ uint32_t expand_bits(uint32_t x, uint32_t m) {
    const uint32_t m0 = m;
    uint32_t mk = ~m << 1, mv[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        uint32_t mp = mk ^ (mk << 1);
        mp ^= mp << 2;
        mp ^= mp << 4;
        mp ^= mp << 8;
        mp ^= mp << 16;
        mv[i] = mp & m;
        m = (m ^ mv[i]) | (mv[i] >> (1 << i));
        mk &= ~mp;
    }
#pragma unroll
    for (int i = 4; i >= 0; --i) x = (x & ~mv[i]) | ((x << (1 << i)) & mv[i]);
    return x & m0;
}

// Philox block b of a row's stream in domain d (0: information bits, 1: noise)
__device__ __forceinline__ U4 stream_block(uint32_t k0, uint32_t k1, int64_t row, uint32_t it, uint32_t d, uint32_t b) {
    return philox(U4{(uint32_t)row, (uint32_t)(row >> 32), it, (d << 31) | b}, k0, k1);
}
__device__ __forceinline__ uint32_t comp(const U4& r, int c) { return c == 0 ? r.x : c == 1 ? r.y : c == 2 ? r.z : r.w; }

// Constants of the logit map: logit = a_s + rs * cos/sin(angle), a_s = +-scale/sqrt(2) by the code
// bit, rs = radius * scale * sqrt(no/2) (the radius' sqrt(2 ln 2) folded into rsc).
struct Logit {
    float a;    // scale / sqrt(2)
    float rsc;  // scale * sqrt(no / 2) * sqrt(2 ln 2)
};

#ifndef PL_AWGN_DIAG
#define PL_AWGN_DIAG 0  // development only (tools/micro/producer_cost.hip): 1 no logit stores,
                        // 2 no noise (Philox + Box-Muller), 3 no Philox for the noise
#endif
#if !PL_DEV && PL_AWGN_DIAG
#error "PL_AWGN_DIAG gives wrong results: development builds (-DPL_DEV=1) only"
#endif

// Two Box-Muller pairs from one Philox block, on the hardware transcendentals (a noise draw, not a
// decoder value: only its distribution is specified); the noise of a pair is rs * (c, s).
//   radius  sqrt(-2 ln u) = sqrt(2 ln 2) sqrt(32 - log2 v'), v' = float(v | 1) in [1, 2^32], i.e.
//           u = v' 2^-32 in (0, 1] (tail to 6.66 sigma), v_log_f32 on a normal argument; rsc carries
//           the sqrt(2 ln 2) and the caller's scale;
//   angle   v_sin / v_cos take revolutions and are periodic: the mantissa bits of v under the
//           exponent of 1.0 give 1 + t, t uniform in [0, 1), and sin(2 pi (1 + t)) = sin(2 pi t).
struct Gauss4 {
    float rs0, c0, s0;  // components x, y of the block
    float rs1, c1, s1;  // components z, w
};
__device__ __forceinline__ Gauss4 box_muller(const U4& rnd, float rsc) {
#if PL_AWGN_DIAG == 2
    return Gauss4{rsc, (float)rnd.x, (float)rnd.y, rsc, (float)rnd.z, 1.0f};
#else
    const float rs0 = rsc * __builtin_amdgcn_sqrtf(32.0f - __builtin_amdgcn_logf((float)(rnd.x | 1u)));
    const float rs1 = rsc * __builtin_amdgcn_sqrtf(32.0f - __builtin_amdgcn_logf((float)(rnd.z | 1u)));
    const float t0 = __uint_as_float(0x3F800000u | (rnd.y >> 9)), t1 = __uint_as_float(0x3F800000u | (rnd.w >> 9));
    return Gauss4{rs0, __builtin_amdgcn_cosf(t0), __builtin_amdgcn_sinf(t0), rs1, __builtin_amdgcn_cosf(t1),
                  __builtin_amdgcn_sinf(t1)};
#endif
}

// Four logits from one Philox block and the four code bits in bits 0..3 of `bits`.
__device__ __forceinline__ float4 logits4(const U4& rnd, uint32_t bits, const Logit& lc) {
    const Gauss4 g = box_muller(rnd, lc.rsc);
    // (1 - 2 c) a: the code bit moved to the sign of a
    const uint32_t au = __float_as_uint(lc.a);
    const float a0 = __uint_as_float(au ^ ((bits << 31) & 0x80000000u));
    const float a1 = __uint_as_float(au ^ ((bits << 30) & 0x80000000u));
    const float a2 = __uint_as_float(au ^ ((bits << 29) & 0x80000000u));
    const float a3 = __uint_as_float(au ^ ((bits << 28) & 0x80000000u));
    return float4{__builtin_fmaf(g.rs0, g.c0, a0), __builtin_fmaf(g.rs0, g.s0, a1), __builtin_fmaf(g.rs1, g.c1, a2),
                  __builtin_fmaf(g.rs1, g.s1, a3)};
}

// A wave holds cpw = 64 / wpc codewords (wpc = max(1, n/32) lanes per codeword).  Three phases:
//   A  lane w < nq of a group: stream word w (32 information bits, ranks 32w .. 32w+31) -> LDS;
//   B  lane w of a group ("word layout", position 32w + j = bit j): x_w = the information bits
//      deposited at the word's information positions, then the XOR butterfly -> LDS;
//   C  the whole wave over the wave's rows in chunks of CH = min(4, n) positions ("chunk layout",
//      consecutive lanes -> consecutive chunks, so the fp32 rows are written as whole lines):
//      u rows from the stream words, logit rows from the code bits and one Philox block per chunk.
// The four producer kernels below are sequences of these phases, one function each.
constexpr int kWordsPerWave = 256;  // LDS words per wave: stream words (<= 128) + code words (64)

// What one wave wrote to LDS, every lane of the wave may read after this.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The layout above for a code of n positions (a power of two), as every producer derives it
struct WaveRows {
    int lane, wv;      // lane of the wave, wave of the block
    int wpc, cpw, nb;  // lanes (words) per codeword, codewords per wave, positions per word
    int g, w;          // this lane's codeword of the wave and word of the codeword
    int64_t b0, row;   // first row of this wave (of the call), stream row of this lane's codeword
    int rows;          // rows of this wave to store (<= 0: none)
};
__device__ __forceinline__ WaveRows wave_rows(int n, int64_t row0, int64_t bs) {
    WaveRows L;
    L.wpc = n >= 32 ? n / 32 : 1, L.cpw = 64 / L.wpc, L.nb = n >= 32 ? 32 : n;
    L.lane = threadIdx.x & 63, L.wv = threadIdx.x >> 6;
    L.b0 = ((int64_t)blockIdx.x * 4 + L.wv) * L.cpw;
    L.g = L.lane / L.wpc, L.w = L.lane % L.wpc;
    L.row = row0 + L.b0 + L.g;
    L.rows = bs - L.b0 < L.cpw ? (int)(bs - L.b0) : L.cpw;
    return L;
}

// A: the nq stream words of this lane's row -> sw [cpw][nq] (rows past bs compute harmless values
// that are never stored)
__device__ __forceinline__ void draw_stream_words(uint32_t* sw, int nq, const WaveRows& L, uint32_t k0, uint32_t k1,
                                                  uint32_t it) {
    for (int q = L.w; q < nq; q += L.wpc) sw[L.g * nq + q] = comp(stream_block(k0, k1, L.row, it, 0, q >> 2), q & 3);
}

// B: this lane's code word from its row's bits (src [cpw][nsrc] words).  Information positions of
// the word (frozen bit 0), their first rank = information positions in the group's earlier words
// (prefix sum over the group's lanes); the next (up to 32) bits of the row deposited at them in
// order; x = u G_n.
__device__ __forceinline__ uint32_t encode_word(const uint32_t* src, int nsrc, const uint32_t* __restrict__ frozen_words,
                                                const WaveRows& L) {
    const uint32_t live = L.nb == 32 ? 0xFFFFFFFFu : ((1u << L.nb) - 1u);
    const uint32_t info = ~frozen_words[L.w] & live;
    int base = 0;
    {
        int c = __popc(info), incl = c;
        for (int d = 1; d < L.wpc; d <<= 1) {
            const int o = __shfl_up(incl, d, 64);
            if (L.w >= d) incl += o;
        }
        base = incl - c;
    }
    uint32_t x = 0u;
    if (info) {
        const uint32_t* srow = src + L.g * nsrc;
        const int q0 = base >> 5, sh = base & 31;
        const uint32_t lo = q0 < nsrc ? srow[q0] : 0u;
        const uint32_t hi = q0 + 1 < nsrc ? srow[q0 + 1] : 0u;
        x = expand_bits((uint32_t)((((uint64_t)hi << 32) | lo) >> sh), info);
    }
    return pl::polar_butterfly(x, L.nb, L.wpc, L.w);
}

// C1: u rows (BinarySource output, float32 0/1) of the wave's rows from sw [cpw][nq]
__device__ __forceinline__ void store_u_rows(float* __restrict__ u_out, const uint32_t* sw, int nq, int k,
                                             const WaveRows& L) {
    if (u_out == nullptr || k <= 0) return;
    if ((k & 3) == 0 && ((reinterpret_cast<uintptr_t>(u_out) & 15) == 0)) {
        const int kq = k >> 2;
        for (int c = L.lane; c < L.rows * kq; c += 64) {
            const int r = c / kq, p = (c - r * kq) * 4;
            const uint32_t v = sw[r * nq + (p >> 5)] >> (p & 31);
            reinterpret_cast<float4*>(u_out + (L.b0 + r) * k)[p >> 2] =
                float4{(float)(v & 1u), (float)((v >> 1) & 1u), (float)((v >> 2) & 1u), (float)((v >> 3) & 1u)};
        }
    } else {
        for (int c = L.lane; c < L.rows * k; c += 64) {
            const int r = c / k, p = c - r * k;
            u_out[(L.b0 + r) * k + p] = (float)((sw[r * nq + (p >> 5)] >> (p & 31)) & 1u);
        }
    }
}

// C1': the information bits packed, nq = ceil(k/32) words per row (bit m of a row = bit m % 32 of
// word m / 32: the stream words themselves, bits past k cleared) -- the reference of
// pl_sc_decode_count and pl_count_errors_packed, 1/32 of the fp32 rows' bytes
__device__ __forceinline__ void store_packed_rows(uint32_t* __restrict__ ubits_out, const uint32_t* sw, int nq, int k,
                                                  const WaveRows& L) {
    if (ubits_out == nullptr) return;
    const uint32_t last = (k & 31) ? ((1u << (k & 31)) - 1u) : 0xFFFFFFFFu;
    for (int r = 0; r < L.rows; ++r)
        for (int q = L.lane; q < nq; q += 64)
            ubits_out[(L.b0 + r) * nq + q] = sw[r * nq + q] & (q == nq - 1 ? last : 0xFFFFFFFFu);
}

__global__ __launch_bounds__(256) void awgn_llr_kernel(int64_t bs, int64_t row0, uint32_t k0, uint32_t k1, uint32_t it,
                                                       float no, const uint32_t* __restrict__ frozen_words, int n, int k,
                                                       float* __restrict__ u_out, float* __restrict__ llr_out,
                                                       uint32_t* __restrict__ ubits_out) {
    __shared__ uint32_t lds[4 * kWordsPerWave];
    const WaveRows L = wave_rows(n, row0, bs);
    const int nq = (k + 31) / 32;                 // stream words per row
    uint32_t* sw = lds + L.wv * kWordsPerWave;    // [cpw][nq] stream words
    uint32_t* cwd = sw + L.cpw * nq;              // [cpw][wpc] code words
    const int lane = L.lane, wpc = L.wpc, rows = L.rows;
    const int64_t b0 = L.b0;

    draw_stream_words(sw, nq, L, k0, k1, it);
    wave_sync();
    cwd[L.g * wpc + L.w] = encode_word(sw, nq, frozen_words, L);
    wave_sync();
    if (rows <= 0) return;
    store_u_rows(u_out, sw, nq, k, L);
    store_packed_rows(ubits_out, sw, nq, k, L);
    // C2: logits.  QPSK component of code bit j: (1 - 2 c_j)/sqrt(2) plus sqrt(no) * N(0, 1/2)
    // (awgn.py:24-29, utils.py:11-15); logit = -2 sqrt(2) y / no.  Chunk c of a row = positions
    // [CH c, CH c + CH) draws noise block c (4 uniforms -> 2 Box-Muller pairs).
    const float scale = -2.8284271f / no;
    const Logit lc{scale * 0.70710677f, scale * sqrtf(no) * 0.70710677f * 1.17741002f};  // sqrt(2 ln 2)
    const int CH = n >= 4 ? 4 : n, nch = n / CH, lnch = __builtin_ctz(nch);  // n is a power of two
    const bool vec = CH == 4 && ((reinterpret_cast<uintptr_t>(llr_out) & 15) == 0);
    if (vec && nch >= 64) {
        // rows outer (the row, hence the first Philox products, uniform across the wave), the
        // wave's lanes over the row's chunks: one 1-KiB float4 store per instruction
        for (int r = 0; r < rows; ++r) {
            const int64_t grow = row0 + b0 + r;
            const uint32_t* cw = cwd + r * wpc;
            float4* o = reinterpret_cast<float4*>(llr_out + (b0 + r) * n);
            for (int ch = lane; ch < nch; ch += 64) {
#if PL_AWGN_DIAG == 3
                const U4 rnd = U4{(uint32_t)ch * 0x9E3779B9u, (uint32_t)ch * 0x85EBCA6Bu, (uint32_t)ch * 0xC2B2AE35u,
                                  (uint32_t)ch * 0x27D4EB2Fu};
#else
                const U4 rnd = stream_block(k0, k1, grow, it, 1, (uint32_t)ch);
#endif
                const float4 l = logits4(rnd, cw[ch >> 3] >> ((ch & 7) * 4), lc);
#if PL_AWGN_DIAG == 1
                if (l.x + l.y + l.z + l.w != 1234.5f) continue;
#endif
                o[ch] = l;
            }
        }
        return;
    }
    for (int c = lane; c < rows * nch; c += 64) {
        const int r = c >> lnch, ch = c & (nch - 1), p = ch * CH;
        const U4 rnd = stream_block(k0, k1, row0 + b0 + r, it, 1, (uint32_t)ch);
        const float4 l = logits4(rnd, cwd[r * wpc + (p >> 5)] >> (p & 31), lc);
        float* o = llr_out + (b0 + r) * n + p;
        if (vec) {
            *reinterpret_cast<float4*>(o) = l;
        } else {
            const float lv[4] = {l.x, l.y, l.z, l.w};
            for (int i = 0; i < CH; ++i) o[i] = lv[i];
        }
    }
}

// nr_awgn_llr_kernel: the 5G NR link up to the mother decoder's input, one launch -- BinarySource,
// Polar5GEncoder.forward (my_sn/fec/polar/enc.py:359-392: CRC attach, polar encode, rate matching),
// Gray QPSK, AWGN, the demapper, and Polar5GDecoder.forward's rate recovery (dec.py:609-638).
// The wave layout is awgn_llr_kernel's (cpw = 64 / wpc rows per wave, wpc = n / 32 lanes per row,
// n = n_polar = 32 ... 1024), with these phases:
//   A   stream words of the kt = k_target information bits (the streams of awgn_llr_kernel) -> LDS;
//   A'  CRC parity (pl_crc_attach's rule): each lane XORs the generator rows of the 1 bits of its
//       word, an XOR reduction over the row's lanes; [information bits | parity] -> LDS;
//   B   as awgn_llr_kernel, over the k = kt + degree bits: deposit, butterfly -> code words in LDS;
//   C   in passes of R rows (R * 4 ceil(E/4) <= kNrStage floats of LDS per wave):
//       C2  the wave's lanes over (row, chunk of 4 transmitted positions): bit e = c[rm_idx[e]],
//           noise block `chunk` of domain 1 (one Philox block per 4 positions, as awgn_llr_kernel
//           with E in place of n), logits -> the LDS stage (and llr_ch_out);
//       C3  the wave's lanes over (row, 4 mother positions): pl_rate_recover's rule gathered from
//           the stage (one fp32 add where two copies combine), whole-line stores to llr_out.
// The generator rows sit in LDS once per block, padded by one word per 32 so that the lanes of a
// row (word stride 32) read distinct banks.
constexpr int kNrStage = 2176;              // stage floats per wave: two rows of E = 1088
constexpr int kNrMaxK = 1024;               // generator rows staged per block
constexpr int kNrGWords = kNrMaxK + kNrMaxK / 32;


// The generator rows of the kt information bits -> s_g (row m at word m + m / 32); block-wide, the
// caller's __syncthreads() follows.
__device__ __forceinline__ void stage_crc_rows(uint32_t* s_g, const uint32_t* __restrict__ g_rows, int kt) {
    for (int m = threadIdx.x; m < kt; m += 256) s_g[m + (m >> 5)] = g_rows[m];
}

// A': parity of this lane's row from sw [cpw][nq] and the staged generator rows; [information bits |
// parity] -> kw [cpw][nkq].  nq <= wpc (kt < n), so lane w < nq owns word w of its row.
__device__ __forceinline__ void crc_attach(uint32_t* kw, int nkq, const uint32_t* sw, int nq, const uint32_t* s_g, int kt,
                                           int degree, const WaveRows& L) {
    const int g = L.g, w = L.w;
    const uint32_t last = (kt & 31) ? ((1u << (kt & 31)) - 1u) : 0xFFFFFFFFu;
    const uint32_t mine = w < nq ? sw[g * nq + w] & (w == nq - 1 ? last : 0xFFFFFFFFu) : 0u;
    uint32_t par = 0u;
    {
        const uint32_t* gr = s_g + w * 33;
#pragma unroll 8
        for (int j = 0; j < 32; ++j)
            if ((mine >> j) & 1u) par ^= gr[j];
    }
    for (int d = 1; d < L.wpc; d <<= 1) par ^= (uint32_t)__shfl_xor((int)par, d, 64);
    if (degree < 32) par &= (1u << degree) - 1u;
    if (w < nkq) {
        const uint64_t pv = (uint64_t)par << (kt & 31);  // parity bit c = bit kt + c of the row
        const int pw = kt >> 5;
        kw[g * nkq + w] = mine | (w == pw ? (uint32_t)pv : 0u) | (w == pw + 1 ? (uint32_t)(pv >> 32) : 0u);
    }
}

// Rate matching: the P code bits transmitted at positions p .. p + P - 1 (bit e = c[rm_idx[e]]) of
// the code word cw [wpc], position p + i in bit i.  vec: rm_idx + p is 16-byte aligned and the P
// positions lie inside the row.
template <int P>
__device__ __forceinline__ uint32_t gather_code_bits(const uint32_t* cw, const int32_t* __restrict__ rm_idx, int p,
                                                     int e_len, bool vec, int n) {
    int id[P];
    if (vec) {
#pragma unroll
        for (int i = 0; i < P; i += 4) {
            const int4 v = *reinterpret_cast<const int4*>(rm_idx + p + i);
            id[i] = v.x, id[i + 1] = v.y, id[i + 2] = v.z, id[i + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < P; ++i) id[i] = p + i < e_len ? rm_idx[p + i] : 0;
    }
    uint32_t bits = 0u;
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const int j = id[i] & (n - 1);  // a table entry outside the codeword cannot leave the row
        bits |= ((cw[j >> 5] >> (j & 31)) & 1u) << i;
    }
    return bits;
}

// C3: rate recovery (pl_rate_recover's tables and arithmetic) of rc rows from the stage (rows of epad
// floats) to rows r0 .. of the wave, followed by the wave's sync (the next pass rewrites the stage).
__device__ __forceinline__ void recover_rows(float* __restrict__ llr_out, const float* st, int epad, int e_len, int r0,
                                             int rc, const int32_t* __restrict__ src_a, const int32_t* __restrict__ src_b,
                                             const float* __restrict__ fill, int n, const WaveRows& L) {
    const bool tab_vec = ((reinterpret_cast<uintptr_t>(src_a) & 15) == 0) &&
                         ((reinterpret_cast<uintptr_t>(src_b) & 15) == 0) &&
                         ((reinterpret_cast<uintptr_t>(fill) & 15) == 0) && ((reinterpret_cast<uintptr_t>(llr_out) & 15) == 0);
    const int nj = n >> 2, lnj = __builtin_ctz(nj);
    for (int c = L.lane; c < rc * nj; c += 64) {
        const int rl = c >> lnj, jc = c & (nj - 1), r = r0 + rl;
        int a[4], b[4];
        float f[4];
        if (tab_vec) {
            const int4 va = reinterpret_cast<const int4*>(src_a)[jc];
            a[0] = va.x, a[1] = va.y, a[2] = va.z, a[3] = va.w;
            b[0] = b[1] = b[2] = b[3] = -1;
            if (src_b != nullptr) {
                const int4 vb = reinterpret_cast<const int4*>(src_b)[jc];
                b[0] = vb.x, b[1] = vb.y, b[2] = vb.z, b[3] = vb.w;
            }
            f[0] = f[1] = f[2] = f[3] = 0.0f;
            if (fill != nullptr) {
                const float4 vf = reinterpret_cast<const float4*>(fill)[jc];
                f[0] = vf.x, f[1] = vf.y, f[2] = vf.z, f[3] = vf.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[i] = src_a[jc * 4 + i];
                b[i] = src_b ? src_b[jc * 4 + i] : -1;
                f[i] = fill ? fill[jc * 4 + i] : 0.0f;
            }
        }
        const float* x4 = st + rl * epad;
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            // entries past E - 1 are clamped: a bad table reads another position, never another row
            const int ia = a[i] < e_len ? a[i] : e_len - 1, ib = b[i] < e_len ? b[i] : e_len - 1;
            v[i] = f[i];
            if (ia >= 0) v[i] = ib >= 0 ? x4[ia] + x4[ib] : x4[ia];  // llr_1 + llr_3 (dec.py:629-633)
        }
        float* o = llr_out + (L.b0 + r) * n + jc * 4;
        if (tab_vec) {
            *reinterpret_cast<float4*>(o) = float4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = v[i];
        }
    }
    wave_sync();
}

__global__ __launch_bounds__(256) void nr_awgn_llr_kernel(
    int64_t bs, int64_t row0, uint32_t k0, uint32_t k1, uint32_t it, float no, const uint32_t* __restrict__ frozen_words,
    int n, int k, int kt, const uint32_t* __restrict__ g_rows, int degree, const int32_t* __restrict__ rm_idx, int e_len,
    const int32_t* __restrict__ src_a, const int32_t* __restrict__ src_b, const float* __restrict__ fill,
    float* __restrict__ u_out, uint32_t* __restrict__ ubits_out, float* __restrict__ llr_ch_out,
    float* __restrict__ llr_out) {
    __shared__ uint32_t s_g[kNrGWords];
    __shared__ uint32_t lds[4 * 192];
    __shared__ __attribute__((aligned(16))) float s_stage[4 * kNrStage];
    __builtin_assume(n >= 32);  // whole words: wpc = n / 32, nb = 32
    const WaveRows L = wave_rows(n, row0, bs);
    const int nq = (kt + 31) / 32, nkq = (k + 31) / 32;  // words of the information bits / with the parity
    uint32_t* sw = lds + L.wv * 192;                      // [cpw][nq] stream words
    uint32_t* kw = sw + 64;                               // [cpw][nkq] information bits | parity
    uint32_t* cwd = sw + 128;                             // [cpw][wpc] code words
    float* st = s_stage + L.wv * kNrStage;
    const int lane = L.lane, wpc = L.wpc, cpw = L.cpw, rows = L.rows;
    const int64_t b0 = L.b0;

    stage_crc_rows(s_g, g_rows, kt);
    draw_stream_words(sw, nq, L, k0, k1, it);
    __syncthreads();
    crc_attach(kw, nkq, sw, nq, s_g, kt, degree, L);
    wave_sync();
    cwd[L.g * wpc + L.w] = encode_word(kw, nkq, frozen_words, L);
    wave_sync();
    if (rows <= 0) return;
    store_u_rows(u_out, sw, nq, kt, L);
    store_packed_rows(ubits_out, sw, nq, kt, L);

    const float scale = -2.8284271f / no;
    const Logit lc{scale * 0.70710677f, scale * sqrtf(no) * 0.70710677f * 1.17741002f};  // sqrt(2 ln 2)
    const int nch = (e_len + 3) >> 2, epad = nch * 4;  // chunks of 4 transmitted positions per row
    const int rpp = kNrStage / epad < cpw ? kNrStage / epad : cpw;  // rows per pass (>= 1: E <= kNrStage)
    const bool ch_vec = (e_len & 3) == 0 && ((reinterpret_cast<uintptr_t>(llr_ch_out) & 15) == 0) &&
                        ((reinterpret_cast<uintptr_t>(rm_idx) & 15) == 0);
    for (int r0 = 0; r0 < rows; r0 += rpp) {
        const int rc = rows - r0 < rpp ? rows - r0 : rpp;
        // C2: rate matching, QPSK, AWGN, demapper -> stage (+ llr_ch_out)
        for (int c = lane; c < rc * nch; c += 64) {
            const int rl = c / nch, ch = c - rl * nch, r = r0 + rl, p = ch * 4;
            const uint32_t bits = gather_code_bits<4>(cwd + r * wpc, rm_idx, p, e_len, ch_vec, n);
            const U4 rnd = stream_block(k0, k1, row0 + b0 + r, it, 1, (uint32_t)ch);
            const float4 l = logits4(rnd, bits, lc);
            *reinterpret_cast<float4*>(st + rl * epad + p) = l;
            if (llr_ch_out != nullptr) {
                float* o = llr_ch_out + (b0 + r) * e_len + p;
                if (ch_vec) {
                    *reinterpret_cast<float4*>(o) = l;
                } else {
                    const float lv[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (p + i < e_len) o[i] = lv[i];
                }
            }
        }
        wave_sync();
        recover_rows(llr_out, st, epad, e_len, r0, rc, src_a, src_b, fill, n, L);
    }
}

// ---- 16/64/256-QAM (M = bits per symbol = 4, 6, 8; H = M / 2 bits per axis) -------------------
// Symbol s of a row carries positions M s .. M s + M - 1, first bit most significant (Mapper,
// my_sn/trans/mapping.py:135-148); its real part is the Gray PAM level of bits b[0::2], its
// imaginary part that of b[1::2] (mapping.py:7-48).  The 2^H unit-energy levels come from the host
// (pl::qam_levels), indexed by the axis label (first bit = MSB).
// Work item: one lane = one Philox noise block (domain 1, block c) = the symbol pair (2c, 2c + 1) =
// 2M consecutive positions; components x, y are the Box-Muller pair of symbol 2c (re, im), z, w that
// of symbol 2c + 1 -- logits4's radius/angle construction, and for M = 2 the QPSK layout above.
struct Qam {
    float lev[16];  // PAM level of axis label a < 2^H
    float d;        // half the level spacing: the levels are the odd multiples of d
    float inv2d;    // 1 / (2 d)
};

// The received pair (re0, im0, re1, im1) from the pair's noise block and its 2M code bits (position
// i of the pair = bit i of `bits`); s_lev: the level table in LDS (the label is masked to 2^H - 1).
template <int M>
__device__ __forceinline__ float4 qam_receive(const U4& rnd, uint32_t bits, const float* s_lev, float rsig) {
    constexpr int H = M / 2;
    float x[4];
#pragma unroll
    for (int ax = 0; ax < 4; ++ax) {  // axis ax & 1 (0 re, 1 im) of symbol ax >> 1
        uint32_t a = 0u;
#pragma unroll
        for (int j = 0; j < H; ++j) a |= ((bits >> ((ax >> 1) * M + 2 * j + (ax & 1))) & 1u) << (H - 1 - j);
        x[ax] = s_lev[a & ((1u << H) - 1u)];
    }
    const Gauss4 g = box_muller(rnd, rsig);
    return float4{__builtin_fmaf(g.rs0, g.c0, x[0]), __builtin_fmaf(g.rs0, g.s0, x[1]), __builtin_fmaf(g.rs1, g.c1, x[2]),
                  __builtin_fmaf(g.rs1, g.s1, x[3])};
}

// The level table -> LDS (one thread; the caller's __syncthreads() follows)
__device__ __forceinline__ void stage_levels(float* s_lev, const Qam& qam) {
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 16; ++a) s_lev[a] = qam.lev[a];
    }
}

// Logits of the H bits of one axis from its received component y, written to out[0], out[2], ...
// (the symbol's bits alternate re, im).  lev: the 2^H levels (the kernel argument itself, scalar
// registers, in the plain kernel; the LDS copy in the NR kernel, which has no scalar registers to
// spare), d / inv2d: Qam's.  The reference's logsumexp over the 2^M points
// (mapping.py:225-241, :195-205) factors per axis for a Gray square constellation: |y - c|^2 =
// (y_re - l_re)^2 + (y_im - l_im)^2, and both sets of a real-axis bit hold every imaginary level,
// so that factor cancels in the ratio.  Exponents are taken relative to l*, the level nearest y:
//   t_l = (-(y - l)^2 + (y - l*)^2) / no = (l - l*) (2 y - l - l*) / no  <= 0,
// the difference formed before the division (no y^2 term to cancel).  One exp per level serves all
// H bits; where a set's sum comes near the fp32 underflow (small no: the set without l* lies far
// from y) the lane repeats the sums with each set's own maximum, as torch.logsumexp does.
// expf / logf are the library functions (a decoder input, not a noise draw).
template <int H>
__device__ __forceinline__ void qam_axis_llr(float y, const float* lev, float d, float inv2d, float inv_no, float* out) {
    constexpr int NL = 1 << H;
    float j = __builtin_rintf(__builtin_fmaf(y, inv2d, -0.5f));
    j = fminf(fmaxf(j, -(float)(NL / 2)), (float)(NL / 2 - 1));
    const float ls = __builtin_fmaf(2.0f, j, 1.0f) * d;
    const float s = 2.0f * y - ls;
    float t[NL], s0[H], s1[H];
#pragma unroll
    for (int i = 0; i < H; ++i) s0[i] = s1[i] = 0.0f;
#pragma unroll
    for (int a = 0; a < NL; ++a) {
        const float l = lev[a];
        t[a] = (l - ls) * (s - l) * inv_no;
        const float w = expf(t[a]);
#pragma unroll
        for (int i = 0; i < H; ++i) {
            if ((a >> (H - 1 - i)) & 1) s1[i] += w;
            else s0[i] += w;
        }
    }
    float low = s0[0];
#pragma unroll
    for (int i = 0; i < H; ++i) low = fminf(low, fminf(s0[i], s1[i]));
    if (low >= 1e-30f) {
#pragma unroll
        for (int i = 0; i < H; ++i) out[2 * i] = logf(s1[i]) - logf(s0[i]);
        return;
    }
#pragma unroll
    for (int i = 0; i < H; ++i) {
        float m0 = -INFINITY, m1 = -INFINITY;
#pragma unroll
        for (int a = 0; a < NL; ++a) {
            if ((a >> (H - 1 - i)) & 1) m1 = fmaxf(m1, t[a]);
            else m0 = fmaxf(m0, t[a]);
        }
        float z0 = 0.0f, z1 = 0.0f;
#pragma unroll
        for (int a = 0; a < NL; ++a) {
            if ((a >> (H - 1 - i)) & 1) z1 += expf(t[a] - m1);
            else z0 += expf(t[a] - m0);
        }
        out[2 * i] = (m1 - m0) + (logf(z1) - logf(z0));
    }
}

// awgn_qam_llr_kernel<M>: awgn_llr_kernel with a 2^M-QAM mapper and demapper (M = 4, 8; M divides n).
// Phases A, B, C1, C1' are awgn_llr_kernel's; C2 takes the wave's lanes over (row, symbol pair).
// y_out (nullable): [bs, n / M, 2] fp32 received symbols (re, im).
template <int M>
__global__ __launch_bounds__(256) void awgn_qam_llr_kernel(int64_t bs, int64_t row0, uint32_t k0, uint32_t k1, uint32_t it,
                                                           float no, const uint32_t* __restrict__ frozen_words, int n,
                                                           int k, Qam qam, float* __restrict__ u_out,
                                                           float* __restrict__ llr_out, uint32_t* __restrict__ ubits_out,
                                                           float* __restrict__ y_out) {
    __shared__ uint32_t lds[4 * kWordsPerWave];
    __shared__ float s_lev[16];
    const WaveRows L = wave_rows(n, row0, bs);
    const int nq = (k + 31) / 32;                 // stream words per row
    uint32_t* sw = lds + L.wv * kWordsPerWave;    // [cpw][nq] stream words
    uint32_t* cwd = sw + L.cpw * nq;              // [cpw][wpc] code words
    const int lane = L.lane, wpc = L.wpc, rows = L.rows;
    const int64_t b0 = L.b0;

    stage_levels(s_lev, qam);
    draw_stream_words(sw, nq, L, k0, k1, it);
    __syncthreads();
    cwd[L.g * wpc + L.w] = encode_word(sw, nq, frozen_words, L);
    wave_sync();
    if (rows <= 0) return;
    store_u_rows(u_out, sw, nq, k, L);
    store_packed_rows(ubits_out, sw, nq, k, L);
    // C2: y = x + sqrt(no) * N(0, 1/2) per component (awgn.py:24-29, utils.py:11-15), the demapper.
    // Pair pc of a row = positions [2M pc, 2M pc + 2M) (n >= 2M: inside one code word, M = 4, 8),
    // noise block pc; with one symbol per row (n = M) the pair's second half is unused.
    const float inv_no = 1.0f / no, rsig = sqrtf(no) * 0.70710677f * 1.17741002f;  // sqrt(2 ln 2)
    const int ns = n / M, npair = (ns + 1) >> 1;
    const bool vec = (reinterpret_cast<uintptr_t>(llr_out) & 15) == 0;
    for (int c = lane; c < rows * npair; c += 64) {
        const int r = c / npair, pc = c - r * npair, p = pc * 2 * M;
        const U4 rnd = stream_block(k0, k1, row0 + b0 + r, it, 1, (uint32_t)pc);
        const float4 y = qam_receive<M>(rnd, cwd[r * wpc + (p >> 5)] >> (p & 31), s_lev, rsig);
#pragma unroll 1
        for (int s = 0; s < 2; ++s) {
            const int sym = 2 * pc + s;
            if (sym >= ns) break;
            const float yr = s ? y.z : y.x, yi = s ? y.w : y.y;
            float l[M];
            qam_axis_llr<M / 2>(yr, qam.lev, qam.d, qam.inv2d, inv_no, l);
            qam_axis_llr<M / 2>(yi, qam.lev, qam.d, qam.inv2d, inv_no, l + 1);
            float* o = llr_out + (b0 + r) * n + sym * M;
            if (vec) {
#pragma unroll
                for (int i = 0; i < M; i += 4) *reinterpret_cast<float4*>(o + i) = float4{l[i], l[i + 1], l[i + 2], l[i + 3]};
            } else {
#pragma unroll
                for (int i = 0; i < M; ++i) o[i] = l[i];
            }
            if (y_out != nullptr) {
                float* yo = y_out + ((b0 + r) * ns + sym) * 2;
                yo[0] = yr, yo[1] = yi;
            }
        }
    }
}

// nr_awgn_qam_llr_kernel<M>: nr_awgn_llr_kernel with a 2^M-QAM mapper and demapper (M = 4, 6, 8; M
// divides E).  Phases A, A', B, C1, C1' and C3 are nr_awgn_llr_kernel's; C2 takes the wave's lanes over
// (row, symbol pair): transmitted positions 2M pc .. 2M pc + 2M - 1 (bit e = c[rm_idx[e]]), noise block
// pc of domain 1; with an odd symbol count the last pair's second half is unused.  The stage rows
// are 4 ceil(E/4) floats as there, so rows per pass and the LDS budget are unchanged.
// y_out (nullable): [bs, E / M, 2] fp32 received symbols (re, im).
template <int M>
__global__ __launch_bounds__(256) void nr_awgn_qam_llr_kernel(
    int64_t bs, int64_t row0, uint32_t k0, uint32_t k1, uint32_t it, float no, const uint32_t* __restrict__ frozen_words,
    int n, int k, int kt, const uint32_t* __restrict__ g_rows, int degree, const int32_t* __restrict__ rm_idx, int e_len,
    const int32_t* __restrict__ src_a, const int32_t* __restrict__ src_b, const float* __restrict__ fill, Qam qam,
    float* __restrict__ u_out, uint32_t* __restrict__ ubits_out, float* __restrict__ llr_ch_out,
    float* __restrict__ llr_out, float* __restrict__ y_out) {
    __shared__ uint32_t s_g[kNrGWords];
    __shared__ uint32_t lds[4 * 192];
    __shared__ __attribute__((aligned(16))) float s_stage[4 * kNrStage];
    __shared__ float s_lev[16];
    __builtin_assume(n >= 32);  // whole words: wpc = n / 32, nb = 32
    const WaveRows L = wave_rows(n, row0, bs);
    const int nq = (kt + 31) / 32, nkq = (k + 31) / 32;  // words of the information bits / with the parity
    uint32_t* sw = lds + L.wv * 192;                      // [cpw][nq] stream words
    uint32_t* kw = sw + 64;                               // [cpw][nkq] information bits | parity
    uint32_t* cwd = sw + 128;                             // [cpw][wpc] code words
    float* st = s_stage + L.wv * kNrStage;
    const int lane = L.lane, wpc = L.wpc, cpw = L.cpw, rows = L.rows;
    const int64_t b0 = L.b0;

    stage_levels(s_lev, qam);
    stage_crc_rows(s_g, g_rows, kt);
    draw_stream_words(sw, nq, L, k0, k1, it);
    __syncthreads();
    crc_attach(kw, nkq, sw, nq, s_g, kt, degree, L);
    wave_sync();
    cwd[L.g * wpc + L.w] = encode_word(kw, nkq, frozen_words, L);
    wave_sync();
    if (rows <= 0) return;
    store_u_rows(u_out, sw, nq, kt, L);
    store_packed_rows(ubits_out, sw, nq, kt, L);

    const float inv_no = 1.0f / no, rsig = sqrtf(no) * 0.70710677f * 1.17741002f;  // sqrt(2 ln 2)
    const int ns = e_len / M, npair = (ns + 1) >> 1;  // symbols and symbol pairs per row
    const int epad = ((e_len + 3) >> 2) * 4;
    const int rpp = kNrStage / epad < cpw ? kNrStage / epad : cpw;  // rows per pass (>= 1: E <= kNrStage)
    const bool idx_vec = (reinterpret_cast<uintptr_t>(rm_idx) & 15) == 0;
    for (int r0 = 0; r0 < rows; r0 += rpp) {
        const int rc = rows - r0 < rpp ? rows - r0 : rpp;
        // C2: rate matching, QAM, AWGN, demapper -> stage (+ llr_ch_out, y_out)
        for (int c = lane; c < rc * npair; c += 64) {
            const int rl = c / npair, pc = c - rl * npair, r = r0 + rl, p = pc * 2 * M;
            const uint32_t bits =
                gather_code_bits<2 * M>(cwd + r * wpc, rm_idx, p, e_len, idx_vec && p + 2 * M <= e_len, n);
            const U4 rnd = stream_block(k0, k1, row0 + b0 + r, it, 1, (uint32_t)pc);
            const float4 y = qam_receive<M>(rnd, bits, s_lev, rsig);
#pragma unroll 1
            for (int s = 0; s < 2; ++s) {
                const int sym = 2 * pc + s;
                if (sym >= ns) break;
                const float yr = s ? y.z : y.x, yi = s ? y.w : y.y;
                float l[M];
                qam_axis_llr<M / 2>(yr, s_lev, qam.d, qam.inv2d, inv_no, l);
                qam_axis_llr<M / 2>(yi, s_lev, qam.d, qam.inv2d, inv_no, l + 1);
                float* so = st + rl * epad + sym * M;  // an even offset: 8-byte stores
#pragma unroll
                for (int i = 0; i < M; i += 2) *reinterpret_cast<float2*>(so + i) = float2{l[i], l[i + 1]};
                if (llr_ch_out != nullptr) {
                    float* o = llr_ch_out + (b0 + r) * e_len + sym * M;  // a test output: plain stores
#pragma unroll
                    for (int i = 0; i < M; ++i) o[i] = l[i];
                }
                if (y_out != nullptr) {
                    float* yo = y_out + ((b0 + r) * ns + sym) * 2;
                    yo[0] = yr, yo[1] = yi;
                }
            }
        }
        wave_sync();
        recover_rows(llr_out, st, epad, e_len, r0, rc, src_a, src_b, fill, n, L);
    }
}

constexpr int kRowsPerWave = 8;  // rows a wave of the counting kernels takes

// counts[0..1] += the block's sum of each wave's (be, ke), the wave's totals in its lane 0: the
// block reduces in LDS, one pair of 64-bit atomics per block, none for a zero.  Block-wide.
__device__ __forceinline__ void block_add_pair(unsigned long long be, unsigned long long ke, int lane, int wv,
                                               unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long part[4][2];
    if (lane == 0) {
        part[wv][0] = be;
        part[wv][1] = ke;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long b = part[0][0] + part[1][0] + part[2][0] + part[3][0];
        const unsigned long long e = part[0][1] + part[1][1] + part[2][1] + part[3][1];
        if (b) atomicAdd(&counts[0], b);
        if (e) atomicAdd(&counts[1], e);
    }
}

// Bit and block errors of the first k_cmp columns of [rows, row_len] decided bits (fp32 0/1 or
// bytes) against packed reference bits ([rows, ceil(k_cmp/32)] words, bit m % 32 of word m / 32):
// the layout of count_errors_kernel, the reference 1/32 of its bytes and no slice copy.
template <typename T>
__global__ __launch_bounds__(256) void count_errors_packed_kernel(const T* __restrict__ bits, int64_t rows, int row_len,
                                                                  int k_cmp, const uint32_t* __restrict__ ref,
                                                                  unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + wv) * kRowsPerWave;
    const int nq = (k_cmp + 31) / 32;
    uint32_t bit_err = 0, blk_err = 0;
    for (int r = 0; r < kRowsPerWave; ++r) {
        const int64_t row = r0 + r;
        uint32_t e = 0;
        if (row < rows)
            for (int i = lane; i < k_cmp; i += 64) {
                const uint32_t want = (ref[row * nq + (i >> 5)] >> (i & 31)) & 1u;
                e += (bits[row * row_len + i] != (T)0 ? 1u : 0u) ^ want;
            }
        bit_err += e;
        blk_err += __builtin_amdgcn_ballot_w64(e != 0) != 0 ? 1u : 0u;
    }
    for (int off = 32; off >= 1; off >>= 1) bit_err += __shfl_xor(bit_err, off, 64);
    block_add_pair(bit_err, blk_err, lane, wv, counts);
}

// Bit and block errors of a [rows, k] pair of 0/1 float tensors (exact comparisons, as
// tc.not_equal): a wave takes kRowsPerWave rows (their loads issued together, 16-byte loads when
// rows are 16-byte aligned), the block reduces in LDS, one pair of 64-bit atomics per block.
__global__ __launch_bounds__(256) void count_errors_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           int64_t rows, int k, unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + wv) * kRowsPerWave;
    uint32_t bit_err = 0, blk_err = 0;
    const bool vec = (k & 3) == 0 && ((reinterpret_cast<uintptr_t>(a) & 15) == 0) &&
                     ((reinterpret_cast<uintptr_t>(b) & 15) == 0);
    if (vec) {
        const int kq = k >> 2;
        const float4* a4 = reinterpret_cast<const float4*>(a);
        const float4* b4 = reinterpret_cast<const float4*>(b);
#pragma unroll
        for (int r = 0; r < kRowsPerWave; ++r) {
            const int64_t row = r0 + r;
            uint32_t e = 0;
            if (row < rows) {
                for (int c = lane; c < kq; c += 64) {
                    const float4 x = a4[row * kq + c], y = b4[row * kq + c];
                    e += (x.x != y.x) + (x.y != y.y) + (x.z != y.z) + (x.w != y.w);
                }
            }
            bit_err += e;
            blk_err += __builtin_amdgcn_ballot_w64(e != 0) != 0 ? 1u : 0u;
        }
    } else {
        for (int r = 0; r < kRowsPerWave; ++r) {
            const int64_t row = r0 + r;
            uint32_t e = 0;
            if (row < rows)
                for (int i = lane; i < k; i += 64) e += a[row * k + i] != b[row * k + i] ? 1u : 0u;
            bit_err += e;
            blk_err += __builtin_amdgcn_ballot_w64(e != 0) != 0 ? 1u : 0u;
        }
    }
    for (int off = 32; off >= 1; off >>= 1) bit_err += __shfl_xor(bit_err, off, 64);
    block_add_pair(bit_err, blk_err, lane, wv, counts);
}

// counts[0..1] += sums of the [bit, block] error pairs the decode+count kernel stored per wave:
// kSumBlocks blocks, one pair of atomics each (no contention worth the name on the two counters)
constexpr int kSumBlocks = 64;

__global__ __launch_bounds__(256) void sum_pairs_kernel(const int32_t* __restrict__ part, int64_t pairs,
                                                        unsigned long long* __restrict__ counts) {
    unsigned long long be = 0, ke = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pairs; i += (int64_t)gridDim.x * 256) {
        be += (uint32_t)part[2 * i];
        ke += (uint32_t)part[2 * i + 1];
    }
    for (int off = 32; off >= 1; off >>= 1) {
        be += __shfl_xor(be, off, 64);
        ke += __shfl_xor(ke, off, 64);
    }
    block_add_pair(be, ke, threadIdx.x & 63, threadIdx.x >> 6, counts);
}

}  // namespace

namespace pl {
int launch_sum_pairs(const int32_t* part, int64_t pairs, int64_t* counts, hipStream_t stream) {
    if (pairs <= 0) return PL_OK;
    const int64_t need = (pairs + 255) / 256;
    const unsigned blocks = (unsigned)(need < kSumBlocks ? need : kSumBlocks);
    hipLaunchKernelGGL(sum_pairs_kernel, dim3(blocks), dim3(256), 0, stream, part, pairs,
                       reinterpret_cast<unsigned long long*>(counts));
    return check_hip(hipGetLastError(), "sum_pairs launch");
}
}  // namespace pl

extern "C" {

static int einval(const std::string& msg) {
    pl::set_error(msg);
    return PL_EINVAL;
}

// The argument check of the two QPSK entry points (one message for all of it)
static int qpsk_checks(const char* what, const pl_plan* p, int64_t bs, int64_t row0, float no, uint64_t iteration,
                       const float* llr_out) {
    if (!p || bs < 0 || row0 < 0 || (bs > 0 && !llr_out) || !(no > 0.0f) || (iteration >> 32) != 0)
        return einval(std::string(what) + ": bad arguments (no must be > 0, iteration < 2^32)");
    return PL_OK;
}

// The checks of the two NR entry points on the mother code, in the order they report: the code
// length, k, the caller's complaint about E (pl_nr_awgn_qpsk_llr's place for it; empty: none), the
// tables.
static int nr_checks(const char* what, const pl_plan* p, int32_t k_target, int32_t crc_degree, const std::string& e_error,
                     int64_t bs, const uint32_t* g_rows, const int32_t* rm_idx, const int32_t* src_a) {
    const std::string w(what);
    if (p->n < 32 || p->n > 1024) return einval(w + ": the mother code length must be 32 ... 1024");
    if (k_target < 0 || crc_degree < 1 || crc_degree > 32 || p->k != k_target + crc_degree)
        return einval(w + ": the plan's k must equal k_target + crc_degree (crc_degree 1 ... 32)");
    if (!e_error.empty()) return einval(w + e_error);
    if (bs > 0 && (!rm_idx || !src_a || (k_target > 0 && !g_rows)))
        return einval(w + ": g_rows, rm_idx and src_a must be given");
    return PL_OK;
}

// Blocks (4 waves of 64 / max(1, n / 32) rows) of a producer launch over bs > 0 rows; 0, and the
// error set, where one launch cannot hold them.
static unsigned producer_blocks(const char* what, int n, int64_t bs) {
    const int64_t cpw = 64 / (n >= 32 ? n / 32 : 1);
    const int64_t blocks = ((bs + cpw - 1) / cpw + 3) / 4;
    if (blocks > 0x7fffffffLL) {
        pl::set_error(std::string(what) + ": batch too large for one launch");
        return 0;
    }
    return (unsigned)blocks;
}

static Qam make_qam(int m) {
    Qam q;
    pl::qam_levels(m, q.lev, &q.d);
    q.inv2d = 1.0f / (2.0f * q.d);
    return q;
}

static int awgn_launch(const pl_plan* p, uint64_t seed, uint64_t iteration, int64_t row0, int64_t bs, float no,
                       float* u_out, uint32_t* ubits_out, float* llr_out, void* stream, const char* what) {
    if (int r = qpsk_checks(what, p, bs, row0, no, iteration, llr_out)) return r;
    if (int r = pl::check_device(p, static_cast<hipStream_t>(stream), what)) return r;
    if (bs == 0) return PL_OK;
    const unsigned blocks = producer_blocks(what, p->n, bs);
    if (!blocks) return PL_EINVAL;
    hipLaunchKernelGGL(awgn_llr_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), bs, row0,
                       (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)iteration, no, p->d_frozen_words, p->n, p->k,
                       u_out, llr_out, ubits_out);
    return pl::check_hip(hipGetLastError(), what);
}

int pl_awgn_qpsk_llr(const pl_plan* p, uint64_t seed, uint64_t iteration, int64_t row0, int64_t bs, float no,
                     float* u_out, float* llr_out, void* stream) {
    return awgn_launch(p, seed, iteration, row0, bs, no, u_out, nullptr, llr_out, stream, "pl_awgn_qpsk_llr");
}

int pl_awgn_qpsk_llr_bits(const pl_plan* p, uint64_t seed, uint64_t iteration, int64_t row0, int64_t bs, float no,
                          uint32_t* ubits_out, float* llr_out, void* stream) {
    return awgn_launch(p, seed, iteration, row0, bs, no, nullptr, ubits_out, llr_out, stream,
                       "pl_awgn_qpsk_llr_bits");
}

int pl_nr_awgn_qpsk_llr(const pl_plan* p, int32_t k_target, const uint32_t* g_rows, int32_t crc_degree,
                        const int32_t* rm_idx, int32_t e, const int32_t* src_a, const int32_t* src_b, const float* fill,
                        uint64_t seed, uint64_t iteration, int64_t row0, int64_t bs, float no, uint32_t* ubits_out,
                        float* u_out, float* llr_ch_out, float* llr_out, void* stream) {
    const char* what = "pl_nr_awgn_qpsk_llr";
    if (int r = qpsk_checks(what, p, bs, row0, no, iteration, llr_out)) return r;
    const std::string e_error = e < 2 || (e & 1) || e > kNrStage
        ? ": E must be even (whole QPSK symbols), 2 ... " + std::to_string(kNrStage) : "";
    if (int r = nr_checks(what, p, k_target, crc_degree, e_error, bs, g_rows, rm_idx, src_a)) return r;
    if (int r = pl::check_device(p, static_cast<hipStream_t>(stream), what)) return r;
    if (bs == 0) return PL_OK;
    const unsigned blocks = producer_blocks(what, p->n, bs);
    if (!blocks) return PL_EINVAL;
    hipLaunchKernelGGL(nr_awgn_llr_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), bs, row0,
                       (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)iteration, no, p->d_frozen_words, p->n, p->k,
                       k_target, g_rows, crc_degree, rm_idx, e, src_a, src_b, fill, u_out, ubits_out, llr_ch_out, llr_out);
    return pl::check_hip(hipGetLastError(), what);
}

// The checks pl_awgn_qam_llr and pl_nr_awgn_qam_llr share, each naming its argument; the ones that
// need no plan come first.
static int qam_common_checks(const char* what, int32_t m, int64_t bs, int64_t row0, float no, uint64_t iteration,
                             const float* y_out, const float* llr_out) {
    const std::string w(what);
    if (m != 2 && m != 4 && m != 6 && m != 8)
        return einval(w + ": bits_per_symbol must be 2, 4, 6 or 8, got " + std::to_string(m));
    if (m == 2 && y_out)
        return einval(w + ": y_out must be NULL with bits_per_symbol 2 (the QPSK kernels do not write it)");
    if (bs < 0 || row0 < 0) return einval(w + ": bs and row0 must be >= 0");
    if (!(no > 0.0f)) return einval(w + ": no must be > 0");
    if ((iteration >> 32) != 0) return einval(w + ": iteration must be < 2^32");
    if (bs > 0 && !llr_out) return einval(w + ": llr_out must be given");
    return PL_OK;
}

int pl_awgn_qam_llr(const pl_plan* p, int32_t bits_per_symbol, uint64_t seed, uint64_t iteration, int64_t row0, int64_t bs,
                    float no, float* u_out, uint32_t* ubits_out, float* y_out, float* llr_out, void* stream) {
    const char* what = "pl_awgn_qam_llr";
    const int m = bits_per_symbol;
    if (int r = qam_common_checks(what, m, bs, row0, no, iteration, y_out, llr_out)) return r;
    if (!p) return einval(std::string(what) + ": plan must be given");
    if (m == 2) return awgn_launch(p, seed, iteration, row0, bs, no, u_out, ubits_out, llr_out, stream, what);
    if (p->n % m != 0 || p->n > 2048)
        return einval(std::string(what) + ": bits_per_symbol " + std::to_string(m) + " must divide the code length n = " +
                      std::to_string(p->n) + " (n <= 2048)");
    if (int r = pl::check_device(p, static_cast<hipStream_t>(stream), what)) return r;
    if (bs == 0) return PL_OK;
    const unsigned blocks = producer_blocks(what, p->n, bs);
    if (!blocks) return PL_EINVAL;
    auto* kern = m == 4 ? awgn_qam_llr_kernel<4> : awgn_qam_llr_kernel<8>;  // 6 never divides a power of two
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), bs, row0, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (uint32_t)iteration, no, p->d_frozen_words, p->n, p->k, make_qam(m), u_out,
                       llr_out, ubits_out, y_out);
    return pl::check_hip(hipGetLastError(), what);
}

int pl_nr_awgn_qam_llr(const pl_plan* p, int32_t bits_per_symbol, int32_t k_target, const uint32_t* g_rows,
                       int32_t crc_degree, const int32_t* rm_idx, int32_t e, const int32_t* src_a, const int32_t* src_b,
                       const float* fill, uint64_t seed, uint64_t iteration, int64_t row0, int64_t bs, float no,
                       uint32_t* ubits_out, float* u_out, float* y_out, float* llr_ch_out, float* llr_out, void* stream) {
    const char* what = "pl_nr_awgn_qam_llr";
    const int m = bits_per_symbol;
    if (int r = qam_common_checks(what, m, bs, row0, no, iteration, y_out, llr_out)) return r;
    if (m == 2)
        return pl_nr_awgn_qpsk_llr(p, k_target, g_rows, crc_degree, rm_idx, e, src_a, src_b, fill, seed, iteration, row0, bs,
                                   no, ubits_out, u_out, llr_ch_out, llr_out, stream);
    if (e < m || e % m != 0 || e > kNrStage)
        return einval(std::string(what) + ": E must be a multiple of bits_per_symbol " + std::to_string(m) +
                      " (whole symbols), " + std::to_string(m) + " ... " + std::to_string(kNrStage) + ", got " +
                      std::to_string(e));
    if (!p) return einval(std::string(what) + ": plan must be given");
    if (int r = nr_checks(what, p, k_target, crc_degree, "", bs, g_rows, rm_idx, src_a)) return r;
    if (int r = pl::check_device(p, static_cast<hipStream_t>(stream), what)) return r;
    if (bs == 0) return PL_OK;
    const unsigned blocks = producer_blocks(what, p->n, bs);
    if (!blocks) return PL_EINVAL;
    auto* kern = m == 4 ? nr_awgn_qam_llr_kernel<4> : m == 6 ? nr_awgn_qam_llr_kernel<6> : nr_awgn_qam_llr_kernel<8>;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), bs, row0, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (uint32_t)iteration, no, p->d_frozen_words, p->n, p->k, k_target, g_rows,
                       crc_degree, rm_idx, e, src_a, src_b, fill, make_qam(m), u_out, ubits_out, llr_ch_out, llr_out,
                       y_out);
    return pl::check_hip(hipGetLastError(), what);
}

int pl_count_errors_packed(const void* bits, int32_t kind, int64_t bs, int32_t row_len, int32_t k_cmp,
                           const uint32_t* ref_bits, int64_t* counts, void* stream) {
    if (bs < 0 || row_len < 0 || k_cmp < 0 || k_cmp > row_len || !counts || (kind != PL_OUT_F32 && kind != PL_OUT_U8) ||
        (bs > 0 && k_cmp > 0 && (!bits || !ref_bits))) {
        pl::set_error("pl_count_errors_packed: bad arguments (0 <= k_cmp <= row_len, kind PL_OUT_F32 / PL_OUT_U8)");
        return PL_EINVAL;
    }
    if (bs == 0 || k_cmp == 0) return PL_OK;
    const int64_t blocks = (bs + 4 * kRowsPerWave - 1) / (4 * kRowsPerWave);
    if (blocks > 0x7fffffffLL) {
        pl::set_error("pl_count_errors_packed: too many rows for one launch");
        return PL_EINVAL;
    }
    unsigned long long* c = reinterpret_cast<unsigned long long*>(counts);
    if (kind == PL_OUT_F32)
        hipLaunchKernelGGL(count_errors_packed_kernel<float>, dim3((unsigned)blocks), dim3(256), 0,
                           static_cast<hipStream_t>(stream), static_cast<const float*>(bits), bs, row_len, k_cmp,
                           ref_bits, c);
    else
        hipLaunchKernelGGL(count_errors_packed_kernel<uint8_t>, dim3((unsigned)blocks), dim3(256), 0,
                           static_cast<hipStream_t>(stream), static_cast<const uint8_t*>(bits), bs, row_len, k_cmp,
                           ref_bits, c);
    return pl::check_hip(hipGetLastError(), "pl_count_errors_packed launch");
}

int pl_count_errors(const float* a, const float* b, int64_t rows, int32_t k, int64_t* counts, void* stream) {
    if (rows < 0 || k < 0 || !counts || (rows > 0 && k > 0 && (!a || !b))) {
        pl::set_error("pl_count_errors: bad arguments");
        return PL_EINVAL;
    }
    if (rows == 0 || k == 0) return PL_OK;
    const int64_t blocks = (rows + 4 * kRowsPerWave - 1) / (4 * kRowsPerWave);
    if (blocks > 0x7fffffffLL) {
        pl::set_error("pl_count_errors: too many rows for one launch");
        return PL_EINVAL;
    }
    hipLaunchKernelGGL(count_errors_kernel, dim3((unsigned)blocks), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a, b, rows, k,
                       reinterpret_cast<unsigned long long*>(counts));
    return pl::check_hip(hipGetLastError(), "pl_count_errors launch");
}

}  // extern "C"
