// pac_kernel.hip -- PAC codes (polarization-adjusted convolutional codes, Arikan 2019) for gfx950 (MI355X):
// the encoder (rate profile, convolutional precoder, polar transform) and the list decoder.
//
// The contract is in include/polar_mi355x.h (pl_pac_encode, pl_pac_decode); tests/golden/pac_ref.py restates it
// in numpy and the decoder equals that restatement value for value.  The reference project has no PAC code.
//
// Code: the data word v (k data bits at the information positions, 0 elsewhere) is precoded to
// u_i = XOR_j c_j v_{i-j} and x = u G_n.  The decoder walks the SC tree of u.  Under the precoder the u of a
// leaf depends on the path's earlier data bits, so every path carries a 32-bit shift register of v, a frozen
// leaf is not a zero (its u is the precoder's output for v = 0), and no node of the tree has a closed form:
// there are no rate-0 / repetition / SPC shortcuts, every leaf is visited.
//
// Decoder layout: one wave64 per codeword, a single-wave work-group, all state in LDS (struct Smem):
//   A[L][n]      fp32 stage buffers: stage s (0 .. S-1) of path p at A[p][2^s + j], read through the per-path
//                per-stage owner sptr[p][s] (lazy copy: a forked path inherits its parent's owners and writes
//                its own buffer only when it descends through that stage again)
//   ch[n]        the negated channel (stage S)
//   beta, v      [L][n/32] packed partial sums of u and decided data bits by absolute position, copied at a fork
//   fc, fpm      the fork table: surviving candidate and its metric by rank
// The metric and the shift register of path p live in registers of lane p.  The 2L <= 64 candidates of an
// information leaf sit one a lane and are ranked by (metric, candidate index) with cross-lane reads.
// LDS bytes: 4 (L n + n + 2 L max(n/32, 1) + 2 L) + round-up-to-4(L log2 n): 143936 at n = 1024, L = 32.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/polar_mi355x.h"
#include "butterfly.h"
#include "plan.h"

#include <string>

namespace {

constexpr int kMaxLogN = 10, kMaxLogL = 5;
constexpr int kLdsPerGroup = 160 * 1024;

template <int LOG_N, int LOG_L>
struct Smem {
    static constexpr int N = 1 << LOG_N, L = 1 << LOG_L, LOGL = LOG_L, S = LOG_N, W = N >= 32 ? N / 32 : 1;
    float A[L][N];
    float ch[N];
    uint32_t beta[L][W];
    uint32_t v[L][W];
    int fc[L];
    float fpm[L];
    uint8_t sptr[L][S];
};

constexpr int lds_bytes(int log_n, int log_l) {
    const int n = 1 << log_n, L = 1 << log_l, W = n >= 32 ? n / 32 : 1;
    return 4 * (L * n + n + 2 * L * W + 2 * L) + ((L * log_n + 3) & ~3);
}
static_assert(sizeof(Smem<10, 5>) == lds_bytes(10, 5) && sizeof(Smem<1, 0>) == lds_bytes(1, 0) &&
              sizeof(Smem<7, 3>) == lds_bytes(7, 3), "the LDS formula of DESIGN.md and the struct disagree");
static_assert(lds_bytes(kMaxLogN, kMaxLogL) <= kLdsPerGroup, "n = 1024, L = 32 must fit one work-group's LDS");

__device__ __forceinline__ float f_ms(float x, float y, float lmax) {
    const float m = fminf(fminf(fabsf(x), fabsf(y)), lmax);
    const bool neg = (int)(__float_as_uint(x) ^ __float_as_uint(y)) < 0;
    return neg ? -m : m;
}
__device__ __forceinline__ float g_op(float x, float y, uint32_t bit) { return (bit ? -x : x) + y; }
__device__ __forceinline__ uint32_t getbit(const uint32_t* w, int pos) { return (w[pos >> 5] >> (pos & 31)) & 1u; }
__device__ __forceinline__ float shfl_f(float v, int src) { return __shfl(v, src, 64); }

// LLR j of the stage-s node of path p.
template <class T>
__device__ __forceinline__ float read_alpha(const T& t, int p, int s, int j) {
    if (s == T::S) return t.ch[j];
    return t.A[t.sptr[p][s]][(1 << s) + j];
}

// f (is_g = false) or g at the stage-s node at position pos, for every path: writes stage s-1 into the path's
// own buffer and takes ownership.  Reads go to stage s, writes to stage s-1: no buffer is read and written.
template <class T>
__device__ void node_fg(T& t, int s, int pos, bool is_g, float lmax, int lane) {
    const int ls = s - 1, h = 1 << ls;
    for (int idx = lane; idx < T::L * h; idx += 64) {
        const int p = idx >> ls, j = idx & (h - 1);
        const float x = read_alpha(t, p, s, j), y = read_alpha(t, p, s, j + h);
        t.A[p][h + j] = is_g ? g_op(x, y, getbit(t.beta[p], pos + j)) : f_ms(x, y, lmax);
    }
    __syncthreads();
    if (lane < T::L) t.sptr[lane][ls] = (uint8_t)lane;
    __syncthreads();
}

// beta[pos, pos+h) ^= beta[pos+h, pos+2h) for every path.
template <class T>
__device__ void combine(T& t, int s, int pos, int lane) {
    const int h = 1 << (s - 1);
    if (h >= 32) {
        const int hw = h >> 5, w0 = pos >> 5;
        for (int idx = lane; idx < T::L * hw; idx += 64) {
            const int p = idx / hw, w = idx - p * hw;
            t.beta[p][w0 + w] ^= t.beta[p][w0 + hw + w];
        }
    } else if (lane < T::L) {
        uint32_t* b = &t.beta[lane][pos >> 5];
        const uint32_t m = ((1u << h) - 1u) << (pos & 31);
        *b ^= (*b >> h) & m;
    }
    __syncthreads();
}

// Leaf i.  Lane p < L holds path p's metric pm and register reg (v_{i-1} at bit 0).  u0 is the precoder's output
// for v_i = 0; choosing v gives u = u0 ^ v, and the metric grows by |l| when u != (l < 0).  A frozen leaf takes
// v = 0.  An information leaf ranks the 2L candidates (c < L: path c, v = 0; c >= L: path c - L, v = 1) by
// (metric, c) and keeps the first L: +inf metrics of dead paths fall under the same rule.
template <class T>
__device__ void leaf(T& t, int i, bool info, uint32_t conv_mask, float& pm, uint32_t& reg, int lane) {
    constexpr int L = T::L, W = T::W, S = T::S;
    const int pl = lane & (L - 1);
    const float l = read_alpha(t, pl, 0, 0);  // lanes >= L read a valid path too: their values are not used
    const uint32_t u0 = __popc((reg << 1) & conv_mask) & 1u;
    const bool neg = l < 0.0f;
    const float mag = fabsf(l);
    const float pen0 = ((u0 != 0u) != neg) ? mag : 0.0f;
    const int wi = i >> 5;
    const uint32_t bi = 1u << (i & 31);
    if (!info) {
        if (lane < L) {
            pm = pm + pen0;
            reg <<= 1;
            if (u0) t.beta[lane][wi] |= bi;
        }
        __syncthreads();
        return;
    }
    const float pen1 = ((u0 == 0u) != neg) ? mag : 0.0f;
    // lane c holds candidate c: lanes L .. 2L-1 fetch their path's values
    const float pm_src = shfl_f(pm, pl), pen1_src = shfl_f(pen1, pl);
    const float inf = __uint_as_float(0x7f800000u);
    const float cand = lane < L ? pm + pen0 : (lane < 2 * L ? pm_src + pen1_src : inf);
    int rank = 0;
#pragma unroll
    for (int c = 0; c < 2 * L; ++c) {
        const float v = shfl_f(cand, c);
        rank += (v < cand) || (v == cand && c < lane);
    }
    if (lane < 2 * L && rank < L) {
        t.fc[rank] = lane;
        t.fpm[rank] = cand;
    }
    __syncthreads();
    // survivors: the parent's partial sums, decisions and stage owners are gathered, then scattered (all reads
    // before any write: several survivors may share one parent).  Words past the one holding leaf i are zero.
    constexpr int R = (L * W + 63) / 64;   // L W <= 32 * 32 words: at most 16 a lane
    constexpr int RS = (L * S + 63) / 64;  // L S <= 32 * 10 owners: at most 5 a lane
    static_assert(R <= 16 && RS <= 5, "fork gather loops sized for L <= 32, n <= 1024");
    uint32_t vb[R], vv[R];
    uint8_t sp[RS];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int idx = r * 64 + lane, np = idx / W, w = idx - np * W;
        if (idx < L * W && w <= wi) {
            const int par = t.fc[np] & (L - 1);
            vb[r] = t.beta[par][w];
            vv[r] = t.v[par][w];
        }
    }
#pragma unroll
    for (int r = 0; r < RS; ++r) {
        const int idx = r * 64 + lane;
        if (idx < L * S) sp[r] = t.sptr[t.fc[idx / S] & (L - 1)][idx % S];
    }
    const int mine = t.fc[pl];
    const int par = mine & (L - 1);
    const uint32_t bit = (uint32_t)mine >> T::LOGL;
    const uint32_t reg_par = (uint32_t)__shfl((int)reg, par, 64);
    const uint32_t u0_par = (uint32_t)__shfl((int)u0, par, 64);
    const float pm_new = t.fpm[pl];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int idx = r * 64 + lane, np = idx / W, w = idx - np * W;
        if (idx < L * W && w <= wi) {
            t.beta[np][w] = vb[r];
            t.v[np][w] = vv[r];
        }
    }
#pragma unroll
    for (int r = 0; r < RS; ++r) {
        const int idx = r * 64 + lane;
        if (idx < L * S) t.sptr[idx / S][idx % S] = sp[r];
    }
    __syncthreads();
    if (lane < L) {
        pm = pm_new;
        reg = (reg_par << 1) | bit;
        if (u0_par ^ bit) t.beta[lane][wi] |= bi;
        if (bit) t.v[lane][wi] |= bi;
    }
    __syncthreads();
}

template <int LOG_N, int LOG_L>
__global__ __launch_bounds__(64) void pac_decode_kernel(const float* __restrict__ llr, void* __restrict__ out,
                                                         int out_kind, float* __restrict__ out_pm,
                                                         const uint32_t* __restrict__ frozen_words,
                                                         const int32_t* __restrict__ info_pos, int k, float lmax,
                                                         uint32_t conv_mask) {
    using T = Smem<LOG_N, LOG_L>;
    constexpr int N = T::N, L = T::L, S = T::S, W = T::W;
    __shared__ T t;
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;

    const float* x = llr + b * N;
    for (int i = lane; i < N; i += 64) t.ch[i] = -x[i];
    for (int i = lane; i < L * W; i += 64) {
        t.beta[i / W][i % W] = 0u;
        t.v[i / W][i % W] = 0u;
    }
    for (int i = lane; i < L * S; i += 64) t.sptr[i / S][i % S] = (uint8_t)(i / S);
    float pm = lane == 0 ? 0.0f : __uint_as_float(0x7f800000u);  // path 0 alive, the others at +inf
    uint32_t reg = 0u;
    __syncthreads();

    // Tree walk in leaf order.  At leaf i: combine the nodes that ended at i-1, compute the input of the node
    // that starts at i (g of its parent), descend with f to the leaf.
    for (int i = 0; i < N; ++i) {
        int start = S;
        if (i > 0) {
            const int tz = __builtin_ctz(i);
            for (int s = 1; s <= tz; ++s) combine(t, s, (i - 1) & ~((1 << s) - 1), lane);
            node_fg(t, tz + 1, i & ~((1 << (tz + 1)) - 1), true, lmax, lane);
            start = tz;
        }
        for (int s = start; s >= 1; --s) node_fg(t, s, i, false, lmax, lane);
        const bool info = ((frozen_words[i >> 5] >> (i & 31)) & 1u) == 0u;
        leaf(t, i, info, conv_mask, pm, reg, lane);
    }

    // final metrics in ascending (metric, path) order; the first minimum is the output path
    const float mine = lane < L ? pm : __uint_as_float(0x7f800000u);
    int rank = 0;
#pragma unroll
    for (int c = 0; c < L; ++c) {
        const float v = shfl_f(mine, c);
        rank += (v < mine) || (v == mine && c < lane);
    }
    if (out_pm != nullptr && lane < L) out_pm[b * L + rank] = pm;
    const unsigned long long first = __ballot(lane < L && rank == 0);
    const int best = __builtin_ctzll(first);
    const uint32_t* V = t.v[best];
    for (int m = lane; m < k; m += 64) {
        const int pos = info_pos[m];
        const uint32_t bit = (V[pos >> 5] >> (pos & 31)) & 1u;
        if (out_kind == PL_OUT_F32) static_cast<float*>(out)[b * k + m] = bit ? 1.0f : 0.0f;
        else static_cast<uint8_t*>(out)[b * k + m] = (uint8_t)bit;
    }
}

// Encoder: each lane owns 32 consecutive positions of a codeword as one packed word (encode_kernel.hip's
// layout).  Rate profile: the data bits are scattered to the information positions.  Precoder, one bit-parallel
// pass: u = XOR_j c_j (v shifted up by j positions); j <= 31, so the bits shifted in come from the previous
// word of the same codeword alone.  Then the shared XOR butterfly.
__global__ __launch_bounds__(256) void pac_encode_kernel(const float* __restrict__ data, int64_t bs,
                                                          float* __restrict__ cw,
                                                          const int32_t* __restrict__ info_rank, int n, int k,
                                                          uint32_t conv_mask) {
    const int wpc = n >= 32 ? n / 32 : 1;  // lanes (words) per codeword
    const int cpw = 64 / wpc;              // codewords per wave
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t row = wave * cpw + lane / wpc;
    const int w = lane % wpc;
    const bool valid = row < bs;
    const int nb = n >= 32 ? 32 : n;  // positions in this word
    uint32_t v = 0u;
    if (valid) {
        const float* dr = data + row * k;
        for (int b = 0; b < nb; ++b) {
            const int r = info_rank[w * 32 + b];
            if (r >= 0 && dr[r] != 0.0f) v |= 1u << b;
        }
    }
    uint32_t prev = (uint32_t)__shfl_up((int)v, 1, 64);
    if (w == 0) prev = 0u;
    uint32_t u = v;
    for (int j = 1; j < 32; ++j)
        if ((conv_mask >> j) & 1u) u ^= (v << j) | (prev >> (32 - j));
    if (nb < 32) u &= (1u << nb) - 1u;
    u = pl::polar_butterfly(u, nb, wpc, w);
    if (valid) {
        float* o = cw + row * n + w * 32;
        for (int b = 0; b < nb; ++b) o[b] = ((u >> b) & 1u) ? 1.0f : 0.0f;
    }
}

using DecFn = void (*)(const float*, void*, int, float*, const uint32_t*, const int32_t*, int, float, uint32_t);

template <int LOG_N>
DecFn pick_l(int log_l) {
    switch (log_l) {
        case 0: return pac_decode_kernel<LOG_N, 0>;
        case 1: return pac_decode_kernel<LOG_N, 1>;
        case 2: return pac_decode_kernel<LOG_N, 2>;
        case 3: return pac_decode_kernel<LOG_N, 3>;
        case 4: return pac_decode_kernel<LOG_N, 4>;
        default: return pac_decode_kernel<LOG_N, 5>;
    }
}

DecFn pick(int log_n, int log_l) {
    switch (log_n) {
        case 1: return pick_l<1>(log_l);
        case 2: return pick_l<2>(log_l);
        case 3: return pick_l<3>(log_l);
        case 4: return pick_l<4>(log_l);
        case 5: return pick_l<5>(log_l);
        case 6: return pick_l<6>(log_l);
        case 7: return pick_l<7>(log_l);
        case 8: return pick_l<8>(log_l);
        case 9: return pick_l<9>(log_l);
        default: return pick_l<10>(log_l);
    }
}

}  // namespace

namespace pl {

// Limits of the decoder: a codeword's list state lives in one single-wave work-group's LDS, a fork gathers the
// L n/32 packed words in at most 16 registers a lane and the L log2 n stage owners in at most 5, and the grid is
// one work-group a row.  list_size is a power of two in 1 ... 32 (pl_pac_decode has checked).
bool pac_supported(const pl_plan* p, int list_size, int64_t bs) {
    int log_l = 0;
    while ((1 << log_l) < list_size) ++log_l;
    const int W = p->n >= 32 ? p->n / 32 : 1;
    if (p->log_n < 1 || p->log_n > kMaxLogN || log_l > kMaxLogL || lds_bytes(p->log_n, log_l) > kLdsPerGroup ||
        list_size * W > 16 * 64 || list_size * p->log_n > 5 * 64) {
        set_error("pl_pac_decode: n = " + std::to_string(p->n) + " with list_size " + std::to_string(list_size) +
                  " is not supported (the list state, 4 (L n + n + 2 L n/32 + 2 L) + L log2 n bytes, must fit one "
                  "work-group's LDS share of 160 KiB: n <= 1024 with list_size <= 32)");
        return false;
    }
    if (bs > 0x7fffffffLL) {
        set_error("pl_pac_decode: bs = " + std::to_string(bs) + " is not supported (one work-group a row: bs < 2^31)");
        return false;
    }
    return true;
}

int launch_pac_decode(const pl_plan* p, uint32_t conv_mask, int list_size, const float* llr, int64_t bs, void* out,
                      int out_kind, float* out_pm, hipStream_t st) {
    if (bs == 0) return PL_OK;
    if (!pac_supported(p, list_size, bs)) return PL_ENOTSUP;
    int log_l = 0;
    while ((1 << log_l) < list_size) ++log_l;
    const DecFn fn = pick(p->log_n, log_l);
    hipLaunchKernelGGL(fn, dim3((unsigned)bs), dim3(64), 0, st, llr, out, out_kind, out_pm, p->d_frozen_words,
                       p->d_info_pos, p->k, p->llr_max, conv_mask);
    return check_hip(hipGetLastError(), "PAC decode launch");
}

int launch_pac_encode(const pl_plan* p, uint32_t conv_mask, const float* data, int64_t bs, float* cw, hipStream_t st) {
    if (bs == 0) return PL_OK;
    const int wpc = p->n >= 32 ? p->n / 32 : 1;
    const int64_t cpw = 64 / wpc;
    const int64_t waves = (bs + cpw - 1) / cpw;
    const int64_t blocks = (waves + 3) / 4;
    if (blocks > 0x7fffffffLL) {
        set_error("pl_pac_encode: bs = " + std::to_string(bs) + " is not supported (the grid has fewer than 2^31 work-groups)");
        return PL_ENOTSUP;
    }
    hipLaunchKernelGGL(pac_encode_kernel, dim3((unsigned)blocks), dim3(256), 0, st, data, bs, cw, p->d_info_rank, p->n,
                       p->k, conv_mask);
    return check_hip(hipGetLastError(), "PAC encode launch");
}

}  // namespace pl
