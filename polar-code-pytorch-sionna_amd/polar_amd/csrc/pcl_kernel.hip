// pcl_kernel.hip -- parity-constrained list decoding of polar codes ("dynamic frozen bits") for gfx950 (MI355X).
//
// The contract is in include/polar_mi355x.h (pl_pcl_table_create, pl_pcl_decode); tests/golden/pcl_ref.py restates
// it in numpy and the decoder equals that restatement value for value.  The reference project has no such decoder.
//
// Code: a polar plan (n, frozen set) plus a table of C constraints.  Constraint c ties the u-bit at the
// non-frozen position pos[c] to earlier u-bits: u_pos = rhs ^ parity(mask[c] & u).  A FORCE constraint is a
// dynamic frozen bit (the decoder computes the bit of every path, no fork); a CHECK constraint is a distributed
// parity check (the leaf forks like an information leaf, then every survivor that violates the relation dies, and
// a row with no path left stops).  Distributed CRC bits (38.212 downlink), parity-check polar codes and PAC codes
// are instances; pac_kernel.hip is the special case of one convolution at every position.
//
// Layout: pac_kernel.hip's, without the shift register.  One wave64 per codeword, a single-wave work-group, all
// list state in LDS (struct Smem):
//   A[L][n]      fp32 stage buffers: stage s (0 .. S-1) of path p at A[p][2^s + j], read through the per-path
//                per-stage owner sptr[p][s] (lazy copy: a forked path inherits its parent's owners and writes
//                its own buffer only when it descends through that stage again)
//   ch[n]        the negated channel (stage S)
//   beta, v      [L][n/32] packed partial sums and decided u-bits by absolute position, copied at a fork
//   fc, fpm      the fork table: surviving candidate and its metric by rank
// The metric of path p lives in a register of lane p.  The 2L <= 64 candidates of a fork sit one a lane and are
// ranked by (metric, candidate index) with cross-lane reads.  The parity of a constrained leaf is a popcount over
// the at most n/32 words of mask & v of each path: the 64 / L lanes lane = p + q L (q = 0 .. 64/L - 1) each take
// every (64/L)-th word of path p and the partial words are XORed across them, so no lane walks a whole row.
// The masks and the per-leaf control words are read-only global data: ctl[i] is read at a wave-uniform address,
// a mask row as a small gather (the lanes of group q read word q, q + 64/L, ...: 64/L distinct addresses a step).
// LDS bytes: 4 (L n + n + 2 L max(n/32, 1) + 2 L) + round-up-to-4(L log2 n): 143936 at n = 1024, L = 32.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/polar_mi355x.h"
#include "pcl.h"
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
__device__ __forceinline__ float pos_inf() { return __uint_as_float(0x7f800000u); }

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

// parity(mask & decisions of path p) for p = lane mod L, the same value in all 64 / L lanes of the path: lane
// p + q L takes the words q, q + 64/L, ... <= wi (a mask has no bit past its own leaf, which is in word wi) and
// the partial words are XORed across the lanes of the path.  The caller has synchronised t.v.
template <class T>
__device__ __forceinline__ uint32_t path_parity(const T& t, const uint32_t* __restrict__ mask, int wi, int lane) {
    constexpr int L = T::L, G = 64 >> T::LOGL;
    const int p = lane & (L - 1);
    uint32_t acc = 0u;
    for (int w = lane >> T::LOGL; w <= wi; w += G) acc ^= mask[w] & t.v[p][w];
#pragma unroll
    for (int off = L; off < 64; off <<= 1) acc ^= (uint32_t)__shfl_xor((int)acc, off, 64);
    return __popc(acc) & 1u;
}

// A leaf without a fork.  Lane p < L holds path p's metric pm; u is the bit path p takes (0 at a frozen leaf,
// rhs ^ parity at a FORCE leaf); the metric grows by |l| when u != (l < 0).
template <class T>
__device__ void leaf_fixed(T& t, int i, uint32_t u, float& pm, int lane) {
    constexpr int L = T::L;
    const float l = read_alpha(t, lane & (L - 1), 0, 0);
    const bool neg = l < 0.0f;
    const float pen = ((u != 0u) != neg) ? fabsf(l) : 0.0f;
    if (lane < L) {
        pm = pm + pen;
        if (u) {
            t.beta[lane][i >> 5] |= 1u << (i & 31);
            t.v[lane][i >> 5] |= 1u << (i & 31);
        }
    }
    __syncthreads();
}

// A leaf with a fork (an information or CHECK leaf): the 2L candidates (c < L: path c, u = 0; c >= L: path c - L,
// u = 1) are ranked by (metric, c) and the first L survive: +inf metrics of dead paths fall under the same rule.
template <class T>
__device__ void leaf_fork(T& t, int i, float& pm, int lane) {
    constexpr int L = T::L, W = T::W, S = T::S;
    const int pl = lane & (L - 1);
    const float l = read_alpha(t, pl, 0, 0);  // lanes >= L read a valid path too: their values are not used
    const bool neg = l < 0.0f;
    const float mag = fabsf(l);
    const float pen0 = neg ? mag : 0.0f, pen1 = neg ? 0.0f : mag;
    const int wi = i >> 5;
    const uint32_t bi = 1u << (i & 31);
    // lane c holds candidate c: lanes L .. 2L-1 fetch their path's values
    const float pm_src = shfl_f(pm, pl), pen1_src = shfl_f(pen1, pl);
    const float cand = lane < L ? pm + pen0 : (lane < 2 * L ? pm_src + pen1_src : pos_inf());
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
    const uint32_t bit = (uint32_t)t.fc[pl] >> T::LOGL;
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
        if (bit) {
            t.beta[lane][wi] |= bi;
            t.v[lane][wi] |= bi;
        }
    }
    __syncthreads();
}

template <int LOG_N, int LOG_L>
__global__ __launch_bounds__(64) void pcl_decode_kernel(const float* __restrict__ llr, void* __restrict__ out,
                                                         int out_kind, float* __restrict__ out_pm,
                                                         uint8_t* __restrict__ out_ok, int32_t* __restrict__ out_stop,
                                                         const uint32_t* __restrict__ frozen_words,
                                                         const int32_t* __restrict__ info_pos, int k, float lmax,
                                                         const int32_t* __restrict__ ctl,
                                                         const uint32_t* __restrict__ masks) {
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
    float pm = lane == 0 ? 0.0f : pos_inf();  // path 0 alive, the others at +inf
    __syncthreads();

    // Tree walk in leaf order.  At leaf i: combine the nodes that ended at i-1, compute the input of the node
    // that starts at i (g of its parent), descend with f to the leaf.  ctl[i], the frozen flag and therefore
    // every branch below are the same in all lanes.
    int stop = N;
    for (int i = 0; i < N; ++i) {
        int start = S;
        if (i > 0) {
            const int tz = __builtin_ctz(i);
            for (int s = 1; s <= tz; ++s) combine(t, s, (i - 1) & ~((1 << s) - 1), lane);
            node_fg(t, tz + 1, i & ~((1 << (tz + 1)) - 1), true, lmax, lane);
            start = tz;
        }
        for (int s = start; s >= 1; --s) node_fg(t, s, i, false, lmax, lane);
        const int c = ctl[i];
        if (c < 0) {
            if ((frozen_words[i >> 5] >> (i & 31)) & 1u) leaf_fixed(t, i, 0u, pm, lane);
            else leaf_fork(t, i, pm, lane);
            continue;
        }
        const uint32_t rhs = (uint32_t)c & 1u;
        const uint32_t* mask = masks + (size_t)(c >> 2) * W;
        if (((c >> 1) & 1) == PL_PCL_FORCE) {
            leaf_fixed(t, i, rhs ^ path_parity(t, mask, i >> 5, lane), pm, lane);
            continue;
        }
        leaf_fork(t, i, pm, lane);
        const uint32_t mine = getbit(t.v[lane & (L - 1)], i) ^ path_parity(t, mask, i >> 5, lane);
        if (mine != rhs) pm = pos_inf();
        if (__ballot(lane < L && pm < pos_inf()) == 0ull) {  // wave-uniform: no path is left
            stop = i;
            break;
        }
    }

    // final metrics in ascending (metric, path) order; the first minimum is the output path
    const float mine = lane < L ? pm : pos_inf();
    int rank = 0;
#pragma unroll
    for (int c = 0; c < L; ++c) {
        const float v = shfl_f(mine, c);
        rank += (v < mine) || (v == mine && c < lane);
    }
    if (out_pm != nullptr && lane < L) out_pm[b * L + rank] = pm;
    const unsigned long long first = __ballot(lane < L && rank == 0);
    const int best = __builtin_ctzll(first);
    const bool ok = shfl_f(mine, best) < pos_inf();
    if (lane == 0) {
        if (out_ok != nullptr) out_ok[b] = ok ? 1 : 0;
        if (out_stop != nullptr) out_stop[b] = stop;
    }
    const uint32_t* V = t.v[best];
    for (int m = lane; m < k; m += 64) {
        const int pos = info_pos[m];
        const uint32_t bit = ok ? (V[pos >> 5] >> (pos & 31)) & 1u : 0u;
        if (out_kind == PL_OUT_F32) static_cast<float*>(out)[b * k + m] = bit ? 1.0f : 0.0f;
        else static_cast<uint8_t*>(out)[b * k + m] = (uint8_t)bit;
    }
}

using DecFn = void (*)(const float*, void*, int, float*, uint8_t*, int32_t*, const uint32_t*, const int32_t*, int,
                       float, const int32_t*, const uint32_t*);

template <int LOG_N>
DecFn pick_l(int log_l) {
    switch (log_l) {
        case 0: return pcl_decode_kernel<LOG_N, 0>;
        case 1: return pcl_decode_kernel<LOG_N, 1>;
        case 2: return pcl_decode_kernel<LOG_N, 2>;
        case 3: return pcl_decode_kernel<LOG_N, 3>;
        case 4: return pcl_decode_kernel<LOG_N, 4>;
        default: return pcl_decode_kernel<LOG_N, 5>;
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

// Limits of the decoder, pac_kernel.hip's: a codeword's list state lives in one single-wave work-group's LDS, a
// fork gathers the L n/32 packed words in at most 16 registers a lane and the L log2 n stage owners in at most
// 5, and the grid is one work-group a row.  list_size is a power of two in 1 ... 32 (pl_pcl_decode has checked).
bool pcl_supported(const pl_plan* p, int list_size, int64_t bs) {
    int log_l = 0;
    while ((1 << log_l) < list_size) ++log_l;
    const int W = p->n >= 32 ? p->n / 32 : 1;
    if (p->log_n < 1 || p->log_n > kMaxLogN || log_l > kMaxLogL || lds_bytes(p->log_n, log_l) > kLdsPerGroup ||
        list_size * W > 16 * 64 || list_size * p->log_n > 5 * 64) {
        set_error("pl_pcl_decode: n = " + std::to_string(p->n) + " with list_size " + std::to_string(list_size) +
                  " is not supported (the list state, 4 (L n + n + 2 L n/32 + 2 L) + L log2 n bytes, must fit one "
                  "work-group's LDS share of 160 KiB: n <= 1024 with list_size <= 32)");
        return false;
    }
    if (bs > 0x7fffffffLL) {
        set_error("pl_pcl_decode: bs = " + std::to_string(bs) + " is not supported (one work-group a row: bs < 2^31)");
        return false;
    }
    return true;
}

int launch_pcl_decode(const pl_plan* p, const pl_pcl_table* tb, int list_size, const float* llr, int64_t bs, void* out,
                      int out_kind, float* out_pm, uint8_t* out_ok, int32_t* out_stop, hipStream_t st) {
    if (bs == 0) return PL_OK;
    if (!pcl_supported(p, list_size, bs)) return PL_ENOTSUP;
    int log_l = 0;
    while ((1 << log_l) < list_size) ++log_l;
    const DecFn fn = pick(p->log_n, log_l);
    hipLaunchKernelGGL(fn, dim3((unsigned)bs), dim3(64), 0, st, llr, out, out_kind, out_pm, out_ok, out_stop,
                       p->d_frozen_words, p->d_info_pos, p->k, p->llr_max, tb->d_ctl, tb->d_mask);
    return check_hip(hipGetLastError(), "PCL decode launch");
}

}  // namespace pl
