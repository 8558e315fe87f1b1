// osd_kernel.hip -- ordered-statistics decoding (OSD) of short binary linear codes on gfx950
// (pl_osd_decode, include/polar_mi355x.h; OSDecoder.forward, my_sn/fec/osd/dec.py:148-192).
//
// One wave (a 64-thread block) decodes one codeword; everything of the codeword stays in registers
// and LDS.  The phases, in the reference's order:
//   rank      the n clipped |llr| get their descending stable rank by counting (n^2 compares, lanes
//             split j): rank_j = #{i : |l_i| > |l_j| or (|l_i| == |l_j| and i < j)}, compared as the bit
//             patterns with the sign cleared, so +0 and -0 tie and the lower index comes first.
//   basis     row r of G with its columns in that order lives in lane r % 64, slot r / 64, as NW
//             words (bits past n zero).  NW and the slots per lane are template parameters, so every
//             row word has a compile-time register index.  All NW in {1, 2, 4, 8} x slots in {1, 2} are
//             instantiated; <1, 2> and <2, 2> are never launched (two slots mean k > 64, hence n >= 65
//             and NW >= 4).
//   eliminate for row c = 0 .. k-1 in turn (dec.py:115-127): the row is broadcast with lane reads, its
//             first set bit p is the pivot (wave-uniform), every other row with bit p set XORs it in.
//   c0        hard decision of the k pivot positions (llr > 0), c0 = XOR of the rows whose bit is 1.
//   search    every subset of 1 .. t basis rows, the orders in turn and each in itertools.combinations
//             order, is one candidate c0 ^ e.  Its metric differs from c0's by
//             Delta(e) / n, Delta(e) = -sum_{j in supp e} a_j, a_j = llr_j (1 - 2 c0_j), because
//             softplus(x) - softplus(-x) = x; no exp or log in the search.  Delta is summed in fp64 from
//             nibble tables of the fp32 a_j in LDS (n / 4 tables of 16 entries, n / 4 adds a candidate).
//             The lanes take contiguous ranges of the pattern index; each unranks its first pattern
//             once and steps to the next combination from there.  The winner is the lexicographic
//             minimum of (Delta, pattern index) with Delta < 0 required: the reference's first argmin
//             within an order and strict < between orders (dec.py:101, :185-187).
//   output    the chosen word scattered back to channel order; optionally its metric (the softplus form,
//             fp64) and the pattern index.
// The reference's last column permutation (pivots first, dec.py:128-147) only renames positions: the
// word, the pattern and -- up to the order of an fp64 sum -- the metric do not depend on it, so the
// kernel stays in the sorted order throughout.
//
// Bounds: ranks are counts over i != j, so < n; a pivot is a bit index of an NW-word row whose bits
// past n are zero, so < n for a rank-k G (pl_osd_plan_create refuses any other) and clamped anyway;
// combination members are < k by the unranking's guard.  No loop's trip count depends on an LLR.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/polar_mi355x.h"
#include "osd.h"
#include "plan.h"

namespace {

struct OsdArgs {
    const float* llr;
    void* out;
    double* dist;
    int32_t* pattern;
    const uint32_t* gcol;
    int32_t n, k, out_kind, np;
    int32_t c1, c2, c3;  // C(k, i) for i < t (0 otherwise): where the orders start in the pattern index
};

// C(m, s) for 0 <= s <= 3 (m <= 127: the products fit an int)
__device__ __forceinline__ int binom_small(int m, int s) {
    if (m < s) return 0;
    if (s == 0) return 1;
    if (s == 1) return m;
    if (s == 2) return m * (m - 1) / 2;
    return m * (m - 1) * (m - 2) / 6;
}

__device__ __forceinline__ uint32_t lane_read(uint32_t v, int lane) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}

template <int NW, int RPL>
__global__ __launch_bounds__(64) void osd_kernel(OsdArgs a, int64_t row0) {
    constexpr int NP = NW * 32;  // positions, padded to whole words
    constexpr int KP = RPL * 64;  // rows, padded to whole slots
    __shared__ uint32_t s_abs[NP];      // |clipped llr| bit patterns, channel order
    __shared__ float s_llr[NP];         // clipped llr, channel order
    __shared__ uint16_t s_order[NP];    // sorted position -> channel index
    __shared__ float s_a[NP];           // sorted llr, then a_q = llr_q (1 - 2 c0_q); 0 past n
    __shared__ uint32_t s_col[NP * 4];  // column of G at sorted position q (k bits in 4 words)
    __shared__ uint32_t s_rows[KP * NW];  // the most reliable basis, row r at r * NW
    __shared__ uint16_t s_piv[KP];
    __shared__ double s_tab[NW * 8 * 16];  // nibble nb, value v: -sum of a[4 nb + b] over the bits b of v

    const int lane = threadIdx.x;
    const int n = a.n, k = a.k;
    const int64_t b = row0 + (int64_t)blockIdx.x;
    const float* x = a.llr + b * n;

    for (int j = lane; j < NP; j += 64) {
        float v = 0.0f;
        if (j < n) v = fminf(fmaxf(x[j], -100.0f), 100.0f);
        s_llr[j] = v;
        s_abs[j] = __float_as_uint(v) & 0x7fffffffu;
        s_a[j] = 0.0f;
    }
    __syncthreads();

    // ---- rank ----
    for (int j = lane; j < n; j += 64) {
        const uint32_t aj = s_abs[j];
        int r = 0;
        for (int i = 0; i < n; ++i) {
            const uint32_t ai = s_abs[i];
            r += (ai > aj || (ai == aj && i < j)) ? 1 : 0;
        }
        s_order[r] = (uint16_t)j;
        s_a[r] = s_llr[j];
    }
    __syncthreads();
    for (int q = lane; q < n; q += 64) {
        const uint4 c = reinterpret_cast<const uint4*>(a.gcol)[s_order[q]];
        s_col[q * 4 + 0] = c.x;
        s_col[q * 4 + 1] = c.y;
        s_col[q * 4 + 2] = c.z;
        s_col[q * 4 + 3] = c.w;
    }
    __syncthreads();

    // ---- basis: this lane's rows, columns in sorted order ----
    uint32_t row[RPL][NW];
#pragma unroll
    for (int s = 0; s < RPL; ++s) {
        const int r = s * 64 + lane;
        const int wsel = r >> 5, sh = r & 31;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            uint32_t acc = 0u;
            for (int bb = 0; bb < 32; ++bb) {
                const int q = w * 32 + bb;
                if (q < n) acc |= ((s_col[q * 4 + wsel] >> sh) & 1u) << bb;
            }
            row[s][w] = acc;
        }
    }

    // ---- elimination, in the reference's row order ----
#pragma unroll
    for (int sc = 0; sc < RPL; ++sc) {
        for (int l = 0; l < 64; ++l) {
            const int c = sc * 64 + l;
            if (c >= k) break;
            uint32_t pr[NW];
#pragma unroll
            for (int w = 0; w < NW; ++w) pr[w] = lane_read(row[sc][w], l);
            int p = 0;
#pragma unroll
            for (int w = NW - 1; w >= 0; --w)
                if (pr[w] != 0u) p = w * 32 + __builtin_ctz(pr[w]);
            p = min(p, n - 1);
            const int pw = p >> 5;
            const uint32_t pb = 1u << (p & 31);
#pragma unroll
            for (int s = 0; s < RPL; ++s) {
                uint32_t word = 0u;
#pragma unroll
                for (int w = 0; w < NW; ++w) word = (pw == w) ? row[s][w] : word;
                const bool hit = (word & pb) != 0u && !(s == sc && lane == l);
#pragma unroll
                for (int w = 0; w < NW; ++w) row[s][w] ^= hit ? pr[w] : 0u;
            }
            if (lane == 0) s_piv[c] = (uint16_t)p;
        }
    }
#pragma unroll
    for (int s = 0; s < RPL; ++s)
#pragma unroll
        for (int w = 0; w < NW; ++w) s_rows[(s * 64 + lane) * NW + w] = row[s][w];
    __syncthreads();

    // ---- c0: re-encode the hard decision of the pivot positions ----
    uint32_t c0[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) c0[w] = 0u;
#pragma unroll
    for (int s = 0; s < RPL; ++s) {
        const int r = s * 64 + lane;
        const bool one = r < k && s_a[s_piv[r < k ? r : 0]] > 0.0f;
#pragma unroll
        for (int w = 0; w < NW; ++w) c0[w] ^= one ? row[s][w] : 0u;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int w = 0; w < NW; ++w) c0[w] ^= (uint32_t)__shfl_xor((int)c0[w], off);
    __syncthreads();
#pragma unroll
    for (int w = 0; w < NW; ++w)
        if (lane < 32) {
            const int q = w * 32 + lane;
            s_a[q] = ((c0[w] >> lane) & 1u) ? -s_a[q] : s_a[q];
        }
    __syncthreads();
    for (int idx = lane; idx < NW * 8 * 16; idx += 64) {
        const int nb = idx >> 4, v = idx & 15;
        double s = 0.0;
#pragma unroll
        for (int bb = 0; bb < 4; ++bb)
            if ((v >> bb) & 1) s -= (double)s_a[nb * 4 + bb];
        s_tab[idx] = s;
    }
    __syncthreads();

    // ---- search ----
    double best = 0.0;
    int bestg = -1, bord = 0;
    int bc[4] = {0, 0, 0, 0};
    {
        const int per = (a.np + 63) / 64;
        const int g0 = min(lane * per, a.np), g1 = min(g0 + per, a.np);
        int ord = 1, r = g0;
        if (ord == 1 && a.c1 > 0 && r >= a.c1) { r -= a.c1; ord = 2; }
        if (ord == 2 && a.c2 > 0 && r >= a.c2) { r -= a.c2; ord = 3; }
        if (ord == 3 && a.c3 > 0 && r >= a.c3) { r -= a.c3; ord = 4; }
        int cmb[4];
        int xx = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < ord) {
                const int rem = ord - 1 - j;
                while (xx < k - 1 && binom_small(k - 1 - xx, rem) <= r) {
                    r -= binom_small(k - 1 - xx, rem);
                    ++xx;
                }
                cmb[j] = min(xx, k - 1);
                ++xx;
            } else {
                cmb[j] = 0;
            }
        }
        for (int g = g0; g < g1; ++g) {
            uint32_t e[NW];
#pragma unroll
            for (int w = 0; w < NW; ++w) e[w] = s_rows[cmb[0] * NW + w];
#pragma unroll
            for (int j = 1; j < 4; ++j)
                if (j < ord) {
#pragma unroll
                    for (int w = 0; w < NW; ++w) e[w] ^= s_rows[cmb[j] * NW + w];
                }
            double d = 0.0;
#pragma unroll
            for (int w = 0; w < NW; ++w)
#pragma unroll
                for (int nb = 0; nb < 8; ++nb) d += s_tab[((w * 8 + nb) << 4) + ((e[w] >> (4 * nb)) & 15u)];
            if (d < best) {
                best = d;
                bestg = g;
                bord = ord;
#pragma unroll
                for (int j = 0; j < 4; ++j) bc[j] = cmb[j];
            }
            // the next combination of this order, or the first of the next order
            bool adv = false;
#pragma unroll
            for (int j = 3; j >= 0; --j) {
                if (!adv && j < ord && cmb[j] < k - ord + j) {
                    ++cmb[j];
#pragma unroll
                    for (int m = j + 1; m < 4; ++m)
                        if (m < ord) cmb[m] = cmb[m - 1] + 1;
                    adv = true;
                }
            }
            if (!adv) {
                ++ord;
#pragma unroll
                for (int m = 0; m < 4; ++m) cmb[m] = m < k ? m : 0;
            }
        }
    }
    const int myg = bestg;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double od = __shfl_xor(best, off);
        const int og = __shfl_xor(bestg, off);
        if (od < best || (od == best && og < bestg)) {
            best = od;
            bestg = og;
        }
    }
    uint32_t cw[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) cw[w] = c0[w];
    uint32_t ee[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) ee[w] = 0u;
    if (bestg >= 0) {  // wave-uniform after the reduction
        const unsigned long long m = __ballot(myg == bestg);
        const int wl = m ? __builtin_ctzll(m) : 0;
        const int word_ord = __shfl(bord, wl);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int cj = __shfl(bc[j], wl);
            cj = min(max(cj, 0), k - 1);
            if (j < word_ord) {
#pragma unroll
                for (int w = 0; w < NW; ++w) ee[w] ^= s_rows[cj * NW + w];
            }
        }
#pragma unroll
        for (int w = 0; w < NW; ++w) cw[w] ^= ee[w];
    }

    // ---- output ----
    double dsum = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const int q = w * 32 + (lane & 31);
        if (lane < 32 && q < n) {
            const uint32_t bit = (cw[w] >> (lane & 31)) & 1u;
            const int64_t o = b * n + s_order[q];
            if (a.out_kind == PL_OUT_U8)
                static_cast<uint8_t*>(a.out)[o] = (uint8_t)bit;
            else
                static_cast<float*>(a.out)[o] = bit ? 1.0f : 0.0f;
            if (a.dist != nullptr) {
                const float av = s_a[q];
                const double z = (double)(((ee[w] >> (lane & 31)) & 1u) ? -av : av);  // llr (1 - 2 c)
                dsum += fmax(z, 0.0) + log1p(exp(-fabs(z)));
            }
        }
    }
    if (a.dist != nullptr) {  // wave-uniform
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) dsum += __shfl_xor(dsum, off);
        if (lane == 0) a.dist[b] = dsum / (double)n;
    }
    if (a.pattern != nullptr && lane == 0) a.pattern[b] = bestg;
}

template <int NW>
void launch_rpl(const OsdArgs& a, int rpl, int64_t row0, unsigned grid, hipStream_t st) {
    if (rpl == 1)
        hipLaunchKernelGGL((osd_kernel<NW, 1>), dim3(grid), dim3(64), 0, st, a, row0);
    else
        hipLaunchKernelGGL((osd_kernel<NW, 2>), dim3(grid), dim3(64), 0, st, a, row0);
}

}  // namespace

namespace pl {

int launch_osd(const pl_osd_plan* p, const float* llr, int64_t bs, void* out, int out_kind, double* out_dist,
               int32_t* out_pattern, hipStream_t st) {
    OsdArgs a;
    a.llr = llr;
    a.out = out;
    a.dist = out_dist;
    a.pattern = out_pattern;
    a.gcol = p->d_gcol;
    a.n = p->n;
    a.k = p->k;
    a.out_kind = out_kind;
    a.np = (int32_t)p->n_patterns;
    a.c1 = p->t > 1 ? p->count[1] : 0;
    a.c2 = p->t > 2 ? p->count[2] : 0;
    a.c3 = p->t > 3 ? p->count[3] : 0;
    const int nw = (p->n + 31) / 32;
    const int rpl = p->k > 64 ? 2 : 1;
    // one block per codeword; large batches go out in chunks of 2^20 rows (as the list decoder's)
    const int64_t chunk = (int64_t)1 << 20;
    for (int64_t row0 = 0; row0 < bs; row0 += chunk) {
        const unsigned grid = (unsigned)(bs - row0 < chunk ? bs - row0 : chunk);
        if (nw <= 1)
            launch_rpl<1>(a, rpl, row0, grid, st);
        else if (nw <= 2)
            launch_rpl<2>(a, rpl, row0, grid, st);
        else if (nw <= 4)
            launch_rpl<4>(a, rpl, row0, grid, st);
        else
            launch_rpl<8>(a, rpl, row0, grid, st);
        if (int r = check_hip(hipGetLastError(), "pl_osd_decode launch")) return r;
    }
    return PL_OK;
}

}  // namespace pl
