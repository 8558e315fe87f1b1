// osd.h -- internal (non-ABI) layout of an ordered-statistics decoding plan (osd_kernel.hip, capi.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kOsdMaxK = 128, kOsdMaxN = 256, kOsdMaxT = 4;
constexpr int64_t kOsdMaxPatterns = (int64_t)1 << 22;

struct pl_osd_plan {
    int32_t k = 0, n = 0, t = 0;
    int32_t device = -1;         // HIP device the table lives on; -1: made without a GPU (pl_osd_plan_info only)
    int64_t n_patterns = 0;      // sum over i = 1 .. t of C(k, i)
    int32_t count[kOsdMaxT + 1] = {0, 0, 0, 0, 0};  // count[i] = C(k, i) for 1 <= i <= t, else 0
    // Device-resident, immutable: column j of G as 4 words, bit (r & 31) of word r >> 5 = G[r][j]
    // (rows past k zero), n x 4 words
    uint32_t* d_gcol = nullptr;
};

namespace pl {
int launch_osd(const pl_osd_plan* plan, const float* llr, int64_t bs, void* out, int out_kind, double* out_dist,
               int32_t* out_pattern, hipStream_t stream);
}  // namespace pl
