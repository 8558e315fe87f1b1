// ae.h -- internal launcher of ae_kernel.hip (pl_ae_decode).  All pointers are device pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plan.h"

namespace pl {
constexpr int kAeMaxPerms = 64;  // candidates (permuted SC decodes) a row can have

// Automorphism-ensemble SC decoding: every row of llr [bs, n] is decoded num_perms times by leaf-by-leaf SC,
// candidate t on the row read through perms[t][.] ([num_perms][n] uint16, entries masked with n - 1); the
// candidate codeword closest to the row (smallest fp32 metric, lowest t among equals) gives out [bs, k],
// best_idx and best_metric (both nullable).  1 <= num_perms <= kAeMaxPerms, 2 <= n <= 1024.
int launch_ae(const pl_plan* plan, const float* llr, int64_t bs, const uint16_t* perms, int num_perms, void* out,
              int out_kind, int32_t* best_idx, float* best_metric, hipStream_t st);
}  // namespace pl
