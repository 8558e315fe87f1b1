// pcl.h -- internal (non-ABI): the constraint table of the parity-constrained list decoder (pcl_kernel.hip)
// and its launcher.  pl_pcl_table_create (capi.cpp) validates the host arrays against the plan and uploads them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "plan.h"

struct pl_pcl_table {
    int32_t n = 0, k = 0, num = 0, words = 1;  // words = max(n / 32, 1): the row length of d_mask
    int32_t device = -1;
    std::vector<uint32_t> frozen_words;  // of the plan the table was made for (host copy)
    // Device-resident, immutable after pl_pcl_table_create:
    int32_t* d_ctl = nullptr;    // n entries: -1 = unconstrained leaf, else (c << 2) | (kind << 1) | rhs
    uint32_t* d_mask = nullptr;  // [num][words] packed u-positions; NULL when num == 0
};

namespace pl {
// whether the decoder takes (n, list_size, bs); sets the error string when not
bool pcl_supported(const pl_plan* plan, int list_size, int64_t bs);
// pl_pcl_decode has checked the arguments
int launch_pcl_decode(const pl_plan* plan, const pl_pcl_table* table, int list_size, const float* llr, int64_t bs,
                      void* out, int out_kind, float* out_pm, uint8_t* out_ok, int32_t* out_stop, hipStream_t stream);
}  // namespace pl
