// scf.h -- internal launchers of scf_kernel.hip (the second stage of pl_scf_decode; capi.cpp
// sequences it after pl_sc_decode, crc_flag and compact_failed).  All pointers are device pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plan.h"

namespace pl {
constexpr int kScfMaxFlips = 64;  // candidates a row can have (max_flips)
constexpr int kScfMaxK = 1024;    // information bits (n <= 1024): entries of the CRC remainder table

// flip_pos[b] = -1, attempts[b] = valid[b] ? 1 : 1 + tp, b < bs (either may be NULL)
int launch_scf_init(const uint8_t* valid, int64_t bs, int tp, int32_t* flip_pos, int32_t* attempts, hipStream_t st);
// For r < *n_fail: row rows[r] of out (its SC result, failing the CRC) is decoded again with the
// decision at each of its tp least reliable information positions inverted in turn; the first
// attempt that passes the plan's CRC replaces the row and sets crc_ok = 1, flip_pos, attempts
// (each nullable).  1 <= tp <= min(kScfMaxFlips, k).  The grid does not depend on *n_fail.
int launch_scf_flip(const pl_plan* plan, const float* llr, int64_t bs, void* out, int out_kind, const int32_t* rows,
                    const int64_t* n_fail, int tp, uint8_t* crc_ok, int32_t* flip_pos, int32_t* attempts,
                    hipStream_t st);
}  // namespace pl
