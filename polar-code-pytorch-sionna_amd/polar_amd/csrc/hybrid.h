// hybrid.h -- internal launchers of hybrid_kernel.hip (the device-side glue of pl_hybrid_decode
// and pl_crc_status; capi.cpp sequences them).  All pointers are device pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pl {
// int32 partial counts compact_failed keeps between its two launches
constexpr int kCompactMaxBlocks = 1024;

// valid[idx ? idx[b] : b] = 1 iff the k bits of row b (PL_OUT_F32 / PL_OUT_U8) leave the MSB-first
// shift register of x^deg + g at zero, else 0.  1 <= deg <= 32, deg <= k <= 2048.
int launch_crc_flag(const void* bits, int kind, int64_t bs, int k, int deg, uint32_t g, const int32_t* idx,
                    uint8_t* valid, hipStream_t st);
// rows[0 .. *n_fail) = the b with valid[b] == 0, ascending; block_counts: kCompactMaxBlocks int32.
int launch_compact_failed(const uint8_t* valid, int64_t bs, int32_t* block_counts, int32_t* rows, int64_t* n_fail,
                          hipStream_t st);
// dst[j, :] = src[idx[j], :], j < cnt, rows of n floats
int launch_gather_rows_idx(const float* src, const int32_t* idx, int64_t cnt, int n, float* dst, hipStream_t st);
// dst[idx[j], :] = src[j, :], j < cnt, rows of k bits of the output kind
int launch_scatter_bits_idx(const void* src, const int32_t* idx, int64_t cnt, int k, int kind, void* dst,
                            hipStream_t st);
}  // namespace pl
