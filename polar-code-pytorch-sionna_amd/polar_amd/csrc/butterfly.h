// butterfly.h -- the XOR butterfly x = u G_n (my_sn/fec/polar/enc.py:85-96) on packed words, shared by
// the encoder (encode_kernel.hip) and the fused link producers (channel_kernel.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pl {

// positions whose index bit log2(h) is 0 (the "upper" element of each butterfly)
__device__ __forceinline__ uint32_t span_mask(int h) {
    switch (h) {
        case 1: return 0x55555555u;
        case 2: return 0x33333333u;
        case 4: return 0x0f0f0f0fu;
        case 8: return 0x00ff00ffu;
        default: return 0x0000ffffu;  // 16
    }
}

// Lane w of the wpc consecutive lanes of a codeword holds its positions 32w .. 32w + nb - 1 as bits
// 0 .. nb - 1 of x (nb = 32, or n for a codeword shorter than a word).  Spans below 32 are in-word
// shifts and masks, spans of 32 and more are lane XOR-shuffles; every lane of the wave must call.
__device__ __forceinline__ uint32_t polar_butterfly(uint32_t x, int nb, int wpc, int w) {
    for (int h = 1; h < nb; h <<= 1) x ^= (x >> h) & span_mask(h);
    for (int hw = 1; hw < wpc; hw <<= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)x, hw, 64);
        if ((w & hw) == 0) x ^= other;
    }
    return x;
}

}  // namespace pl
