// Device helpers the retrieval kernels of both engines share (recommend_kernels.hip: the step towers; graph_retrieval.h:
// the generic-layer engine's single-output towers): the score, the 64-bit ranking key and the wave's key sort.  One
// definition each, so a key and a score mean the same bits in every call of the family.
#pragma once
#include "mamdr_kernels.h"

namespace mamdr {

typedef unsigned long long u64;

__device__ __forceinline__ float rec_sigmoid(float logit) {          // as the evaluation's tower computes it
    if (logit >= 0.f) return 1.0f / (1.0f + __expf(-logit));
    const float ez = __expf(logit);
    return ez / (1.0f + ez);
}
__device__ __forceinline__ u64 rec_key(float logit, int id) {
    const uint32_t b = __float_as_uint(logit);
    uint32_t hi = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    if (logit != logit) hi = 1u;                  // below -inf (0x007fffff), above "no entry"
    return ((u64)hi << 32) | (u64)(~(uint32_t)id);
}
__device__ __forceinline__ float rec_key_logit(u64 key) {
    const uint32_t hi = (uint32_t)(key >> 32);
    if (hi == 1u) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((hi & 0x80000000u) ? (hi & 0x7fffffffu) : ~hi);
}

// descending bitonic sort of one key per lane of a wave
__device__ __forceinline__ u64 rec_wave_sort(u64 key, int lane) {
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const uint32_t olo = __shfl_xor((uint32_t)key, j), ohi = __shfl_xor((uint32_t)(key >> 32), j);
            const u64 other = ((u64)ohi << 32) | olo;
            const bool take_max = ((lane & j) == 0) == ((lane & k) == 0);
            key = take_max ? (key > other ? key : other) : (key < other ? key : other);
        }
    }
    return key;
}

}  // namespace mamdr
