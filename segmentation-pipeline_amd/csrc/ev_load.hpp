// Score loads and the argmax rule shared by the evaluation kernels (evaluate.hip, contour.hip).
#pragma once
#include "common.hpp"
#include <hip/hip_fp16.h>

namespace m355 {
namespace ev {

constexpr int SCORE_V = 8;   // scores per load_scores8 (one or two 16-byte loads)

template <int SD>
__device__ __forceinline__ void load_scores8(const void* p, int64_t i, float s[SCORE_V]) {
  if (SD == M355_EV_F32) {
    const float4 a = *(const float4*)((const float*)p + i), b = *(const float4*)((const float*)p + i + 4);
    s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w; s[4] = b.x; s[5] = b.y; s[6] = b.z; s[7] = b.w;
  } else {
    const uint4 r = *(const uint4*)((const uint16_t*)p + i);
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int j = 0; j < SCORE_V; ++j) {
      const uint16_t h = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
      if (SD == M355_EV_BF16) s[j] = __uint_as_float((uint32_t)h << 16);
      else s[j] = __half2float(__ushort_as_half(h));
    }
  }
}
template <int SD>
__device__ __forceinline__ float load_score1(const void* p, int64_t i) {
  if (SD == M355_EV_F32) return ((const float*)p)[i];
  const uint16_t h = ((const uint16_t*)p)[i];
  if (SD == M355_EV_BF16) return __uint_as_float((uint32_t)h << 16);
  return __half2float(__ushort_as_half(h));
}

// torch.argmax: the first maximum; a NaN is larger than everything and the first NaN wins
__device__ __forceinline__ bool takes(double best, double v) { return !(best != best) && (v != v || v > best); }

}  // namespace ev
}  // namespace m355
