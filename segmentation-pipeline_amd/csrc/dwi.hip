// Mean diffusion-weighted image of picked gradient channels: the per-voxel work of the reference's ReconstructMeanDWI /
// ReconstructMeanDWIClassic (segmentation_pipeline/transforms/reconstruct_mean_dwi.py).  The channels are drawn on the
// host (augmentation.py); the kernel is deterministic given them.
//
//   dwi_mean_kernel   out[v] = (x[i0][v] + x[i1][v] + ... + x[ik-1][v]) / k, summed in fp32 in pick order, then ONE
//                     correctly rounded fp32 division: what np.mean(x[idx], axis=0) and torch.mean(x[idx], 0) compute
//                     for float32.  One plain streaming pass; each thread takes DWI_G groups of 4 voxels, with 16-byte
//                     loads when every channel base is 16-byte aligned (voxel count a multiple of 4), else the scalar
//                     path over the same groups (a last group shorter than 4 voxels is the tail).
#include "common.hpp"

// no contraction, no reciprocal: the division below is IEEE fp32 `/` (hipcc's default correctly rounded divide)
#pragma clang fp contract(off)

namespace m355 {

constexpr int DWI_NT = 256;
constexpr int DWI_G = 2;   // groups of 4 voxels per thread

template <bool VEC>
__global__ void __launch_bounds__(DWI_NT) dwi_mean_kernel(const float* __restrict__ x, const int32_t* __restrict__ idx,
                                                          int32_t k, int32_t N, int64_t S, float* __restrict__ y) {
  const float kf = (float)k;
  const int64_t groups = (S + 3) / 4;
  const int64_t g0 = (int64_t)blockIdx.x * (DWI_NT * DWI_G) + threadIdx.x;
#pragma unroll
  for (int r = 0; r < DWI_G; ++r) {
    const int64_t g = g0 + (int64_t)r * DWI_NT;   // consecutive lanes take consecutive groups
    if (g >= groups) return;
    const int64_t v = 4 * g;
    if (VEC) {
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int32_t j = 0; j < k; ++j) {
        const int32_t c = idx[j];
        if ((uint32_t)c >= (uint32_t)N) {   // outside [0, N): NaN, never an out-of-bounds read
          s = make_float4(__int_as_float(0x7fc00000), __int_as_float(0x7fc00000), __int_as_float(0x7fc00000),
                          __int_as_float(0x7fc00000));
          continue;
        }
        const float4 a = *reinterpret_cast<const float4*>(x + (int64_t)c * S + v);
        if (j == 0) {
          s = a;
        } else {
          s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w;
        }
      }
      *reinterpret_cast<float4*>(y + v) = make_float4(s.x / kf, s.y / kf, s.z / kf, s.w / kf);
    } else {
      const int n = (int)((S - v) < 4 ? (S - v) : 4);
      float s[4] = {0.f, 0.f, 0.f, 0.f};
      for (int32_t j = 0; j < k; ++j) {
        const int32_t c = idx[j];
        if ((uint32_t)c >= (uint32_t)N) {
          for (int e = 0; e < 4; ++e) s[e] = __int_as_float(0x7fc00000);
          continue;
        }
        const float* p = x + (int64_t)c * S + v;
        for (int e = 0; e < n; ++e) s[e] = j == 0 ? p[e] : s[e] + p[e];
      }
      for (int e = 0; e < n; ++e) y[v + e] = s[e] / kf;
    }
  }
}

}  // namespace m355

using namespace m355;

extern "C" int m355_dwi_mean(const float* x, int32_t N, const int32_t* size3, const int32_t* idx, int32_t k, float* y,
                             void* stream) {
  M355_REQUIRE(size3, M355_EINVALID_ARG, "dwi_mean: null size");
  M355_REQUIRE(size3[0] > 0 && size3[1] > 0 && size3[2] > 0, M355_EINVALID_ARG, "dwi_mean: non-positive size %d x %d x %d",
               size3[0], size3[1], size3[2]);
  const int64_t S = (int64_t)size3[0] * size3[1] * size3[2];
  M355_REQUIRE(S < ((int64_t)1 << 31), M355_EINVALID_ARG, "dwi_mean: %lld voxels per channel (< 2^31)", (long long)S);
  M355_REQUIRE(x && idx && y, M355_EINVALID_ARG, "dwi_mean: null pointer");
  M355_REQUIRE(N > 0 && k > 0, M355_EINVALID_ARG, "dwi_mean: %d channels, %d picks (both > 0)", N, k);
  M355_REQUIRE((const void*)y != (const void*)x, M355_EINVALID_ARG, "dwi_mean: y == x");
  const bool vec = S % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0;
  const int64_t groups = (S + 3) / 4;
  const unsigned grid = (unsigned)ceil_div(groups, (int64_t)DWI_NT * DWI_G);
  if (vec)
    hipLaunchKernelGGL(dwi_mean_kernel<true>, dim3(grid), dim3(DWI_NT), 0, (hipStream_t)stream, x, idx, k, N, S, y);
  else
    hipLaunchKernelGGL(dwi_mean_kernel<false>, dim3(grid), dim3(DWI_NT), 0, (hipStream_t)stream, x, idx, k, N, S, y);
  return check_launch("dwi_mean");
}
