// Boundary loss (criterions/boundary_loss.py): the mean of p * phi over the weighted channels, phi the signed
// distance map of the target (m355_signed_distance, csrc/distance.hip).
//
//   loss = sum_n sum_c w_c sum_v p[n, c, v] phi[n, c, v] / (N S sum_c w_c)
//   dp[n, c, v] = dloss (w_c / (N S sum_c w_c)) phi[n, c, v]
//
// Forward: a partial-sum kernel over chunks of one (n, c) row and a one-block finalize kernel (the shared pieces:
// loss_common.hpp).  Every product and every sum is fp64: an fp32 x fp32 product is exact there (48 bits), so the
// only rounding that matters is the one to the fp32 result.  phi takes both signs and the sum cancels; fp32 partial sums
// would lose what the loss is about.  Lanes, waves, chunks and rows are added in a fixed order, no float atomics: a call
// repeats bit for bit.  Rows with w_c == 0 are not read.
// Backward: one pass; the row's coefficient is formed in fp64 and rounded once, the product once more.
#include "loss_common.hpp"

namespace m355 {

constexpr int BL_CHUNK = 8192;   // elements of a row per block of the partial-sum kernel (32 per thread)

// sum_c w_c in fp64, in channel order
__device__ __forceinline__ double bl_weight_sum(const float* __restrict__ w, int C) {
  if (!w) return (double)C;
  double s = 0.0;
  for (int c = 0; c < C; ++c) s += (double)w[c];
  return s;
}

// partial[nc * nblk + b] = sum over chunk b of row nc of p * phi
__global__ __launch_bounds__(256) void bl_partial_kernel(const float* __restrict__ p, const float* __restrict__ phi,
                                                         const float* __restrict__ w, double* __restrict__ partial, int C,
                                                         int64_t S, int nblk) {
  __shared__ double scratch[4];
  const int b = blockIdx.x;
  const int64_t nc = blockIdx.y;
  if (w && w[nc % C] == 0.f) return;                 // (the whole block; the finalize kernel skips the row too)
  const float* pp = p + nc * S;
  const float* fp = phi + nc * S;
  const int64_t begin = (int64_t)b * BL_CHUNK, end = min(S, begin + BL_CHUNK);
  double acc = 0.0;
#pragma unroll 4
  for (int64_t v0 = begin + threadIdx.x * 4; v0 < end; v0 += 1024) {
    const int nv = row_valid(v0, end, 4);
    float a[4], f[4];
    row_load<4>(pp + v0, nv, a);
    row_load<4>(fp + v0, nv, f);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = fma((double)a[j], (double)f[j], acc);   // (elements past the row are 0 * 0)
  }
  const double s[1] = {acc};
  store_block_sums(s, partial, nc * nblk + b, scratch);
}

// single block.  Wave k takes the rows k, k + 4, ..: its lanes add the row's chunks l, l + 64, .. in fp64, then a butterfly.
__global__ __launch_bounds__(256) void bl_finalize_kernel(const double* __restrict__ partial, const float* __restrict__ w,
                                                          float* __restrict__ loss, int N, int C, int64_t S, int nblk) {
  __shared__ double scratch[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc = 0.0;
  for (int nc = wave; nc < N * C; nc += 4) {
    const float wc = w ? w[nc % C] : 1.f;
    if (wc == 0.f) continue;                         // wave-uniform
    double v = 0.0;
    for (int b = lane; b < nblk; b += 64) v += partial[(int64_t)nc * nblk + b];
    v = wave_sum(v);
    if (lane == 0) acc += (double)wc * v;
  }
  const double total = block_sum<double, 256>(acc, scratch);
  if (threadIdx.x == 0) loss[0] = (float)(total / ((double)N * (double)S * bl_weight_sum(w, C)));
}

__global__ __launch_bounds__(256) void bl_bwd_kernel(const float* __restrict__ phi, const float* __restrict__ dloss,
                                                     const float* __restrict__ w, float* __restrict__ dp, int N, int C,
                                                     int64_t S) {
  const int64_t nc = blockIdx.y;
  const float wc = w ? w[nc % C] : 1.f;
  const float k = (float)((double)dloss[0] * (double)wc / ((double)N * (double)S * bl_weight_sum(w, C)));
  const float* fp = phi + nc * S;
  float* op = dp + nc * S;
  for (int64_t v0 = (blockIdx.x * 256ll + threadIdx.x) * 4; v0 < S; v0 += gridDim.x * 1024ll) {
    const int nv = row_valid(v0, S, 4);
    float f[4], o[4] = {0.f, 0.f, 0.f, 0.f};
    if (wc != 0.f) {                                 // (a row without weight gets zeros whatever dloss and phi hold)
      row_load<4>(fp + v0, nv, f);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = __fmul_rn(k, f[j]);
    }
    row_store<4>(op + v0, nv, o);
  }
}

}  // namespace m355

using namespace m355;

extern "C" size_t m355_boundary_loss_workspace(int32_t N, int32_t C, int64_t S) {
  return loss_workspace_bytes(N, C, S, BL_CHUNK, 1);
}

extern "C" int m355_boundary_loss_fwd(const float* p, const float* phi, const float* class_weights, int32_t N, int32_t C,
                                      int64_t S, float* loss, void* workspace, size_t workspace_bytes, void* stream) {
  M355_REQUIRE(p && phi && loss && workspace, M355_EINVALID_ARG, "boundary_loss_fwd: null pointer");
  if (int rc = loss_check("boundary_loss_fwd", N, C, S)) return rc;
  M355_REQUIRE(workspace_bytes >= m355_boundary_loss_workspace(N, C, S), M355_EWORKSPACE,
               "boundary_loss_fwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int nblk = (int)ceil_div(S, BL_CHUNK);
  hipLaunchKernelGGL(bl_partial_kernel, dim3((unsigned)nblk, (unsigned)(N * C)), dim3(256), 0, st, p, phi, class_weights,
                     (double*)workspace, (int)C, S, nblk);
  if (int rc = check_launch("boundary_loss_fwd: partial sums")) return rc;
  hipLaunchKernelGGL(bl_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)workspace, class_weights, loss, (int)N,
                     (int)C, S, nblk);
  return check_launch("boundary_loss_fwd");
}

extern "C" int m355_boundary_loss_bwd(const float* phi, const float* dloss, const float* class_weights, int32_t N, int32_t C,
                                      int64_t S, float* dp, void* stream) {
  M355_REQUIRE(phi && dloss && dp, M355_EINVALID_ARG, "boundary_loss_bwd: null pointer");
  if (int rc = loss_check("boundary_loss_bwd", N, C, S)) return rc;
  hipLaunchKernelGGL(bl_bwd_kernel, loss_bwd_grid(S, 2048, N * C), dim3(256), 0, (hipStream_t)stream, phi, dloss, class_weights, dp, (int)N, (int)C, S);
  return check_launch("boundary_loss_bwd");
}
