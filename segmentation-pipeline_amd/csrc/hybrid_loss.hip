// Hybrid logistic + Dice loss (fwd/bwd).  HBM-bound single-pass kernels: a partial-sum kernel over chunks of one (n, c)
// row, a one-block finalize kernel, a one-pass closed-form backward (the shared pieces: loss_common.hpp).
//
// Reference code replaced:
//   HybridLogisticDiceLoss.forward  criterions/hybrid_logistic_dice_loss.py:13-43
#include "loss_common.hpp"

namespace m355 {

constexpr int LOSS_CHUNK = 16384;
constexpr int LOSS_K = 4;

// partial[((n*C + c)*nblk + b)*4 + k], k: 0 = sum p*t, 1 = sum p(^2), 2 = sum t(^2),
// 3 = sum t*log(p_safe)
__global__ __launch_bounds__(256) void loss_partial_kernel(const float* __restrict__ p,
                                                           const float* __restrict__ t,
                                                           double* __restrict__ partial, int64_t S,
                                                           int square_dice, int nblk) {
  __shared__ double scratch[4];
  const int b = blockIdx.x;
  const int64_t nc = blockIdx.y;
  const float* pp = p + nc * S;
  const float* tp = t + nc * S;
  const int64_t begin = (int64_t)b * LOSS_CHUNK, end = min(S, begin + LOSS_CHUNK);
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  for (int64_t i = begin + threadIdx.x; i < end; i += 256) {
    const float pv = pp[i], tv = tp[i];
    dice_accumulate(pv, tv, square_dice, s0, s1, s2);
    s3 = fmaf(tv, safe_log_prob(pv), s3);
  }
  const float s[LOSS_K] = {s0, s1, s2, s3};
  store_block_sums(s, partial, nc * nblk + b, scratch);
}

// single block, one thread per row, its chunks added in order: sums[nc*4+k], out3 = {loss, dice_loss, logistic_loss}
__global__ __launch_bounds__(256) void loss_finalize_kernel(const double* __restrict__ partial,
                                                            const float* __restrict__ class_w,
                                                            float* __restrict__ sums,
                                                            float* __restrict__ out3, int N, int C,
                                                            int64_t S, int nblk, float dice_weight) {
  __shared__ double scratch[4];
  const int NC = N * C;
  double dice_acc = 0.0, log_acc = 0.0;
  for (int nc = threadIdx.x; nc < NC; nc += 256) {
    double v[LOSS_K] = {0, 0, 0, 0};
    for (int b = 0; b < nblk; ++b)
      for (int k = 0; k < LOSS_K; ++k) v[k] += partial[((int64_t)nc * nblk + b) * LOSS_K + k];
    for (int k = 0; k < LOSS_K; ++k) sums[nc * LOSS_K + k] = (float)v[k];
    dice_acc += (double)dice_term(v[0], v[1], v[2]);
    float logistic = (float)(v[3] / (double)S);  // torch.mean over spatial dims
    if (class_w) logistic *= class_w[nc % C];
    log_acc += (double)(-logistic);
  }
  const double d = block_sum<double, 256>(dice_acc, scratch);
  const double l = block_sum<double, 256>(log_acc, scratch);
  if (threadIdx.x == 0) write_out3(out3, dice_weight, (float)(d / NC), (float)(l / NC));
}

// dp = dloss * [ (1-w) * d(logistic_loss)/dp + w * d(dice_loss)/dp ]
//   d logistic_loss / dp = -cw[c] * t / ((p + eps) ) / (N*C*S)          (denominator 1+eps == 1)
//   d dice_loss / dp: dice_bwd_coeffs
__global__ __launch_bounds__(256) void loss_bwd_kernel(const float* __restrict__ p,
                                                       const float* __restrict__ t,
                                                       const float* __restrict__ sums,
                                                       const float* __restrict__ dloss,
                                                       const float* __restrict__ class_w,
                                                       float* __restrict__ dp, int N, int C,
                                                       int64_t S, float dice_weight,
                                                       int square_dice) {
  const int64_t nc = blockIdx.y;
  const float g = dloss[0];
  const float inv_nc = 1.f / (float)(N * C);
  const DiceBwd k = dice_bwd_coeffs(sums + nc * LOSS_K, dice_weight, inv_nc, g);
  const float cw = class_w ? class_w[nc % C] : 1.f;
  const float klog = -(1.f - dice_weight) * cw * inv_nc / (float)S * g;
  const float denom = (float)(1.0 + 1e-8);
  const float* pp = p + nc * S;
  const float* tp = t + nc * S;
  float* op = dp + nc * S;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < S; i += gridDim.x * 256ll) {
    const float pv = pp[i], tv = tp[i];
    const float ps = (pv + 1e-8f) / denom;
    float d = klog * tv / (ps * denom);
    d = fmaf(k.kd1, tv, d);
    d = fmaf(k.kd2, square_dice ? 2.f * pv : 1.f, d);
    op[i] = d;
  }
}

}  // namespace m355

using namespace m355;

extern "C" size_t m355_hybrid_loss_workspace(int32_t N, int32_t C, int64_t S) {
  return loss_workspace_bytes(N, C, S, LOSS_CHUNK, LOSS_K);
}

extern "C" int m355_hybrid_loss_fwd(const float* p, const float* t, int32_t N, int32_t C, int64_t S,
                                    float dice_weight, const float* class_weights,
                                    int32_t square_dice, float* out3, float* sums, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  M355_REQUIRE(p && t && out3 && sums && workspace, M355_EINVALID_ARG, "hybrid_loss_fwd: null pointer");
  if (int rc = loss_check("hybrid_loss_fwd", N, C, S)) return rc;
  M355_REQUIRE(workspace_bytes >= m355_hybrid_loss_workspace(N, C, S), M355_EWORKSPACE,
               "hybrid_loss_fwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int nblk = (int)ceil_div(S, LOSS_CHUNK);
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(loss_partial_kernel, dim3((unsigned)nblk, (unsigned)(N * C)), dim3(256), 0, st,
                     p, t, partial, S, square_dice, nblk);
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, st, partial, class_weights, sums,
                     out3, N, C, S, nblk, dice_weight);
  return check_launch("hybrid_loss_fwd");
}

extern "C" int m355_hybrid_loss_bwd(const float* p, const float* t, const float* sums,
                                    const float* dloss, int32_t N, int32_t C, int64_t S,
                                    float dice_weight, const float* class_weights,
                                    int32_t square_dice, float* dp, void* stream) {
  M355_REQUIRE(p && t && sums && dloss && dp, M355_EINVALID_ARG, "hybrid_loss_bwd: null pointer");
  if (int rc = loss_check("hybrid_loss_bwd", N, C, S)) return rc;
  hipLaunchKernelGGL(loss_bwd_kernel, loss_bwd_grid(S, 1024, N * C), dim3(256), 0, (hipStream_t)stream,
                     p, t, sums, dloss, class_weights, dp, N, C, S, dice_weight, square_dice);
  return check_launch("hybrid_loss_bwd");
}
