// Binary cross-entropy + Dice loss for sigmoid heads (criterions/hybrid_binary_logistic_dice_loss.py):
// the binary / multi-label counterpart of the hybrid loss in hybrid_loss.hip, with the same structure -- a
// partial-sum kernel over chunks of one (n, c) row, a one-block finalize kernel, a one-pass closed-form backward
// (the shared pieces: loss_common.hpp).
//
//   PROB    x = p, probabilities (the Sigmoid head's output).  q = 1 - p (one fp32 subtraction, exact for p >= 0.5),
//           lp = log((p + eps) / (1 + eps)), lq = log((q + eps) / (1 + eps)), eps = 1e-8 (1 + eps == 1.0f, as in the
//           softmax loss).  No expf is evaluated.
//   LOGITS  x = z.  p = sigmoid_f32(z), the bits of m355_sigmoid_fwd and of the fused head; lp = -softplus(-z),
//           lq = -softplus(z), softplus(v) = max(v, 0) + log1p(exp(-|v|)): no eps, finite for every finite z.
//
// sums[nc * 5 + k] = {sum p t, sum p(^2), sum t(^2), sum t lp, sum (1 - t) lq}; class and positive weights enter in the
// finalize step and in the backward only.  The first three sums are accumulated by dice_accumulate in the order of
// hybrid_loss.hip's partial-sum kernel (thread i of a chunk takes elements i, i + 256, ... in fp32, then fp64 in a fixed
// order) and turned into the Dice term by the same dice_term, so the Dice term of a PROB launch has the bits of
// m355_hybrid_loss_fwd's.  That fixes one element per lane and load: rows start at nc * S
// for any S, and scalar loads need no alignment.  No float atomics: two launches give the same bits.
#include "loss_common.hpp"

namespace m355 {

constexpr int BLOSS_CHUNK = 16384;   // elements of a row per block of the partial-sum kernel (64 per thread)
constexpr int BLOSS_K = 5;
constexpr int BLOSS_U = 8;           // elements a lane loads ahead in the partial-sum kernel

// log-sigmoid pair of a logit: lp = log sigmoid(z), lq = log sigmoid(-z) = log(1 - sigmoid(z))
__device__ __forceinline__ void log_sigmoid_pair(float z, float& lp, float& lq) {
  const float l = log1pf(expf(-fabsf(z)));
  lp = -(fmaxf(-z, 0.f) + l);
  lq = -(fmaxf(z, 0.f) + l);
}

// partial[((n*C + c)*nblk + b)*5 + k]
template <bool LOGITS>
__global__ __launch_bounds__(256) void binary_loss_partial_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                                  double* __restrict__ partial, int64_t S, int square_dice,
                                                                  int nblk) {
  __shared__ double scratch[4];
  const int b = blockIdx.x;
  const int64_t nc = blockIdx.y;
  const float* xp = x + nc * S;
  const float* tp = t + nc * S;
  const int64_t begin = (int64_t)b * BLOSS_CHUNK, end = min(S, begin + BLOSS_CHUNK);
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
  // BLOSS_U elements of the lane's sequence are loaded before the first is used (two waves per SIMD at cfg2's output:
  // one load in flight per lane leaves the pass bound by memory latency); they are still added in sequence order
  for (int64_t i0 = begin + threadIdx.x; i0 < end; i0 += 256 * BLOSS_U) {
    float xs[BLOSS_U], ts[BLOSS_U];
#pragma unroll
    for (int u = 0; u < BLOSS_U; ++u) {
      const int64_t i = i0 + 256 * u;
      xs[u] = i < end ? xp[i] : 0.f;
      ts[u] = i < end ? tp[i] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < BLOSS_U; ++u) {
      if (i0 + 256 * u >= end) break;
      const float xv = xs[u], tv = ts[u];
      float pv, lp, lq;
      if (LOGITS) {
        pv = sigmoid_f32(xv);
        log_sigmoid_pair(xv, lp, lq);
      } else {
        pv = xv;
        const float qv = 1.f - pv;
        lp = safe_log_prob(pv);
        lq = safe_log_prob(qv);
      }
      dice_accumulate(pv, tv, square_dice, s0, s1, s2);
      s3 = fmaf(tv, lp, s3);
      s4 = fmaf(1.f - tv, lq, s4);
    }
  }
  const float s[BLOSS_K] = {s0, s1, s2, s3, s4};
  store_block_sums(s, partial, nc * nblk + b, scratch);
}

// single block, one thread per row, its chunks added in order: sums[nc*5+k], out3 = {loss, dice_loss, logistic_loss}
__global__ __launch_bounds__(256) void binary_loss_finalize_kernel(const double* __restrict__ partial,
                                                                   const float* __restrict__ class_w,
                                                                   const float* __restrict__ pos_w, float* __restrict__ sums,
                                                                   float* __restrict__ out3, int N, int C, int64_t S,
                                                                   int nblk, float dice_weight) {
  __shared__ double scratch[4];
  const int NC = N * C;
  double dice_acc = 0.0, log_acc = 0.0;
  for (int nc = threadIdx.x; nc < NC; nc += 256) {
    double v[BLOSS_K] = {0, 0, 0, 0, 0};
    for (int b = 0; b < nblk; ++b)
      for (int k = 0; k < BLOSS_K; ++k) v[k] += partial[((int64_t)nc * nblk + b) * BLOSS_K + k];
    for (int k = 0; k < BLOSS_K; ++k) sums[nc * BLOSS_K + k] = (float)v[k];
    dice_acc += (double)dice_term(v[0], v[1], v[2]);
    const double pw = pos_w ? (double)pos_w[nc % C] : 1.0;
    float logistic = (float)((pw * v[3] + v[4]) / (double)S);
    if (class_w) logistic *= class_w[nc % C];
    log_acc += (double)(-logistic);
  }
  const double d = block_sum<double, 256>(dice_acc, scratch);
  const double l = block_sum<double, 256>(log_acc, scratch);
  if (threadIdx.x == 0) write_out3(out3, dice_weight, (float)(d / NC), (float)(l / NC));
}

// dx = dloss * [ (1-w) * d(logistic_loss)/dx + w * d(dice_loss)/dx ],   k = cw[c] / (N*C*S)
//   d dice_loss / dp: dice_bwd_coeffs
//   PROB    d logistic_loss / dp = -k * (pw t / (p + eps) - (1 - t) / (q + eps))
//   LOGITS  d logistic_loss / dz =  k * (-pw t sigmoid(-z) + (1 - t) sigmoid(z));  dp/dz = p * sigmoid(-z)
//           (sigmoid(-z) is evaluated, not 1 - sigmoid(z): that difference cancels where the loss has to pull hardest)
template <bool LOGITS>
__global__ __launch_bounds__(256) void binary_loss_bwd_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                              const float* __restrict__ sums, const float* __restrict__ dloss,
                                                              const float* __restrict__ class_w,
                                                              const float* __restrict__ pos_w, float* __restrict__ dx, int N,
                                                              int C, int64_t S, float dice_weight, int square_dice) {
  const int64_t nc = blockIdx.y;
  const float g = dloss[0];
  const float inv_nc = 1.f / (float)(N * C);
  const DiceBwd k = dice_bwd_coeffs(sums + nc * BLOSS_K, dice_weight, inv_nc, g);
  const float cw = class_w ? class_w[nc % C] : 1.f;
  const float pw = pos_w ? pos_w[nc % C] : 1.f;
  const float klog = (1.f - dice_weight) * cw * inv_nc / (float)S * g;
  const float eps = 1e-8f;
  const float* xp = x + nc * S;
  const float* tp = t + nc * S;
  float* op = dx + nc * S;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < S; i += gridDim.x * 256ll) {
    const float xv = xp[i], tv = tp[i];
    float d;
    if (LOGITS) {
      const float pv = sigmoid_f32(xv), nv = sigmoid_f32(-xv);
      float dd = k.kd1 * tv;
      dd = fmaf(k.kd2, square_dice ? 2.f * pv : 1.f, dd);
      d = klog * fmaf(-pw * tv, nv, (1.f - tv) * pv);
      d = fmaf(dd, pv * nv, d);
    } else {
      const float qv = 1.f - xv;
      d = -klog * (pw * tv / (xv + eps) - (1.f - tv) / (qv + eps));
      d = fmaf(k.kd1, tv, d);
      d = fmaf(k.kd2, square_dice ? 2.f * xv : 1.f, d);
    }
    op[i] = d;
  }
}

}  // namespace m355

using namespace m355;

extern "C" size_t m355_binary_loss_workspace(int32_t N, int32_t C, int64_t S) {
  return loss_workspace_bytes(N, C, S, BLOSS_CHUNK, BLOSS_K);
}

extern "C" int m355_binary_loss_fwd(const float* x, const float* t, int32_t N, int32_t C, int64_t S, float dice_weight,
                                    const float* class_weights, const float* pos_weight, int32_t square_dice,
                                    int32_t from_logits, float* out3, float* sums, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  M355_REQUIRE(x && t && out3 && sums && workspace, M355_EINVALID_ARG, "binary_loss_fwd: null pointer");
  if (int rc = loss_check("binary_loss_fwd", N, C, S)) return rc;
  M355_REQUIRE(workspace_bytes >= m355_binary_loss_workspace(N, C, S), M355_EWORKSPACE,
               "binary_loss_fwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int nblk = (int)ceil_div(S, BLOSS_CHUNK);
  double* partial = (double*)workspace;
  const dim3 grid((unsigned)nblk, (unsigned)(N * C));
  if (from_logits)
    hipLaunchKernelGGL(binary_loss_partial_kernel<true>, grid, dim3(256), 0, st, x, t, partial, S, square_dice, nblk);
  else
    hipLaunchKernelGGL(binary_loss_partial_kernel<false>, grid, dim3(256), 0, st, x, t, partial, S, square_dice, nblk);
  hipLaunchKernelGGL(binary_loss_finalize_kernel, dim3(1), dim3(256), 0, st, partial, class_weights, pos_weight, sums, out3,
                     N, C, S, nblk, dice_weight);
  return check_launch("binary_loss_fwd");
}

extern "C" int m355_binary_loss_bwd(const float* x, const float* t, const float* sums, const float* dloss, int32_t N,
                                    int32_t C, int64_t S, float dice_weight, const float* class_weights,
                                    const float* pos_weight, int32_t square_dice, int32_t from_logits, float* dx,
                                    void* stream) {
  M355_REQUIRE(x && t && sums && dloss && dx, M355_EINVALID_ARG, "binary_loss_bwd: null pointer");
  if (int rc = loss_check("binary_loss_bwd", N, C, S)) return rc;
  const dim3 grid = loss_bwd_grid(S, 1024, N * C);
  if (from_logits)
    hipLaunchKernelGGL(binary_loss_bwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, t, sums, dloss,
                       class_weights, pos_weight, dx, N, C, S, dice_weight, square_dice);
  else
    hipLaunchKernelGGL(binary_loss_bwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, t, sums, dloss,
                       class_weights, pos_weight, dx, N, C, S, dice_weight, square_dice);
  return check_launch("binary_loss_bwd");
}
