// Focal Tversky criterion (criterions/hybrid_focal_tversky_loss.py): a Tversky overlap term with separate
// weights for false positives and false negatives, raised to a power, plus a focal cross-entropy on the positive half.
//
//   PROB    x = p.  q = 1 - p, lp = log((p + eps) / (1 + eps)), eps = 1e-8 (1 + eps == 1.0f).  No expf is evaluated.
//           Row-major: a partial-sum kernel over chunks of one (n, c) row, a one-block finalize kernel, a one-pass
//           closed-form backward (the shared pieces: loss_common.hpp).
//   LOGITS  x = z, the log-softmax over the C channels of a voxel is taken here: m = max_c z_c, s = sum_c exp(z_c - m),
//           lp_c = (z_c - m) - log s, p_c = exp(z_c - m) / s, q_c = -expm1(lp_c) (1 - p cancels near p = 1).  No eps.
//           Voxel-major: a lane owns VPL consecutive voxels and walks the C channel planes, every plane read coalesced
//           along S.  Up to FT_CREG channels the values of a voxel stay in registers between the reduction over C and
//           their use; above it the planes are read again (they are in L2: a block touches FT_LCHUNK voxels per plane).
//
// sums[nc * 4 + k] = {TP = sum p t, FP = sum p (1 - t), FN = sum q t, sum t q^gamma lp}, each accumulated directly: the
// class weights, alpha, beta and the power enter in the finalize step and in the backward only.
//
// Loads and stores: a lane's group of VPL consecutive elements goes through row_load / row_store, so a misaligned view
// gives the bits of its aligned clone.  fp32 per lane in a fixed order, then fp64 across the block and across the chunks
// in a fixed order; no float atomics.
#include "loss_common.hpp"

#include <cmath>

namespace m355 {

constexpr int FT_PCHUNK = 8192;   // PROB: elements of a row per block of the partial-sum kernel (32 per thread)
constexpr int FT_LCHUNK = 4096;   // LOGITS: voxels per block, every channel of them; the workspace is sized by this one
constexpr int FT_CREG = 16;       // LOGITS: most channels whose per-voxel values are held in registers
constexpr int FT_U = 4;           // PROB: groups of 4 elements a lane loads ahead

// the focal factor's exponent: 0 = gamma == 0 (the factor is 1 and nothing is evaluated), 1 = gamma in {1, 2, 3} (`gi`,
// by multiplication), 2 = any other gamma > 1 (powf)
template <int GM>
__device__ __forceinline__ float focal_pow(float q, float gamma, int gi) {
  if (GM == 0) return 1.f;
  if (GM == 1) return gi == 1 ? q : gi == 2 ? q * q : q * q * q;
  return powf(fmaxf(q, 0.f), gamma);           // 0 at q == 0
}
// the backward's pair: dq = q^(gamma - 1) and qg = q^gamma = q dq, one powf for both (never used with gamma == 0)
template <int GM>
__device__ __forceinline__ void focal_pow_pair(float q, float gamma, int gi, float& qg, float& dq) {
  if (GM == 1) dq = gi == 1 ? 1.f : gi == 2 ? q : q * q;
  else dq = powf(fmaxf(q, 0.f), gamma - 1.f);  // gamma > 1 here: 0 at q == 0
  qg = q * dq;
}

// one element's contribution to the four sums of its row
template <int GM>
__device__ __forceinline__ void ft_accumulate(float pv, float qv, float lp, float tv, float gamma, int gi, float& s0,
                                              float& s1, float& s2, float& s3) {
  s0 = fmaf(pv, tv, s0);
  s1 = fmaf(pv, 1.f - tv, s1);
  s2 = fmaf(qv, tv, s2);
  s3 = fmaf(tv * focal_pow<GM>(qv, gamma, gi), lp, s3);
}

// ---------------------------------------------------------------------------------------------------- PROB forward
// partial[((n*C + c)*nblk + b)*4 + k]
template <int GM>
__global__ __launch_bounds__(256) void ft_prob_partial_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                              double* __restrict__ partial, int64_t S, int nblk,
                                                              float gamma, int gi) {
  __shared__ double scratch[4];
  const int b = blockIdx.x;
  const int64_t nc = blockIdx.y;
  const float* xp = x + nc * S;
  const float* tp = t + nc * S;
  const int64_t begin = (int64_t)b * FT_PCHUNK, end = min(S, begin + FT_PCHUNK);
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  // FT_U groups of x and of t are in flight per lane before the first is used; they are added in sequence order
  for (int64_t g0 = begin + threadIdx.x * 4; g0 < end; g0 += 256 * 4 * FT_U) {
    float xs[FT_U][4], ts[FT_U][4];
    int nv[FT_U];
#pragma unroll
    for (int u = 0; u < FT_U; ++u) {
      const int64_t v0 = g0 + 1024 * u;
      nv[u] = row_valid(v0, end, 4);
      row_load<4>(xp + v0, nv[u], xs[u]);
      row_load<4>(tp + v0, nv[u], ts[u]);
    }
#pragma unroll
    for (int u = 0; u < FT_U; ++u) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j >= nv[u]) break;
        const float pv = xs[u][j];
        ft_accumulate<GM>(pv, 1.f - pv, safe_log_prob(pv), ts[u][j], gamma, gi, s0, s1, s2, s3);
      }
    }
  }
  const float s[4] = {s0, s1, s2, s3};
  store_block_sums(s, partial, nc * nblk + b, scratch);
}

// -------------------------------------------------------------------------------------------------- LOGITS forward
// Channels in registers: C <= CR.  A block takes FT_LCHUNK voxels of one n and emits C x 4 partials.
template <int CR, int VPL, int GM>
__global__ __launch_bounds__(256) void ft_logits_partial_kernel(const float* __restrict__ z, const float* __restrict__ t,
                                                                double* __restrict__ partial, int C, int64_t S, int nblk,
                                                                float gamma, int gi) {
  __shared__ double red[4][CR * 4];
  const int b = blockIdx.x;
  const int64_t n = blockIdx.y;
  const float* zn = z + n * C * S;
  const float* tn = t + n * C * S;
  const int64_t begin = (int64_t)b * FT_LCHUNK, end = min(S, begin + FT_LCHUNK);
  float acc[CR][4];
#pragma unroll
  for (int c = 0; c < CR; ++c)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[c][k] = 0.f;
  for (int64_t v0 = begin + threadIdx.x * VPL; v0 < end; v0 += 256 * VPL) {
    const int nv = row_valid(v0, end, VPL);
    float d[CR][VPL], e[CR][VPL], m[VPL], s[VPL];
#pragma unroll
    for (int c = 0; c < CR; ++c)
      if (c < C) row_load<VPL>(zn + c * S + v0, nv, d[c]);
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      m[j] = d[0][j];
      s[j] = 0.f;
    }
#pragma unroll
    for (int c = 1; c < CR; ++c)
      if (c < C)
#pragma unroll
        for (int j = 0; j < VPL; ++j) m[j] = fmaxf(m[j], d[c][j]);
#pragma unroll
    for (int c = 0; c < CR; ++c)
      if (c < C)
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
          d[c][j] -= m[j];
          e[c][j] = expf(d[c][j]);
          s[j] += e[c][j];
        }
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      m[j] = logf(s[j]);      // from here on m is log s
      s[j] = 1.f / s[j];      // and s its reciprocal
    }
#pragma unroll
    for (int c = 0; c < CR; ++c)
      if (c < C) {
        float tt[VPL];
        row_load<VPL>(tn + c * S + v0, nv, tt);
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
          if (j >= nv) break;
          const float lp = d[c][j] - m[j];
          ft_accumulate<GM>(e[c][j] * s[j], -expm1f(lp), lp, tt[j], gamma, gi, acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
        }
      }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < CR; ++c)
    if (c < C)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double r = wave_sum((double)acc[c][k]);
        if (lane == 0) red[w][c * 4 + k] = r;
      }
  __syncthreads();
  if ((int)threadIdx.x < C * 4) {
    const int c = threadIdx.x >> 2, k = threadIdx.x & 3;
    const double r = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    partial[((n * C + c) * nblk + b) * 4 + k] = r;
  }
}

constexpr int FT_IT = FT_LCHUNK / 1024;   // groups of 4 voxels per lane in the kernels that read the planes again

// C > FT_CREG: max and log-sum of every voxel of the chunk first (two reads of the z planes), then plane by plane
template <int GM>
__global__ __launch_bounds__(256) void ft_logits_partial_reread_kernel(const float* __restrict__ z,
                                                                       const float* __restrict__ t,
                                                                       double* __restrict__ partial, int C, int64_t S,
                                                                       int nblk, float gamma, int gi) {
  __shared__ double scratch[4];
  const int b = blockIdx.x;
  const int64_t n = blockIdx.y;
  const float* zn = z + n * C * S;
  const float* tn = t + n * C * S;
  const int64_t begin = (int64_t)b * FT_LCHUNK, end = min(S, begin + FT_LCHUNK);
  float m[FT_IT][4], ls[FT_IT][4], inv[FT_IT][4];
  int nv[FT_IT];
#pragma unroll
  for (int it = 0; it < FT_IT; ++it) {
    const int64_t v0 = begin + (it * 256 + threadIdx.x) * 4;
    nv[it] = row_valid(v0, end, 4);
    float v[4];
    row_load<4>(zn + v0, nv[it], m[it]);
    for (int c = 1; c < C; ++c) {
      row_load<4>(zn + c * S + v0, nv[it], v);
#pragma unroll
      for (int j = 0; j < 4; ++j) m[it][j] = fmaxf(m[it][j], v[j]);
    }
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < C; ++c) {
      row_load<4>(zn + c * S + v0, nv[it], v);
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] += expf(v[j] - m[it][j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ls[it][j] = logf(s[j]);
      inv[it][j] = 1.f / s[j];
    }
  }
  for (int c = 0; c < C; ++c) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int it = 0; it < FT_IT; ++it) {
      const int64_t v0 = begin + (it * 256 + threadIdx.x) * 4;
      float zz[4], tt[4];
      row_load<4>(zn + c * S + v0, nv[it], zz);
      row_load<4>(tn + c * S + v0, nv[it], tt);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j >= nv[it]) break;
        const float dd = zz[j] - m[it][j], lp = dd - ls[it][j];
        ft_accumulate<GM>(expf(dd) * inv[it][j], -expm1f(lp), lp, tt[j], gamma, gi, s0, s1, s2, s3);
      }
    }
    const float s[4] = {s0, s1, s2, s3};
    store_block_sums(s, partial, (n * C + c) * nblk + b, scratch);
  }
}

// --------------------------------------------------------------------------------------------------------- finalize
// The Tversky index of a row in fp32 from its fp32 sums -- the backward's expressions, so u == 0 there where it is here.
__device__ __forceinline__ float ft_one_minus_ti(float TP, float FP, float FN, float alpha, float beta, float& D) {
  D = TP + alpha * FP + beta * FN + 0.5e-8f;
  return fmaxf(0.f, 1.f - TP / D);
}

// single block.  `lanes` (a power of two <= 64) threads share the chunks of one row: lane l adds chunks l, l + lanes, ..
// in fp64, then the lanes are added in a butterfly -- a fixed order for a given shape.
__global__ __launch_bounds__(256) void ft_finalize_kernel(const double* __restrict__ partial, const float* __restrict__ focal_w,
                                                          const float* __restrict__ tversky_w, float* __restrict__ sums,
                                                          float* __restrict__ out3, int N, int C, int64_t S, int nblk,
                                                          int lanes, float tversky_weight, float alpha, float beta,
                                                          float power) {
  __shared__ double scratch[4];
  const int NC = N * C;
  const int per = 256 / lanes, sub = threadIdx.x % lanes, slot = threadIdx.x / lanes;
  double tv_acc = 0.0, fo_acc = 0.0;
  for (int nc0 = 0; nc0 < NC; nc0 += per) {
    const int nc = nc0 + slot;
    double v[4] = {0, 0, 0, 0};
    if (nc < NC)
      for (int b = sub; b < nblk; b += lanes)
        for (int k = 0; k < 4; ++k) v[k] += partial[((int64_t)nc * nblk + b) * 4 + k];
    for (int off = lanes >> 1; off > 0; off >>= 1)
      for (int k = 0; k < 4; ++k) v[k] += __shfl_xor(v[k], off, 64);
    if (nc < NC && sub == 0) {
      for (int k = 0; k < 4; ++k) sums[nc * 4 + k] = (float)v[k];
      float D;
      const float u = ft_one_minus_ti((float)v[0], (float)v[1], (float)v[2], alpha, beta, D);
      float term = power == 1.f ? u : powf(u, power);
      if (tversky_w) term *= tversky_w[nc % C];
      tv_acc += (double)term;
      float focal = (float)(v[3] / (double)S);
      if (focal_w) focal *= focal_w[nc % C];
      fo_acc += (double)(-focal);
    }
  }
  const double tv = block_sum<double, 256>(tv_acc, scratch);
  const double fo = block_sum<double, 256>(fo_acc, scratch);
  if (threadIdx.x == 0) write_out3(out3, tversky_weight, (float)(tv / NC), (float)(fo / NC));
}

// --------------------------------------------------------------------------------------------------------- backward
// Row coefficients, dloss included.  With D = TP + alpha FP + beta FN + eps/2 and u = max(0, 1 - TP / D):
//   h = -lambda/(N C) v_c e u^(e-1) dTI/dp = A t + B,   dTI/dp = (t (D - TP (1 - alpha - beta)) - alpha TP) / D^2
//   (A = B = 0 where u == 0, for e < 1 too);   kf = -(1 - lambda)/(N C S) w_c
struct FtCoef {
  float A, B, kf;
};

__device__ __forceinline__ FtCoef ft_coef(const float* __restrict__ sums, int64_t nc, int c, const float* __restrict__ focal_w,
                                          const float* __restrict__ tversky_w, float g, float inv_nc, float inv_s,
                                          float tversky_weight, float alpha, float beta, float power) {
  const float TP = sums[nc * 4 + 0];
  float D;
  const float u = ft_one_minus_ti(TP, sums[nc * 4 + 1], sums[nc * 4 + 2], alpha, beta, D);
  float kt = 0.f;
  if (u > 0.f) {
    kt = -tversky_weight * inv_nc * g * (tversky_w ? tversky_w[c] : 1.f);
    if (power != 1.f) kt *= power * powf(u, power - 1.f);
  }
  FtCoef k;
  k.A = kt * ((D - TP * (1.f - alpha - beta)) / D) / D;
  k.B = -kt * (alpha * TP / D) / D;
  k.kf = -(1.f - tversky_weight) * inv_nc * inv_s * g * (focal_w ? focal_w[c] : 1.f);
  return k;
}

// PROB: dp = A t + B + kf t (q^gamma / (p + eps) - gamma q^(gamma-1) lp)
template <int GM>
__global__ __launch_bounds__(256) void ft_prob_bwd_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                          const float* __restrict__ sums, const float* __restrict__ dloss,
                                                          const float* __restrict__ focal_w, const float* __restrict__ tversky_w,
                                                          float* __restrict__ dx, int N, int C, int64_t S, float tversky_weight,
                                                          float alpha, float beta, float power, float gamma, int gi) {
  const int64_t nc = blockIdx.y;
  const FtCoef k = ft_coef(sums, nc, (int)(nc % C), focal_w, tversky_w, dloss[0], 1.f / (float)(N * C), 1.f / (float)S,
                           tversky_weight, alpha, beta, power);
  const float eps = 1e-8f;
  const float* xp = x + nc * S;
  const float* tp = t + nc * S;
  float* op = dx + nc * S;
  for (int64_t v0 = (blockIdx.x * 256ll + threadIdx.x) * 4; v0 < S; v0 += gridDim.x * 1024ll) {
    const int nv = row_valid(v0, S, 4);
    float xs[4], ts[4], o[4];
    row_load<4>(xp + v0, nv, xs);
    row_load<4>(tp + v0, nv, ts);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float pv = xs[j], tv = ts[j];
      float f;
      if (GM == 0) {
        f = 1.f / (pv + eps);
      } else {
        float qg, dq;
        focal_pow_pair<GM>(1.f - pv, gamma, gi, qg, dq);
        f = qg / (pv + eps) - gamma * dq * safe_log_prob(pv);
      }
      o[j] = fmaf(k.kf * tv, f, fmaf(k.A, tv, k.B));
    }
    row_store<4>(op + v0, nv, o);
  }
}

// one (channel, voxel) of the LOGITS backward: p and a = g + p h from d = z - max (or exp(d) already, without a focal
// factor), log s, 1 / s and t.  g = kf t (q^gamma - gamma q^(gamma-1) p lp)
template <int GM>
__device__ __forceinline__ void ft_logits_terms(float dv, float ls, float inv, float tv, const FtCoef& k, float gamma, int gi,
                                                float& p, float& a) {
  float g;
  if (GM == 0) {
    p = dv * inv;
    g = k.kf * tv;
  } else {
    const float lp = dv - ls;
    p = expf(dv) * inv;
    float qg, dq;
    focal_pow_pair<GM>(-expm1f(lp), gamma, gi, qg, dq);
    g = k.kf * tv * (qg - gamma * dq * p * lp);
  }
  a = fmaf(p, fmaf(k.A, tv, k.B), g);
}

// LOGITS, C <= CR: dz_k = a_k - p_k sum_c a_c   (a_c = g_c + p_c h_c: the two reductions over C are one sum)
template <int CR, int VPL, int GM>
__global__ __launch_bounds__(256) void ft_logits_bwd_kernel(const float* __restrict__ z, const float* __restrict__ t,
                                                            const float* __restrict__ sums, const float* __restrict__ dloss,
                                                            const float* __restrict__ focal_w, const float* __restrict__ tversky_w,
                                                            float* __restrict__ dz, int N, int C, int64_t S, float tversky_weight,
                                                            float alpha, float beta, float power, float gamma, int gi) {
  __shared__ FtCoef coef[CR];
  const int64_t n = blockIdx.y;
  if ((int)threadIdx.x < C)
    coef[threadIdx.x] = ft_coef(sums, n * C + threadIdx.x, threadIdx.x, focal_w, tversky_w, dloss[0], 1.f / (float)(N * C),
                                1.f / (float)S, tversky_weight, alpha, beta, power);
  __syncthreads();
  const float* zn = z + n * C * S;
  const float* tn = t + n * C * S;
  float* on = dz + n * C * S;
  const int64_t begin = (int64_t)blockIdx.x * FT_LCHUNK, end = min(S, begin + FT_LCHUNK);
  for (int64_t v0 = begin + threadIdx.x * VPL; v0 < end; v0 += 256 * VPL) {
    const int nv = row_valid(v0, end, VPL);
    float d[CR][VPL], a[CR][VPL], m[VPL], s[VPL], sum_a[VPL];
#pragma unroll
    for (int c = 0; c < CR; ++c)
      if (c < C) row_load<VPL>(zn + c * S + v0, nv, d[c]);
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      m[j] = d[0][j];
      s[j] = 0.f;
      sum_a[j] = 0.f;
    }
#pragma unroll
    for (int c = 1; c < CR; ++c)
      if (c < C)
#pragma unroll
        for (int j = 0; j < VPL; ++j) m[j] = fmaxf(m[j], d[c][j]);
#pragma unroll
    for (int c = 0; c < CR; ++c)
      if (c < C)
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
          const float dd = d[c][j] - m[j], ee = expf(dd);
          s[j] += ee;
          d[c][j] = GM == 0 ? ee : dd;
        }
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      m[j] = logf(s[j]);
      s[j] = 1.f / s[j];
    }
#pragma unroll
    for (int c = 0; c < CR; ++c)
      if (c < C) {
        float tt[VPL];
        row_load<VPL>(tn + c * S + v0, nv, tt);
        const FtCoef k = coef[c];
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
          float p;
          ft_logits_terms<GM>(d[c][j], m[j], s[j], tt[j], k, gamma, gi, p, a[c][j]);
          sum_a[j] += a[c][j];
          d[c][j] = p;
        }
      }
#pragma unroll
    for (int c = 0; c < CR; ++c)
      if (c < C) {
        float o[VPL];
#pragma unroll
        for (int j = 0; j < VPL; ++j) o[j] = fmaf(-d[c][j], sum_a[j], a[c][j]);
        row_store<VPL>(on + c * S + v0, nv, o);
      }
  }
}

// LOGITS, C > FT_CREG: the planes are read three times more (max, sum of exp, sum of a) before the pass that writes
template <int GM>
__global__ __launch_bounds__(256) void ft_logits_bwd_reread_kernel(const float* __restrict__ z, const float* __restrict__ t,
                                                                   const float* __restrict__ sums,
                                                                   const float* __restrict__ dloss,
                                                                   const float* __restrict__ focal_w,
                                                                   const float* __restrict__ tversky_w, float* __restrict__ dz,
                                                                   int N, int C, int64_t S, float tversky_weight, float alpha,
                                                                   float beta, float power, float gamma, int gi) {
  const int64_t n = blockIdx.y;
  const float* zn = z + n * C * S;
  const float* tn = t + n * C * S;
  float* on = dz + n * C * S;
  const int64_t begin = (int64_t)blockIdx.x * FT_LCHUNK, end = min(S, begin + FT_LCHUNK);
  const float g = dloss[0], inv_nc = 1.f / (float)(N * C), inv_s = 1.f / (float)S;
  float m[FT_IT][4], ls[FT_IT][4], inv[FT_IT][4], sum_a[FT_IT][4];
  int nv[FT_IT];
#pragma unroll
  for (int it = 0; it < FT_IT; ++it) {
    const int64_t v0 = begin + (it * 256 + threadIdx.x) * 4;
    nv[it] = row_valid(v0, end, 4);
    float v[4];
    row_load<4>(zn + v0, nv[it], m[it]);
    for (int c = 1; c < C; ++c) {
      row_load<4>(zn + c * S + v0, nv[it], v);
#pragma unroll
      for (int j = 0; j < 4; ++j) m[it][j] = fmaxf(m[it][j], v[j]);
    }
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < C; ++c) {
      row_load<4>(zn + c * S + v0, nv[it], v);
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] += expf(v[j] - m[it][j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ls[it][j] = logf(s[j]);
      inv[it][j] = 1.f / s[j];
      sum_a[it][j] = 0.f;
    }
  }
  for (int pass = 0; pass < 2; ++pass)
    for (int c = 0; c < C; ++c) {
      const FtCoef k = ft_coef(sums, n * C + c, c, focal_w, tversky_w, g, inv_nc, inv_s, tversky_weight, alpha, beta, power);
#pragma unroll
      for (int it = 0; it < FT_IT; ++it) {
        const int64_t v0 = begin + (it * 256 + threadIdx.x) * 4;
        float zz[4], tt[4], o[4];
        row_load<4>(zn + c * S + v0, nv[it], zz);
        row_load<4>(tn + c * S + v0, nv[it], tt);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float dd = zz[j] - m[it][j];
          float p, a;
          ft_logits_terms<GM>(GM == 0 ? expf(dd) : dd, ls[it][j], inv[it][j], tt[j], k, gamma, gi, p, a);
          if (pass == 0) sum_a[it][j] += a;
          o[j] = fmaf(-p, sum_a[it][j], a);
        }
        if (pass == 1) row_store<4>(on + c * S + v0, nv[it], o);
      }
    }
}

// gamma == 0, gamma in {1, 2, 3}, any other gamma >= 1
static inline int focal_mode(float gamma, int& gi) {
  gi = 0;
  if (gamma == 0.f) return 0;
  if (gamma == 1.f || gamma == 2.f || gamma == 3.f) {
    gi = (int)gamma;
    return 1;
  }
  return 2;
}

static int ft_check_params(const char* what, float alpha, float beta, float power, float gamma) {
  M355_REQUIRE(std::isfinite(alpha) && alpha >= 0.f && std::isfinite(beta) && beta >= 0.f, M355_EINVALID_ARG,
               "%s: alpha and beta must be finite and >= 0", what);
  M355_REQUIRE(std::isfinite(power) && power > 0.f, M355_EINVALID_ARG, "%s: tversky_power must be finite and > 0", what);
  M355_REQUIRE(std::isfinite(gamma) && (gamma == 0.f || gamma >= 1.f), M355_EINVALID_ARG,
               "%s: focal_gamma must be 0 or >= 1", what);
  return M355_OK;
}

using FtFwdLogitsK = void (*)(const float*, const float*, double*, int, int64_t, int, float, int);
using FtBwdK = void (*)(const float*, const float*, const float*, const float*, const float*, const float*, float*, int, int,
                        int64_t, float, float, float, float, float, int);

// the instantiation of focal mode gm
template <int CR, int VPL>
static FtFwdLogitsK ft_fwd_logits(int gm) {
  return gm == 0 ? ft_logits_partial_kernel<CR, VPL, 0> : gm == 1 ? ft_logits_partial_kernel<CR, VPL, 1>
                                                                   : ft_logits_partial_kernel<CR, VPL, 2>;
}
template <int CR, int VPL>
static FtBwdK ft_bwd_logits(int gm) {
  return gm == 0 ? ft_logits_bwd_kernel<CR, VPL, 0> : gm == 1 ? ft_logits_bwd_kernel<CR, VPL, 1>
                                                               : ft_logits_bwd_kernel<CR, VPL, 2>;
}

}  // namespace m355

using namespace m355;

extern "C" size_t m355_focal_tversky_workspace(int32_t N, int32_t C, int64_t S) {
  return loss_workspace_bytes(N, C, S, FT_LCHUNK, 4);
}

extern "C" int m355_focal_tversky_fwd(const float* x, const float* t, int32_t N, int32_t C, int64_t S, float tversky_weight,
                                      float alpha, float beta, float tversky_power, float focal_gamma,
                                      const float* focal_class_weights, const float* tversky_class_weights,
                                      int32_t from_logits, float* out3, float* sums, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  M355_REQUIRE(x && t && out3 && sums && workspace, M355_EINVALID_ARG, "focal_tversky_fwd: null pointer");
  // (the parameters before the sizes: both are M355_EINVALID_ARG, and the row count's M355_EUNSUPPORTED comes after them)
  if (int rc = ft_check_params("focal_tversky_fwd", alpha, beta, tversky_power, focal_gamma)) return rc;
  if (int rc = loss_check("focal_tversky_fwd", N, C, S)) return rc;
  M355_REQUIRE(workspace_bytes >= m355_focal_tversky_workspace(N, C, S), M355_EWORKSPACE,
               "focal_tversky_fwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)workspace;
  int gi;
  const int gm = focal_mode(focal_gamma, gi);
  int nblk;
  if (from_logits) {
    nblk = (int)ceil_div(S, FT_LCHUNK);
    const dim3 grid((unsigned)nblk, (unsigned)N);
    const FtFwdLogitsK k = C <= 4 ? ft_fwd_logits<4, 4>(gm) : C <= 8 ? ft_fwd_logits<8, 4>(gm)
                           : C <= FT_CREG ? ft_fwd_logits<16, 2>(gm)
                           : gm == 0 ? ft_logits_partial_reread_kernel<0>
                           : gm == 1 ? ft_logits_partial_reread_kernel<1> : ft_logits_partial_reread_kernel<2>;
    hipLaunchKernelGGL(k, grid, dim3(256), 0, st, x, t, partial, (int)C, S, nblk, focal_gamma, gi);
  } else {
    nblk = (int)ceil_div(S, FT_PCHUNK);
    const dim3 grid((unsigned)nblk, (unsigned)(N * C));
    using K = void (*)(const float*, const float*, double*, int64_t, int, float, int);
    const K k = gm == 0 ? ft_prob_partial_kernel<0> : gm == 1 ? ft_prob_partial_kernel<1> : ft_prob_partial_kernel<2>;
    hipLaunchKernelGGL(k, grid, dim3(256), 0, st, x, t, partial, S, nblk, focal_gamma, gi);
  }
  int lanes = 1;
  while (lanes < 64 && lanes < nblk) lanes *= 2;
  hipLaunchKernelGGL(ft_finalize_kernel, dim3(1), dim3(256), 0, st, partial, focal_class_weights, tversky_class_weights, sums,
                     out3, (int)N, (int)C, S, nblk, lanes, tversky_weight, alpha, beta, tversky_power);
  return check_launch("focal_tversky_fwd");
}

extern "C" int m355_focal_tversky_bwd(const float* x, const float* t, const float* sums, const float* dloss, int32_t N,
                                      int32_t C, int64_t S, float tversky_weight, float alpha, float beta, float tversky_power,
                                      float focal_gamma, const float* focal_class_weights, const float* tversky_class_weights,
                                      int32_t from_logits, float* dx, void* stream) {
  M355_REQUIRE(x && t && sums && dloss && dx, M355_EINVALID_ARG, "focal_tversky_bwd: null pointer");
  // (the parameters before the sizes: both are M355_EINVALID_ARG, and the row count's M355_EUNSUPPORTED comes after them)
  if (int rc = ft_check_params("focal_tversky_bwd", alpha, beta, tversky_power, focal_gamma)) return rc;
  if (int rc = loss_check("focal_tversky_bwd", N, C, S)) return rc;
  hipStream_t st = (hipStream_t)stream;
  int gi;
  const int gm = focal_mode(focal_gamma, gi);
  FtBwdK k;
  dim3 grid;
  if (from_logits) {
    grid = dim3((unsigned)ceil_div(S, FT_LCHUNK), (unsigned)N);
    k = C <= 4 ? ft_bwd_logits<4, 4>(gm) : C <= 8 ? ft_bwd_logits<8, 4>(gm) : C <= FT_CREG ? ft_bwd_logits<16, 2>(gm)
        : gm == 0 ? ft_logits_bwd_reread_kernel<0> : gm == 1 ? ft_logits_bwd_reread_kernel<1> : ft_logits_bwd_reread_kernel<2>;
  } else {
    grid = loss_bwd_grid(S, 2048, N * C);
    k = gm == 0 ? ft_prob_bwd_kernel<0> : gm == 1 ? ft_prob_bwd_kernel<1> : ft_prob_bwd_kernel<2>;
  }
  hipLaunchKernelGGL(k, grid, dim3(256), 0, st, x, t, sums, dloss, focal_class_weights, tversky_class_weights, dx, (int)N,
                     (int)C, S, tversky_weight, alpha, beta, tversky_power, focal_gamma, gi);
  return check_launch("focal_tversky_bwd");
}
