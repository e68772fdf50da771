// GroupNorm / BatchNorm3d + activation, forward and backward (HBM-bound).
//
// Reference ops replaced: normalization_class(out_channels) and
// activation_class() inside Block3d (models/components.py:52-55): nn.BatchNorm3d
// by default, nn.GroupNorm through functools.partial (the north-star config).
//
// A "statistic" s is a mean/rstd pair:
//   BN : s = channel c,          data = N runs of S contiguous floats
//   GN : s = n*groups + g,       data = 1 run of (C/groups)*S contiguous floats
// Pass 1 (stats): blocks reduce chunks to (sum, sumsq) in fp32 per thread over
// short runs, combined in double -> partial[s][blk][2]; a finalize kernel sums
// the partials in fixed order.  Pass 2 (apply): float4 streaming, one (n,c)
// channel chunk per block so gamma/beta/mean/rstd are block-uniform.
#include "norm_host.hpp"
#include "activation.hpp"

namespace m355 {

__device__ __forceinline__ int64_t stat_base(int64_t s, int64_t run, int groups, int C, int64_t S,
                                             int64_t xbs, int64_t len) {
  if (groups == 0) return run * xbs + s * S;  // BN: s = channel, run = n
  const int64_t n = s / groups, g = s % groups;
  return n * xbs + g * len;
}

// partial[(s*nblk + b)*2 + {0,1}] = (sum, sumsq) of chunk b of statistic s
// VEC: len % 4 == 0 and 16-byte aligned runs, so a float4 never straddles a run.
template <bool VEC>
__global__ __launch_bounds__(256) void norm_partial_kernel(const float* __restrict__ x,
                                                           double* __restrict__ partial,
                                                           int groups, int C, int64_t S,
                                                           int64_t xbs, int64_t runs, int64_t len,
                                                           int nblk) {
  __shared__ double scratch[4];
  const int64_t s = blockIdx.y;
  const int b = blockIdx.x;
  const int64_t count = runs * len;
  const int64_t begin = (int64_t)b * NORM_CHUNK;
  const int64_t end = min(count, begin + NORM_CHUNK);
  constexpr int STEP = VEC ? 4 : 1;
  float s1 = 0.f, s2 = 0.f;
  // one division per thread, then incremental (run, off) bookkeeping
  int64_t i = begin + (int64_t)threadIdx.x * STEP;
  int64_t run = i / len, off = i - run * len;
  for (; i < end; i += 256 * STEP) {
    const float* p = x + stat_base(s, run, groups, C, S, xbs, len) + off;
    if (VEC) {
      const float4 v = *reinterpret_cast<const float4*>(p);
      s1 += (v.x + v.y) + (v.z + v.w);
      s2 = fmaf(v.x, v.x, s2); s2 = fmaf(v.y, v.y, s2);
      s2 = fmaf(v.z, v.z, s2); s2 = fmaf(v.w, v.w, s2);
    } else {
      const float v = *p;
      s1 += v;
      s2 = fmaf(v, v, s2);
    }
    off += 256 * STEP;
    while (off >= len) { off -= len; ++run; }
  }
  const double t1 = block_sum<double, 256>((double)s1, scratch);
  const double t2 = block_sum<double, 256>((double)s2, scratch);
  if (threadIdx.x == 0) {
    partial[((int64_t)s * nblk + b) * 2 + 0] = t1;
    partial[((int64_t)s * nblk + b) * 2 + 1] = t2;
  }
}

// one wave (64 lanes) per statistic: lanes stride over the partials, fixed-order shuffle tree
__global__ __launch_bounds__(64) void norm_finalize_kernel(const double* __restrict__ partial, float* __restrict__ mean,
                                     float* __restrict__ rstd, float* __restrict__ running_mean,
                                     float* __restrict__ running_var, float momentum, float eps,
                                     int64_t nstats, int nblk, int64_t count, const double* __restrict__ count_ptr) {
  const int64_t s = blockIdx.x;
  if (count_ptr) count = (int64_t)count_ptr[0];   // synchronised batch norm: the element count summed over the ranks
  double t1 = 0.0, t2 = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 64) {
    t1 += partial[(s * nblk + b) * 2 + 0];
    t2 += partial[(s * nblk + b) * 2 + 1];
  }
  t1 = wave_sum(t1);
  t2 = wave_sum(t2);
  if (threadIdx.x != 0) return;
  const double m = t1 / (double)count;
  double var = t2 / (double)count - m * m;
  if (var < 0.0) var = 0.0;
  mean[s] = (float)m;
  rstd[s] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean) running_mean[s] = (1.f - momentum) * running_mean[s] + momentum * (float)m;
  if (running_var) {
    const double unbiased = count > 1 ? var * (double)count / (double)(count - 1) : var;
    running_var[s] = (1.f - momentum) * running_var[s] + momentum * (float)unbiased;
  }
}

// Synchronised batch norm, local half: sums[s][2] = (sum x, sum x^2) of statistic s in double (one wave per statistic,
// fixed order), sums[nstats*2] = the local element count.  The ranks all-reduce this buffer (SUM) and finalize from it.
__global__ __launch_bounds__(64) void norm_sums_kernel(const double* __restrict__ partial, double* __restrict__ sums,
                                                        int64_t nstats, int nblk, int64_t count) {
  const int64_t s = blockIdx.x;
  double t1 = 0.0, t2 = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 64) {
    t1 += partial[(s * nblk + b) * 2 + 0];
    t2 += partial[(s * nblk + b) * 2 + 1];
  }
  t1 = wave_sum(t1);
  t2 = wave_sum(t2);
  if (threadIdx.x != 0) return;
  sums[s * 2 + 0] = t1;
  sums[s * 2 + 1] = t2;
  if (s == 0) sums[nstats * 2] = (double)count;
}

// statistics from the conv epilogue partials part[n][slot][C][2] (float), stage 1: block (b, s) sums a
// contiguous share of the (sample, slot, channel-in-group) items of statistic s in a fixed order
// (double) -> partial[(s*nblk + b)*2 + {0,1}]; norm_finalize_kernel then combines the nblk partials.
__global__ __launch_bounds__(256) void norm_from_partials_kernel(
    const float* __restrict__ part, double* __restrict__ partial, int groups, int N, int C, int64_t slots,
    int nblk) {
  __shared__ double scratch[4];
  const int64_t s = blockIdx.y;
  const int b = blockIdx.x;
  // GN: s = n*groups + g -> sample n, channels [g*cg, (g+1)*cg); BN: s = channel, all samples
  const int cg = groups == 0 ? 1 : C / groups;
  const int c_begin = groups == 0 ? (int)s : (int)(s % groups) * cg;
  const int64_t n_begin = groups == 0 ? 0 : s / groups, runs = groups == 0 ? N : 1;
  const int64_t per_n = slots * cg, items = runs * per_n;
  const int64_t share = (items + nblk - 1) / nblk;
  const int64_t begin = (int64_t)b * share, end = min(items, begin + share);
  double t1 = 0.0, t2 = 0.0;
  for (int64_t i = begin + threadIdx.x; i < end; i += 256) {
    const int64_t run = i / per_n, j = i - run * per_n;
    const int64_t slot = j / cg;
    const int c = c_begin + (int)(j - slot * cg);
    const float2 v = *reinterpret_cast<const float2*>(part + (((n_begin + run) * slots + slot) * C + c) * 2);
    t1 += (double)v.x;
    t2 += (double)v.y;
  }
  t1 = block_sum<double, 256>(t1, scratch);
  t2 = block_sum<double, 256>(t2, scratch);
  if (threadIdx.x == 0) {
    partial[((int64_t)s * nblk + b) * 2 + 0] = t1;
    partial[((int64_t)s * nblk + b) * 2 + 1] = t2;
  }
}

// The same for statistics with few partial items (<= 8192: every level below 64^3 of a U-Net), finalize included:
// one block per statistic sums ALL its items and writes mean / rstd (and the BatchNorm running statistics) itself,
// so the pair of latency-bound launches (~8 + ~5 us) is one.
__global__ __launch_bounds__(1024) void norm_from_partials_final_kernel(
    const float* __restrict__ part, float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ running_mean,
    float* __restrict__ running_var, float momentum, float eps, int groups, int N, int C, int64_t slots, int64_t count) {
  __shared__ double scratch[16];   // 1024 threads: the pass is a latency chain, 8 items per thread keep it short
  const int64_t s = blockIdx.x;
  const int cg = groups == 0 ? 1 : C / groups;
  const int c_begin = groups == 0 ? (int)s : (int)(s % groups) * cg;
  const int64_t n_begin = groups == 0 ? 0 : s / groups, runs = groups == 0 ? N : 1;
  const int64_t per_n = slots * cg, items = runs * per_n;
  double t1 = 0.0, t2 = 0.0;
  for (int64_t i = threadIdx.x; i < items; i += 1024) {
    const int64_t run = i / per_n, j = i - run * per_n;
    const int64_t slot = j / cg;
    const int c = c_begin + (int)(j - slot * cg);
    const float2 v = *reinterpret_cast<const float2*>(part + (((n_begin + run) * slots + slot) * C + c) * 2);
    t1 += (double)v.x;
    t2 += (double)v.y;
  }
  t1 = block_sum<double, 1024>(t1, scratch);
  t2 = block_sum<double, 1024>(t2, scratch);
  if (threadIdx.x != 0) return;
  const double m = t1 / (double)count;
  double var = t2 / (double)count - m * m;
  if (var < 0.0) var = 0.0;
  mean[s] = (float)m;
  rstd[s] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean) running_mean[s] = (1.f - momentum) * running_mean[s] + momentum * (float)m;
  if (running_var) {
    const double unbiased = count > 1 ? var * (double)count / (double)(count - 1) : var;
    running_var[s] = (1.f - momentum) * running_var[s] + momentum * (float)unbiased;
  }
}

__global__ void norm_from_running_kernel(const float* __restrict__ rm, const float* __restrict__ rv,
                                         float* __restrict__ mean, float* __restrict__ rstd,
                                         float eps, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  mean[c] = rm[c];
  rstd[c] = 1.f / sqrtf(rv[c] + eps);
}

// grid: (chunks over S, C, N).  y = act((x-mean)*rstd*gamma + beta) + add
template <bool VEC, bool SMOOTH>
__global__ __launch_bounds__(256) void norm_act_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ add,
    float* __restrict__ y, int C, int64_t S, int groups, int act, float slope, int64_t xbs,
    int64_t ybs, int64_t abs_) {
  const int c = blockIdx.y, n = blockIdx.z;
  const int64_t s = groups == 0 ? c : (int64_t)n * groups + c / (C / groups);
  const float m = mean[s], r = rstd[s];
  const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
  const float sc = r * g;
  const float sh = b - m * sc;
  const float* xp = x + (int64_t)n * xbs + (int64_t)c * S;
  float* yp = y + (int64_t)n * ybs + (int64_t)c * S;
  const float* ap = add ? add + (int64_t)n * abs_ + (int64_t)c * S : nullptr;
  if (VEC) {
    const int64_t S4 = S >> 2;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < S4; i += gridDim.x * 256ll) {
      float4 v = reinterpret_cast<const float4*>(xp)[i];
      v.x = act_fwd<SMOOTH>(fmaf(v.x, sc, sh), act, slope);
      v.y = act_fwd<SMOOTH>(fmaf(v.y, sc, sh), act, slope);
      v.z = act_fwd<SMOOTH>(fmaf(v.z, sc, sh), act, slope);
      v.w = act_fwd<SMOOTH>(fmaf(v.w, sc, sh), act, slope);
      if (ap) {
        const float4 a = reinterpret_cast<const float4*>(ap)[i];
        v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
      }
      reinterpret_cast<float4*>(yp)[i] = v;
    }
  } else {
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < S; i += gridDim.x * 256ll) {
      float v = act_fwd<SMOOTH>(fmaf(xp[i], sc, sh), act, slope);
      if (ap) v += ap[i];
      yp[i] = v;
    }
  }
}

// The same pass with nn.AvgPool3d(2, 2) of the result as a SECOND output (models/modular_unet.py:90-92: an encoder
// block's output continues both into the skip connection and, pooled, into the next level): one thread per pooled
// voxel normalises + activates its 2x2x2 window (four 8-byte row pairs), stores the eight values and their mean --
// the pool's own pass over the activated tensor (a full re-read of the level) disappears.  Summation order and the
// normalise expression are those of avgpool2_fwd_kernel / norm_act_fwd_kernel: bit-identical to the two-pass result.
// grid: (chunks over pooled voxels, C, N)
template <bool SMOOTH>
__global__ __launch_bounds__(256) void norm_act_pool_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ y, float* __restrict__ pooled,
    int C, int D, int H, int W, int groups, int act, float slope, int64_t xbs, int64_t ybs, int64_t pbs) {
  const int c = blockIdx.y, n = blockIdx.z;
  const int64_t s = groups == 0 ? c : (int64_t)n * groups + c / (C / groups);
  const float m = mean[s], r = rstd[s];
  const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
  const float sc = r * g;
  const float sh = b - m * sc;
  const int OD = D / 2, OH = H / 2, OW = W / 2;
  const int64_t S = (int64_t)D * H * W, OS = (int64_t)OD * OH * OW;
  const float* xp = x + (int64_t)n * xbs + (int64_t)c * S;
  float* yp = y + (int64_t)n * ybs + (int64_t)c * S;
  float* pp = pooled + (int64_t)n * pbs + (int64_t)c * OS;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < OS; i += gridDim.x * 256ll) {
    const int ox = (int)(i % OW);
    const int64_t t = i / OW;
    const int oy = (int)(t % OH), oz = (int)(t / OH);
    const int64_t r00 = ((int64_t)(2 * oz) * H + 2 * oy) * W + 2 * ox;
    const int64_t off[4] = {r00, r00 + W, r00 + (int64_t)H * W, r00 + (int64_t)H * W + W};
    float2 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const float2*>(xp + off[q]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[q].x = act_fwd<SMOOTH>(fmaf(v[q].x, sc, sh), act, slope);
      v[q].y = act_fwd<SMOOTH>(fmaf(v[q].y, sc, sh), act, slope);
      *reinterpret_cast<float2*>(yp + off[q]) = v[q];
    }
    pp[i] = (((((((v[0].x + v[0].y) + v[1].x) + v[1].y) + v[2].x) + v[2].y) + v[3].x) + v[3].y) * 0.125f;
  }
}

// Backward pass 1: per (n,c) partial sums A = sum g, B = sum g*xhat with
// g = dy * act'(pre).  partial[((n*C + c)*nblk + b)*2 + {0,1}]
template <bool VEC, bool SMOOTH>
__global__ __launch_bounds__(256) void norm_bwd_partial_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
    double* __restrict__ partial, int C, int64_t S, int groups, int act, float slope, int64_t xbs,
    int64_t ybs, int nblk) {
  __shared__ double scratch[4];
  const int b = blockIdx.x, c = blockIdx.y, n = blockIdx.z;
  const int64_t s = groups == 0 ? c : (int64_t)n * groups + c / (C / groups);
  const float m = mean[s], r = rstd[s];
  const float g = gamma ? gamma[c] : 1.f, bt = beta ? beta[c] : 0.f;
  const float* xp = x + (int64_t)n * xbs + (int64_t)c * S;
  const float* dp = dy + (int64_t)n * ybs + (int64_t)c * S;
  const int64_t begin = (int64_t)b * NORM_CHUNK, end = min(S, begin + NORM_CHUNK);
  float a1 = 0.f, a2 = 0.f;
  const float sc = r * g, sh = bt - m * sc;  // same expression as the forward pass
  auto acc = [&](float xv, float dv) {
    const float xh = (xv - m) * r;
    const float pre = fmaf(xv, sc, sh);
    const float gg = dv * act_grad<SMOOTH>(pre, act, slope);
    a1 += gg;
    a2 = fmaf(gg, xh, a2);
  };
  if (VEC) {
    for (int64_t i = begin + threadIdx.x * 4; i < end; i += 1024) {
      const float4 xv = *reinterpret_cast<const float4*>(xp + i);
      const float4 dv = *reinterpret_cast<const float4*>(dp + i);
      acc(xv.x, dv.x); acc(xv.y, dv.y); acc(xv.z, dv.z); acc(xv.w, dv.w);
    }
  } else {
    for (int64_t i = begin + threadIdx.x; i < end; i += 256) acc(xp[i], dp[i]);
  }
  const double t1 = block_sum<double, 256>((double)a1, scratch);
  const double t2 = block_sum<double, 256>((double)a2, scratch);
  if (threadIdx.x == 0) {
    const int64_t o = (((int64_t)n * C + c) * nblk + b) * 2;
    partial[o] = t1;
    partial[o + 1] = t2;
  }
}

// Both finalize stages in one launch (one wave per block index s; every sum in a fixed lane-strided order + the
// fixed shuffle tree of wave_sum): for s < nstats the per-statistic means m1 = mean(dxhat), m2 = mean(dxhat * xhat)
// straight from the per-block partials, for s < C the parameter gradients dgamma[c] = sum_n B, dbeta[c] = sum_n A.
// These launches are latency-bound (~5 us each between two bandwidth-bound passes), so one instead of two is
// 108 launches less per cfg2 train step.
__global__ __launch_bounds__(64) void norm_bwd_reduce_kernel(const double* __restrict__ partial,
                                                              const float* __restrict__ gamma, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta, float* __restrict__ stat_m, int N,
                                                              int C, int groups, int nblk, int64_t count, int training,
                                                              const double* __restrict__ count_ptr, float grad_unscale,
                                                              int* __restrict__ oflag) {
  // synchronised batch norm: divide by the element count over all ranks; the SUM all-reduce of stat_m is then the mean
  if (count_ptr) count = (int64_t)count_ptr[0];
  const int64_t nstats = groups == 0 ? C : (int64_t)N * groups;
  const int64_t s = blockIdx.x;
  const int lane = threadIdx.x;
  if (s < nstats) {
    double m1 = 0.0, m2 = 0.0;
    if (training) {
      if (groups == 0) {
        const int c = (int)s;
        const int64_t items = (int64_t)N * nblk;
        for (int64_t i = lane; i < items; i += 64) {
          const int64_t n = i / nblk, k = i - n * nblk;
          m1 += partial[((n * C + c) * nblk + k) * 2];
          m2 += partial[((n * C + c) * nblk + k) * 2 + 1];
        }
        const double g = gamma ? (double)gamma[c] : 1.0;
        m1 *= g;
        m2 *= g;
      } else {
        const int cpg = C / groups;
        const int64_t n = s / groups;
        const int c0 = (int)(s % groups) * cpg;
        const int64_t items = (int64_t)cpg * nblk;
        for (int64_t i = lane; i < items; i += 64) {
          const int cc = (int)(i / nblk);
          const int64_t k = i - (int64_t)cc * nblk;
          const double g = gamma ? (double)gamma[c0 + cc] : 1.0;
          m1 += g * partial[((n * C + c0 + cc) * nblk + k) * 2];
          m2 += g * partial[((n * C + c0 + cc) * nblk + k) * 2 + 1];
        }
      }
      m1 = wave_sum(m1);
      m2 = wave_sum(m2);
    }
    if (lane == 0) {
      stat_m[s * 2 + 0] = (float)(m1 / (double)count);
      stat_m[s * 2 + 1] = (float)(m2 / (double)count);
    }
  }
  if (s < C && (dgamma || dbeta)) {
    const int c = (int)s;
    double a = 0.0, bb = 0.0;
    const int64_t items = (int64_t)N * nblk;
    for (int64_t i = lane; i < items; i += 64) {
      const int64_t n = i / nblk, k = i - n * nblk;
      a += partial[((n * C + c) * nblk + k) * 2];
      bb += partial[((n * C + c) * nblk + k) * 2 + 1];
    }
    a = wave_sum(a);
    bb = wave_sum(bb);
    if (lane == 0) {
      // grad_unscale: 1 except in the fp16 training flow, whose activation gradients travel multiplied by a power of
      // two (loss scaling); the parameter gradients leave in true units
      if (dbeta) dbeta[c] = (float)(a * (double)grad_unscale);
      if (dgamma) dgamma[c] = (float)(bb * (double)grad_unscale);
      report_nonfinite((float)(a * (double)grad_unscale), oflag);
      report_nonfinite((float)(bb * (double)grad_unscale), oflag);
    }
  }
}

// Backward pass 2: dx = rstd * (g*gamma - m1 - xhat*m2)
template <bool VEC, bool SMOOTH>
__global__ __launch_bounds__(256) void norm_bwd_apply_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ stat_m, float* __restrict__ dx, int C, int64_t S, int groups, int act,
    float slope, int64_t xbs, int64_t ybs) {
  const int c = blockIdx.y, n = blockIdx.z;
  const int64_t s = groups == 0 ? c : (int64_t)n * groups + c / (C / groups);
  const float m = mean[s], r = rstd[s];
  const float g = gamma ? gamma[c] : 1.f, bt = beta ? beta[c] : 0.f;
  const float m1 = stat_m[s * 2], m2 = stat_m[s * 2 + 1];
  const float* xp = x + (int64_t)n * xbs + (int64_t)c * S;
  const float* dp = dy + (int64_t)n * ybs + (int64_t)c * S;
  float* op = dx + (int64_t)n * xbs + (int64_t)c * S;
  const float sc = r * g, sh = bt - m * sc;  // same expression as the forward pass
  auto f = [&](float xv, float dv) {
    const float xh = (xv - m) * r;
    const float pre = fmaf(xv, sc, sh);
    const float gg = dv * act_grad<SMOOTH>(pre, act, slope) * g;
    return r * (gg - m1 - xh * m2);
  };
  if (VEC) {
    const int64_t S4 = S >> 2;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < S4; i += gridDim.x * 256ll) {
      const float4 xv = reinterpret_cast<const float4*>(xp)[i];
      const float4 dv = reinterpret_cast<const float4*>(dp)[i];
      float4 o;
      o.x = f(xv.x, dv.x); o.y = f(xv.y, dv.y); o.z = f(xv.z, dv.z); o.w = f(xv.w, dv.w);
      reinterpret_cast<float4*>(op)[i] = o;
    }
  } else {
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < S; i += gridDim.x * 256ll)
      op[i] = f(xp[i], dp[i]);
  }
}

// ---- the backward of a block whose output also went through nn.AvgPool3d(2, 2) (norm_act_pool_fwd_kernel) ----
// The gradient of the activated tensor is the skip-path gradient (may be absent) plus the un-pooled gradient of the
// pooled output.  avgpool2_bwd_kernel forms that sum and writes it so that the two passes above can read it back; the
// POOL kernels below form it in registers instead, with that kernel's expression (skip + dpool * 0.125f; the product
// is exact, so contraction cannot change it), and the pass over the level that wrote and re-read it is gone.
// One channel's sources; offsets within a channel fit 32 bits (the entry point checks S).
struct PoolGradSrc {
  const float* ds;   // dskip of this (n, c), null: no skip gradient
  const float* dp;   // dpool of this (n, c): [D/2][H/2][W/2]
  uint32_t W, HW, OW, OHW;
  __device__ __forceinline__ uint32_t pooled(uint32_t i) const {
    const uint32_t z = i / HW, rem = i - z * HW;
    const uint32_t y = rem / W, xw = rem - y * W;
    return (z >> 1) * OHW + (y >> 1) * OW + (xw >> 1);
  }
  __device__ __forceinline__ float one(uint32_t i) const {
    const float g = dp[pooled(i)] * 0.125f;
    return ds ? ds[i] + g : g;
  }
  // elements i .. i+3, i % 4 == 0.  GVEC: W % 4 == 0 (the four share a row and two pooled voxels) and ds 16-byte aligned
  template <bool GVEC>
  __device__ __forceinline__ float4 four(uint32_t i) const {
    if (GVEC) {
      const uint32_t q = pooled(i);
      const float g0 = dp[q] * 0.125f, g1 = dp[q + 1] * 0.125f;
      if (!ds) return make_float4(g0, g0, g1, g1);
      const float4 a = *reinterpret_cast<const float4*>(ds + i);
      return make_float4(a.x + g0, a.y + g0, a.z + g1, a.w + g1);
    }
    return make_float4(one(i), one(i + 1), one(i + 2), one(i + 3));
  }
};

__device__ __forceinline__ PoolGradSrc pool_grad_src(const float* dskip, int64_t dsbs, const float* dpool, int64_t dpbs,
                                                     int n, int c, int64_t S, int H, int W) {
  PoolGradSrc g;
  g.ds = dskip ? dskip + (int64_t)n * dsbs + (int64_t)c * S : nullptr;
  g.dp = dpool + (int64_t)n * dpbs + (int64_t)c * (S >> 3);
  g.W = (uint32_t)W;
  g.HW = (uint32_t)H * (uint32_t)W;
  g.OW = (uint32_t)W >> 1;
  g.OHW = ((uint32_t)H >> 1) * g.OW;
  return g;
}

// norm_bwd_partial_kernel on that sum.  MAP4 is the element-to-thread mapping of its VEC variant (four consecutive
// elements per thread), chosen by the host exactly where the two-step form would have run VEC on the dense sum, and
// the accumulation order within a thread is the same: the partials are bit-identical to the two-step form whether the
// gradient sources allow vector loads (GVEC) or not.
template <bool MAP4, bool GVEC, bool SMOOTH>
__global__ __launch_bounds__(256) void norm_bwd_partial_pool_kernel(
    const float* __restrict__ x, const float* __restrict__ dskip, const float* __restrict__ dpool,
    const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, double* __restrict__ partial, int C, int64_t S, int H, int W, int groups, int act,
    float slope, int64_t xbs, int64_t dsbs, int64_t dpbs, int nblk) {
  __shared__ double scratch[4];
  const int b = blockIdx.x, c = blockIdx.y, n = blockIdx.z;
  const int64_t s = groups == 0 ? c : (int64_t)n * groups + c / (C / groups);
  const float m = mean[s], r = rstd[s];
  const float g = gamma ? gamma[c] : 1.f, bt = beta ? beta[c] : 0.f;
  const float* xp = x + (int64_t)n * xbs + (int64_t)c * S;
  const PoolGradSrc src = pool_grad_src(dskip, dsbs, dpool, dpbs, n, c, S, H, W);
  const int64_t begin = (int64_t)b * NORM_CHUNK, end = min(S, begin + NORM_CHUNK);
  float a1 = 0.f, a2 = 0.f;
  const float sc = r * g, sh = bt - m * sc;  // same expression as the forward pass
  auto acc = [&](float xv, float dv) {
    const float xh = (xv - m) * r;
    const float pre = fmaf(xv, sc, sh);
    const float gg = dv * act_grad<SMOOTH>(pre, act, slope);
    a1 += gg;
    a2 = fmaf(gg, xh, a2);
  };
  if (MAP4) {
    for (int64_t i = begin + threadIdx.x * 4; i < end; i += 1024) {
      const float4 xv = *reinterpret_cast<const float4*>(xp + i);
      const float4 dv = src.four<GVEC>((uint32_t)i);
      acc(xv.x, dv.x); acc(xv.y, dv.y); acc(xv.z, dv.z); acc(xv.w, dv.w);
    }
  } else {
    for (int64_t i = begin + threadIdx.x; i < end; i += 256) acc(xp[i], src.one((uint32_t)i));
  }
  const double t1 = block_sum<double, 256>((double)a1, scratch);
  const double t2 = block_sum<double, 256>((double)a2, scratch);
  if (threadIdx.x == 0) {
    const int64_t o = (((int64_t)n * C + c) * nblk + b) * 2;
    partial[o] = t1;
    partial[o + 1] = t2;
  }
}

// norm_bwd_apply_kernel on that sum (element-wise: any mapping gives the same dx; MAP4 also asks for an aligned dx)
template <bool MAP4, bool GVEC, bool SMOOTH>
__global__ __launch_bounds__(256) void norm_bwd_apply_pool_kernel(
    const float* __restrict__ x, const float* __restrict__ dskip, const float* __restrict__ dpool,
    const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ stat_m, float* __restrict__ dx, int C, int64_t S, int H,
    int W, int groups, int act, float slope, int64_t xbs, int64_t dsbs, int64_t dpbs) {
  const int c = blockIdx.y, n = blockIdx.z;
  const int64_t s = groups == 0 ? c : (int64_t)n * groups + c / (C / groups);
  const float m = mean[s], r = rstd[s];
  const float g = gamma ? gamma[c] : 1.f, bt = beta ? beta[c] : 0.f;
  const float m1 = stat_m[s * 2], m2 = stat_m[s * 2 + 1];
  const float* xp = x + (int64_t)n * xbs + (int64_t)c * S;
  float* op = dx + (int64_t)n * xbs + (int64_t)c * S;
  const PoolGradSrc src = pool_grad_src(dskip, dsbs, dpool, dpbs, n, c, S, H, W);
  const float sc = r * g, sh = bt - m * sc;  // same expression as the forward pass
  auto f = [&](float xv, float dv) {
    const float xh = (xv - m) * r;
    const float pre = fmaf(xv, sc, sh);
    const float gg = dv * act_grad<SMOOTH>(pre, act, slope) * g;
    return r * (gg - m1 - xh * m2);
  };
  if (MAP4) {
    const int64_t S4 = S >> 2;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < S4; i += gridDim.x * 256ll) {
      const float4 xv = reinterpret_cast<const float4*>(xp)[i];
      const float4 dv = src.four<GVEC>((uint32_t)(i * 4));
      float4 o;
      o.x = f(xv.x, dv.x); o.y = f(xv.y, dv.y); o.z = f(xv.z, dv.z); o.w = f(xv.w, dv.w);
      reinterpret_cast<float4*>(op)[i] = o;
    }
  } else {
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < S; i += gridDim.x * 256ll)
      op[i] = f(xp[i], src.one((uint32_t)i));
  }
}

// ---------------------------------------------------------------- host half
// Every entry point: validate, plan (norm_host.hpp), check the workspace against the plan, launch.  Each kernel of this
// file is launched from exactly one function.

static void launch_partial(const m355_norm_desc* d, const NormPlan& p, const float* x, double* partial, hipStream_t st) {
  const NormLaunch L = norm_pass(d, p, NORM_STATS, (uintptr_t)x);
  with_bool(L.vec, [&](auto V) {
    hipLaunchKernelGGL(norm_partial_kernel<decltype(V)::value>, L.grid, dim3(256), 0, st, x, partial, d->groups, d->C, d->S,
                       p.xbs, p.runs, p.len, L.nblk);
  });
}

// statistics from the conv epilogue partials [N][slots][C][2]: items per statistic, and the blocks that share them in
// the two-launch reduction (~2048 items each, never more than the statistics partials of the plan hold)
static int64_t partials_items(const m355_norm_desc* d, int64_t slots) {
  return (d->groups == 0 ? (int64_t)d->N : 1) * slots * (d->groups == 0 ? 1 : d->C / d->groups);
}
static int launch_from_partials(const m355_norm_desc* d, const NormPlan& p, const float* part, int64_t slots, double* partial,
                                hipStream_t st) {
  const int nblk = (int)std::max<int64_t>(1, std::min<int64_t>(p.nblk, ceil_div(partials_items(d, slots), 2048)));
  hipLaunchKernelGGL(norm_from_partials_kernel, dim3((unsigned)nblk, (unsigned)p.nstats), dim3(256), 0, st, part, partial,
                     d->groups, d->N, d->C, slots, nblk);
  return nblk;
}

// mean / rstd (+ running statistics) from nblk partials per statistic; count_ptr: see norm_finalize_kernel
static void launch_finalize(const m355_norm_desc* d, const NormPlan& p, const double* partial, int nblk, float* mean,
                            float* rstd, float* running_mean, float* running_var, float momentum, const double* count_ptr,
                            hipStream_t st) {
  hipLaunchKernelGGL(norm_finalize_kernel, dim3((unsigned)p.nstats), dim3(64), 0, st, partial, mean, rstd, running_mean,
                     running_var, momentum, d->eps, p.nstats, nblk, p.count, count_ptr);
}

// what the statistics entry points check after their pointers, in this order
static int check_stats(const m355_norm_desc* d, const NormPlan& p, const char* who, size_t workspace_bytes, bool running) {
  M355_REQUIRE(workspace_bytes >= p.workspace_bytes, M355_EWORKSPACE, "%s: workspace too small", who);
  M355_REQUIRE(d->groups == 0 || !running, M355_EINVALID_ARG, "%s: running statistics are only defined for batch norm", who);
  M355_REQUIRE(p.nstats <= 65535, M355_EUNSUPPORTED, "%s: too many statistics", who);
  return M355_OK;
}

int launch_norm_bwd_reduce(const m355_norm_desc* d, const NormPlan& p, const double* partial, const float* gamma, float* dgamma,
                           float* dbeta, float* stat_m, int training, const double* count_ptr, float grad_unscale, int* oflag,
                           hipStream_t st) {
  hipLaunchKernelGGL(norm_bwd_reduce_kernel, dim3((unsigned)std::max<int64_t>(p.nstats, d->C)), dim3(64), 0, st, partial,
                     gamma, dgamma, dbeta, stat_m, d->N, d->C, d->groups, p.bwd().nblk, p.count, training, count_ptr,
                     grad_unscale, oflag);
  return check_launch("norm_bwd_reduce");
}

// first half of the fp32 backward: partial sums + reduction -> stat_m[s][2] (means of dxhat and dxhat*xhat), dgamma,
// dbeta.  stat_m may be the caller's buffer (synchronised batch norm: all-reduced before the second half).
static int bwd_reduce_half(const m355_norm_desc* d, const NormPlan& p, const float* x, const float* dy, const float* mean,
                           const float* rstd, const float* gamma, const float* beta, float* dgamma, float* dbeta, int training,
                           const double* count_ptr, float* stat_m, void* workspace, size_t workspace_bytes, hipStream_t st,
                           const char* who) {
  M355_REQUIRE(x && dy && mean && rstd && workspace && stat_m, M355_EINVALID_ARG, "%s: null pointer", who);
  M355_REQUIRE(workspace_bytes >= p.workspace_bytes, M355_EWORKSPACE, "%s: workspace too small", who);
  const NormLaunch L = norm_pass(d, p, NORM_BWD1, (uintptr_t)x | (uintptr_t)dy);
  with_bool(L.vec, [&](auto V) {
    with_bool(act_is_smooth(d->act), [&](auto SM) {
      hipLaunchKernelGGL((norm_bwd_partial_kernel<decltype(V)::value, decltype(SM)::value>), L.grid, dim3(256), 0, st, x, dy, mean,
                         rstd, gamma, beta, p.partial(workspace), d->C, d->S, d->groups, d->act, d->act_slope, p.xbs, p.ybs,
                         L.nblk);
    });
  });
  return launch_norm_bwd_reduce(d, p, p.partial(workspace), gamma, dgamma, dbeta, stat_m, training, count_ptr, 1.f, nullptr, st);
}

// second half: dx (and, dx16 != null, its c8 twin in the same pass) from x, dy and the per-statistic means
static int bwd_apply_half(const m355_norm_desc* d, const NormPlan& p, const float* x, const float* dy, const float* mean,
                          const float* rstd, const float* gamma, const float* beta, const float* stat_m, float* dx, void* dx16,
                          int64_t dx16_batch_stride, int compute, hipStream_t st, const char* who) {
  M355_REQUIRE(x && dy && mean && rstd && dx && stat_m, M355_EINVALID_ARG, "%s: null pointer", who);
  if (dx16)
    return launch_norm_bwd_apply_c8(d, p, x, dy, mean, rstd, gamma, beta, stat_m, dx, dx16, p.bs16(dx16_batch_stride), compute,
                                    st);
  const NormLaunch L = norm_pass(d, p, NORM_BWD2, (uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx);
  with_bool(L.vec, [&](auto V) {
    with_bool(act_is_smooth(d->act), [&](auto SM) {
      hipLaunchKernelGGL((norm_bwd_apply_kernel<decltype(V)::value, decltype(SM)::value>), L.grid, dim3(256), 0, st, x, dy, mean,
                         rstd, gamma, beta, stat_m, dx, d->C, d->S, d->groups, d->act, d->act_slope, p.xbs, p.ybs);
    });
  });
  return check_launch(who);
}

// what m355_norm_act_bwd_h16 / _bwd_apply ask of a c8 twin of dx
static bool dx16_ok(const void* dx16, int64_t dx16_batch_stride, int32_t compute) {
  return (compute == M355_COMPUTE_BF16 || compute == M355_COMPUTE_F16) && ((uintptr_t)dx16 & 15) == 0 &&
         dx16_batch_stride % 8 == 0;
}

// the fused backward: both halves on one plan, stat_m inside the workspace.  (The twin's first pass is the fp32 kernel
// with grid.y = C, so the descriptor is validated for the fp32 layout either way.)
static int norm_act_bwd_impl(const m355_norm_desc* d, const float* x, const float* dy, const float* mean, const float* rstd,
                             const float* gamma, const float* beta, float* dx, float* dgamma, float* dbeta, int training,
                             void* workspace, size_t workspace_bytes, void* stream, void* dx16, int64_t dx16_batch_stride,
                             int compute) {
  M355_REQUIRE(d && workspace && dx, M355_EINVALID_ARG, "norm_act_bwd: null pointer");
  if (int rc = validate_norm(d, "norm_act_bwd", NORM_F32)) return rc;
  const NormPlan p = plan_norm(d, dx16 ? NORM_F32_C8 : NORM_F32);
  float* stat_m = p.stat_m(workspace);
  if (int rc = bwd_reduce_half(d, p, x, dy, mean, rstd, gamma, beta, dgamma, dbeta, training, nullptr, stat_m, workspace,
                               workspace_bytes, (hipStream_t)stream, "norm_act_bwd"))
    return rc;
  return bwd_apply_half(d, p, x, dy, mean, rstd, gamma, beta, stat_m, dx, dx16, dx16_batch_stride, compute,
                        (hipStream_t)stream, "norm_act_bwd");
}

// The backward behind norm_act_pool_fwd: both halves read skip + un-pooled gradient from their sources (the POOL
// kernels).  The chunk geometry, the workspace and the element-to-thread mapping are those of norm_act_bwd_impl on a
// dense, aligned sum tensor, so every result has the bits of m355_avgpool3d_2x_bwd[_add] + m355_norm_act_bwd.
static int norm_act_bwd_pool_impl(const m355_norm_desc* d0, const float* x, const float* dskip, int64_t dskip_bs,
                                  const float* dpool, int64_t dpool_bs, int D, int H, int W, const float* mean,
                                  const float* rstd, const float* gamma, const float* beta, float* dx, float* dgamma,
                                  float* dbeta, int training, void* workspace, size_t workspace_bytes, hipStream_t st) {
  const char* who = "norm_act_bwd_pool";
  if (int rc = validate_norm(d0, who, NORM_F32)) return rc;
  M355_REQUIRE(x && dpool && mean && rstd && dx && workspace, M355_EINVALID_ARG, "%s: null pointer", who);
  M355_REQUIRE(D > 0 && H > 0 && W > 0 && (int64_t)D * H * W == d0->S, M355_EINVALID_ARG, "%s: D*H*W != desc->S", who);
  M355_REQUIRE(D % 2 == 0 && H % 2 == 0 && W % 2 == 0, M355_EUNSUPPORTED, "%s: odd spatial size (%d,%d,%d)", who, D, H, W);
  M355_REQUIRE(d0->S <= INT32_MAX, M355_EUNSUPPORTED, "%s: more than 2^31 - 1 voxels per channel", who);
  m355_norm_desc dd = *d0;   // the sum tensor of the two-step form is dense
  dd.y_batch_stride = 0;
  const m355_norm_desc* d = &dd;
  const NormPlan p = plan_norm(d, NORM_F32);
  M355_REQUIRE(workspace_bytes >= p.workspace_bytes, M355_EWORKSPACE, "%s: workspace too small", who);
  const int64_t dsbs = dense_or(dskip_bs, (int64_t)d->C * d->S), dpbs = dense_or(dpool_bs, (int64_t)d->C * (d->S / 8));
  const bool gvec = W % 4 == 0 && (!dskip || (((uintptr_t)dskip & 15) == 0 && dsbs % 4 == 0));
  float* stat_m = p.stat_m(workspace);
  // MAP4 / GVEC: (1,1), (1,0) or (0,0)
  auto variant = [&](bool map4, auto&& launch) {
    with_bool(act_is_smooth(d->act), [&](auto SM) {
      if (map4 && gvec) launch(std::true_type{}, std::true_type{}, SM);
      else if (map4) launch(std::true_type{}, std::false_type{}, SM);
      else launch(std::false_type{}, std::false_type{}, SM);
    });
  };
  const NormLaunch L1 = norm_pass(d, p, NORM_BWD1, (uintptr_t)x);
  variant(L1.vec, [&](auto M4, auto GV, auto SM) {
    hipLaunchKernelGGL((norm_bwd_partial_pool_kernel<decltype(M4)::value, decltype(GV)::value, decltype(SM)::value>), L1.grid,
                       dim3(256), 0, st, x, dskip, dpool, mean, rstd, gamma, beta, p.partial(workspace), d->C, d->S, H, W,
                       d->groups, d->act, d->act_slope, p.xbs, dsbs, dpbs, L1.nblk);
  });
  if (int rc = launch_norm_bwd_reduce(d, p, p.partial(workspace), gamma, dgamma, dbeta, stat_m, training, nullptr, 1.f, nullptr,
                                      st))
    return rc;
  const NormLaunch L2 = norm_pass(d, p, NORM_BWD2, (uintptr_t)x | (uintptr_t)dx);
  variant(L2.vec, [&](auto M4, auto GV, auto SM) {
    hipLaunchKernelGGL((norm_bwd_apply_pool_kernel<decltype(M4)::value, decltype(GV)::value, decltype(SM)::value>), L2.grid,
                       dim3(256), 0, st, x, dskip, dpool, mean, rstd, gamma, beta, stat_m, dx, d->C, d->S, H, W, d->groups,
                       d->act, d->act_slope, p.xbs, dsbs, dpbs);
  });
  return check_launch(who);
}

}  // namespace m355

using namespace m355;

extern "C" int m355_norm_act_bwd_pool(const m355_norm_desc* d, const float* x, const float* dskip, int64_t dskip_batch_stride,
                                      const float* dpool, int64_t dpool_batch_stride, int32_t D, int32_t H, int32_t W,
                                      const float* mean, const float* rstd, const float* gamma, const float* beta, float* dx,
                                      float* dgamma, float* dbeta, int training, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  return norm_act_bwd_pool_impl(d, x, dskip, dskip_batch_stride, dpool, dpool_batch_stride, D, H, W, mean, rstd, gamma, beta,
                                dx, dgamma, dbeta, training, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int64_t m355_norm_num_stats(const m355_norm_desc* d) {
  if (!d) return 0;
  return d->groups == 0 ? d->C : (int64_t)d->N * d->groups;
}

extern "C" size_t m355_norm_workspace(const m355_norm_desc* d) {
  if (!d || d->N <= 0 || d->C <= 0 || d->S <= 0) return 0;
  return plan_norm(d, NORM_F32).workspace_bytes;
}

extern "C" int m355_norm_plan(const m355_norm_desc* d, int32_t which, int32_t* out4) {
  M355_REQUIRE(d && out4, M355_EINVALID_ARG, "norm_plan: null pointer");
  M355_REQUIRE(which >= 0 && which < NORM_PASS_COUNT, M355_EINVALID_ARG, "norm_plan: no pass %d", which);
  const NormPass pass = (NormPass)which;
  const NormLayout layout = (pass == NORM_FWD_C8 || pass >= NORM_BWD1_C8) ? NORM_C8 : pass == NORM_FWD_H16 ? NORM_F32_C8 : NORM_F32;
  if (int rc = validate_norm(d, "norm_plan", layout)) return rc;
  const NormPlan p = plan_norm(d, layout);
  const NormLaunch L = norm_pass(d, p, pass);
  out4[0] = L.vec;
  out4[1] = L.nblk;
  out4[2] = (int32_t)L.grid.x;
  out4[3] = pass < NORM_BWD1 ? 0 : (int32_t)std::min<size_t>(p.bwd().stat_m_off, INT32_MAX);
  return M355_OK;
}

extern "C" int m355_norm_stats(const m355_norm_desc* d, const float* x, float* mean, float* rstd,
                               float* running_mean, float* running_var, float momentum,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = validate_norm(d, "norm_stats", NORM_F32)) return rc;
  M355_REQUIRE(x && mean && rstd && workspace, M355_EINVALID_ARG, "norm_stats: null pointer");
  const NormPlan p = plan_norm(d, NORM_F32);
  if (int rc = check_stats(d, p, "norm_stats", workspace_bytes, running_mean || running_var)) return rc;
  hipStream_t st = (hipStream_t)stream;
  launch_partial(d, p, x, p.partial(workspace), st);
  launch_finalize(d, p, p.partial(workspace), p.nblk, mean, rstd, running_mean, running_var, momentum, nullptr, st);
  return check_launch("norm_stats");
}

extern "C" int m355_norm_stats_from_partials(const m355_norm_desc* d, const float* stat_partials, int64_t slots,
                                             float* mean, float* rstd, float* running_mean,
                                             float* running_var, float momentum, void* workspace,
                                             size_t workspace_bytes, void* stream) {
  if (int rc = validate_norm(d, "norm_stats_from_partials", NORM_F32)) return rc;
  M355_REQUIRE(stat_partials && mean && rstd && workspace && slots > 0, M355_EINVALID_ARG,
               "norm_stats_from_partials: null pointer / no slots");
  const NormPlan p = plan_norm(d, NORM_F32);
  if (int rc = check_stats(d, p, "norm_stats_from_partials", workspace_bytes, running_mean || running_var)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (partials_items(d, slots) <= 8192) {   // one launch, finalize included (norm_from_partials_final_kernel)
    hipLaunchKernelGGL(norm_from_partials_final_kernel, dim3((unsigned)p.nstats), dim3(1024), 0, st, stat_partials, mean,
                       rstd, running_mean, running_var, momentum, d->eps, d->groups, d->N, d->C, slots, p.count);
    return check_launch("norm_stats_from_partials");
  }
  const int nblk = launch_from_partials(d, p, stat_partials, slots, p.partial(workspace), st);
  launch_finalize(d, p, p.partial(workspace), nblk, mean, rstd, running_mean, running_var, momentum, nullptr, st);
  return check_launch("norm_stats_from_partials");
}

extern "C" int m355_norm_stats_from_running(const m355_norm_desc* d, const float* running_mean,
                                            const float* running_var, float* mean, float* rstd,
                                            void* stream) {
  if (int rc = validate_norm(d, "norm_stats_from_running", NORM_F32)) return rc;
  M355_REQUIRE(d->groups == 0, M355_EINVALID_ARG, "norm_stats_from_running: batch norm only");
  M355_REQUIRE(running_mean && running_var && mean && rstd, M355_EINVALID_ARG,
               "norm_stats_from_running: null pointer");
  hipLaunchKernelGGL(norm_from_running_kernel, dim3((unsigned)ceil_div(d->C, 64)), dim3(64), 0,
                     (hipStream_t)stream, running_mean, running_var, mean, rstd, d->eps, d->C);
  return check_launch("norm_stats_from_running");
}

extern "C" int m355_norm_act_fwd(const m355_norm_desc* d, const float* x, const float* mean,
                                 const float* rstd, const float* gamma, const float* beta,
                                 const float* add, float* y, void* stream) {
  if (int rc = validate_norm(d, "norm_act_fwd", NORM_F32)) return rc;
  M355_REQUIRE(x && mean && rstd && y, M355_EINVALID_ARG, "norm_act_fwd: null pointer");
  const NormPlan p = plan_norm(d, NORM_F32);
  const NormLaunch L = norm_pass(d, p, NORM_FWD, (uintptr_t)x | (uintptr_t)y | (uintptr_t)add);
  with_bool(L.vec, [&](auto V) {
    with_bool(act_is_smooth(d->act), [&](auto SM) {
      hipLaunchKernelGGL((norm_act_fwd_kernel<decltype(V)::value, decltype(SM)::value>), L.grid, dim3(256), 0,
                         (hipStream_t)stream, x, mean, rstd, gamma, beta, add, y, d->C, d->S, d->groups, d->act, d->act_slope,
                         p.xbs, p.ybs, p.abs_);
    });
  });
  return check_launch("norm_act_fwd");
}

extern "C" int m355_norm_act_pool_fwd(const m355_norm_desc* d, const float* x, const float* mean, const float* rstd,
                                      const float* gamma, const float* beta, float* y, float* pooled,
                                      int64_t pooled_batch_stride, int32_t D, int32_t H, int32_t W, void* stream) {
  if (int rc = validate_norm(d, "norm_act_pool_fwd", NORM_F32)) return rc;
  M355_REQUIRE(x && mean && rstd && y && pooled, M355_EINVALID_ARG, "norm_act_pool_fwd: null pointer");
  M355_REQUIRE(D > 0 && H > 0 && W > 0 && (int64_t)D * H * W == d->S, M355_EINVALID_ARG,
               "norm_act_pool_fwd: D*H*W != desc->S");
  M355_REQUIRE(D % 2 == 0 && H % 2 == 0 && W % 2 == 0, M355_EUNSUPPORTED, "norm_act_pool_fwd: odd spatial size (%d,%d,%d)",
               D, H, W);
  const NormPlan p = plan_norm(d, NORM_F32);
  const int64_t pbs = dense_or(pooled_batch_stride, (int64_t)d->C * (d->S / 8));
  M355_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 7) == 0 && p.xbs % 2 == 0 && p.ybs % 2 == 0, M355_EINVALID_ARG,
               "norm_act_pool_fwd: x / y not 8B aligned");
  with_bool(act_is_smooth(d->act), [&](auto SM) {
    hipLaunchKernelGGL(norm_act_pool_fwd_kernel<decltype(SM)::value>, norm_pass(d, p, NORM_POOL_FWD).grid, dim3(256), 0,
                       (hipStream_t)stream, x, mean, rstd, gamma, beta, y, pooled, d->C, D, H, W, d->groups, d->act,
                       d->act_slope, p.xbs, p.ybs, pbs);
  });
  return check_launch("norm_act_pool_fwd");
}

extern "C" int m355_norm_act_bwd(const m355_norm_desc* d, const float* x, const float* dy,
                                 const float* mean, const float* rstd, const float* gamma,
                                 const float* beta, float* dx, float* dgamma, float* dbeta,
                                 int training, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  return norm_act_bwd_impl(d, x, dy, mean, rstd, gamma, beta, dx, dgamma, dbeta, training, workspace, workspace_bytes,
                           stream, nullptr, 0, 0);
}

extern "C" int m355_norm_act_bwd_h16(const m355_norm_desc* d, const float* x, const float* dy, const float* mean,
                                     const float* rstd, const float* gamma, const float* beta, float* dx,
                                     float* dgamma, float* dbeta, int training, void* dx16, int64_t dx16_batch_stride,
                                     int32_t compute, void* workspace, size_t workspace_bytes, void* stream) {
  M355_REQUIRE(dx16 && dx16_ok(dx16, dx16_batch_stride, compute), M355_EINVALID_ARG,
               "norm_act_bwd_h16: needs an aligned c8 destination and a 16-bit compute type");
  return norm_act_bwd_impl(d, x, dy, mean, rstd, gamma, beta, dx, dgamma, dbeta, training, workspace, workspace_bytes,
                           stream, dx16, dx16_batch_stride, compute);
}

// ---- synchronised batch norm (statistics over the batch of ALL ranks): the local halves around the all-reduce ----

extern "C" int m355_norm_sums(const m355_norm_desc* d, const float* x, const float* stat_partials, int64_t slots,
                              double* sums, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = validate_norm(d, "norm_sums", NORM_F32)) return rc;
  M355_REQUIRE((x || stat_partials) && sums && workspace, M355_EINVALID_ARG, "norm_sums: null pointer");
  M355_REQUIRE(!stat_partials || slots > 0, M355_EINVALID_ARG, "norm_sums: partials without slots");
  M355_REQUIRE(d->groups == 0, M355_EINVALID_ARG, "norm_sums: batch norm only (group statistics never cross samples)");
  const NormPlan p = plan_norm(d, NORM_F32);
  if (int rc = check_stats(d, p, "norm_sums", workspace_bytes, false)) return rc;
  hipStream_t st = (hipStream_t)stream;
  int nblk = p.nblk;
  if (stat_partials)   // the producing conv's epilogue partials [N][slots][C][2]
    nblk = launch_from_partials(d, p, stat_partials, slots, p.partial(workspace), st);
  else
    launch_partial(d, p, x, p.partial(workspace), st);
  hipLaunchKernelGGL(norm_sums_kernel, dim3((unsigned)p.nstats), dim3(64), 0, st, p.partial(workspace), sums, p.nstats, nblk,
                     p.count);
  return check_launch("norm_sums");
}

extern "C" int m355_norm_stats_from_sums(const m355_norm_desc* d, const double* sums, float* mean, float* rstd,
                                         float* running_mean, float* running_var, float momentum, void* stream) {
  if (int rc = validate_norm(d, "norm_stats_from_sums", NORM_F32)) return rc;
  M355_REQUIRE(sums && mean && rstd, M355_EINVALID_ARG, "norm_stats_from_sums: null pointer");
  M355_REQUIRE(d->groups == 0, M355_EINVALID_ARG, "norm_stats_from_sums: batch norm only");
  const NormPlan p = plan_norm(d, NORM_F32);
  // the all-reduced sums are one "partial" per statistic, the element count over all ranks sits behind them
  launch_finalize(d, p, sums, 1, mean, rstd, running_mean, running_var, momentum, sums + p.nstats * 2, (hipStream_t)stream);
  return check_launch("norm_stats_from_sums");
}

extern "C" int m355_norm_act_bwd_reduce(const m355_norm_desc* d, const float* x, const float* dy, const float* mean,
                                        const float* rstd, const float* gamma, const float* beta, float* dgamma,
                                        float* dbeta, int training, const double* total_count, float* stat_m,
                                        void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = validate_norm(d, "norm_act_bwd_reduce", NORM_F32)) return rc;
  return bwd_reduce_half(d, plan_norm(d, NORM_F32), x, dy, mean, rstd, gamma, beta, dgamma, dbeta, training, total_count,
                         stat_m, workspace, workspace_bytes, (hipStream_t)stream, "norm_act_bwd_reduce");
}

extern "C" int m355_norm_act_bwd_apply(const m355_norm_desc* d, const float* x, const float* dy, const float* mean,
                                       const float* rstd, const float* gamma, const float* beta, const float* stat_m,
                                       float* dx, void* dx16, int64_t dx16_batch_stride, int32_t compute, void* stream) {
  M355_REQUIRE(!dx16 || dx16_ok(dx16, dx16_batch_stride, compute), M355_EINVALID_ARG,
               "norm_act_bwd_apply: the c8 destination needs alignment and a 16-bit compute type");
  if (int rc = validate_norm(d, "norm_act_bwd_apply", NORM_F32)) return rc;
  return bwd_apply_half(d, plan_norm(d, dx16 ? NORM_F32_C8 : NORM_F32), x, dy, mean, rstd, gamma, beta, stat_m, dx, dx16,
                        dx16_batch_stride, compute, (hipStream_t)stream, "norm_act_bwd_apply");
}
