// HBM-bound passes of the 16-bit compute modes that WRITE the c8 activation layout (h16.hpp) the
// convolution kernels read: the normalise + activation pass after a convolution is the layout
// transposer (it already owns one full read + write of the tensor), the 2x2x2 average pool works c8 -> c8.
//
// Reference ops replaced: normalization_class + activation_class inside Block3d
// (models/components.py:52-55, + the residual sum :67-68) and nn.AvgPool3d(2, 2)
// (models/modular_unet.py:22,41,64,92), for the data flow conv -> norm/act -> conv under BASELINE cfg3 / cfg5.
#include "norm_host.hpp"
#include "activation.hpp"
#include "resample_host.hpp"

namespace m355 {

// grid: (chunks over S, channel blocks, N).  x: fp32 NCDHW conv output; y16: c8; y32 (may be null): fp32
// NCDHW copy for consumers that are not convolutions.
template <typename HT, bool VEC, bool SMOOTH>
__global__ __launch_bounds__(256) void norm_act_fwd_c8_kernel(
    const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ add,
    float* __restrict__ y32, HT* __restrict__ y16, int C, int64_t S, int groups, int act, float slope, int64_t xbs,
    int64_t y32bs, int64_t abs_, int64_t y16bs) {
  using hx8 = typename H16<HT>::x8;
  const int cb = blockIdx.y, n = blockIdx.z;
  const int c0 = cb * 8, nc = min(8, C - c0);
  float sc[8], sh[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = min(c0 + j, C - 1);
    const int64_t s = groups == 0 ? c : (int64_t)n * groups + c / (C / groups);
    const float m = mean[s], r = rstd[s];
    const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
    sc[j] = r * g;
    sh[j] = b - m * sc[j];  // same expression as norm_act_fwd_kernel
  }
  const float* xp = x + (int64_t)n * xbs + (int64_t)c0 * S;
  const float* ap = add ? add + (int64_t)n * abs_ + (int64_t)c0 * S : nullptr;
  float* yp = y32 ? y32 + (int64_t)n * y32bs + (int64_t)c0 * S : nullptr;
  hx8* dst = reinterpret_cast<hx8*>(y16 + (int64_t)n * y16bs) + (int64_t)cb * S;
  // Each lane reads one voxel of each of the 8 planes (a wave: 256 contiguous bytes per plane) and writes one
  // 16-byte item (a wave: 1 KiB contiguous).  U voxels per thread, a whole grid stride apart, are in flight
  // together (8*U independent loads).  (Four ADJACENT voxels per thread -- 16-byte plane loads -- was tried:
  // its item stores are 64 bytes apart across lanes and the pass ran 1.9x slower.)
  constexpr int U = VEC ? 4 : 1;
  const int64_t stride = gridDim.x * 256ll;
  for (int64_t i0 = blockIdx.x * 256ll + threadIdx.x; i0 < S; i0 += stride * U) {
    float v[U][8];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = min(i0 + u * stride, S - 1);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[u][j] = j < nc ? xp[(int64_t)j * S + i] : 0.f;
    }
    if (ap) {
      float a[U][8];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t i = min(i0 + u * stride, S - 1);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[u][j] = j < nc ? ap[(int64_t)j * S + i] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) v[u][j] = act_fwd<SMOOTH>(fmaf(v[u][j], sc[j], sh[j]), act, slope) + a[u][j];
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) v[u][j] = act_fwd<SMOOTH>(fmaf(v[u][j], sc[j], sh[j]), act, slope);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      if (i >= S) break;
      hx8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (HT)(j < nc ? v[u][j] : 0.f);
      dst[i] = o;
      if (yp) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (j < nc) yp[(int64_t)j * S + i] = v[u][j];
      }
    }
  }
}

// Backward twin of the pass above (16-bit TRAINING flow): the second pass of the normalisation backward
// (norm_bwd_apply_kernel in norm.hip: dx = rstd * (g * gamma - m1 - xhat * m2), g = dy * act'(pre)) over 8 channel
// planes per thread, writing dx as fp32 NCDHW (same expressions, bit-identical to the fp32 pass) AND as c8 items --
// dx is the output gradient of the convolution in front of the norm, whose data- and weight-gradient kernels read
// it as c8; emitting the twin here replaces a separate conversion pass (read 4 + write 2 bytes per element) by
// 2 bytes per element written.
template <typename HT, bool SMOOTH>
__global__ __launch_bounds__(256) void norm_bwd_apply_c8_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ stat_m, float* __restrict__ dx, HT* __restrict__ dx16, int C, int64_t S, int groups,
    int act, float slope, int64_t xbs, int64_t ybs, int64_t dx16bs, int* __restrict__ oflag) {
  using hx8 = typename H16<HT>::x8;
  const int cb = blockIdx.y, n = blockIdx.z;
  bool sat = false;   // fp16: the c8 twin of a loss-scaled dx had to be clamped (reported at the end)
  const int c0 = cb * 8, nc = min(8, C - c0);
  float m[8], r[8], g[8], sc[8], sh[8], m1[8], m2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = min(c0 + j, C - 1);
    const int64_t s = groups == 0 ? c : (int64_t)n * groups + c / (C / groups);
    m[j] = mean[s];
    r[j] = rstd[s];
    g[j] = gamma ? gamma[c] : 1.f;
    const float bt = beta ? beta[c] : 0.f;
    sc[j] = r[j] * g[j];
    sh[j] = bt - m[j] * sc[j];  // same expressions as norm_bwd_apply_kernel
    m1[j] = stat_m[s * 2];
    m2[j] = stat_m[s * 2 + 1];
  }
  const float* xp = x + (int64_t)n * xbs + (int64_t)c0 * S;
  const float* dp = dy + (int64_t)n * ybs + (int64_t)c0 * S;
  float* op = dx + (int64_t)n * xbs + (int64_t)c0 * S;
  hx8* dst = reinterpret_cast<hx8*>(dx16 + (int64_t)n * dx16bs) + (int64_t)cb * S;
  constexpr int U = 2;
  const int64_t stride = gridDim.x * 256ll;
  for (int64_t i0 = blockIdx.x * 256ll + threadIdx.x; i0 < S; i0 += stride * U) {
    float xv[U][8], dv[U][8];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = min(i0 + u * stride, S - 1);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        xv[u][j] = j < nc ? xp[(int64_t)j * S + i] : 0.f;
        dv[u][j] = j < nc ? dp[(int64_t)j * S + i] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      if (i >= S) break;
      hx8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xh = (xv[u][j] - m[j]) * r[j];
        const float pre = fmaf(xv[u][j], sc[j], sh[j]);
        const float gg = dv[u][j] * act_grad<SMOOTH>(pre, act, slope) * g[j];
        const float v = r[j] * (gg - m1[j] - xh * m2[j]);
        o[j] = to_h16_sat<HT>(j < nc ? v : 0.f, sat);
        if (j < nc) op[(int64_t)j * S + i] = v;
      }
      dst[i] = o;
    }
  }
  report_saturation(sat, oflag);
}

int launch_norm_bwd_apply_c8(const m355_norm_desc* d, const NormPlan& p, const float* x, const float* dy, const float* mean,
                             const float* rstd, const float* gamma, const float* beta, const float* stat_m, float* dx,
                             void* dx16, int64_t dx16bs, int compute, hipStream_t st) {
  with_h16(compute, [&](auto T) {
    typedef typename decltype(T)::type HT;   // (bf16 has fp32's range: nothing to clamp, no overflow word)
    with_bool(act_is_smooth(d->act), [&](auto SM) {
      hipLaunchKernelGGL((norm_bwd_apply_c8_kernel<HT, decltype(SM)::value>), norm_pass(d, p, NORM_BWD2_H16).grid, dim3(256), 0,
                         st, x, dy, mean, rstd, gamma, beta, stat_m, dx, (HT*)dx16, d->C, d->S, d->groups, d->act, d->act_slope,
                         p.xbs, p.ybs, dx16bs, std::is_same<HT, __bf16>::value ? nullptr : overflow_flag());
    });
  });
  return check_launch("norm_bwd_apply_c8");
}

// c8 -> c8 average pool: one thread per output voxel and channel block; the 2x2x2 window is four 32-byte
// runs (two x-adjacent items each).  Sums in fp32 in torch's (z, y, x) order, one rounding at the end.
template <typename HT>
__global__ __launch_bounds__(256) void avgpool2_c8_kernel(const HT* __restrict__ x16, HT* __restrict__ y16, int CB,
                                                          int D, int H, int W, int64_t xbs, int64_t ybs, int N) {
  using hx8 = typename H16<HT>::x8;
  const int OD = D / 2, OH = H / 2, OW = W / 2;
  const int64_t OS = (int64_t)OD * OH * OW, S = (int64_t)D * H * W;
  const int64_t total = (int64_t)N * CB * OS;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll) {
    const int64_t ov = i % OS;
    const int64_t r = i / OS;
    const int cb = (int)(r % CB), n = (int)(r / CB);
    const int ox = (int)(ov % OW), oy = (int)((ov / OW) % OH), oz = (int)(ov / ((int64_t)OW * OH));
    const hx8* src = reinterpret_cast<const hx8*>(x16 + (int64_t)n * xbs) + (int64_t)cb * S;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const hx8 v = src[((int64_t)(2 * oz + (q >> 2)) * H + 2 * oy + ((q >> 1) & 1)) * W + 2 * ox + (q & 1)];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = q == 0 ? (float)v[j] : acc[j] + (float)v[j];
    }
    hx8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (HT)(acc[j] * 0.125f);
    (reinterpret_cast<hx8*>(y16 + (int64_t)n * ybs) + (int64_t)cb * OS)[ov] = o;
  }
}

// c8 -> c8 normalise + activation (+ residual, also c8): the pre-norm tensor was written by the conv epilogue as
// c8 (m355_conv3d_fwd_h16_c8), so the pass is purely elementwise on 16-byte items: 2 + 2 bytes per element
// instead of 4 + 4 for the fp32 pass.  U items per thread, a grid stride apart, in flight together.
template <typename HT, bool SMOOTH>
__global__ __launch_bounds__(256) void norm_act_c8c8_kernel(
    const HT* __restrict__ x16, const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma, const float* __restrict__ beta, const HT* __restrict__ add16,
    HT* __restrict__ y16, int C, int64_t S, int groups, int act, float slope, int64_t xbs16, int64_t abs16,
    int64_t ybs16) {
  using hx8 = typename H16<HT>::x8;
  constexpr int U = 4;
  const int cb = blockIdx.y, n = blockIdx.z;
  const int c0 = cb * 8, nc = min(8, C - c0);
  float sc[8], sh[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = min(c0 + j, C - 1);
    const int64_t s = groups == 0 ? c : (int64_t)n * groups + c / (C / groups);
    const float m = mean[s], r = rstd[s];
    const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
    sc[j] = r * g;
    sh[j] = b - m * sc[j];
  }
  const hx8* src = reinterpret_cast<const hx8*>(x16 + (int64_t)n * xbs16) + (int64_t)cb * S;
  const hx8* asrc = add16 ? reinterpret_cast<const hx8*>(add16 + (int64_t)n * abs16) + (int64_t)cb * S : nullptr;
  hx8* dst = reinterpret_cast<hx8*>(y16 + (int64_t)n * ybs16) + (int64_t)cb * S;
  const int64_t stride = gridDim.x * 256ll;
  for (int64_t i0 = blockIdx.x * 256ll + threadIdx.x; i0 < S; i0 += stride * U) {
    hx8 v[U], a[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = src[min(i0 + u * stride, S - 1)];
    if (asrc) {
#pragma unroll
      for (int u = 0; u < U; ++u) a[u] = asrc[min(i0 + u * stride, S - 1)];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * stride;
      if (i >= S) break;
      hx8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float t = act_fwd<SMOOTH>(fmaf((float)v[u][j], sc[j], sh[j]), act, slope);
        if (asrc) t += (float)a[u][j];
        o[j] = (HT)(j < nc ? t : 0.f);
      }
      dst[i] = o;
    }
  }
}

// (sum, sum of squares) per channel of a c8 tensor, in the format of the conv epilogue partials
// part[n][slot][C][2] (consumed by m355_norm_stats_from_partials): the statistics of a pre-norm tensor whose
// producing conv had no fused statistics (split-K plans on the small levels).  grid (slots, CB, N).
template <typename HT>
__global__ __launch_bounds__(256) void act16_channel_partials_kernel(const HT* __restrict__ x16,
                                                                     float* __restrict__ part, int C, int64_t S,
                                                                     int64_t xbs16, int slots) {
  using hx8 = typename H16<HT>::x8;
  __shared__ float red[4][16];
  const int slot = blockIdx.x, cb = blockIdx.y, n = blockIdx.z;
  const int64_t chunk = (S + slots - 1) / slots;
  const int64_t begin = (int64_t)slot * chunk, end = min(S, begin + chunk);
  const hx8* src = reinterpret_cast<const hx8*>(x16 + (int64_t)n * xbs16) + (int64_t)cb * S;
  float s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
  for (int64_t i = begin + threadIdx.x; i < end; i += 256) {
    const hx8 v = src[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float t = (float)v[j];
      s1[j] += t;
      s2[j] = fmaf(t, t, s2[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    s1[j] = wave_sum(s1[j]);
    s2[j] = wave_sum(s2[j]);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[w][j] = s1[j];
      red[w][8 + j] = s2[j];
    }
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    const int j = threadIdx.x & 7, k = threadIdx.x >> 3;
    const float t = ((red[0][k * 8 + j] + red[1][k * 8 + j]) + red[2][k * 8 + j]) + red[3][k * 8 + j];
    const int c = cb * 8 + j;
    if (c < C) part[(((int64_t)n * slots + slot) * C + c) * 2 + k] = t;
  }
}

}  // namespace m355

using namespace m355;

extern "C" int m355_norm_act_fwd_h16(const m355_norm_desc* d, const float* x, const float* mean, const float* rstd,
                                     const float* gamma, const float* beta, const float* add, float* y,
                                     void* y16, int64_t y16_batch_stride, int32_t compute, void* stream) {
  M355_REQUIRE(d && x && mean && rstd && y16, M355_EINVALID_ARG, "norm_act_fwd_h16: null pointer");
  if (int rc = validate_norm(d, "norm_act_fwd_h16", NORM_F32_C8)) return rc;
  if (int rc = check_h16("norm_act_fwd_h16", compute)) return rc;
  const NormPlan p = plan_norm(d, NORM_F32_C8);
  const int64_t y16bs = p.bs16(y16_batch_stride);
  M355_REQUIRE(((uintptr_t)y16 & 15) == 0 && y16bs % 8 == 0, M355_EINVALID_ARG, "norm_act_fwd_h16: c8 tensor not 16B aligned");
  const NormLaunch L = norm_pass(d, p, NORM_FWD_H16);
  with_h16(compute, [&](auto T) {
    typedef typename decltype(T)::type HT;
    with_bool(L.vec, [&](auto V) {
      with_bool(act_is_smooth(d->act), [&](auto SM) {
        hipLaunchKernelGGL((norm_act_fwd_c8_kernel<HT, decltype(V)::value, decltype(SM)::value>), L.grid, dim3(256), 0,
                           (hipStream_t)stream, x, mean, rstd, gamma, beta, add, y, (HT*)y16, d->C, d->S, d->groups, d->act,
                           d->act_slope, p.xbs, p.ybs, p.abs_, y16bs);
      });
    });
  });
  return check_launch("norm_act_fwd_h16");
}

extern "C" int m355_avgpool3d_2x_fwd_h16(const void* x16, void* y16, int32_t N, int32_t C, int32_t D, int32_t H,
                                         int32_t W, int64_t x16_batch_stride, int64_t y16_batch_stride,
                                         int32_t compute, void* stream) {
  const ResampleArgs a = {N, C, D, H, W, compute, {x16_batch_stride, y16_batch_stride, 0}, {(uintptr_t)x16, (uintptr_t)y16, 0, 0}};
  if (int rc = validate_resample(RS_AVG_FWD_H16, a)) return rc;
  const ResamplePlan p = plan_resample(RS_AVG_FWD_H16, a);
  with_h16(compute, [&](auto T) {
    typedef typename decltype(T)::type HT;
    hipLaunchKernelGGL(avgpool2_c8_kernel<HT>, p.grid, dim3(256), 0, (hipStream_t)stream, (const HT*)x16, (HT*)y16,
                       (int)c8_blocks(C), D, H, W, p.bs[0], p.bs[1], N);
  });
  return check_launch("avgpool3d_2x_fwd_h16");
}

extern "C" int m355_norm_act_fwd_c8(const m355_norm_desc* d, const void* x16, int64_t x16_batch_stride,
                                    const float* mean, const float* rstd, const float* gamma, const float* beta,
                                    const void* add16, int64_t add16_batch_stride, void* y16,
                                    int64_t y16_batch_stride, int32_t compute, void* stream) {
  if (int rc = validate_norm(d, "norm_act_fwd_c8", NORM_C8)) return rc;
  if (int rc = check_h16("norm_act_fwd_c8", compute)) return rc;
  M355_REQUIRE(x16 && mean && rstd && y16, M355_EINVALID_ARG, "norm_act_fwd_c8: null pointer");
  const NormPlan p = plan_norm(d, NORM_C8);
  const int64_t xbs = p.bs16(x16_batch_stride), abs_ = p.bs16(add16_batch_stride), ybs = p.bs16(y16_batch_stride);
  M355_REQUIRE((((uintptr_t)x16 | (uintptr_t)y16 | (uintptr_t)add16) & 15) == 0 && xbs % 8 == 0 && ybs % 8 == 0 &&
                   abs_ % 8 == 0, M355_EINVALID_ARG, "norm_act_fwd_c8: c8 tensor not 16B aligned");
  with_h16(compute, [&](auto T) {
    typedef typename decltype(T)::type HT;
    with_bool(act_is_smooth(d->act), [&](auto SM) {
      hipLaunchKernelGGL((norm_act_c8c8_kernel<HT, decltype(SM)::value>), norm_pass(d, p, NORM_FWD_C8).grid, dim3(256), 0,
                         (hipStream_t)stream, (const HT*)x16, mean, rstd, gamma, beta, (const HT*)add16, (HT*)y16, d->C, d->S,
                         d->groups, d->act, d->act_slope, xbs, abs_, ybs);
    });
  });
  return check_launch("norm_act_fwd_c8");
}

extern "C" int64_t m355_act16_partials_slots(int64_t S) {
  return S <= 0 ? 0 : std::max<int64_t>(1, std::min<int64_t>(ceil_div(S, 4096), 1024));
}

extern "C" int m355_act16_channel_partials(const void* x16, int64_t x16_batch_stride, int32_t N, int32_t C, int64_t S,
                                           int32_t compute, float* stat_partials, void* stream) {
  M355_REQUIRE(x16 && stat_partials, M355_EINVALID_ARG, "act16_channel_partials: null pointer");
  M355_REQUIRE(N > 0 && C > 0 && S > 0 && N <= 65535 && c8_blocks(C) <= 65535, M355_EINVALID_ARG,
               "act16_channel_partials: bad shape");
  M355_REQUIRE(compute == M355_COMPUTE_BF16 || compute == M355_COMPUTE_F16, M355_EINVALID_ARG,
               "act16_channel_partials: compute must be M355_COMPUTE_BF16 or M355_COMPUTE_F16");
  const int64_t xbs = dense_or(x16_batch_stride, c8_blocks(C) * S * 8);
  M355_REQUIRE(((uintptr_t)x16 & 15) == 0 && xbs % 8 == 0, M355_EINVALID_ARG, "act16_channel_partials: c8 tensor not 16B aligned");
  const int slots = (int)m355_act16_partials_slots(S);
  dim3 grid((unsigned)slots, (unsigned)c8_blocks(C), (unsigned)N);
  if (compute == M355_COMPUTE_BF16)
    hipLaunchKernelGGL(act16_channel_partials_kernel<__bf16>, grid, dim3(256), 0, (hipStream_t)stream,
                       (const __bf16*)x16, stat_partials, C, S, xbs, slots);
  else
    hipLaunchKernelGGL(act16_channel_partials_kernel<_Float16>, grid, dim3(256), 0, (hipStream_t)stream,
                       (const _Float16*)x16, stat_partials, C, S, xbs, slots);
  return check_launch("act16_channel_partials");
}
