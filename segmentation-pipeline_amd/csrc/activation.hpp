// The activation of the fused normalisation passes (norm.hip, act16.hip, train16.hip): y = f(pre) in the forward passes,
// g' = g * f'(pre) in the backward passes, pre = fmaf(x, sc, sh) recomputed from the saved pre-norm tensor with the
// forward's own expression -- so f' is a function of the pre-activation value and nothing else is saved.
//
// Reference op replaced: activation_class(**activation_params) inside Block3d (models/components.py:26,54-55) and its
// autograd, for nn.ReLU, nn.LeakyReLU, nn.Identity (codes 0-2) and nn.ELU, nn.GELU (both approximations), nn.SiLU (3-6).
//
// `act` is wave-uniform (m355_norm_desc.act), `p` is m355_norm_desc.act_slope: LeakyReLU's negative slope, ELU's alpha.
// SMOOTH is chosen on the host (act_is_smooth): the instantiation without it holds the three piecewise-linear codes only
// (an unknown code is "none" there) and is what they launch; the one with it adds the libm calls, which cost two of the c8
// kernels an occupancy step (profiles/activation_resources.txt) -- hence two instantiations and not one kernel.
//
// Everything is evaluated in fp32 with the accurate device functions.  No expression yields NaN from finite input:
//   ELU    expm1f, not expf - 1 (cancellation near 0); expm1f(-large) = -1, expf(-large) = 0
//   GELU   erff saturates at +-1; exp(-x^2 / 2) underflows to 0 (x^2 = +inf included) and x * 0 = 0
//   tanh   x^3 may overflow to +-inf: tanhf(+-inf) = +-1; in f' the factor (1 + 0.134145 x^2) may be +inf where
//          1 - tanh^2 is already 0, so that term is selected to 0 there instead of being multiplied out
//   SiLU   expf(-x) = +inf for x < -88.7: f = x / inf = -0; s = 1 / inf = 0, f' = 0 * (1 + x) = -0
// and f'(pre) is finite for every finite pre, so a padded lane of the unrolled c8 loops (x = 0, g = 0) contributes
// g * f'(sh) = 0 exactly.
#pragma once
#include "common.hpp"

namespace m355 {

static inline bool act_is_smooth(int act) { return act >= M355_ACT_ELU && act <= M355_ACT_SILU; }

template <bool SMOOTH>
__device__ __forceinline__ float act_fwd(float v, int act, float p) {
  if (act == M355_ACT_RELU) return v > 0.f ? v : 0.f;
  if (act == M355_ACT_LEAKY_RELU) return v > 0.f ? v : v * p;
  if constexpr (SMOOTH) {
    if (act == M355_ACT_ELU) return v > 0.f ? v : p * expm1f(v);
    if (act == M355_ACT_GELU) return 0.5f * v * (1.f + erff(v * 0.70710678118654752f));
    if (act == M355_ACT_GELU_TANH) {
      const float u = 0.79788456080286536f * fmaf(0.044715f * v * v, v, v);
      return 0.5f * v * (1.f + tanhf(u));
    }
    if (act == M355_ACT_SILU) return v / (1.f + expf(-v));
  }
  return v;
}

// f'(pre)
template <bool SMOOTH>
__device__ __forceinline__ float act_grad(float pre, int act, float p) {
  if (act == M355_ACT_RELU) return pre > 0.f ? 1.f : 0.f;
  if (act == M355_ACT_LEAKY_RELU) return pre > 0.f ? 1.f : p;
  if constexpr (SMOOTH) {
    if (act == M355_ACT_ELU) return pre > 0.f ? 1.f : p * expf(pre);
    if (act == M355_ACT_GELU) {
      const float cdf = 0.5f * (1.f + erff(pre * 0.70710678118654752f));
      return fmaf(pre * 0.39894228040143268f, expf(-0.5f * pre * pre), cdf);
    }
    if (act == M355_ACT_GELU_TANH) {
      const float x2 = pre * pre;
      const float t = tanhf(0.79788456080286536f * fmaf(0.044715f * x2, pre, pre));
      const float sech2 = 1.f - t * t;
      const float du = 0.79788456080286536f * fmaf(0.134145f, x2, 1.f);
      return 0.5f * (1.f + t) + (sech2 > 0.f ? 0.5f * pre * sech2 * du : 0.f);
    }
    if (act == M355_ACT_SILU) {
      const float s = 1.f / (1.f + expf(-pre));
      return s * fmaf(pre, 1.f - s, 1.f);
    }
  }
  return 1.f;
}

}  // namespace m355
