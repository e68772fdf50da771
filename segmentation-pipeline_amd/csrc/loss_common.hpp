// What the criteria share (hybrid_loss.hip, binary_loss.hip, focal_tversky_loss.hip, boundary_loss.hip).
// All four have one structure: a partial-sum kernel over chunks of one (n, c) row, a one-block finalize kernel, a one-pass
// closed-form backward.  Shared here are the expressions and the tails of those kernels and the host-side guards.  The
// loops, the chunk sizes and the order in which a finalize kernel adds a row's chunks stay with each criterion: they are
// the bits of its result.  Everything on the device is force-inlined, so a kernel is the code it was with the text in it.
#pragma once
#include "common.hpp"

namespace m355 {

// ------------------------------------------------------------------------------------------------- rows in groups
// A lane's group of V consecutive floats of a row, the first `nv` of them inside it: one 8- or 16-byte access where the
// address allows it and the whole group is inside the row, element by element otherwise.  Which lane takes which element
// does not depend on the alignment (no peeled head), so a misaligned view gives the bits of its aligned clone.
template <int V>
__device__ __forceinline__ void row_load(const float* __restrict__ p, int nv, float (&v)[V]) {
  static_assert(V == 2 || V == 4, "group of 2 or 4");
  if (nv >= V && ((uintptr_t)p & (4 * V - 1)) == 0) {
    if constexpr (V == 4) {
      const float4 r = *reinterpret_cast<const float4*>(p);
      v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
    } else {
      const float2 r = *reinterpret_cast<const float2*>(p);
      v[0] = r.x; v[1] = r.y;
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = j < nv ? p[j] : 0.f;
  }
}

template <int V>
__device__ __forceinline__ void row_store(float* __restrict__ p, int nv, const float (&v)[V]) {
  static_assert(V == 2 || V == 4, "group of 2 or 4");
  if (nv >= V && ((uintptr_t)p & (4 * V - 1)) == 0) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (j < nv) p[j] = v[j];
  }
}

// how many of the V elements from v0 on lie before `end`
__device__ __forceinline__ int row_valid(int64_t v0, int64_t end, int V) {
  const int64_t left = end - v0;
  return left <= 0 ? 0 : left >= V ? V : (int)left;
}

// ---------------------------------------------------------------------------------------------------- expressions
// log(prediction_safe) of the reference: eps = 1e-8, prediction_safe = (prediction + eps) / (1 + eps), evaluated by torch
// in fp32 with the python scalars rounded to fp32 (1 + 1e-8 == 1.0f)
__device__ __forceinline__ float safe_log_prob(float p) { return logf((p + 1e-8f) / (float)(1.0 + 1e-8)); }

// one element's contribution to the Dice sums of its row: s0 = sum p t, s1 = sum p(^2), s2 = sum t(^2)
__device__ __forceinline__ void dice_accumulate(float p, float t, int square_dice, float& s0, float& s1, float& s2) {
  s0 = fmaf(p, t, s0);
  if (square_dice) {
    s1 = fmaf(p, p, s1);
    s2 = fmaf(t, t, s2);
  } else {
    s1 += p;
    s2 += t;
  }
}

// 1 - dice_coeff of a row from its three sums: dice_coeffs = 2*overlap / (total + eps)   (fp32 in the reference)
__device__ __forceinline__ float dice_term(double v0, double v1, double v2) {
  const float overlap = (float)v0, total = (float)v1 + (float)v2;
  const float dice = 2.f * overlap / (total + 1e-8f);
  return 1.f - dice;
}

// d dice_loss / dp = -(1/(N*C)) * (2 t / (T+eps) - 2 O * dT/dp / (T+eps)^2),   dT/dp = 2p (square_dice) or 1:
// the row's coefficients, dloss (g) and the Dice weight included.  `row` = the row's saved sums, the Dice ones first.
struct DiceBwd {
  float O, T;      // overlap; total + eps
  float kd1, kd2;  // * t; * dT/dp
};
__device__ __forceinline__ DiceBwd dice_bwd_coeffs(const float* __restrict__ row, float dice_weight, float inv_nc, float g) {
  DiceBwd k;
  k.O = row[0];
  k.T = row[1] + row[2] + 1e-8f;
  k.kd1 = -dice_weight * inv_nc * 2.f / k.T * g;
  k.kd2 = dice_weight * inv_nc * 2.f * k.O / (k.T * k.T) * g;
  return k;
}

// ---------------------------------------------------------------------------------------------------------- tails
// The end of a partial-sum kernel: the block's K sums in fp64, reduced one after the other in index order (the fixed tree
// of block_sum), then one thread writes the K doubles.  256 threads; `scratch`: 4 doubles of LDS.
template <int K, typename T>
__device__ __forceinline__ void store_block_sums(const T (&s)[K], double* __restrict__ partial, int64_t slot,
                                                 double* scratch) {
  double r[K];
#pragma unroll
  for (int k = 0; k < K; ++k) r[k] = block_sum<double, 256>((double)s[k], scratch);
  if (threadIdx.x == 0) {
    double* o = partial + slot * K;
#pragma unroll
    for (int k = 0; k < K; ++k) o[k] = r[k];
  }
}

// out3 = {loss, a, b}: the overlap term `a` mixed with the log term `b` by `weight`
__device__ __forceinline__ void write_out3(float* __restrict__ out3, float weight, float a, float b) {
  out3[0] = (1.f - weight) * b + weight * a;
  out3[1] = a;
  out3[2] = b;
}

// ----------------------------------------------------------------------------------------------------------- host
// The sizes every entry point accepts: rows are blockIdx.y.
static inline int loss_check(const char* what, int32_t N, int32_t C, int64_t S) {
  M355_REQUIRE(N > 0 && C > 0 && S > 0, M355_EINVALID_ARG, "%s: non-positive size", what);
  M355_REQUIRE((int64_t)N * C <= 65535, M355_EUNSUPPORTED, "%s: N*C > 65535", what);
  return M355_OK;
}

// K doubles per chunk of `chunk` elements of every row (0 for sizes loss_check refuses as non-positive)
static inline size_t loss_workspace_bytes(int32_t N, int32_t C, int64_t S, int chunk, int K) {
  if (N <= 0 || C <= 0 || S <= 0) return 0;
  return (size_t)N * C * ceil_div(S, chunk) * K * sizeof(double) + 256;
}

// the grid of a row-major backward: blocks of `elems_per_block` elements along a row, 2048 at the most, times NC rows
static inline dim3 loss_bwd_grid(int64_t S, int elems_per_block, int NC) {
  return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(S, elems_per_block), 2048)), (unsigned)NC);
}

}  // namespace m355
