// Uncertainty maps: the entropy of a probability volume, alone and through the test-time ensembles.
//
//   uq_entropy_kernel     predictive entropy (and the maximum channel value) of probabilities [N, C, S], one pass, 16-byte
//                         loads of 8 voxels per lane where the rows allow it.
//   uq_accumulate_kernel  a member's entropy read THROUGH the inverse transform of ensemble.hip's accumulate pass and
//                         added to a float32 accumulator in canonical orientation.
//   uq_finalize_kernel    from the running sum of m355_ensemble_accumulate (mode 0), the entropy accumulator and the member
//                         count: entropy of the mean, expected member entropy, their difference and the mean's maximum.
//
// entropy_term below is the only place the entropy expression exists; every kernel sums its terms in channel order with
// one rounding per operation (no contraction), so the three agree bit for bit on equal probabilities.
#include "axis_map.hpp"
#include "ev_load.hpp"

namespace m355 {
namespace {

using ev::load_score1;
using ev::load_scores8;
using ev::takes;

constexpr int UQ_V = ev::SCORE_V;

// p log p with the zero rule: 0 for p <= 0 (the limit at 0; a negative value is no probability), a NaN passes through.
// logf is float32; the product of two floats is exact in fp64, so its float32 rounding is the float32 product.
__device__ __forceinline__ double entropy_term(float p) { return p > 0.f ? (double)p * (double)logf(p) : (p != p ? (double)p : 0.0); }
// the running sum of a categorical entropy, float32 in channel order: h = -(((0 + t_0) + t_1) + ...)
__device__ __forceinline__ float entropy_step(float s, float p) { return __fadd_rn(s, (float)entropy_term(p)); }
// the entropy of one sigmoid channel, -p log p - (1 - p) log(1 - p) with 1 - p in float32: the two products and their sum
// are formed in fp64 and rounded once, so what is left is the error of the two logf
__device__ __forceinline__ float entropy_binary(float p) { return (float)-(entropy_term(p) + entropy_term(__fsub_rn(1.f, p))); }

// one voxel whose C channel values come from `at(c)`: categorical writes one entropy, binary one per channel
template <typename At, typename Put>
__device__ __forceinline__ void uq_voxel(int C, int kind, At at, Put put, float* conf) {
  float s = 0.f, best = 0.f;
  for (int c = 0; c < C; ++c) {
    const float p = at(c);
    if (kind == M355_UQ_BINARY) put(c, entropy_binary(p));
    else s = entropy_step(s, p);
    if (c == 0 || takes(best, p)) best = p;
  }
  if (kind != M355_UQ_BINARY) put(0, -s);
  if (conf) *conf = best;
}

template <int SD>
__global__ __launch_bounds__(256) void uq_entropy_kernel(const void* __restrict__ probs, float* __restrict__ entropy,
                                                         float* __restrict__ confidence, int N, int C, int64_t S, int kind,
                                                         int aligned) {
  const int K = kind == M355_UQ_BINARY ? C : 1;
  const int64_t g = blockIdx.x * 256ll + threadIdx.x, gs = gridDim.x * 256ll;
  if (aligned) {
    const int64_t Sg = S / UQ_V, total = (int64_t)N * Sg;
    for (int64_t i = g; i < total; i += gs) {
      const int64_t n = i / Sg, v = (i - n * Sg) * UQ_V;
      float s[UQ_V], best[UQ_V];
#pragma unroll
      for (int j = 0; j < UQ_V; ++j) s[j] = best[j] = 0.f;
      for (int c = 0; c < C; ++c) {
        float p[UQ_V], h[UQ_V];
        load_scores8<SD>(probs, (n * C + c) * S + v, p);
#pragma unroll
        for (int j = 0; j < UQ_V; ++j) {
          if (kind == M355_UQ_BINARY) h[j] = entropy_binary(p[j]);
          else s[j] = entropy_step(s[j], p[j]);
          if (c == 0 || takes(best[j], p[j])) best[j] = p[j];
        }
        if (kind == M355_UQ_BINARY) {
          float* o = entropy + (n * K + c) * S + v;
          *(float4*)o = make_float4(h[0], h[1], h[2], h[3]);
          *(float4*)(o + 4) = make_float4(h[4], h[5], h[6], h[7]);
        }
      }
      if (kind != M355_UQ_BINARY) {
        float* o = entropy + n * S + v;
        *(float4*)o = make_float4(-s[0], -s[1], -s[2], -s[3]);
        *(float4*)(o + 4) = make_float4(-s[4], -s[5], -s[6], -s[7]);
      }
      if (confidence) {
        float* o = confidence + n * S + v;
        *(float4*)o = make_float4(best[0], best[1], best[2], best[3]);
        *(float4*)(o + 4) = make_float4(best[4], best[5], best[6], best[7]);
      }
    }
    return;
  }
  const int64_t total = (int64_t)N * S;
  for (int64_t i = g; i < total; i += gs) {
    const int64_t n = i / S, v = i - n * S;
    uq_voxel(C, kind, [&](int c) { return load_score1<SD>(probs, (n * C + c) * S + v); },
             [&](int k, float h) { entropy[(n * K + k) * S + v] = h; }, confidence ? confidence + n * S + v : nullptr);
  }
}

__global__ __launch_bounds__(256) void uq_accumulate_kernel(const float* __restrict__ pred, float* __restrict__ eacc, int N,
                                                            int C, AxisMap m, int64_t S, int kind, int first) {
  const int K = kind == M355_UQ_BINARY ? C : 1;
  const int64_t total = (int64_t)N * S;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll) {
    const int64_t n = i / S, v = i - n * S;
    const float* p = pred + n * C * S + member_offset(m, v);
    float* a = eacc + n * K * S + v;
    uq_voxel(C, kind, [&](int c) { return p[(int64_t)c * S]; },
             [&](int k, float h) { a[(int64_t)k * S] = first ? h : __fadd_rn(a[(int64_t)k * S], h); }, nullptr);
  }
}

__global__ __launch_bounds__(256) void uq_finalize_kernel(const float* __restrict__ acc, const float* __restrict__ eacc,
                                                          float* __restrict__ entropy, float* __restrict__ expected,
                                                          float* __restrict__ mutual, float* __restrict__ confidence, int N,
                                                          int C, int64_t S, float inv_members, float members, int kind) {
  const int K = kind == M355_UQ_BINARY ? C : 1;
  const int64_t total = (int64_t)N * S;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll) {
    const int64_t n = i / S, v = i - n * S;
    const float* a = acc + n * C * S + v;
    // acc * inv_members: the mean as m355_ensemble_finalize writes it
    uq_voxel(C, kind, [&](int c) { return __fmul_rn(a[(int64_t)c * S], inv_members); },
             [&](int k, float h) {
               const int64_t o = (n * K + k) * S + v;
               const float x = eacc[o] / members, d = __fsub_rn(h, x);
               entropy[o] = h;
               expected[o] = x;
               mutual[o] = d < 0.f ? 0.f : d;   // a NaN stays NaN
             },
             confidence + n * S + v);
  }
}

int uq_check(const char* who, int32_t N, int32_t C, int64_t S, int32_t kind) {
  M355_REQUIRE(N > 0 && C > 0 && S > 0, M355_EINVALID_ARG, "%s: non-positive size", who);
  M355_REQUIRE((int64_t)N * C * S < ((int64_t)1 << 40), M355_EINVALID_ARG, "%s: tensor too large", who);
  M355_REQUIRE(kind == M355_UQ_CATEGORICAL || kind == M355_UQ_BINARY, M355_EINVALID_ARG, "%s: kind %d", who, kind);
  return M355_OK;
}

}  // namespace
}  // namespace m355

using namespace m355;

extern "C" int m355_predictive_entropy(const void* probs, int32_t dtype, float* entropy, float* confidence, int32_t N,
                                       int32_t C, int64_t S, int32_t kind, void* stream) {
  if (int rc = uq_check("predictive_entropy", N, C, S, kind)) return rc;
  M355_REQUIRE(probs && entropy, M355_EINVALID_ARG, "predictive_entropy: null pointer");
  M355_REQUIRE(dtype == M355_EV_F32 || dtype == M355_EV_BF16 || dtype == M355_EV_F16, M355_EINVALID_ARG,
               "predictive_entropy: element type %d (float32, bfloat16, float16)", dtype);
  const bool aligned = S % UQ_V == 0 && ((uintptr_t)probs & 15) == 0 && ((uintptr_t)entropy & 15) == 0 &&
                       ((uintptr_t)confidence & 15) == 0;
  const dim3 g(grid_of(aligned ? (int64_t)N * (S / UQ_V) : (int64_t)N * S)), b(256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == M355_EV_F32)
    hipLaunchKernelGGL(uq_entropy_kernel<M355_EV_F32>, g, b, 0, st, probs, entropy, confidence, N, C, S, kind, (int)aligned);
  else if (dtype == M355_EV_BF16)
    hipLaunchKernelGGL(uq_entropy_kernel<M355_EV_BF16>, g, b, 0, st, probs, entropy, confidence, N, C, S, kind, (int)aligned);
  else
    hipLaunchKernelGGL(uq_entropy_kernel<M355_EV_F16>, g, b, 0, st, probs, entropy, confidence, N, C, S, kind, (int)aligned);
  return check_launch("predictive_entropy");
}

extern "C" int m355_ensemble_entropy_accumulate(const float* pred, float* eacc, int32_t N, int32_t C, const int32_t* size3,
                                                const int32_t* perm3, int32_t flip_mask, int32_t kind, int32_t first,
                                                void* stream) {
  if (int rc = check_map_args("ensemble_entropy_accumulate", size3, perm3, flip_mask)) return rc;
  const int64_t S = (int64_t)size3[0] * size3[1] * size3[2];
  if (int rc = uq_check("ensemble_entropy_accumulate", N, C, S, kind)) return rc;
  M355_REQUIRE(pred && eacc, M355_EINVALID_ARG, "ensemble_entropy_accumulate: null pointer");
  const AxisMap m = make_axis_map(size3, perm3, flip_mask);
  hipLaunchKernelGGL(uq_accumulate_kernel, dim3(grid_of((int64_t)N * S)), dim3(256), 0, (hipStream_t)stream, pred, eacc, N, C,
                     m, S, kind, first);
  return check_launch("ensemble_entropy_accumulate");
}

extern "C" int m355_ensemble_uncertainty_finalize(const float* acc, const float* eacc, float* entropy,
                                                  float* expected_entropy, float* mutual_information, float* confidence,
                                                  int32_t N, int32_t C, int64_t S, int32_t members, int32_t kind,
                                                  void* stream) {
  if (int rc = uq_check("ensemble_uncertainty_finalize", N, C, S, kind)) return rc;
  M355_REQUIRE(members > 0, M355_EINVALID_ARG, "ensemble_uncertainty_finalize: %d members", members);
  M355_REQUIRE(acc && eacc && entropy && expected_entropy && mutual_information && confidence, M355_EINVALID_ARG,
               "ensemble_uncertainty_finalize: null pointer");
  hipLaunchKernelGGL(uq_finalize_kernel, dim3(grid_of((int64_t)N * S)), dim3(256), 0, (hipStream_t)stream, acc, eacc, entropy,
                     expected_entropy, mutual_information, confidence, N, C, S, 1.0f / (float)members, (float)members, kind);
  return check_launch("ensemble_uncertainty_finalize");
}
