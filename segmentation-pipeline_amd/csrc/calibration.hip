// Calibration of predicted probabilities on the device: reliability tables, Brier score and negative
// log-likelihood of every subject in one pass over the scores, whatever the subjects' sizes (the descriptor pattern of
// m355_eval_multilabel: host descriptors are copied to dev_descs on the stream, nothing synchronises).
//
//   cal_kernel      grid (blocks, subjects).  Voxel-major: a lane owns 8 consecutive voxels (16-byte loads along S; voxel
//                   by voxel for a subject whose rows are not 16-byte aligned) and walks the channels with running state
//                   only: maximum, argmax, the target's class and its probability, the Brier sum, validity.  Every
//                   (voxel, channel) goes into the workgroup's LDS tables [1 + C][B][{count, hits, conf_sum}] with 64-bit
//                   integer atomics; a categorical voxel that turns out invalid at a later channel takes its earlier
//                   entries out again (integer adds are exact both ways).  The tables are flushed once per workgroup with
//                   global integer atomics; the two fp64 sums leave as one pair of partials per workgroup.
//   cal_sum_kernel  one wave per subject adds the workgroups' partials in a fixed order and writes the voxel count.
// Counts and fixed-point sums are exact and independent of order; the fp64 sums depend only on the grid, so a repeated
// call gives the same bits.
#include "ev_load.hpp"

namespace m355 {
namespace {

using ev::load_score1;
using ev::load_scores8;
using ev::takes;

constexpr int CAL_NT = 256, CAL_V = ev::SCORE_V;
constexpr int CAL_MAX_BLOCKS = 2048;   // workgroups per subject at the most: the size of a subject's partials

struct CalArgs {
  int32_t C, B;
};

// a target element of any M355_EV_* type as a double (exact)
__device__ __forceinline__ double cal_t1(const void* p, int dt, int64_t i) {
  switch (dt) {
    case M355_EV_I8: return ((const int8_t*)p)[i];
    case M355_EV_I16: return ((const int16_t*)p)[i];
    case M355_EV_I32: return ((const int32_t*)p)[i];
    case M355_EV_I64: return (double)((const int64_t*)p)[i];
    case M355_EV_F32: return ((const float*)p)[i];
    case M355_EV_BF16: return __uint_as_float((uint32_t)((const uint16_t*)p)[i] << 16);
    case M355_EV_F16: return __half2float(__ushort_as_half(((const uint16_t*)p)[i]));
    default: return ((const uint8_t*)p)[i];   // bool, uint8
  }
}

// CAL_V consecutive target elements from element i (a multiple of CAL_V, the row 16-byte aligned)
__device__ __forceinline__ void cal_t8(const void* p, int dt, int64_t i, double t[CAL_V]) {
  switch (dt) {
    case M355_EV_I32:
    case M355_EV_F32: {
      const uint4 a = *(const uint4*)((const uint32_t*)p + i), b = *(const uint4*)((const uint32_t*)p + i + 4);
      const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
      for (int j = 0; j < CAL_V; ++j) t[j] = dt == M355_EV_I32 ? (double)(int32_t)w[j] : (double)__uint_as_float(w[j]);
      break;
    }
    case M355_EV_I64: {
#pragma unroll
      for (int h = 0; h < CAL_V / 2; ++h) {
        const longlong2 r = *(const longlong2*)((const int64_t*)p + i + 2 * h);
        t[2 * h] = (double)r.x; t[2 * h + 1] = (double)r.y;
      }
      break;
    }
    case M355_EV_I16:
    case M355_EV_BF16:
    case M355_EV_F16: {
      const uint4 r = *(const uint4*)((const uint16_t*)p + i);
      const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int j = 0; j < CAL_V; ++j) {
        const uint16_t h = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
        t[j] = dt == M355_EV_I16 ? (double)(int16_t)h
             : dt == M355_EV_BF16 ? (double)__uint_as_float((uint32_t)h << 16) : (double)__half2float(__ushort_as_half(h));
      }
      break;
    }
    default: {   // bool, uint8, int8
      const uint2 r = *(const uint2*)((const uint8_t*)p + i);
      const uint32_t w[2] = {r.x, r.y};
#pragma unroll
      for (int j = 0; j < CAL_V; ++j) {
        const uint32_t b = (w[j >> 2] >> (8 * (j & 3))) & 0xff;
        t[j] = dt == M355_EV_I8 ? (double)(int8_t)b : (double)b;
      }
    }
  }
}

// a channel index of an integer M355_EV_* type
__device__ __forceinline__ int64_t cal_index(const void* p, int dt, int64_t i) {
  switch (dt) {
    case M355_EV_I8: return ((const int8_t*)p)[i];
    case M355_EV_I16: return ((const int16_t*)p)[i];
    case M355_EV_I32: return ((const int32_t*)p)[i];
    case M355_EV_I64: return ((const int64_t*)p)[i];
    default: return ((const uint8_t*)p)[i];   // bool, uint8
  }
}

__device__ __forceinline__ bool cal_in_range(float p) { return p >= 0.f && p <= 1.f; }   // a NaN is not
// the bin of a confidence in [0, 1]: one float32 multiply and a truncation
__device__ __forceinline__ int cal_bin(float q, int B) { return min((int)(q * (float)B), B - 1); }
// the confidence in 2^-32 fixed point (an integer already for q >= 2^-8)
__device__ __forceinline__ unsigned long long cal_fixed(float q) { return (unsigned long long)rint((double)q * 4294967296.0); }
// the reference criterion's prediction_safe shift, in fp64
__device__ __forceinline__ double cal_neg_log(double p) { return -log((p + 1e-8) / (1.0 + 1e-8)); }

// one entry of table `t` (0: top label, 1 + c: channel c), added (sign = 1) or taken out again (sign = -1, modulo 2^64)
__device__ __forceinline__ void cal_add(unsigned long long* hist, int B, int t, float q, bool hit, unsigned long long sign) {
  unsigned long long* e = hist + ((int64_t)t * B + cal_bin(q, B)) * 3;
  atomicAdd(e, sign);
  if (hit) atomicAdd(e + 1, sign);
  atomicAdd(e + 2, sign * cal_fixed(q));
}

// Rare: the invalid voxels of a lane's group (bits of `bad`) are counted, and each takes out what its channels before the
// first value outside [0, 1] put into the classwise tables.
template <int SD, int V, bool onehot>
__device__ __forceinline__ void cal_take_out(const m355_eval_calibration_desc& d, int C, int B, int64_t i, uint32_t bad,
                                          uint32_t tokm, unsigned long long* hist, unsigned long long* inval) {
#pragma unroll 1
  for (int j = 0; j < V; ++j) {
    if (!((bad >> j) & 1u)) continue;
    atomicAdd(&inval[0], 1ull);
    if (!((tokm >> j) & 1u)) continue;   // an index out of range: nothing went in
    const int64_t tc = onehot ? 0 : cal_index(d.target, d.target_dtype, i + j);
    for (int c = 0; c < C; ++c) {
      const int64_t at = (int64_t)c * d.S + i + j;
      const float p = load_score1<SD>(d.scores, at);
      if (!cal_in_range(p)) break;
      const bool pos = onehot ? cal_t1(d.target, d.target_dtype, at) != 0.0 : tc == c;
      cal_add(hist, B, 1 + c, p, pos, ~0ull);
    }
  }
}

// V voxels of one lane from voxel i on (V = CAL_V: vector loads; V = 1: element loads)
template <int SD, int V, bool binary, bool onehot>
__device__ __forceinline__ void cal_group(const m355_eval_calibration_desc& d, const CalArgs& a, int64_t i,
                                          unsigned long long* hist, unsigned long long* inval, double& brier, double& nll) {
  const int C = a.C, B = a.B;
  const int64_t S = d.S;
  float best[V], pt[V];
  double tb[V], br[V];
  int arg[V], tcls[V];
  // flags as bits of a lane's own word (bit j = voxel j): ok = valid so far, tok = the target index is in range
  uint32_t okm = (1u << V) - 1u, tokm = okm;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    best[j] = pt[j] = 0.f; tb[j] = br[j] = 0.0; arg[j] = 0; tcls[j] = 0;
  }
  if (!onehot) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int64_t t = cal_index(d.target, d.target_dtype, i + j);
      const bool inside = t >= 0 && t < C;
      tcls[j] = inside ? (int)t : -1;
      if (!inside) tokm &= ~(1u << j);
    }
    okm = tokm;
  }
  for (int c = 0; c < C; ++c) {
    float p[V];
    double t[V];
    const int64_t at = (int64_t)c * S + i;
    if constexpr (V == CAL_V) {
      load_scores8<SD>(d.scores, at, p);
      if (onehot) cal_t8(d.target, d.target_dtype, at, t);
    } else {
      p[0] = load_score1<SD>(d.scores, at);
      if (onehot) t[0] = cal_t1(d.target, d.target_dtype, at);
    }
    if (onehot) {
#pragma unroll
      for (int j = 0; j < V; ++j)
        if (c == 0 || takes(tb[j], t[j])) { tb[j] = t[j]; tcls[j] = c; pt[j] = p[j]; }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      // positive: a NaN is, -0.0 is not (torch's `!= 0`)
      const bool pos = onehot ? t[j] != 0.0 : tcls[j] == c;
      if (!onehot && pos) pt[j] = p[j];
      if (c == 0 || takes(best[j], p[j])) { best[j] = p[j]; arg[j] = c; }
      const bool inr = cal_in_range(p[j]);
      const double y = pos ? 1.0 : 0.0, dp = (double)p[j] - y;
      if (binary) {
        if (inr && ((tokm >> j) & 1u)) {
          cal_add(hist, B, 1 + c, p[j], pos, 1ull);
          brier += dp * dp;
          nll += cal_neg_log(pos ? (double)p[j] : 1.0 - (double)p[j]);
        } else {
          atomicAdd(&inval[c], 1ull);
        }
      } else {
        if (!inr) okm &= ~(1u << j);
        if ((okm >> j) & 1u) {
          cal_add(hist, B, 1 + c, p[j], pos, 1ull);
          br[j] += dp * dp;
        }
      }
    }
  }
  if (binary) return;
  const uint32_t bad = ~okm & ((1u << V) - 1u);
  if (bad) cal_take_out<SD, V, onehot>(d, C, B, i, bad, tokm, hist, inval);
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const bool on = (okm >> j) & 1u, hit = arg[j] == tcls[j];
    if (on) cal_add(hist, B, 0, best[j], hit, 1ull);
    if (on) brier += br[j];
    else pt[j] = 1.f;   // -log(prediction_safe(1)) is exactly 0
  }
  // the fp64 logarithm once in the code, not once per voxel of the group: the value picked by selects, no indexing
#pragma unroll 1
  for (int j = 0; j < V; ++j) {
    float x = pt[0];
#pragma unroll
    for (int k = 1; k < V; ++k) x = j == k ? pt[k] : x;
    nll += cal_neg_log((double)x);
  }
}

template <int SD, bool BINARY, bool ONEHOT>
__global__ __launch_bounds__(CAL_NT) void cal_kernel(const m355_eval_calibration_desc* __restrict__ descs, CalArgs a,
                                                    unsigned long long* __restrict__ top,
                                                    unsigned long long* __restrict__ classwise,
                                                    unsigned long long* __restrict__ invalid, double* __restrict__ partial) {
  extern __shared__ unsigned long long cal_lds[];   // [1 + C][B][3], then inval[C]
  __shared__ double scratch[CAL_NT / 64];
  const m355_eval_calibration_desc d = descs[blockIdx.y];
  const int nh = (1 + a.C) * a.B * 3;
  unsigned long long* hist = cal_lds;
  unsigned long long* inval = cal_lds + nh;
  for (int i = threadIdx.x; i < nh + a.C; i += CAL_NT) cal_lds[i] = 0;
  __syncthreads();

  const int64_t S = d.S;
  const bool aligned = S % CAL_V == 0 && ((uintptr_t)d.scores & 15) == 0 && ((uintptr_t)d.target & 15) == 0;
  const int64_t Sv = aligned ? S : 0;
  const int64_t g = (int64_t)blockIdx.x * CAL_NT + threadIdx.x, gs = (int64_t)gridDim.x * CAL_NT;
  double brier = 0.0, nll = 0.0;
  for (int64_t i = g * CAL_V; i < Sv; i += gs * CAL_V) cal_group<SD, CAL_V, BINARY, ONEHOT>(d, a, i, hist, inval, brier, nll);
  for (int64_t i = Sv + g; i < S; i += gs) cal_group<SD, 1, BINARY, ONEHOT>(d, a, i, hist, inval, brier, nll);
  __syncthreads();
  const int64_t sub = blockIdx.y;
  const int nt = a.B * 3;
  for (int i = threadIdx.x; i < nh; i += CAL_NT) {
    if (!hist[i]) continue;
    if (i < nt) atomicAdd(&top[sub * nt + i], hist[i]);
    else atomicAdd(&classwise[sub * a.C * nt + (i - nt)], hist[i]);
  }
  for (int c = threadIdx.x; c < a.C; c += CAL_NT)
    if (inval[c]) atomicAdd(&invalid[sub * a.C + c], inval[c]);
  const double b = block_sum<double, CAL_NT>(brier, scratch), l = block_sum<double, CAL_NT>(nll, scratch);
  if (threadIdx.x == 0) {
    double* o = partial + (sub * gridDim.x + blockIdx.x) * 2;
    o[0] = b; o[1] = l;
  }
}

// sums[subject] = the workgroups' partials, lane j adding blocks j, j + 64, ... in turn, then the 64 lanes in a fixed tree
__global__ __launch_bounds__(64) void cal_sum_kernel(const m355_eval_calibration_desc* __restrict__ descs,
                                                     const double* __restrict__ partial, int nblk, double* __restrict__ sums,
                                                     int64_t* __restrict__ voxels) {
  const int64_t sub = blockIdx.x;
  double b = 0.0, l = 0.0;
  for (int k = threadIdx.x; k < nblk; k += 64) {
    b += partial[(sub * nblk + k) * 2];
    l += partial[(sub * nblk + k) * 2 + 1];
  }
  b = wave_sum(b);
  l = wave_sum(l);
  if (threadIdx.x == 0) {
    sums[sub * 2] = b;
    sums[sub * 2 + 1] = l;
    voxels[sub] = descs[sub].S;
  }
}

}  // namespace
}  // namespace m355

using namespace m355;

extern "C" size_t m355_eval_calibration_workspace(int32_t n) {
  return n < 1 ? 0 : (size_t)n * CAL_MAX_BLOCKS * 2 * sizeof(double);
}

extern "C" int m355_eval_calibration(const m355_eval_calibration_desc* descs, int32_t n, void* dev_descs,
                                     int32_t scores_dtype, int32_t target_kind, int32_t C, int32_t bins, int32_t kind,
                                     uint64_t* top,
                                     uint64_t* classwise, uint64_t* invalid, double* sums, int64_t* voxels, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  M355_REQUIRE(descs && dev_descs && top && classwise && invalid && sums && voxels && workspace, M355_EINVALID_ARG,
               "eval_calibration: null pointer");
  M355_REQUIRE(n >= 1 && n <= 65535, M355_EINVALID_ARG, "eval_calibration: %d subjects (1 .. 65535)", n);
  M355_REQUIRE(C >= 1 && C <= M355_EV_MAX_CHANNELS, M355_EUNSUPPORTED, "eval_calibration: %d channels (1 .. %d)", C,
               M355_EV_MAX_CHANNELS);
  M355_REQUIRE(bins >= 1 && bins <= M355_CAL_MAX_BINS, M355_EUNSUPPORTED, "eval_calibration: %d bins (1 .. %d)", bins,
               M355_CAL_MAX_BINS);
  M355_REQUIRE(kind == M355_CAL_CATEGORICAL || kind == M355_CAL_BINARY, M355_EINVALID_ARG, "eval_calibration: kind %d", kind);
  M355_REQUIRE(scores_dtype == M355_EV_F32 || scores_dtype == M355_EV_BF16 || scores_dtype == M355_EV_F16, M355_EINVALID_ARG,
               "eval_calibration: score type %d (float32, bfloat16, float16)", scores_dtype);
  M355_REQUIRE(workspace_bytes >= m355_eval_calibration_workspace(n), M355_EWORKSPACE, "eval_calibration: workspace too small");
  M355_REQUIRE(target_kind == M355_EV_TARGET_ONEHOT || target_kind == M355_EV_TARGET_MAP, M355_EINVALID_ARG,
               "eval_calibration: target kind %d", target_kind);
  const bool onehot = target_kind == M355_EV_TARGET_ONEHOT;
  int64_t maxS = 1;
  for (int i = 0; i < n; ++i) {
    const m355_eval_calibration_desc& d = descs[i];
    M355_REQUIRE(d.scores, M355_EINVALID_ARG, "eval_calibration: subject %d: null scores", i);
    M355_REQUIRE(d.target, M355_EINVALID_ARG, "eval_calibration: subject %d: null target", i);
    M355_REQUIRE(d.S >= 1 && d.S * C < ((int64_t)1 << 40), M355_EINVALID_ARG, "eval_calibration: subject %d: %lld voxels", i,
                 (long long)d.S);
    if (onehot)
      M355_REQUIRE(d.target_dtype >= M355_EV_BOOL && d.target_dtype <= M355_EV_F16, M355_EINVALID_ARG,
                   "eval_calibration: subject %d: target element type %d", i, d.target_dtype);
    else
      M355_REQUIRE(d.target_dtype >= M355_EV_BOOL && d.target_dtype <= M355_EV_I64, M355_EINVALID_ARG,
                   "eval_calibration: subject %d: index map of element type %d (an integer type)", i, d.target_dtype);
    maxS = std::max<int64_t>(maxS, d.S);
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t nt = (size_t)bins * 3 * sizeof(uint64_t);
  if (hipMemcpyAsync(dev_descs, descs, sizeof(m355_eval_calibration_desc) * n, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(top, 0, nt * n, st) != hipSuccess || hipMemsetAsync(classwise, 0, nt * C * n, st) != hipSuccess ||
      hipMemsetAsync(invalid, 0, sizeof(uint64_t) * C * n, st) != hipSuccess)
    return check_launch("eval_calibration: descriptor copy / memset");
  // one row of workgroups per subject, enough for the largest subject, about 8 per CU in all
  const int64_t want = ceil_div(maxS, (int64_t)CAL_NT * CAL_V);
  const int64_t cap = std::max<int64_t>(1, (int64_t)num_cus() * 8 / n);
  int64_t gx = std::max<int64_t>(1, std::min(want, cap));
  if (tuning().cal_blocks > 0) gx = tuning().cal_blocks;
  gx = std::min<int64_t>(gx, CAL_MAX_BLOCKS);
  CalArgs a{C, bins};
  const dim3 g((unsigned)gx, (unsigned)n), b(CAL_NT);
  const size_t lds = ((size_t)(1 + C) * bins * 3 + C) * sizeof(uint64_t);
  auto* dd = (const m355_eval_calibration_desc*)dev_descs;
  auto *t = (unsigned long long*)top, *c = (unsigned long long*)classwise, *iv = (unsigned long long*)invalid;
  double* part = (double*)workspace;
#define CAL_LAUNCH2(SD, BIN)                                                                           \
  if (onehot) hipLaunchKernelGGL((cal_kernel<SD, BIN, true>), g, b, lds, st, dd, a, t, c, iv, part);   \
  else hipLaunchKernelGGL((cal_kernel<SD, BIN, false>), g, b, lds, st, dd, a, t, c, iv, part);
#define CAL_LAUNCH(SD) \
  if (kind == M355_CAL_BINARY) { CAL_LAUNCH2(SD, true) } else { CAL_LAUNCH2(SD, false) }
  if (scores_dtype == M355_EV_F32) { CAL_LAUNCH(M355_EV_F32) }
  else if (scores_dtype == M355_EV_BF16) { CAL_LAUNCH(M355_EV_BF16) }
  else { CAL_LAUNCH(M355_EV_F16) }
#undef CAL_LAUNCH
#undef CAL_LAUNCH2
  if (int rc = check_launch("eval_calibration")) return rc;
  hipLaunchKernelGGL(cal_sum_kernel, dim3(n), dim3(64), 0, st, dd, part, (int)gx, sums, voxels);
  return check_launch("eval_calibration: sums");
}
