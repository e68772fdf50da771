// Segmentation evaluation counts (evaluators.py, prediction.add_evaluation_labels).
//
//   ev_confusion_kernel  counts[subject, label, {TP, FP, FN}] of a prediction label map against an optional target label
//                        map, every subject of a call in one launch (descriptor table, one grid row per subject)
//   ev_scores_kernel     the same counts straight from model scores: first-maximum argmax over the channels (a NaN is
//                        the maximum, as torch.argmax), a channel -> label value table chosen per voxel by a mask (the
//                        inverse of a masked CustomRemapLabels), optionally the int64 label maps written out
//   ev_multilabel_kernel counts[subject, channel, {TP, FP, FN}] of (score > threshold[channel]) against (target != 0),
//                        every channel on its own (sigmoid heads; evaluators.MultiLabelEvaluator)
//
// Voxel values are compared as the reference's `data == label_value` does: the label is first cast to the map's element
// type (uint8 -1 is 255, float32 compares with float(label)), then compared.  Every value becomes an int32 key on load;
// a value no label can equal (a non-integral or non-finite float, an int64 outside int32) becomes `nokey`, which the
// host picked outside every label's key.  Counting: labels <= 8 keep three counters per label in registers, more use an
// LDS histogram; the block's totals go out with one 64-bit atomic per (block, subject, label, stat) that is not zero.
// Integer counts: exact and independent of the order of the atomics.
#include "common.hpp"
#include "ev_load.hpp"

namespace {

using namespace m355::ev;

constexpr int EV_NT = 256;
constexpr int EV_REG_L = 8;
constexpr int EV_E = 16;      // label-map elements per lane and step (one 16-byte load of a byte map)
constexpr int EV_V = m355::ev::SCORE_V;   // voxels per lane and step of the score kernel (8 scores per channel load)

__device__ __forceinline__ int32_t fkey(float f, int32_t nokey) {
  return (f == truncf(f) && fabsf(f) < 2147483520.f) ? (int32_t)f : nokey;
}
__device__ __forceinline__ int32_t lkey(int64_t v, int32_t nokey) {
  return (v >= INT32_MIN && v <= INT32_MAX) ? (int32_t)v : nokey;
}

// the label's key in a map of element type dt (torch casts the Python scalar to the tensor's type)
__device__ __forceinline__ int32_t label_key(int32_t v, int dt, int32_t nokey) {
  switch (dt) {
    case M355_EV_U8: return (uint8_t)v;
    case M355_EV_I8: return (int8_t)v;
    case M355_EV_I16: return (int16_t)v;
    case M355_EV_F32: return fkey((float)v, nokey);
    default: return v;   // bool (0 / 1 compared as integers), int32, int64
  }
}

__device__ __forceinline__ int32_t load1(const void* p, int dt, int64_t i, int32_t nokey) {
  switch (dt) {
    case M355_EV_I8: return ((const int8_t*)p)[i];
    case M355_EV_I16: return ((const int16_t*)p)[i];
    case M355_EV_I32: return ((const int32_t*)p)[i];
    case M355_EV_I64: return lkey(((const int64_t*)p)[i], nokey);
    case M355_EV_F32: return fkey(((const float*)p)[i], nokey);
    default: return ((const uint8_t*)p)[i];   // bool, uint8
  }
}

// EV_E consecutive keys from element i (a multiple of EV_E; the map is 16-byte aligned): 16-byte loads
__device__ __forceinline__ void load16(const void* p, int dt, int64_t i, int32_t nokey, int32_t k[EV_E]) {
  switch (dt) {
    case M355_EV_I8: {
      const uint4 r = *(const uint4*)((const int8_t*)p + i);
      const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int j = 0; j < EV_E; ++j) k[j] = (int8_t)(w[j >> 2] >> (8 * (j & 3)));
      break;
    }
    case M355_EV_I16: {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint4 r = *(const uint4*)((const int16_t*)p + i + 8 * h);
        const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) k[8 * h + j] = (int16_t)(w[j >> 1] >> (16 * (j & 1)));
      }
      break;
    }
    case M355_EV_I32: {
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const int4 r = *(const int4*)((const int32_t*)p + i + 4 * h);
        k[4 * h] = r.x; k[4 * h + 1] = r.y; k[4 * h + 2] = r.z; k[4 * h + 3] = r.w;
      }
      break;
    }
    case M355_EV_F32: {
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const float4 r = *(const float4*)((const float*)p + i + 4 * h);
        k[4 * h] = fkey(r.x, nokey); k[4 * h + 1] = fkey(r.y, nokey);
        k[4 * h + 2] = fkey(r.z, nokey); k[4 * h + 3] = fkey(r.w, nokey);
      }
      break;
    }
    case M355_EV_I64: {
#pragma unroll
      for (int h = 0; h < 8; ++h) {
        const longlong2 r = *(const longlong2*)((const int64_t*)p + i + 2 * h);
        k[2 * h] = lkey(r.x, nokey); k[2 * h + 1] = lkey(r.y, nokey);
      }
      break;
    }
    default: {   // bool, uint8
      const uint4 r = *(const uint4*)((const uint8_t*)p + i);
      const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int j = 0; j < EV_E; ++j) k[j] = (w[j >> 2] >> (8 * (j & 3))) & 0xff;
    }
  }
}

// Per-block counters.  REG: three per label in registers (L <= EV_REG_L), summed over the wave and then the block at
// the end.  Otherwise an LDS histogram [label][stat].
template <bool REG>
struct Counter {
  uint32_t tp[EV_REG_L], fp[EV_REG_L], fn[EV_REG_L];
  int32_t kp[EV_REG_L], kt[EV_REG_L];
  int L;
  bool has_t;
  uint32_t* hist;        // LDS [64][3] (LDS mode)
  const int32_t* lkp;    // LDS label keys (LDS mode)
  const int32_t* lkt;

  __device__ void init(const int32_t* kp_lds, const int32_t* kt_lds, int L_, bool has_t_, uint32_t* hist_) {
    L = L_; has_t = has_t_; hist = hist_; lkp = kp_lds; lkt = kt_lds;
    if (REG) {
#pragma unroll
      for (int l = 0; l < EV_REG_L; ++l) {
        tp[l] = fp[l] = fn[l] = 0;
        kp[l] = l < L ? kp_lds[l] : 0;
        kt[l] = l < L ? kt_lds[l] : 0;
      }
    }
  }

  __device__ __forceinline__ void add(int32_t p, int32_t t) {
    if (REG) {
#pragma unroll
      for (int l = 0; l < EV_REG_L; ++l) {
        if (l < L) {
          const bool mp = p == kp[l], mt = has_t && t == kt[l];
          tp[l] += mp & mt;
          fp[l] += mp & !mt;
          fn[l] += !mp & mt;
        }
      }
    } else {
      for (int l = 0; l < L; ++l) {
        const bool mp = p == lkp[l], mt = has_t && t == lkt[l];
        if (mp | mt) atomicAdd(&hist[3 * l + (mp ? (mt ? 0 : 1) : 2)], 1u);
      }
    }
  }

  // block totals -> counts[3 * L] (global, 64-bit).  `red` is LDS of (EV_NT / 64) * 3 * EV_REG_L words.
  __device__ void flush(uint32_t* red, unsigned long long* counts) {
    if (REG) {
      const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
      for (int l = 0; l < EV_REG_L; ++l) {
        const uint32_t a = m355::wave_sum(tp[l]), b = m355::wave_sum(fp[l]), c = m355::wave_sum(fn[l]);
        if (lane == 0) {
          red[(w * EV_REG_L + l) * 3 + 0] = a;
          red[(w * EV_REG_L + l) * 3 + 1] = b;
          red[(w * EV_REG_L + l) * 3 + 2] = c;
        }
      }
      __syncthreads();
      if ((int)threadIdx.x < 3 * L) {
        unsigned long long s = 0;
        for (int i = 0; i < EV_NT / 64; ++i) s += red[i * EV_REG_L * 3 + threadIdx.x];
        if (s) atomicAdd(&counts[threadIdx.x], s);
      }
    } else {
      __syncthreads();
      for (int i = threadIdx.x; i < 3 * L; i += EV_NT)
        if (hist[i]) atomicAdd(&counts[i], (unsigned long long)hist[i]);
    }
  }
};

struct LabelArgs {
  int32_t v[M355_EV_MAX_LABELS];
  int32_t L, nokey;
};

// block setup shared by both kernels: label keys of the two maps' element types, zeroed histogram
__device__ void setup_keys(const LabelArgs& la, int dtp, int dtt, int32_t* kp, int32_t* kt, uint32_t* hist) {
  for (int i = threadIdx.x; i < la.L; i += EV_NT) {
    kp[i] = label_key(la.v[i], dtp, la.nokey);
    kt[i] = label_key(la.v[i], dtt, la.nokey);
  }
  for (int i = threadIdx.x; i < 3 * M355_EV_MAX_LABELS; i += EV_NT) hist[i] = 0;
  __syncthreads();
}

template <bool REG>
__global__ __launch_bounds__(EV_NT) void ev_confusion_kernel(const m355_eval_map_desc* __restrict__ descs, LabelArgs la,
                                                            unsigned long long* __restrict__ counts) {
  __shared__ int32_t kp_s[M355_EV_MAX_LABELS], kt_s[M355_EV_MAX_LABELS];
  __shared__ uint32_t hist[3 * M355_EV_MAX_LABELS];
  __shared__ uint32_t red[(EV_NT / 64) * 3 * EV_REG_L];
  const m355_eval_map_desc d = descs[blockIdx.y];
  const bool has_t = d.target != nullptr;
  const int dtp = d.pred_dtype, dtt = has_t ? d.target_dtype : M355_EV_I32;
  setup_keys(la, dtp, dtt, kp_s, kt_s, hist);
  Counter<REG> cnt;
  cnt.init(kp_s, kt_s, la.L, has_t, hist);

  const int64_t S = d.S;
  const int64_t g = (int64_t)blockIdx.x * EV_NT + threadIdx.x, gs = (int64_t)gridDim.x * EV_NT;
  const bool aligned = ((uintptr_t)d.pred & 15) == 0 && (!has_t || ((uintptr_t)d.target & 15) == 0);
  const int64_t Sv = aligned ? S / EV_E * EV_E : 0;
  for (int64_t i = g * EV_E; i < Sv; i += gs * EV_E) {
    int32_t p[EV_E], t[EV_E];
    load16(d.pred, dtp, i, la.nokey, p);
    if (has_t) load16(d.target, dtt, i, la.nokey, t);
#pragma unroll
    for (int j = 0; j < EV_E; ++j) cnt.add(p[j], has_t ? t[j] : la.nokey);
  }
  for (int64_t i = Sv + g; i < S; i += gs)
    cnt.add(load1(d.pred, dtp, i, la.nokey), has_t ? load1(d.target, dtt, i, la.nokey) : la.nokey);
  cnt.flush(red, counts + (int64_t)blockIdx.y * 3 * la.L);
}

// ---------------------------------------------------------------------------------------------- scores
struct ScoreArgs {
  int32_t table[2][M355_EV_MAX_CHANNELS];   // label value of channel c: [0] outside the mask, [1] inside
  int32_t C, scores_dtype, mask_kind, mask_axis, mask_upper;
};

// one-hot target values as doubles (exact for every integer type and for float32)
__device__ __forceinline__ double load_t1(const void* p, int dt, int64_t i) {
  switch (dt) {
    case M355_EV_I8: return ((const int8_t*)p)[i];
    case M355_EV_I16: return ((const int16_t*)p)[i];
    case M355_EV_I32: return ((const int32_t*)p)[i];
    case M355_EV_I64: return (double)((const int64_t*)p)[i];
    case M355_EV_F32: return ((const float*)p)[i];
    default: return ((const uint8_t*)p)[i];
  }
}

// EV_V consecutive one-hot values from element i (16-byte aligned, i a multiple of EV_V)
__device__ __forceinline__ void load_t8(const void* p, int dt, int64_t i, double t[EV_V]) {
  switch (dt) {
    case M355_EV_I32: {
      const int4 a = *(const int4*)((const int32_t*)p + i), b = *(const int4*)((const int32_t*)p + i + 4);
      t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w; t[4] = b.x; t[5] = b.y; t[6] = b.z; t[7] = b.w;
      break;
    }
    case M355_EV_F32: {
      const float4 a = *(const float4*)((const float*)p + i), b = *(const float4*)((const float*)p + i + 4);
      t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w; t[4] = b.x; t[5] = b.y; t[6] = b.z; t[7] = b.w;
      break;
    }
    case M355_EV_I64: {
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const longlong2 r = *(const longlong2*)((const int64_t*)p + i + 2 * h);
        t[2 * h] = (double)r.x; t[2 * h + 1] = (double)r.y;
      }
      break;
    }
    case M355_EV_I16: {
      const uint4 r = *(const uint4*)((const int16_t*)p + i);
      const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int j = 0; j < EV_V; ++j) t[j] = (int16_t)(w[j >> 1] >> (16 * (j & 1)));
      break;
    }
    default: {   // bool, uint8, int8
      const uint2 r = *(const uint2*)((const uint8_t*)p + i);
      const uint32_t w[2] = {r.x, r.y};
#pragma unroll
      for (int j = 0; j < EV_V; ++j) {
        const uint32_t b = (w[j >> 2] >> (8 * (j & 3))) & 0xff;
        t[j] = dt == M355_EV_I8 ? (double)(int8_t)b : (double)b;
      }
    }
  }
}

__device__ __forceinline__ bool nonzero(const void* p, int dt, int64_t s) {
  switch (dt) {
    case M355_EV_I16: return ((const int16_t*)p)[s] != 0;
    case M355_EV_I32: return ((const int32_t*)p)[s] != 0;
    case M355_EV_I64: return ((const int64_t*)p)[s] != 0;
    case M355_EV_F32: return ((const float*)p)[s] != 0.f;   // NaN counts, as torch's .bool()
    default: return ((const uint8_t*)p)[s] != 0;
  }
}

__device__ __forceinline__ bool inside(const ScoreArgs& a, const m355_eval_scores_desc& d, int64_t s) {
  if (a.mask_kind == M355_EV_MASK_HALF) {
    const int64_t hw = (int64_t)d.size3[1] * d.size3[2];
    int64_t o;
    if (a.mask_axis == 0) o = s / hw;
    else if (a.mask_axis == 1) o = (uint32_t)(s % hw) / (uint32_t)d.size3[2];
    else o = (uint32_t)(s % hw) % (uint32_t)d.size3[2];
    return (o >= d.size3[a.mask_axis] / 2) == (a.mask_upper != 0);
  }
  if (a.mask_kind == M355_EV_MASK_MAP) return nonzero(d.mask, d.mask_dtype, s);
  return false;
}

template <bool REG, int SD>
__global__ __launch_bounds__(EV_NT) void ev_scores_kernel(const m355_eval_scores_desc* __restrict__ descs, ScoreArgs a,
                                                         LabelArgs la, unsigned long long* __restrict__ counts) {
  __shared__ int32_t kp_s[M355_EV_MAX_LABELS], kt_s[M355_EV_MAX_LABELS];
  __shared__ uint32_t hist[3 * M355_EV_MAX_LABELS];
  __shared__ uint32_t red[(EV_NT / 64) * 3 * EV_REG_L];
  __shared__ int32_t table_s[2][M355_EV_MAX_CHANNELS];
  const m355_eval_scores_desc d = descs[blockIdx.y];
  const int tk = d.target ? d.target_kind : M355_EV_TARGET_NONE;
  // predicted labels come from the table and one-hot targets too; a target label map compares in its element type
  setup_keys(la, M355_EV_I32, tk == M355_EV_TARGET_MAP ? d.target_dtype : M355_EV_I32, kp_s, kt_s, hist);
  for (int i = threadIdx.x; i < 2 * a.C; i += EV_NT) table_s[i / a.C][i % a.C] = a.table[i / a.C][i % a.C];
  __syncthreads();
  Counter<REG> cnt;
  cnt.init(kp_s, kt_s, la.L, tk != M355_EV_TARGET_NONE, hist);

  const int C = a.C;
  const int64_t S = (int64_t)d.size3[0] * d.size3[1] * d.size3[2];
  const int64_t g = (int64_t)blockIdx.x * EV_NT + threadIdx.x, gs = (int64_t)gridDim.x * EV_NT;
  const bool aligned = S % EV_V == 0 && ((uintptr_t)d.scores & 15) == 0 &&
                       (tk != M355_EV_TARGET_ONEHOT || ((uintptr_t)d.target & 15) == 0) &&
                       (!d.pred_out || ((uintptr_t)d.pred_out & 15) == 0) &&
                       (!d.target_out || ((uintptr_t)d.target_out & 15) == 0);
  const int64_t Sv = aligned ? S : 0;
  for (int64_t i = g * EV_V; i < Sv; i += gs * EV_V) {
    float best[EV_V];
    int arg[EV_V];
    load_scores8<SD>(d.scores, i, best);
#pragma unroll
    for (int j = 0; j < EV_V; ++j) arg[j] = 0;
    for (int c = 1; c < C; ++c) {
      float s[EV_V];
      load_scores8<SD>(d.scores, (int64_t)c * S + i, s);
#pragma unroll
      for (int j = 0; j < EV_V; ++j)
        if (takes(best[j], s[j])) { best[j] = s[j]; arg[j] = c; }
    }
    int targ[EV_V];
    int32_t tmap[EV_V];
    if (tk == M355_EV_TARGET_ONEHOT) {
      double tb[EV_V];
      load_t8(d.target, d.target_dtype, i, tb);
#pragma unroll
      for (int j = 0; j < EV_V; ++j) targ[j] = 0;
      for (int c = 1; c < C; ++c) {
        double v[EV_V];
        load_t8(d.target, d.target_dtype, (int64_t)c * S + i, v);
#pragma unroll
        for (int j = 0; j < EV_V; ++j)
          if (takes(tb[j], v[j])) { tb[j] = v[j]; targ[j] = c; }
      }
    } else if (tk == M355_EV_TARGET_MAP) {
#pragma unroll
      for (int j = 0; j < EV_V; ++j) tmap[j] = load1(d.target, d.target_dtype, i + j, la.nokey);
    }
    int64_t po[EV_V], to[EV_V];
#pragma unroll
    for (int j = 0; j < EV_V; ++j) {
      const int m = inside(a, d, i + j) ? 1 : 0;
      const int32_t p = table_s[m][arg[j]];
      const int32_t t = tk == M355_EV_TARGET_ONEHOT ? table_s[m][targ[j]] : tk == M355_EV_TARGET_MAP ? tmap[j] : la.nokey;
      po[j] = p; to[j] = t;
      cnt.add(p, t);
    }
    if (d.pred_out)
#pragma unroll
      for (int h = 0; h < EV_V / 2; ++h) *(longlong2*)(d.pred_out + i + 2 * h) = make_longlong2(po[2 * h], po[2 * h + 1]);
    if (d.target_out && tk == M355_EV_TARGET_ONEHOT)
#pragma unroll
      for (int h = 0; h < EV_V / 2; ++h) *(longlong2*)(d.target_out + i + 2 * h) = make_longlong2(to[2 * h], to[2 * h + 1]);
  }
  for (int64_t i = Sv + g; i < S; i += gs) {
    float best = load_score1<SD>(d.scores, i);
    int arg = 0;
    for (int c = 1; c < C; ++c) {
      const float s = load_score1<SD>(d.scores, (int64_t)c * S + i);
      if (takes(best, s)) { best = s; arg = c; }
    }
    const int m = inside(a, d, i) ? 1 : 0;
    const int32_t p = table_s[m][arg];
    int32_t t = la.nokey;
    if (tk == M355_EV_TARGET_ONEHOT) {
      double tb = load_t1(d.target, d.target_dtype, i);
      int targ = 0;
      for (int c = 1; c < C; ++c) {
        const double v = load_t1(d.target, d.target_dtype, (int64_t)c * S + i);
        if (takes(tb, v)) { tb = v; targ = c; }
      }
      t = table_s[m][targ];
      if (d.target_out) d.target_out[i] = t;
    } else if (tk == M355_EV_TARGET_MAP) {
      t = load1(d.target, d.target_dtype, i, la.nokey);
    }
    if (d.pred_out) d.pred_out[i] = p;
    cnt.add(p, t);
  }
  cnt.flush(red, counts + (int64_t)blockIdx.y * 3 * la.L);
}

// ---------------------------------------------------------------------------------------------- multi-label
struct MultiArgs {
  float thr[M355_EV_MAX_CHANNELS];
  int32_t C;
};

// `!= 0` of a target element of any type: a float is positive unless it is +-0 (a NaN is), as torch's `!= 0`
__device__ __forceinline__ bool ml_pos1(const void* p, int dt, int64_t i) {
  switch (dt) {
    case M355_EV_I16: return ((const int16_t*)p)[i] != 0;
    case M355_EV_BF16:
    case M355_EV_F16: return (((const uint16_t*)p)[i] & 0x7fffu) != 0;
    case M355_EV_I32: return ((const int32_t*)p)[i] != 0;
    case M355_EV_I64: return ((const int64_t*)p)[i] != 0;
    case M355_EV_F32: return (((const uint32_t*)p)[i] & 0x7fffffffu) != 0;
    default: return ((const uint8_t*)p)[i] != 0;   // bool, uint8, int8
  }
}

// the same for EV_V consecutive elements from element i (a multiple of EV_V, the map 16-byte aligned): bit j = element j
__device__ __forceinline__ uint32_t ml_pos8(const void* p, int dt, int64_t i) {
  uint32_t m = 0;
  switch (dt) {
    case M355_EV_I16:
    case M355_EV_BF16:
    case M355_EV_F16: {
      const uint4 r = *(const uint4*)((const uint16_t*)p + i);
      const uint32_t w[4] = {r.x, r.y, r.z, r.w};
      const uint32_t keep = dt == M355_EV_I16 ? 0xffffu : 0x7fffu;
#pragma unroll
      for (int j = 0; j < EV_V; ++j) m |= (uint32_t)(((w[j >> 1] >> (16 * (j & 1))) & keep) != 0) << j;
      break;
    }
    case M355_EV_I32:
    case M355_EV_F32: {
      const uint4 a = *(const uint4*)((const uint32_t*)p + i), b = *(const uint4*)((const uint32_t*)p + i + 4);
      const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
      const uint32_t keep = dt == M355_EV_I32 ? 0xffffffffu : 0x7fffffffu;
#pragma unroll
      for (int j = 0; j < EV_V; ++j) m |= (uint32_t)((w[j] & keep) != 0) << j;
      break;
    }
    case M355_EV_I64: {
#pragma unroll
      for (int h = 0; h < EV_V / 2; ++h) {
        const longlong2 r = *(const longlong2*)((const int64_t*)p + i + 2 * h);
        m |= (uint32_t)(r.x != 0) << (2 * h) | (uint32_t)(r.y != 0) << (2 * h + 1);
      }
      break;
    }
    default: {   // bool, uint8, int8
      const uint2 r = *(const uint2*)((const uint8_t*)p + i);
      const uint32_t w[2] = {r.x, r.y};
#pragma unroll
      for (int j = 0; j < EV_V; ++j) m |= (uint32_t)(((w[j >> 2] >> (8 * (j & 3))) & 0xffu) != 0) << j;
    }
  }
  return m;
}

// counts[subject][c][{TP, FP, FN}] of (score > thr[c]) against (target != 0), channel by channel: three counters per
// lane, summed over the wave, added to the block's LDS table [C][3] by one lane, and from there with one 64-bit atomic
// per (block, channel, stat) that is not zero.  A lane counts fewer than 2^32 voxels (S < 2^40, 256 lanes a block).
template <int SD>
__global__ __launch_bounds__(EV_NT) void ev_multilabel_kernel(const m355_eval_multilabel_desc* __restrict__ descs,
                                                             MultiArgs a, unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long hist[3 * M355_EV_MAX_CHANNELS];
  const m355_eval_multilabel_desc d = descs[blockIdx.y];
  for (int i = threadIdx.x; i < 3 * a.C; i += EV_NT) hist[i] = 0;
  __syncthreads();
  const int64_t S = d.S;
  const int dt = d.target_dtype;
  const int64_t g = (int64_t)blockIdx.x * EV_NT + threadIdx.x, gs = (int64_t)gridDim.x * EV_NT;
  const bool aligned = S % EV_V == 0 && ((uintptr_t)d.scores & 15) == 0 && ((uintptr_t)d.target & 15) == 0;
  const int64_t Sv = aligned ? S : 0;
  for (int c = 0; c < a.C; ++c) {
    const float thr = a.thr[c];
    const int64_t row = (int64_t)c * S;
    uint32_t tp = 0, fp = 0, fn = 0;
    for (int64_t i = g * EV_V; i < Sv; i += gs * EV_V) {
      float s[EV_V];
      load_scores8<SD>(d.scores, row + i, s);
      const uint32_t m = ml_pos8(d.target, dt, row + i);
#pragma unroll
      for (int j = 0; j < EV_V; ++j) {
        const bool pr = s[j] > thr, ps = (m >> j) & 1u;   // a NaN score is not predicted
        tp += pr & ps;
        fp += pr & !ps;
        fn += !pr & ps;
      }
    }
    for (int64_t i = Sv + g; i < S; i += gs) {
      const bool pr = load_score1<SD>(d.scores, row + i) > thr, ps = ml_pos1(d.target, dt, row + i);
      tp += pr & ps;
      fp += pr & !ps;
      fn += !pr & ps;
    }
    const unsigned long long w0 = m355::wave_sum((unsigned long long)tp), w1 = m355::wave_sum((unsigned long long)fp),
                             w2 = m355::wave_sum((unsigned long long)fn);
    if ((threadIdx.x & 63) == 0) {
      if (w0) atomicAdd(&hist[3 * c + 0], w0);
      if (w1) atomicAdd(&hist[3 * c + 1], w1);
      if (w2) atomicAdd(&hist[3 * c + 2], w2);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * a.C; i += EV_NT)
    if (hist[i]) atomicAdd(&counts[(int64_t)blockIdx.y * 3 * a.C + i], hist[i]);
}

int check_labels(const char* what, const int32_t* labels, int32_t L, int32_t nokey, LabelArgs& la) {
  M355_REQUIRE(L >= 1 && L <= M355_EV_MAX_LABELS, M355_EUNSUPPORTED, "%s: %d labels (1 .. %d)", what, L,
               M355_EV_MAX_LABELS);
  M355_REQUIRE(labels, M355_EINVALID_ARG, "%s: null label table", what);
  la.L = L;
  la.nokey = nokey;
  for (int l = 0; l < L; ++l) {
    for (int m = 0; m < l; ++m)
      M355_REQUIRE(labels[m] != labels[l], M355_EINVALID_ARG, "%s: label value %d given twice", what, labels[l]);
    la.v[l] = labels[l];
  }
  return M355_OK;
}

int check_dt(const char* what, int32_t dt, bool scores) {
  if (scores)
    M355_REQUIRE(dt == M355_EV_F32 || dt == M355_EV_BF16 || dt == M355_EV_F16, M355_EINVALID_ARG,
                 "%s: score type %d (float32, bfloat16, float16)", what, dt);
  else
    M355_REQUIRE(dt >= M355_EV_BOOL && dt <= M355_EV_F32, M355_EINVALID_ARG, "%s: element type %d", what, dt);
  return M355_OK;
}

// grid: one row per subject, enough blocks for the largest subject, at most ~8 blocks per CU in all
dim3 ev_grid(int64_t maxS, int per_lane, int n) {
  const int64_t want = m355::ceil_div(maxS, (int64_t)EV_NT * per_lane);
  const int64_t cap = std::max<int64_t>(1, (int64_t)m355::num_cus() * 8 / n);
  return dim3((unsigned)std::max<int64_t>(1, std::min(want, cap)), (unsigned)n);
}

}  // namespace

extern "C" int m355_eval_confusion(const m355_eval_map_desc* descs, int32_t n, void* dev_descs, const int32_t* labels,
                                   int32_t L, int32_t nokey, uint64_t* counts, void* stream) {
  M355_REQUIRE(descs && dev_descs && counts, M355_EINVALID_ARG, "eval_confusion: null pointer");
  M355_REQUIRE(n >= 1 && n <= 65535, M355_EINVALID_ARG, "eval_confusion: %d subjects (1 .. 65535)", n);
  LabelArgs la{};
  if (int rc = check_labels("eval_confusion", labels, L, nokey, la)) return rc;
  int64_t maxS = 1;
  for (int i = 0; i < n; ++i) {
    M355_REQUIRE(descs[i].pred && descs[i].S >= 1, M355_EINVALID_ARG, "eval_confusion: subject %d: null map or %lld voxels",
                 i, (long long)descs[i].S);
    if (int rc = check_dt("eval_confusion: prediction", descs[i].pred_dtype, false)) return rc;
    if (descs[i].target)
      if (int rc = check_dt("eval_confusion: target", descs[i].target_dtype, false)) return rc;
    maxS = std::max<int64_t>(maxS, descs[i].S);
  }
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(dev_descs, descs, sizeof(m355_eval_map_desc) * n, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(counts, 0, sizeof(uint64_t) * 3 * L * n, st) != hipSuccess)
    return m355::check_launch("eval_confusion: descriptor copy / memset");
  const dim3 g = ev_grid(maxS, EV_E, n);
  auto* dd = (const m355_eval_map_desc*)dev_descs;
  auto* c = (unsigned long long*)counts;
  if (L <= EV_REG_L) hipLaunchKernelGGL(ev_confusion_kernel<true>, g, dim3(EV_NT), 0, st, dd, la, c);
  else hipLaunchKernelGGL(ev_confusion_kernel<false>, g, dim3(EV_NT), 0, st, dd, la, c);
  return m355::check_launch("eval_confusion");
}

extern "C" int m355_eval_scores(const m355_eval_scores_desc* descs, int32_t n, void* dev_descs, int32_t scores_dtype,
                                int32_t C, const int32_t* table, int32_t mask_kind, int32_t mask_axis, int32_t mask_upper,
                                const int32_t* labels, int32_t L, int32_t nokey, uint64_t* counts, void* stream) {
  M355_REQUIRE(descs && dev_descs && counts && table, M355_EINVALID_ARG, "eval_scores: null pointer");
  M355_REQUIRE(n >= 1 && n <= 65535, M355_EINVALID_ARG, "eval_scores: %d subjects (1 .. 65535)", n);
  M355_REQUIRE(C >= 1 && C <= M355_EV_MAX_CHANNELS, M355_EUNSUPPORTED, "eval_scores: %d channels (1 .. %d)", C,
               M355_EV_MAX_CHANNELS);
  if (int rc = check_dt("eval_scores", scores_dtype, true)) return rc;
  M355_REQUIRE(mask_kind >= M355_EV_MASK_NONE && mask_kind <= M355_EV_MASK_MAP, M355_EINVALID_ARG,
               "eval_scores: mask kind %d", mask_kind);
  M355_REQUIRE(mask_kind != M355_EV_MASK_HALF || (mask_axis >= 0 && mask_axis <= 2), M355_EINVALID_ARG,
               "eval_scores: half-space axis %d", mask_axis);
  LabelArgs la{};
  if (int rc = check_labels("eval_scores", labels, L, nokey, la)) return rc;
  ScoreArgs a{};
  a.C = C; a.scores_dtype = scores_dtype; a.mask_kind = mask_kind; a.mask_axis = mask_axis; a.mask_upper = mask_upper;
  for (int m = 0; m < 2; ++m)
    for (int c = 0; c < C; ++c) a.table[m][c] = table[m * C + c];
  int64_t maxS = 1;
  for (int i = 0; i < n; ++i) {
    const m355_eval_scores_desc& d = descs[i];
    M355_REQUIRE(d.scores, M355_EINVALID_ARG, "eval_scores: subject %d: null scores", i);
    for (int j = 0; j < 3; ++j)
      M355_REQUIRE(d.size3[j] >= 1, M355_EINVALID_ARG, "eval_scores: subject %d: size %d on axis %d", i, d.size3[j], j);
    const int64_t S = (int64_t)d.size3[0] * d.size3[1] * d.size3[2];
    M355_REQUIRE(S * C < ((int64_t)1 << 40), M355_EINVALID_ARG, "eval_scores: subject %d too large", i);
    M355_REQUIRE(d.target_kind >= M355_EV_TARGET_NONE && d.target_kind <= M355_EV_TARGET_MAP, M355_EINVALID_ARG,
                 "eval_scores: subject %d: target kind %d", i, d.target_kind);
    if (d.target && d.target_kind != M355_EV_TARGET_NONE)
      if (int rc = check_dt("eval_scores: target", d.target_dtype, false)) return rc;
    M355_REQUIRE(!d.target_out || d.target_kind == M355_EV_TARGET_ONEHOT, M355_EINVALID_ARG,
                 "eval_scores: subject %d: a target label map is written only from a one-hot target", i);
    if (mask_kind == M355_EV_MASK_MAP) {
      M355_REQUIRE(d.mask, M355_EINVALID_ARG, "eval_scores: subject %d: null mask map", i);
      if (int rc = check_dt("eval_scores: mask", d.mask_dtype, false)) return rc;
    }
    maxS = std::max<int64_t>(maxS, S);
  }
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(dev_descs, descs, sizeof(m355_eval_scores_desc) * n, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(counts, 0, sizeof(uint64_t) * 3 * L * n, st) != hipSuccess)
    return m355::check_launch("eval_scores: descriptor copy / memset");
  const dim3 g = ev_grid(maxS, EV_V, n), b(EV_NT);
  auto* dd = (const m355_eval_scores_desc*)dev_descs;
  auto* c = (unsigned long long*)counts;
  const bool reg = L <= EV_REG_L;
#define EV_LAUNCH(SD)                                                                      \
  if (reg) hipLaunchKernelGGL((ev_scores_kernel<true, SD>), g, b, 0, st, dd, a, la, c);    \
  else hipLaunchKernelGGL((ev_scores_kernel<false, SD>), g, b, 0, st, dd, a, la, c);
  if (scores_dtype == M355_EV_F32) { EV_LAUNCH(M355_EV_F32) }
  else if (scores_dtype == M355_EV_BF16) { EV_LAUNCH(M355_EV_BF16) }
  else { EV_LAUNCH(M355_EV_F16) }
#undef EV_LAUNCH
  return m355::check_launch("eval_scores");
}

extern "C" int m355_eval_multilabel(const m355_eval_multilabel_desc* descs, int32_t n, void* dev_descs, int32_t scores_dtype,
                                    int32_t C, const float* thresholds, uint64_t* counts, void* stream) {
  M355_REQUIRE(descs && dev_descs && counts && thresholds, M355_EINVALID_ARG, "eval_multilabel: null pointer");
  M355_REQUIRE(n >= 1 && n <= 65535, M355_EINVALID_ARG, "eval_multilabel: %d subjects (1 .. 65535)", n);
  M355_REQUIRE(C >= 1 && C <= M355_EV_MAX_CHANNELS, M355_EUNSUPPORTED, "eval_multilabel: %d channels (1 .. %d)", C,
               M355_EV_MAX_CHANNELS);
  if (int rc = check_dt("eval_multilabel", scores_dtype, true)) return rc;
  MultiArgs a{};
  a.C = C;
  for (int c = 0; c < C; ++c) a.thr[c] = thresholds[c];
  int64_t maxS = 1;
  for (int i = 0; i < n; ++i) {
    const m355_eval_multilabel_desc& d = descs[i];
    M355_REQUIRE(d.scores, M355_EINVALID_ARG, "eval_multilabel: subject %d: null scores", i);
    M355_REQUIRE(d.target, M355_EINVALID_ARG, "eval_multilabel: subject %d: null target", i);
    M355_REQUIRE(d.S >= 1 && d.S * C < ((int64_t)1 << 40), M355_EINVALID_ARG, "eval_multilabel: subject %d: %lld voxels", i,
                 (long long)d.S);
    M355_REQUIRE(d.target_dtype >= M355_EV_BOOL && d.target_dtype <= M355_EV_F16, M355_EINVALID_ARG,
                 "eval_multilabel: subject %d: target element type %d", i, d.target_dtype);
    maxS = std::max<int64_t>(maxS, d.S);
  }
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(dev_descs, descs, sizeof(m355_eval_multilabel_desc) * n, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(counts, 0, sizeof(uint64_t) * 3 * C * n, st) != hipSuccess)
    return m355::check_launch("eval_multilabel: descriptor copy / memset");
  const dim3 g = ev_grid(maxS, EV_V, n), b(EV_NT);
  auto* dd = (const m355_eval_multilabel_desc*)dev_descs;
  auto* c = (unsigned long long*)counts;
  if (scores_dtype == M355_EV_F32) hipLaunchKernelGGL(ev_multilabel_kernel<M355_EV_F32>, g, b, 0, st, dd, a, c);
  else if (scores_dtype == M355_EV_BF16) hipLaunchKernelGGL(ev_multilabel_kernel<M355_EV_BF16>, g, b, 0, st, dd, a, c);
  else hipLaunchKernelGGL(ev_multilabel_kernel<M355_EV_F16>, g, b, 0, st, dd, a, c);
  return m355::check_launch("eval_multilabel");
}
