// Preprocessing on the device: the per-voxel work of the deterministic torchio transforms that wrap the augmentations
// of the reference's production configs (research/dmri_hippo/configs/main_config.py:78-120,
// research/msseg2/msseg2.py:36-80).  Every bound, offset and shape is decided by preprocessing.py.
//
//   pre_bbox_kernel        bounding box + count of a predicate on one channel; one integer atomic per workgroup and value
//   pre_offsets_kernel     CropOrPad's mask-centred (or, for an empty mask, centred) offsets, one workgroup
//   pre_min_slice_kernel   np.pad 'minimum' tables: one workgroup per (channel, slice) reads the input once
//   pre_min_derive_kernel  ... the tables of two and three axes from the one-axis tables, one workgroup per channel
//   pre_gather_kernel      fused NaN -> crop / pad -> simultaneous label remap -> cast, one pass per tensor
//   pre_one_hot_kernel     one-hot in one pass, out-of-range labels counted
//   pre_ifl_kernel         image from labels, up to M355_PRE_MAX_ENTRIES entries in one pass
// Only integer atomics (min / max / add): results are deterministic.  No kernel hands data to another workgroup.
#include "common.hpp"

namespace m355 {

constexpr int PRE_NT = 256;
constexpr int PRE_MAX_LDS_KEYS = 8192;   // V1 + V2 of the 'minimum' tables (64 KiB of LDS)

static unsigned pre_grid(int64_t n, int64_t cap = 8192) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, PRE_NT), cap));
}

// ------------------------------------------------------------------------------------------------ element types
// order-preserving uint64 keys of every element type (the 'minimum' tables are mins of keys)
__device__ __forceinline__ uint64_t to_key(uint8_t v) { return v; }
__device__ __forceinline__ uint64_t to_key(int32_t v) { return (uint64_t)(int64_t)v ^ 0x8000000000000000ull; }
__device__ __forceinline__ uint64_t to_key(int64_t v) { return (uint64_t)v ^ 0x8000000000000000ull; }
__device__ __forceinline__ uint64_t to_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
template <typename T> __device__ __forceinline__ T from_key(uint64_t k);
template <> __device__ __forceinline__ uint8_t from_key<uint8_t>(uint64_t k) { return (uint8_t)k; }
template <> __device__ __forceinline__ int32_t from_key<int32_t>(uint64_t k) {
  return (int32_t)(int64_t)(k ^ 0x8000000000000000ull);
}
template <> __device__ __forceinline__ int64_t from_key<int64_t>(uint64_t k) { return (int64_t)(k ^ 0x8000000000000000ull); }
template <> __device__ __forceinline__ float from_key<float>(uint64_t k) {
  const uint32_t u = (uint32_t)k;
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

template <typename T> __device__ __forceinline__ T fix_nan(T v, int, double) { return v; }
template <> __device__ __forceinline__ float fix_nan<float>(float v, int on, double r) {
  return (on && v != v) ? (float)r : v;
}

// a double (label id, pad constant) in the element type: bool is v != 0, integers truncate
template <typename T> __device__ __forceinline__ T from_double(double d, bool is_bool) {
  if (is_bool) return (T)(d != 0.0);
  return (T)(int64_t)d;
}
template <> __device__ __forceinline__ float from_double<float>(double d, bool) { return (float)d; }

// element i of a map of any type, as a double
__device__ __forceinline__ double load_any(const void* p, int dtype, int64_t i) {
  switch (dtype) {
    case M355_PRE_I32: return (double)((const int32_t*)p)[i];
    case M355_PRE_I64: return (double)((const int64_t*)p)[i];
    case M355_PRE_F32: return (double)((const float*)p)[i];
    default: return (double)((const uint8_t*)p)[i];
  }
}

// store v (of type T) as element i of y in out_dtype, with torch's conversions
template <typename T> __device__ __forceinline__ void store_as(void* y, int dtype, int64_t i, T v) {
  switch (dtype) {
    case M355_PRE_U8: ((uint8_t*)y)[i] = (uint8_t)(int64_t)v; break;
    case M355_PRE_BOOL: ((uint8_t*)y)[i] = v != (T)0 ? 1 : 0; break;
    case M355_PRE_I32: ((int32_t*)y)[i] = (int32_t)v; break;
    case M355_PRE_I64: ((int64_t*)y)[i] = (int64_t)v; break;
    default: ((float*)y)[i] = (float)v; break;
  }
}

// ------------------------------------------------------------------------------------------------ bounding box
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
  return v;
}

template <typename T>
__global__ __launch_bounds__(PRE_NT) void pre_bbox_kernel(const T* __restrict__ x, int V0, int V1, int V2, int pred,
                                                          double value, int32_t* __restrict__ bb) {
  const int64_t S = (int64_t)V0 * V1 * V2;
  int lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {-1, -1, -1}, cnt = 0;
  for (int64_t s = (int64_t)blockIdx.x * PRE_NT + threadIdx.x; s < S; s += (int64_t)gridDim.x * PRE_NT) {
    const double v = (double)x[s];
    if (pred ? v == value : v != 0.0) {
      const int i2 = (int)(s % V2), r = (int)(s / V2), i1 = r % V1, i0 = r / V1;
      lo[0] = min(lo[0], i0); lo[1] = min(lo[1], i1); lo[2] = min(lo[2], i2);
      hi[0] = max(hi[0], i0); hi[1] = max(hi[1], i1); hi[2] = max(hi[2], i2);
      ++cnt;
    }
  }
  __shared__ int red[7][PRE_NT / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = wave_min_i(lo[a]);
    hi[a] = wave_max_i(hi[a]);
  }
  cnt = wave_sum(cnt);
  if (lane == 0) {
    for (int a = 0; a < 3; ++a) { red[a][w] = lo[a]; red[3 + a][w] = hi[a]; }
    red[6][w] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < PRE_NT / 64; ++k) {
      for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], red[a][k]); hi[a] = max(hi[a], red[3 + a][k]); }
      cnt += red[6][k];
    }
    if (cnt > 0) {
      const int V[3] = {V0, V1, V2};
      for (int a = 0; a < 3; ++a) {
        atomicMax(&bb[a], V[a] - lo[a]);
        atomicMax(&bb[3 + a], hi[a] + 1);
      }
      atomicAdd(&bb[6], cnt);
    }
  }
}

struct Int3 { int v[3]; };

__global__ void pre_offsets_kernel(const int32_t* __restrict__ bb, Int3 in, Int3 tgt, int32_t* __restrict__ off) {
  if (threadIdx.x != 0) return;
  const bool empty = bb[6] == 0;
  for (int a = 0; a < 3; ++a) {
    const int V = in.v[a], T = tgt.v[a];
    int o;
    if (!empty) {
      // 2 x centre = bb_min + bb_max; torchio moves it half a voxel down when target_even XOR centre_on_index, which
      // makes begin = centre - T / 2 an integer
      int c2 = (V - bb[a]) + bb[3 + a];
      if (((T & 1) == 0) != ((c2 & 1) == 0)) c2 -= 1;
      o = (c2 - T) / 2;
    } else {
      const int n = V - T;   // crop n > 0 or pad -n > 0: ceil(n / 2) in front
      o = n >= 0 ? (n + 1) / 2 : -((-n + 1) / 2);
    }
    off[a] = o;
  }
}

// ------------------------------------------------------------------------------------------------ 'minimum' tables
// per channel (uint64 keys): m0[V1 V2], m1[V0 V2], m2[V0 V1] (min over axis 0 / 1 / 2), m01[V2], m02[V1], m12[V0], m012
struct TableLayout {
  int64_t m0, m1, m2, m01, m02, m12, m012, per;
};
__host__ __device__ __forceinline__ TableLayout table_layout(int V0, int V1, int V2) {
  TableLayout t;
  t.m0 = 0;
  t.m1 = t.m0 + (int64_t)V1 * V2;
  t.m2 = t.m1 + (int64_t)V0 * V2;
  t.m01 = t.m2 + (int64_t)V0 * V1;
  t.m02 = t.m01 + V2;
  t.m12 = t.m02 + V1;
  t.m012 = t.m12 + V0;
  t.per = t.m012 + 1;
  return t;
}

template <typename T>
__global__ __launch_bounds__(PRE_NT) void pre_min_slice_kernel(const T* __restrict__ x, int V0, int V1, int V2, int rnan,
                                                               double nan_value, uint64_t* __restrict__ tab) {
  extern __shared__ unsigned long long lds_keys[];
  unsigned long long* row = lds_keys;        // [V1]: min over i2
  unsigned long long* col = lds_keys + V1;   // [V2]: min over i1
  const int i0 = blockIdx.x, c = blockIdx.y;
  const TableLayout L = table_layout(V0, V1, V2);
  uint64_t* t = tab + (int64_t)c * L.per;
  for (int k = threadIdx.x; k < V1 + V2; k += PRE_NT) lds_keys[k] = ~0ull;
  __syncthreads();
  const int plane = V1 * V2;
  const T* xs = x + ((int64_t)c * V0 + i0) * plane;
  for (int s = threadIdx.x; s < plane; s += PRE_NT) {
    const unsigned long long k = to_key(fix_nan(xs[s], rnan, nan_value));
    const int i1 = s / V2, i2 = s - i1 * V2;
    atomicMin(&row[i1], k);
    atomicMin(&col[i2], k);
    atomicMin((unsigned long long*)&t[L.m0 + s], k);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < V1; k += PRE_NT) t[L.m2 + (int64_t)i0 * V1 + k] = row[k];
  for (int k = threadIdx.x; k < V2; k += PRE_NT) t[L.m1 + (int64_t)i0 * V2 + k] = col[k];
}

__global__ __launch_bounds__(PRE_NT) void pre_min_derive_kernel(int V0, int V1, int V2, uint64_t* __restrict__ tab) {
  const TableLayout L = table_layout(V0, V1, V2);
  uint64_t* t = tab + (int64_t)blockIdx.x * L.per;
  uint64_t all = ~0ull;
  for (int i0 = threadIdx.x; i0 < V0; i0 += PRE_NT) {   // m12[i0] = min over i1 of m2[i0, i1]
    uint64_t m = ~0ull;
    for (int i1 = 0; i1 < V1; ++i1) m = min(m, t[L.m2 + (int64_t)i0 * V1 + i1]);
    t[L.m12 + i0] = m;
    all = min(all, m);
  }
  for (int i1 = threadIdx.x; i1 < V1; i1 += PRE_NT) {   // m02[i1] = min over i0 of m2[i0, i1]
    uint64_t m = ~0ull;
    for (int i0 = 0; i0 < V0; ++i0) m = min(m, t[L.m2 + (int64_t)i0 * V1 + i1]);
    t[L.m02 + i1] = m;
  }
  for (int i2 = threadIdx.x; i2 < V2; i2 += PRE_NT) {   // m01[i2] = min over i1 of m0[i1, i2]
    uint64_t m = ~0ull;
    for (int i1 = 0; i1 < V1; ++i1) m = min(m, t[L.m0 + (int64_t)i1 * V2 + i2]);
    t[L.m01 + i2] = m;
  }
  __shared__ unsigned long long red;
  if (threadIdx.x == 0) red = ~0ull;
  __syncthreads();
  atomicMin(&red, (unsigned long long)all);
  __syncthreads();
  if (threadIdx.x == 0) t[L.m012] = red;
}

// ------------------------------------------------------------------------------------------------ fused gather
struct GatherArgs {
  int C, src[3], base[3], in[3], out[3], off[3];
  const int32_t* off_dev;
  int pad_mode, rnan, nremap, mask_kind, mask_axis, mask_upper, mask_dtype, mask_C, out_dtype, in_bool;
  double pad_value, nan_value;
  double old_[M355_PRE_MAX_REMAP], new_[M355_PRE_MAX_REMAP];
  const void* mask_map;
  const uint64_t* tables;
};

template <typename T>
__global__ __launch_bounds__(PRE_NT) void pre_gather_kernel(const T* __restrict__ x, void* __restrict__ y, GatherArgs a) {
  const int64_t So = (int64_t)a.out[0] * a.out[1] * a.out[2], n = (int64_t)a.C * So;
  const int64_t Si = (int64_t)a.src[0] * a.src[1] * a.src[2];
  int off[3] = {a.off[0], a.off[1], a.off[2]};
  if (a.off_dev) {
    off[0] = a.off_dev[0]; off[1] = a.off_dev[1]; off[2] = a.off_dev[2];
  }
  const TableLayout L = table_layout(a.src[0], a.src[1], a.src[2]);
  const T padc = from_double<T>(a.pad_value, a.in_bool);
  for (int64_t e = (int64_t)blockIdx.x * PRE_NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * PRE_NT) {
    const int c = (int)(e / So);
    const int64_t s = e - (int64_t)c * So;
    const int o2 = (int)(s % a.out[2]), r = (int)(s / a.out[2]), o1 = r % a.out[1], o0 = r / a.out[1];
    const int i0 = o0 + off[0], i1 = o1 + off[1], i2 = o2 + off[2];
    const bool b0 = i0 < 0 || i0 >= a.in[0], b1 = i1 < 0 || i1 >= a.in[1], b2 = i2 < 0 || i2 >= a.in[2];
    T v;
    if (!(b0 || b1 || b2)) {
      const int64_t at = (int64_t)c * Si + ((int64_t)(i0 + a.base[0]) * a.src[1] + i1 + a.base[1]) * a.src[2] + i2 + a.base[2];
      v = fix_nan(x[at], a.rnan, a.nan_value);
    } else if (a.pad_mode == 0) {
      v = padc;
    } else {
      const uint64_t* t = a.tables + (int64_t)c * L.per;
      int64_t k;
      if (b0 && b1 && b2) k = L.m012;
      else if (b0 && b1) k = L.m01 + i2;
      else if (b0 && b2) k = L.m02 + i1;
      else if (b1 && b2) k = L.m12 + i0;
      else if (b0) k = L.m0 + (int64_t)i1 * a.in[2] + i2;
      else if (b1) k = L.m1 + (int64_t)i0 * a.in[2] + i2;
      else k = L.m2 + (int64_t)i0 * a.in[1] + i1;
      v = from_key<T>(t[k]);
    }
    if (a.nremap > 0) {
      bool m = true;
      if (a.mask_kind == M355_PRE_MASK_HALF) {
        const int o = a.mask_axis == 0 ? o0 : a.mask_axis == 1 ? o1 : o2;
        const int w = a.mask_axis == 0 ? a.out[0] : a.mask_axis == 1 ? a.out[1] : a.out[2];
        m = (o >= w / 2) == (a.mask_upper != 0);
      } else if (a.mask_kind == M355_PRE_MASK_MAP) {
        m = load_any(a.mask_map, a.mask_dtype, (a.mask_C == 1 ? 0 : (int64_t)c * So) + s) != 0.0;
      }
      if (m) {
        const double d = (double)v;
        int hit = -1;
#pragma unroll
        for (int k = 0; k < M355_PRE_MAX_REMAP; ++k)
          if (k < a.nremap && d == a.old_[k]) hit = k;
        double nv = 0.0;
#pragma unroll
        for (int k = 0; k < M355_PRE_MAX_REMAP; ++k)
          if (k == hit) nv = a.new_[k];
        if (hit >= 0) v = from_double<T>(nv, a.in_bool);
      }
    }
    store_as<T>(y, a.out_dtype, e, v);
  }
}

// ------------------------------------------------------------------------------------------------ one-hot
template <typename T> __device__ __forceinline__ int label_class(T v, int K) {   // -1: outside [0, K)
  const int64_t k = (int64_t)v;
  return (k >= 0 && k < K) ? (int)k : -1;
}
template <> __device__ __forceinline__ int label_class<float>(float v, int K) {
  return (v > -1.0f && v < (float)K) ? (int)v : -1;   // .long() truncates; NaN is outside
}

template <typename T>
__global__ __launch_bounds__(PRE_NT) void pre_one_hot_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t S, int K,
                                                             int32_t* __restrict__ bad) {
  int nbad = 0;
  for (int64_t s = (int64_t)blockIdx.x * PRE_NT + threadIdx.x; s < S; s += (int64_t)gridDim.x * PRE_NT) {
    const int k = label_class<T>(x[s], K);
    nbad += k < 0;
    for (int j = 0; j < K; ++j) y[(int64_t)j * S + s] = (T)(j == k ? 1 : 0);
  }
  __shared__ int red[PRE_NT / 64];
  nbad = block_sum<int, PRE_NT>(nbad, red);
  if (threadIdx.x == 0 && nbad) atomicAdd(bad, nbad);
}

// ------------------------------------------------------------------------------------------------ image from labels
struct IflArgs {
  m355_pre_label_entry e[M355_PRE_MAX_ENTRIES];
  int n, mode;
  int64_t S;
};

__global__ __launch_bounds__(PRE_NT) void pre_ifl_kernel(float* __restrict__ y, IflArgs a) {
  for (int64_t s = (int64_t)blockIdx.x * PRE_NT + threadIdx.x; s < a.S; s += (int64_t)gridDim.x * PRE_NT) {
    float out = 0.f;
#pragma unroll
    for (int j = 0; j < M355_PRE_MAX_ENTRIES; ++j) {
      if (j >= a.n) break;
      const m355_pre_label_entry& en = a.e[j];
      double lab;
      if (en.one_hot) {   // torch.argmax: the first maximum
        double best = load_any(en.map, en.dtype, s);
        int arg = 0;
        for (int k = 1; k < en.C; ++k) {
          const double v = load_any(en.map, en.dtype, (int64_t)k * a.S + s);
          if (v > best) { best = v; arg = k; }
        }
        lab = (double)arg;
      } else {
        lab = load_any(en.map, en.dtype, s);
      }
      const bool m = lab == en.id;
      if (a.mode == 0) {
        if (m) out = en.weight;
      } else {
        out = out + (m ? 1.f : 0.f) * en.weight;
      }
    }
    y[s] = out;
  }
}

// ------------------------------------------------------------------------------------------------ host
static int check_size3(const char* who, const int32_t* s) {
  M355_REQUIRE(s, M355_EINVALID_ARG, "%s: null size", who);
  M355_REQUIRE(s[0] > 0 && s[1] > 0 && s[2] > 0, M355_EINVALID_ARG, "%s: non-positive size %d x %d x %d", who, s[0],
               s[1], s[2]);
  M355_REQUIRE((int64_t)s[0] * s[1] * s[2] < ((int64_t)1 << 31), M355_EINVALID_ARG,
               "%s: %d x %d x %d has 2^31 voxels or more", who, s[0], s[1], s[2]);
  return M355_OK;
}

static int check_dtype(const char* who, int32_t d) {
  M355_REQUIRE(d >= M355_PRE_U8 && d <= M355_PRE_F32, M355_EINVALID_ARG, "%s: element type %d not in 0 .. 4", who, d);
  return M355_OK;
}

static int elem_bytes(int32_t d) { return d == M355_PRE_I64 ? 8 : (d == M355_PRE_I32 || d == M355_PRE_F32) ? 4 : 1; }

}  // namespace m355

using namespace m355;

extern "C" int m355_pre_bbox(const void* map, int32_t dtype, int32_t C, const int32_t* size3, int32_t channel,
                             int32_t pred, double value, int32_t* bbox, void* stream) {
  if (int rc = check_size3("pre_bbox", size3)) return rc;
  if (int rc = check_dtype("pre_bbox", dtype)) return rc;
  M355_REQUIRE(map && bbox, M355_EINVALID_ARG, "pre_bbox: null pointer");
  M355_REQUIRE(C > 0 && channel >= 0 && channel < C, M355_EINVALID_ARG, "pre_bbox: channel %d of %d", channel, C);
  M355_REQUIRE(pred == 0 || pred == 1, M355_EINVALID_ARG, "pre_bbox: predicate %d not in {0 (!= 0), 1 (== value)}", pred);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(bbox, 0, 7 * sizeof(int32_t), st) != hipSuccess) return check_launch("pre_bbox: memset");
  const int64_t S = (int64_t)size3[0] * size3[1] * size3[2];
  const dim3 g(pre_grid(S, 1024)), b(PRE_NT);
  const char* base = (const char*)map + (int64_t)channel * S * elem_bytes(dtype);
  switch (dtype) {
    case M355_PRE_I32:
      hipLaunchKernelGGL(pre_bbox_kernel<int32_t>, g, b, 0, st, (const int32_t*)base, size3[0], size3[1], size3[2], pred,
                         value, bbox);
      break;
    case M355_PRE_I64:
      hipLaunchKernelGGL(pre_bbox_kernel<int64_t>, g, b, 0, st, (const int64_t*)base, size3[0], size3[1], size3[2], pred,
                         value, bbox);
      break;
    case M355_PRE_F32:
      hipLaunchKernelGGL(pre_bbox_kernel<float>, g, b, 0, st, (const float*)base, size3[0], size3[1], size3[2], pred,
                         value, bbox);
      break;
    default:
      hipLaunchKernelGGL(pre_bbox_kernel<uint8_t>, g, b, 0, st, (const uint8_t*)base, size3[0], size3[1], size3[2], pred,
                         value, bbox);
  }
  return check_launch("pre_bbox");
}

extern "C" int m355_pre_crop_or_pad_offsets(const int32_t* bbox, const int32_t* in3, const int32_t* target3,
                                            int32_t* offsets, void* stream) {
  if (int rc = check_size3("pre_crop_or_pad_offsets: input", in3)) return rc;
  if (int rc = check_size3("pre_crop_or_pad_offsets: target", target3)) return rc;
  M355_REQUIRE(bbox && offsets, M355_EINVALID_ARG, "pre_crop_or_pad_offsets: null pointer");
  Int3 in{{in3[0], in3[1], in3[2]}}, tg{{target3[0], target3[1], target3[2]}};
  hipLaunchKernelGGL(pre_offsets_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, bbox, in, tg, offsets);
  return check_launch("pre_crop_or_pad_offsets");
}

extern "C" size_t m355_pre_min_tables_bytes(int32_t C, const int32_t* size3) {
  if (C <= 0 || check_size3("pre_min_tables_bytes", size3)) return 0;
  return (size_t)C * (size_t)table_layout(size3[0], size3[1], size3[2]).per * sizeof(uint64_t);
}

extern "C" int m355_pre_min_tables(const void* x, int32_t dtype, int32_t C, const int32_t* size3, int32_t replace_nan,
                                   double nan_value, void* tables, size_t bytes, void* stream) {
  if (int rc = check_size3("pre_min_tables", size3)) return rc;
  if (int rc = check_dtype("pre_min_tables", dtype)) return rc;
  M355_REQUIRE(x && tables && C > 0 && C <= 65535, M355_EINVALID_ARG, "pre_min_tables: null pointer or %d channels", C);
  M355_REQUIRE(size3[1] + size3[2] <= PRE_MAX_LDS_KEYS, M355_EINVALID_ARG, "pre_min_tables: V1 + V2 = %d > %d",
               size3[1] + size3[2], PRE_MAX_LDS_KEYS);
  const size_t need = m355_pre_min_tables_bytes(C, size3);
  M355_REQUIRE(bytes >= need, M355_EWORKSPACE, "pre_min_tables: %zu < %zu bytes", bytes, need);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(tables, 0xff, need, st) != hipSuccess) return check_launch("pre_min_tables: memset");
  const dim3 g(size3[0], C), b(PRE_NT);
  const size_t lds = (size_t)(size3[1] + size3[2]) * sizeof(uint64_t);
  uint64_t* t = (uint64_t*)tables;
  const int rn = replace_nan != 0;
  switch (dtype) {
    case M355_PRE_I32:
      hipLaunchKernelGGL(pre_min_slice_kernel<int32_t>, g, b, lds, st, (const int32_t*)x, size3[0], size3[1], size3[2], rn,
                         nan_value, t);
      break;
    case M355_PRE_I64:
      hipLaunchKernelGGL(pre_min_slice_kernel<int64_t>, g, b, lds, st, (const int64_t*)x, size3[0], size3[1], size3[2], rn,
                         nan_value, t);
      break;
    case M355_PRE_F32:
      hipLaunchKernelGGL(pre_min_slice_kernel<float>, g, b, lds, st, (const float*)x, size3[0], size3[1], size3[2], rn,
                         nan_value, t);
      break;
    default:
      hipLaunchKernelGGL(pre_min_slice_kernel<uint8_t>, g, b, lds, st, (const uint8_t*)x, size3[0], size3[1], size3[2], rn,
                         nan_value, t);
  }
  hipLaunchKernelGGL(pre_min_derive_kernel, dim3(C), dim3(PRE_NT), 0, st, size3[0], size3[1], size3[2], t);
  return check_launch("pre_min_tables");
}

extern "C" int m355_pre_gather(const m355_pre_gather_desc* d, void* stream) {
  M355_REQUIRE(d, M355_EINVALID_ARG, "pre_gather: null descriptor");
  if (int rc = check_size3("pre_gather: input", d->src3)) return rc;
  if (int rc = check_size3("pre_gather: box", d->in3)) return rc;
  if (int rc = check_size3("pre_gather: output", d->out3)) return rc;
  if (int rc = check_dtype("pre_gather: input", d->in_dtype)) return rc;
  if (int rc = check_dtype("pre_gather: output", d->out_dtype)) return rc;
  M355_REQUIRE(d->x && d->y && d->x != d->y, M355_EINVALID_ARG, "pre_gather: null pointer, or x == y");
  M355_REQUIRE(d->C > 0, M355_EINVALID_ARG, "pre_gather: %d channels", d->C);
  for (int j = 0; j < 3; ++j)
    M355_REQUIRE(d->base3[j] >= 0 && d->base3[j] + d->in3[j] <= d->src3[j], M355_EINVALID_ARG,
                 "pre_gather: box [%d, %d) outside 0 .. %d on axis %d", d->base3[j], d->base3[j] + d->in3[j], d->src3[j], j);
  if (d->pad_mode == 1)
    for (int j = 0; j < 3; ++j)
      M355_REQUIRE(d->base3[j] == 0 && d->in3[j] == d->src3[j], M355_EINVALID_ARG,
                   "pre_gather: 'minimum' padding of a box smaller than x (the tables are of all of x)");
  M355_REQUIRE(d->pad_mode == 0 || (d->pad_mode == 1 && d->tables), M355_EINVALID_ARG,
               "pre_gather: pad mode %d (0 constant, 1 minimum with tables)", d->pad_mode);
  M355_REQUIRE(d->nremap >= 0 && d->nremap <= M355_PRE_MAX_REMAP, M355_EINVALID_ARG, "pre_gather: %d remap pairs (0 .. %d)",
               d->nremap, M355_PRE_MAX_REMAP);
  M355_REQUIRE(d->mask_kind >= M355_PRE_MASK_NONE && d->mask_kind <= M355_PRE_MASK_MAP, M355_EINVALID_ARG,
               "pre_gather: mask kind %d", d->mask_kind);
  if (d->mask_kind == M355_PRE_MASK_HALF)
    M355_REQUIRE(d->mask_axis >= 0 && d->mask_axis <= 2, M355_EINVALID_ARG, "pre_gather: half-space axis %d", d->mask_axis);
  if (d->mask_kind == M355_PRE_MASK_MAP) {
    if (int rc = check_dtype("pre_gather: mask", d->mask_dtype)) return rc;
    M355_REQUIRE(d->mask_map && (d->mask_C == 1 || d->mask_C == d->C), M355_EINVALID_ARG,
                 "pre_gather: mask map null or of %d channels (1 or %d)", d->mask_C, d->C);
  }
  GatherArgs a{};
  a.C = d->C;
  for (int j = 0; j < 3; ++j) {
    a.src[j] = d->src3[j]; a.base[j] = d->base3[j];
    a.in[j] = d->in3[j]; a.out[j] = d->out3[j]; a.off[j] = d->off3[j];
  }
  a.off_dev = d->off_dev;
  a.pad_mode = d->pad_mode; a.pad_value = d->pad_value; a.tables = (const uint64_t*)d->tables;
  a.rnan = d->replace_nan != 0; a.nan_value = d->nan_value;
  a.nremap = d->nremap;
  for (int k = 0; k < d->nremap; ++k) { a.old_[k] = d->remap_old[k]; a.new_[k] = d->remap_new[k]; }
  a.mask_kind = d->nremap ? d->mask_kind : M355_PRE_MASK_NONE;
  a.mask_axis = d->mask_axis; a.mask_upper = d->mask_upper;
  a.mask_map = d->mask_map; a.mask_dtype = d->mask_dtype; a.mask_C = d->mask_C;
  a.out_dtype = d->out_dtype; a.in_bool = d->in_dtype == M355_PRE_BOOL;
  const int64_t n = (int64_t)d->C * d->out3[0] * d->out3[1] * d->out3[2];
  hipStream_t st = (hipStream_t)stream;
  const dim3 g(pre_grid(n)), b(PRE_NT);
  switch (d->in_dtype) {
    case M355_PRE_I32: hipLaunchKernelGGL(pre_gather_kernel<int32_t>, g, b, 0, st, (const int32_t*)d->x, d->y, a); break;
    case M355_PRE_I64: hipLaunchKernelGGL(pre_gather_kernel<int64_t>, g, b, 0, st, (const int64_t*)d->x, d->y, a); break;
    case M355_PRE_F32: hipLaunchKernelGGL(pre_gather_kernel<float>, g, b, 0, st, (const float*)d->x, d->y, a); break;
    default: hipLaunchKernelGGL(pre_gather_kernel<uint8_t>, g, b, 0, st, (const uint8_t*)d->x, d->y, a);
  }
  return check_launch("pre_gather");
}

extern "C" int m355_pre_one_hot(const void* x, int32_t dtype, const int32_t* size3, int32_t K, void* y, int32_t* bad,
                                void* stream) {
  if (int rc = check_size3("pre_one_hot", size3)) return rc;
  if (int rc = check_dtype("pre_one_hot", dtype)) return rc;
  M355_REQUIRE(x && y && bad && x != y, M355_EINVALID_ARG, "pre_one_hot: null pointer, or x == y");
  M355_REQUIRE(K >= 1 && K <= 1024, M355_EINVALID_ARG, "pre_one_hot: %d classes (1 .. 1024)", K);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(bad, 0, sizeof(int32_t), st) != hipSuccess) return check_launch("pre_one_hot: memset");
  const int64_t S = (int64_t)size3[0] * size3[1] * size3[2];
  const dim3 g(pre_grid(S)), b(PRE_NT);
  switch (dtype) {
    case M355_PRE_I32:
      hipLaunchKernelGGL(pre_one_hot_kernel<int32_t>, g, b, 0, st, (const int32_t*)x, (int32_t*)y, S, K, bad);
      break;
    case M355_PRE_I64:
      hipLaunchKernelGGL(pre_one_hot_kernel<int64_t>, g, b, 0, st, (const int64_t*)x, (int64_t*)y, S, K, bad);
      break;
    case M355_PRE_F32:
      hipLaunchKernelGGL(pre_one_hot_kernel<float>, g, b, 0, st, (const float*)x, (float*)y, S, K, bad);
      break;
    default:
      hipLaunchKernelGGL(pre_one_hot_kernel<uint8_t>, g, b, 0, st, (const uint8_t*)x, (uint8_t*)y, S, K, bad);
  }
  return check_launch("pre_one_hot");
}

extern "C" int m355_pre_image_from_labels(const m355_pre_label_entry* entries, int32_t n, const int32_t* size3,
                                          int32_t mode, float* y, void* stream) {
  if (int rc = check_size3("pre_image_from_labels", size3)) return rc;
  M355_REQUIRE(y && (n == 0 || entries), M355_EINVALID_ARG, "pre_image_from_labels: null pointer");
  M355_REQUIRE(n >= 0 && n <= M355_PRE_MAX_ENTRIES, M355_EINVALID_ARG, "pre_image_from_labels: %d entries (0 .. %d)", n,
               M355_PRE_MAX_ENTRIES);
  M355_REQUIRE(mode == 0 || mode == 1, M355_EINVALID_ARG, "pre_image_from_labels: mode %d (0 overwrite, 1 additive)", mode);
  IflArgs a{};
  a.n = n; a.mode = mode;
  a.S = (int64_t)size3[0] * size3[1] * size3[2];
  for (int j = 0; j < n; ++j) {
    if (int rc = check_dtype("pre_image_from_labels", entries[j].dtype)) return rc;
    M355_REQUIRE(entries[j].map && entries[j].C >= 1, M355_EINVALID_ARG, "pre_image_from_labels: entry %d: null map or "
                 "%d channels", j, entries[j].C);
    a.e[j] = entries[j];
  }
  hipLaunchKernelGGL(pre_ifl_kernel, dim3(pre_grid(a.S)), dim3(PRE_NT), 0, (hipStream_t)stream, y, a);
  return check_launch("pre_image_from_labels");
}
