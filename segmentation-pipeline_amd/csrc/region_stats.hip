// Statistics of image values grouped by the label of the voxel (ops.region_stats, evaluators.ImageRegionEvaluator,
// data_processing/dataset_fingerprint.py).
//
// Regions of a call with L label values: 0 .. L-1 the listed values (`data == value`, the value cast to the map's
// element type as in evaluate.hip), L = 'all' (label != 0), L + 1 = 'whole' (every voxel).  A voxel lies in at most one
// listed region, so it feeds at most three.
//
//   rs_init_kernel      sentinels of counts / bounds, the 'whole' row, zeroed histograms and min / max keys
//   rs_count_kernel     voxel count and bounding box of every region: one pass over the label map
//   rs_sum_kernel       per image: sum of the values (fp64), min / max as order-preserving keys
//   rs_mean_kernel      fixed-order sum of the block partials -> mean, and the rank (n - 1) / 2 of the median
//   rs_scan_kernel      sum of (x - mean)^2 (DEV) and / or one digit histogram of the radix select (HIST); pass 0 does
//                       both in one read of the volume
//   rs_pick_kernel      one wave per region: bucket of the remaining rank, next prefix, histogram cleared
//   rs_finalize_kernel  mean, unbiased std, median, min, max as float32, each rounded once from fp64 / exact keys
//
// How a block keeps its L + 2 accumulators.  Counts and bounds are integers: a thread keeps its current run of voxels
// of one listed region in registers and adds it to the block's LDS table with integer atomics when the region changes.
// Floating-point sums: 'all' and 'whole' live in registers of every thread and meet in a fixed-order block reduction.
// For the listed regions every step of a wave visits the distinct regions among its 64 voxels (usually one), reduces
// the lanes of that region with a masked butterfly and lets lane 0 add the result to the wave's own LDS slot of that
// region: which lanes are summed in which order depends on the data and the launch geometry only, never on timing.
// Block partials go to the workspace and are summed by one wave per region, lane j taking blocks j, j + 64, ... in
// turn before a butterfly over the lanes: a fixed order again.  Min / max keys and histograms are integers and use
// integer atomics as well.  No floating-point atomic anywhere: two calls give the same bits.
//
// The median is the radix select of radix_select.hpp, one query per region.  RS_HG histograms of RADIX_BINS bins fit a
// block, so a pass runs ceil((L + 2) / RS_HG) region groups as grid.y; each group reads the volume and counts only its
// own regions.
#include "radix_select.hpp"
#include <hip/hip_fp16.h>
#include <limits.h>
#include <math.h>

namespace {

using namespace m355;

constexpr int RS_NT = 256;          // threads of a block
constexpr int RS_U = 8;             // voxels a lane loads ahead per step of the grid-stride loop
constexpr int RS_GRID_CAP = 1024;   // blocks along x: four per CU
constexpr int RS_HG = 7;            // histograms (regions) of one block of a select pass: 56 KB of LDS
constexpr int RS_MAX_L = 64;
constexpr int RS_MAX_R = RS_MAX_L + 2;
constexpr int64_t RS_TILE = (int64_t)RS_NT * RS_U;

struct Keys {
  int32_t k[RS_MAX_L];   // the label values as keys of the map's element type
  int32_t L, nokey;
};

__host__ __device__ __forceinline__ int32_t fkey(float f, int32_t nokey) {
  return (f == truncf(f) && fabsf(f) < 2147483520.f) ? (int32_t)f : nokey;
}

__device__ __forceinline__ int32_t load_key(const void* p, int dt, int64_t i, int32_t nokey) {
  switch (dt) {
    case M355_EV_I8: return ((const int8_t*)p)[i];
    case M355_EV_I16: return ((const int16_t*)p)[i];
    case M355_EV_I32: return ((const int32_t*)p)[i];
    case M355_EV_I64: {
      const int64_t v = ((const int64_t*)p)[i];
      return (v >= INT32_MIN && v <= INT32_MAX) ? (int32_t)v : nokey;
    }
    case M355_EV_F32: return fkey(((const float*)p)[i], nokey);
    default: return ((const uint8_t*)p)[i];   // bool, uint8
  }
}

// every image type converts to fp32 exactly
__device__ __forceinline__ float load_val(const void* p, int dt, int64_t i) {
  switch (dt) {
    case M355_EV_F16: return __half2float(__ushort_as_half(((const uint16_t*)p)[i]));
    case M355_EV_BF16: return __uint_as_float((uint32_t)((const uint16_t*)p)[i] << 16);
    case M355_EV_U8: return (float)((const uint8_t*)p)[i];
    case M355_EV_I16: return (float)((const int16_t*)p)[i];
    default: return ((const float*)p)[i];
  }
}

// index of the first listed value equal to `key`, -1 when there is none; (lastkey, lastidx) remember the thread's
// previous voxel, which in a label map is nearly always the same region
__device__ __forceinline__ int find_region(int32_t key, const int32_t* skeys, int L, int32_t& lastkey, int& lastidx) {
  if (key != lastkey) {
    int idx = -1;
    for (int l = L - 1; l >= 0; --l)
      if (skeys[l] == key) idx = l;
    lastkey = key;
    lastidx = idx;
  }
  return lastidx;
}

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
__device__ __forceinline__ uint32_t wave_max_u(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, off, 64));
  return v;
}

// f(r, mine) once for every distinct region r >= 0 among the wave's `idx`, in the order of the lowest lane holding
// it; `mine` marks the lanes of r.  Every lane of the wave must call this (the loop is wave-uniform).
template <typename F>
__device__ __forceinline__ void for_each_region(int idx, F f) {
  unsigned long long todo = __ballot(idx >= 0);
  while (todo) {
    const int lead = __ffsll((long long)todo) - 1;
    const int r = __shfl(idx, lead, 64);
    const bool mine = idx == r;
    f(r, mine);
    todo &= ~__ballot(mine);
  }
}

// the keys of U voxels of a tile: idx[u] (-1: in no listed region, or past the end), nz bit u (label != 0)
struct TileLabels {
  int idx[RS_U];
  uint32_t nz, valid;
};

__device__ __forceinline__ void load_tile_labels(const void* lab, int dt, int64_t base, int64_t S, const int32_t* skeys,
                                                 const Keys& K, int32_t& lastkey, int& lastidx, TileLabels& t) {
  int32_t key[RS_U];
#pragma unroll
  for (int u = 0; u < RS_U; ++u) {
    const int64_t i = base + (int64_t)u * RS_NT + threadIdx.x;
    key[u] = i < S ? load_key(lab, dt, i, K.nokey) : 0;
  }
  t.nz = 0;
  t.valid = 0;
#pragma unroll
  for (int u = 0; u < RS_U; ++u) {
    const int64_t i = base + (int64_t)u * RS_NT + threadIdx.x;
    const bool v = i < S;
    t.idx[u] = v ? find_region(key[u], skeys, K.L, lastkey, lastidx) : -1;
    t.valid |= (uint32_t)v << u;
    t.nz |= (uint32_t)(v && key[u] != 0) << u;
  }
}

__device__ __forceinline__ void stage_keys(int32_t* skeys, const Keys& K) {
  for (int l = threadIdx.x; l < RS_MAX_L; l += RS_NT) skeys[l] = l < K.L ? K.k[l] : K.nokey;
}

// ------------------------------------------------------------------------------------------------ init
__global__ __launch_bounds__(RS_NT) void rs_init_kernel(int64_t* __restrict__ count, int32_t* __restrict__ bounds, int L,
                                                        int W, int H, int D, uint32_t* __restrict__ kmm,
                                                        uint32_t* __restrict__ hist, int64_t nhist) {
  const int64_t t = blockIdx.x * (int64_t)RS_NT + threadIdx.x;
  const int size[3] = {W, H, D};
  if (t <= L + 1) {
    const bool whole = t == L + 1;
    count[t] = whole ? (int64_t)W * H * D : 0;
    for (int a = 0; a < 3; ++a) {
      bounds[t * 6 + 2 * a] = whole ? 0 : size[a];
      bounds[t * 6 + 2 * a + 1] = whole ? size[a] - 1 : -1;
    }
    if (kmm) { kmm[2 * t] = 0u; kmm[2 * t + 1] = 0u; }
  }
  for (int64_t i = t; i < nhist; i += (int64_t)gridDim.x * RS_NT) hist[i] = 0u;
}

// ------------------------------------------------------------------------------------------------ counts and bounds
__global__ __launch_bounds__(RS_NT) void rs_count_kernel(const void* __restrict__ lab, int dt, int64_t S, int H, int D,
                                                         Keys K, int64_t* __restrict__ count,
                                                         int32_t* __restrict__ bounds) {
  __shared__ int32_t skeys[RS_MAX_L];
  __shared__ uint32_t scnt[RS_MAX_L + 1];
  __shared__ int32_t smin[RS_MAX_L + 1][3], smax[RS_MAX_L + 1][3];
  stage_keys(skeys, K);
  for (int r = threadIdx.x; r <= RS_MAX_L; r += RS_NT) {
    scnt[r] = 0u;
    for (int a = 0; a < 3; ++a) { smin[r][a] = INT_MAX; smax[r][a] = -1; }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t HD = (int64_t)H * D;
  uint32_t acnt = 0;
  int amin[3] = {INT_MAX, INT_MAX, INT_MAX}, amax[3] = {-1, -1, -1};
  int32_t lastkey = K.nokey;
  int lastidx = -1;
  int cur = -1;
  uint32_t ccnt = 0;
  int cmin[3] = {INT_MAX, INT_MAX, INT_MAX}, cmax[3] = {-1, -1, -1};
  auto flush_run = [&]() {
    if (ccnt) {
      atomicAdd(&scnt[cur], ccnt);
#pragma unroll
      for (int a = 0; a < 3; ++a) { atomicMin(&smin[cur][a], cmin[a]); atomicMax(&smax[cur][a], cmax[a]); }
    }
    ccnt = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) { cmin[a] = INT_MAX; cmax[a] = -1; }
  };
  for (int64_t base = blockIdx.x * RS_TILE; base < S; base += (int64_t)gridDim.x * RS_TILE) {
    TileLabels t;
    load_tile_labels(lab, dt, base, S, skeys, K, lastkey, lastidx, t);
#pragma unroll
    for (int u = 0; u < RS_U; ++u) {
      const int64_t i = base + (int64_t)u * RS_NT + threadIdx.x;
      int c[3] = {0, 0, 0};
      if ((t.valid >> u) & 1) {
        if (S <= INT32_MAX) {
          const uint32_t ii = (uint32_t)i, hd = (uint32_t)HD, x = ii / hd, rem = ii - x * hd, y = rem / (uint32_t)D;
          c[0] = (int)x; c[1] = (int)y; c[2] = (int)(rem - y * (uint32_t)D);
        } else {
          const int64_t x = i / HD, rem = i - x * HD, y = rem / D;
          c[0] = (int)x; c[1] = (int)y; c[2] = (int)(rem - y * D);
        }
      }
      if ((t.nz >> u) & 1) {
        ++acnt;
#pragma unroll
        for (int a = 0; a < 3; ++a) { amin[a] = min(amin[a], c[a]); amax[a] = max(amax[a], c[a]); }
      }
      // the thread's run of voxels of one listed region stays in registers; it goes to the block's table when the
      // region changes (integer atomics: the order does not matter)
      if (((t.valid >> u) & 1) && t.idx[u] != cur) {
        flush_run();
        cur = t.idx[u];
      }
      if (t.idx[u] >= 0) {
        ++ccnt;
#pragma unroll
        for (int a = 0; a < 3; ++a) { cmin[a] = min(cmin[a], c[a]); cmax[a] = max(cmax[a], c[a]); }
      }
    }
  }
  flush_run();
  // 'all': the threads' registers meet in the block's table
  {
    uint32_t n = acnt;
    for (int off = 32; off > 0; off >>= 1) n += (uint32_t)__shfl_xor((int)n, off, 64);
    int lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = wave_min_i(amin[a]); hi[a] = wave_max_i(amax[a]); }
    if (lane == 0 && n) {
      atomicAdd(&scnt[K.L], n);
#pragma unroll
      for (int a = 0; a < 3; ++a) { atomicMin(&smin[K.L][a], lo[a]); atomicMax(&smax[K.L][a], hi[a]); }
    }
  }
  __syncthreads();
  for (int r = threadIdx.x; r <= K.L; r += RS_NT) {
    if (!scnt[r]) continue;
    atomicAdd((unsigned long long*)&count[r], (unsigned long long)scnt[r]);
    for (int a = 0; a < 3; ++a) {
      atomicMin(&bounds[r * 6 + 2 * a], smin[r][a]);
      atomicMax(&bounds[r * 6 + 2 * a + 1], smax[r][a]);
    }
  }
}

// ------------------------------------------------------------------------------------------------ sum, min, max
// part[block * R + r]: the block's sum of region r; kmm[2 r] = max(~key), kmm[2 r + 1] = max(key)
__global__ __launch_bounds__(RS_NT) void rs_sum_kernel(const void* __restrict__ lab, int dt, const void* __restrict__ img,
                                                       int idt, int C, int64_t S, Keys K, double* __restrict__ part,
                                                       uint32_t* __restrict__ kmm) {
  __shared__ int32_t skeys[RS_MAX_L];
  __shared__ double ssum[RS_NT / 64][RS_MAX_L];
  __shared__ uint32_t skmin[RS_MAX_R], skmax[RS_MAX_R];
  __shared__ double scratch[RS_NT / 64];
  stage_keys(skeys, K);
  for (int r = threadIdx.x; r < RS_MAX_R; r += RS_NT) { skmin[r] = 0u; skmax[r] = 0u; }
  for (int j = threadIdx.x; j < (RS_NT / 64) * RS_MAX_L; j += RS_NT) (&ssum[0][0])[j] = 0.0;
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int R = K.L + 2;
  double s_all = 0.0, s_whole = 0.0;
  uint32_t kmin_all = 0u, kmax_all = 0u, kmin_whole = 0u, kmax_whole = 0u;
  int32_t lastkey = K.nokey;
  int lastidx = -1;
  for (int64_t base = blockIdx.x * RS_TILE; base < S; base += (int64_t)gridDim.x * RS_TILE) {
    TileLabels t;
    load_tile_labels(lab, dt, base, S, skeys, K, lastkey, lastidx, t);
    for (int c = 0; c < C; ++c) {
      float xs[RS_U];
#pragma unroll
      for (int u = 0; u < RS_U; ++u) {
        const int64_t i = base + (int64_t)u * RS_NT + threadIdx.x;
        xs[u] = i < S ? load_val(img, idt, (int64_t)c * S + i) : 0.f;
      }
#pragma unroll
      for (int u = 0; u < RS_U; ++u) {
        const double xd = (double)xs[u];
        const uint32_t key = f2key(xs[u]);
        if ((t.valid >> u) & 1) {
          s_whole += xd;
          kmin_whole = max(kmin_whole, ~key);
          kmax_whole = max(kmax_whole, key);
        }
        if ((t.nz >> u) & 1) {
          s_all += xd;
          kmin_all = max(kmin_all, ~key);
          kmax_all = max(kmax_all, key);
        }
        for_each_region(t.idx[u], [&](int r, bool mine) {
          const double v = wave_sum(mine ? xd : 0.0);
          const uint32_t a = wave_max_u(mine ? ~key : 0u), b = wave_max_u(mine ? key : 0u);
          if (lane == 0) {
            ssum[w][r] += v;
            atomicMax(&skmin[r], a);
            atomicMax(&skmax[r], b);
          }
        });
      }
    }
  }
  const uint32_t a0 = wave_max_u(kmin_all), a1 = wave_max_u(kmax_all);
  const uint32_t w0 = wave_max_u(kmin_whole), w1 = wave_max_u(kmax_whole);
  if (lane == 0) {
    atomicMax(&skmin[K.L], a0);
    atomicMax(&skmax[K.L], a1);
    atomicMax(&skmin[K.L + 1], w0);
    atomicMax(&skmax[K.L + 1], w1);
  }
  const double t_all = block_sum<double, RS_NT>(s_all, scratch);
  const double t_whole = block_sum<double, RS_NT>(s_whole, scratch);
  __syncthreads();
  double* o = part + (int64_t)blockIdx.x * R;
  if (threadIdx.x == 0) { o[K.L] = t_all; o[K.L + 1] = t_whole; }
  for (int r = threadIdx.x; r < K.L; r += RS_NT) {
    double v = 0.0;
#pragma unroll
    for (int ww = 0; ww < RS_NT / 64; ++ww) v += ssum[ww][r];
    o[r] = v;
  }
  for (int r = threadIdx.x; r < R; r += RS_NT) {
    if (skmin[r]) atomicMax(&kmm[2 * r], skmin[r]);
    if (skmax[r]) atomicMax(&kmm[2 * r + 1], skmax[r]);
  }
}

// the block partials of region r in a fixed order: lane j of the wave adds blocks j, j + 64, ... in turn, then the 64
// lane sums meet in a butterfly; every lane returns the total
__device__ __forceinline__ double sum_partials(const double* __restrict__ part, int nblk, int R, int r) {
  double s = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 64) s += part[(int64_t)b * R + r];
  return wave_sum(s);
}

// one wave per region: mean[r] = (sum of the block partials) / n, n = count[r] * C; the select starts at rank
// (n - 1) / 2 with an empty prefix
__global__ __launch_bounds__(64) void rs_mean_kernel(const double* __restrict__ part, int nblk, int R,
                                                     const int64_t* __restrict__ count, int C, double* __restrict__ mean,
                                                     uint32_t* __restrict__ prefix, uint32_t* __restrict__ rank) {
  const int r = blockIdx.x;
  const double s = sum_partials(part, nblk, R, r);
  if (threadIdx.x != 0) return;
  const int64_t n = count[r] * C;
  mean[r] = n > 0 ? s / (double)n : nan("");
  prefix[r] = 0u;
  rank[r] = n > 0 ? (uint32_t)((n - 1) / 2) : 0u;
}

// ------------------------------------------------------------------------------------------------ deviations, digits
// grid (blocks, region groups): group g owns the regions [g * gsize, (g + 1) * gsize).  DEV: part[block * R + r] =
// the block's sum of (x - mean[r])^2.  HIST: digit `pass` of every key of region r whose higher digits equal
// prefix[r], counted in LDS and added to hist[r][digit].
template <bool DEV, bool HIST>
__global__ __launch_bounds__(RS_NT) void rs_scan_kernel(const void* __restrict__ lab, int dt, const void* __restrict__ img,
                                                        int idt, int C, int64_t S, Keys K, int pass, int gsize,
                                                        const double* __restrict__ mean,
                                                        const uint32_t* __restrict__ prefix, double* __restrict__ part,
                                                        uint32_t* __restrict__ hist) {
  __shared__ int32_t skeys[RS_MAX_L];
  __shared__ double smean[RS_MAX_R];
  __shared__ double sdev[RS_NT / 64][RS_MAX_L];
  __shared__ uint32_t spre[RS_MAX_R];
  __shared__ double scratch[RS_NT / 64];
  __shared__ uint32_t lh[HIST ? RS_HG : 1][RADIX_BINS];
  const int R = K.L + 2;
  const int g0 = blockIdx.y * gsize, g1 = min(R, g0 + gsize);
  const RadixDigit dg = radix_digit(pass);
  stage_keys(skeys, K);
  for (int r = threadIdx.x; r < RS_MAX_R; r += RS_NT) {
    smean[r] = DEV && r < R ? mean[r] : 0.0;
    spre[r] = HIST && pass > 0 && r < R ? prefix[r] >> dg.upper : 0u;
  }
  if (DEV)
    for (int j = threadIdx.x; j < (RS_NT / 64) * RS_MAX_L; j += RS_NT) (&sdev[0][0])[j] = 0.0;
  if (HIST) radix_hist_clear<RS_NT>(&lh[0][0], RS_HG * RADIX_BINS);
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bool has_all = K.L >= g0 && K.L < g1, has_whole = K.L + 1 >= g0 && K.L + 1 < g1;
  const double m_all = smean[K.L], m_whole = smean[K.L + 1];
  const uint32_t p_all = spre[K.L], p_whole = spre[K.L + 1];
  double d_all = 0.0, d_whole = 0.0;
  int32_t lastkey = K.nokey;
  int lastidx = -1;
  for (int64_t base = blockIdx.x * RS_TILE; base < S; base += (int64_t)gridDim.x * RS_TILE) {
    TileLabels t;
    load_tile_labels(lab, dt, base, S, skeys, K, lastkey, lastidx, t);
#pragma unroll
    for (int u = 0; u < RS_U; ++u)
      if (t.idx[u] < g0 || t.idx[u] >= g1) t.idx[u] = -1;   // another group's region
    for (int c = 0; c < C; ++c) {
      float xs[RS_U];
#pragma unroll
      for (int u = 0; u < RS_U; ++u) {
        const int64_t i = base + (int64_t)u * RS_NT + threadIdx.x;
        xs[u] = i < S ? load_val(img, idt, (int64_t)c * S + i) : 0.f;
      }
#pragma unroll
      for (int u = 0; u < RS_U; ++u) {
        const double xd = (double)xs[u];
        const bool in_whole = has_whole && ((t.valid >> u) & 1), in_all = has_all && ((t.nz >> u) & 1);
        const int idx = t.idx[u];
        if (DEV) {
          if (in_whole) { const double d = xd - m_whole; d_whole += d * d; }
          if (in_all) { const double d = xd - m_all; d_all += d * d; }
          for_each_region(idx, [&](int r, bool mine) {
            const double d = xd - smean[r];
            const double v = wave_sum(mine ? d * d : 0.0);
            if (lane == 0) sdev[w][r] += v;
          });
        }
        if (HIST) {
          const uint32_t key = f2key(xs[u]);
          const uint32_t hi = pass == 0 ? 0u : key >> dg.upper;
          const uint32_t d = radix_digit_of(key, dg);
          if (idx >= 0 && hi == spre[idx]) atomicAdd(&lh[idx - g0][d], 1u);
          if (in_all && hi == p_all) atomicAdd(&lh[K.L - g0][d], 1u);
          if (in_whole && hi == p_whole) atomicAdd(&lh[K.L + 1 - g0][d], 1u);
        }
      }
    }
  }
  if (DEV) {
    const double t_all = block_sum<double, RS_NT>(d_all, scratch);
    const double t_whole = block_sum<double, RS_NT>(d_whole, scratch);
    __syncthreads();
    double* o = part + (int64_t)blockIdx.x * R;
    if (threadIdx.x == 0) {
      if (has_all) o[K.L] = t_all;
      if (has_whole) o[K.L + 1] = t_whole;
    }
    for (int r = g0 + threadIdx.x; r < min(g1, K.L); r += RS_NT) {
      double v = 0.0;
#pragma unroll
      for (int ww = 0; ww < RS_NT / 64; ++ww) v += sdev[ww][r];
      o[r] = v;
    }
  }
  if (HIST) {
    __syncthreads();
    radix_hist_flush<RS_NT>(&lh[0][0], hist + (int64_t)g0 * RADIX_BINS, (g1 - g0) * RADIX_BINS);
  }
}

// one wave per region: the bucket of rank[r] extends prefix[r]; the histogram is cleared
__global__ __launch_bounds__(64) void rs_pick_kernel(int pass, const int64_t* __restrict__ count,
                                                     uint32_t* __restrict__ prefix, uint32_t* __restrict__ rank,
                                                     uint32_t* __restrict__ hist) {
  const int r = blockIdx.x;
  uint32_t* h = hist + (int64_t)r * RADIX_BINS;
  if (count[r] > 0) {
    uint32_t digit, rest;
    if (radix_pick_wave(h, rank[r], digit, rest)) {   // exactly one lane
      prefix[r] |= digit << radix_digit(pass).shift;
      rank[r] = rest;
    }
  }
  __syncthreads();
  radix_hist_clear<64>(h, RADIX_BINS);
}

// one wave per region: stats[r][k][0..5) = mean, std, median, min, max of image k, and the min / max keys reset for
// the next image
__global__ __launch_bounds__(64) void rs_finalize_kernel(const double* __restrict__ part, int nblk, int R,
                                                         const int64_t* __restrict__ count, int C,
                                                         const double* __restrict__ mean,
                                                         const uint32_t* __restrict__ prefix, uint32_t* __restrict__ kmm,
                                                         int median, float* __restrict__ stats, int K, int k) {
  const int r = blockIdx.x;
  const double s = sum_partials(part, nblk, R, r);
  if (threadIdx.x != 0) return;
  const int64_t n = count[r] * C;
  const uint32_t kmin = ~kmm[2 * r], kmax = kmm[2 * r + 1];
  kmm[2 * r] = 0u;
  kmm[2 * r + 1] = 0u;
  float* o = stats + ((int64_t)r * K + k) * 5;
  const float fnan = __uint_as_float(0x7fc00000u);
  if (n <= 0 || kmax > KEY_PINF || kmin < KEY_NINF) {   // empty, or the region holds a NaN
    for (int j = 0; j < 5; ++j) o[j] = fnan;
    return;
  }
  o[0] = (float)mean[r];
  o[1] = n > 1 ? (float)sqrt(s / (double)(n - 1)) : fnan;
  o[2] = median ? key2f(prefix[r]) : fnan;
  o[3] = key2f(kmin);
  o[4] = key2f(kmax);
}

int32_t host_label_key(int32_t v, int dt, int32_t nokey) {
  switch (dt) {
    case M355_EV_U8: return (uint8_t)v;
    case M355_EV_I8: return (int8_t)v;
    case M355_EV_I16: return (int16_t)v;
    case M355_EV_F32: return fkey((float)v, nokey);
    default: return v;   // bool (0 / 1 compared as integers), int32, int64
  }
}

bool label_type_ok(int dt) { return dt >= M355_EV_BOOL && dt <= M355_EV_F32; }
bool image_type_ok(int dt) {
  return dt == M355_EV_F32 || dt == M355_EV_F16 || dt == M355_EV_BF16 || dt == M355_EV_U8 || dt == M355_EV_I16;
}

struct Layout {
  size_t mean, prefix, rank, kmm, part, hist, total;
};
Layout layout_of(int L, int median) {
  const size_t R = (size_t)L + 2;
  Layout o;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t p = at; at += (size_t)round_up((int64_t)bytes, 256); return p; };
  o.mean = take(R * sizeof(double));
  o.prefix = take(R * sizeof(uint32_t));
  o.rank = take(R * sizeof(uint32_t));
  o.kmm = take(2 * R * sizeof(uint32_t));
  o.part = take((size_t)RS_GRID_CAP * R * sizeof(double));
  o.hist = take(median ? R * RADIX_BINS * sizeof(uint32_t) : 0);
  o.total = at;
  return o;
}

}  // namespace

extern "C" size_t m355_region_stats_workspace(int32_t L, int32_t K, int32_t median) {
  if (L < 0 || L > RS_MAX_L || K <= 0) return 0;
  return layout_of(L, median).total;
}

extern "C" int m355_region_stats_plan(int32_t* plan4) {
  M355_REQUIRE(plan4, M355_EINVALID_ARG, "region_stats_plan: null pointer");
  plan4[0] = RS_GRID_CAP;
  plan4[1] = RS_NT;
  plan4[2] = RS_U;
  plan4[3] = RS_HG;
  return M355_OK;
}

extern "C" int m355_region_stats(const void* labels, int32_t label_dtype, const int32_t* size3,
                                 const m355_region_image* images, int32_t K, const int32_t* values, int32_t L,
                                 int32_t median, int64_t* count, int32_t* bounds, float* stats, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  M355_REQUIRE(L >= 0 && K >= 0, M355_EINVALID_ARG, "region_stats: negative number of labels or images");
  M355_REQUIRE(labels && size3 && count && bounds && (L == 0 || values) && (K == 0 || (images && stats && workspace)),
               M355_EINVALID_ARG, "region_stats: null pointer");
  M355_REQUIRE(size3[0] > 0 && size3[1] > 0 && size3[2] > 0, M355_EINVALID_ARG, "region_stats: non-positive size");
  for (int k = 0; k < K; ++k) {
    M355_REQUIRE(images[k].data, M355_EINVALID_ARG, "region_stats: image %d: null pointer", k);
    M355_REQUIRE(images[k].channels > 0, M355_EINVALID_ARG, "region_stats: image %d: non-positive channels", k);
  }
  M355_REQUIRE(L <= RS_MAX_L, M355_EUNSUPPORTED, "region_stats: %d label values (at most %d a call)", L, RS_MAX_L);
  M355_REQUIRE(label_type_ok(label_dtype), M355_EUNSUPPORTED, "region_stats: label element type %d", label_dtype);
  for (int l = 0; l < L; ++l)   // float32(value) must stay inside int32
    M355_REQUIRE(values[l] > -2147483520 && values[l] < 2147483520, M355_EUNSUPPORTED,
                 "region_stats: label value %d out of range", (int)values[l]);
  const int64_t S = (int64_t)size3[0] * size3[1] * size3[2];
  for (int k = 0; k < K; ++k) {
    M355_REQUIRE(image_type_ok(images[k].dtype), M355_EUNSUPPORTED,
                 "region_stats: image %d: element type %d (float32, float16, bfloat16, uint8 or int16)", k, images[k].dtype);
    M355_REQUIRE(S * images[k].channels < ((int64_t)1 << 32), M355_EUNSUPPORTED,
                 "region_stats: image %d: 2^32 values or more", k);
  }
  M355_REQUIRE(K == 0 || workspace_bytes >= m355_region_stats_workspace(L, K, median), M355_EWORKSPACE,
               "region_stats: workspace too small");

  hipStream_t st = (hipStream_t)stream;
  const int R = L + 2;
  Keys keys;
  // a key no voxel of a listed region and no zero voxel takes: what non-integral floats and wide int64 values become
  int32_t nokey = INT32_MIN;
  for (bool again = true; again;) {
    again = false;
    for (int l = 0; l < L; ++l)
      if (host_label_key(values[l], label_dtype, nokey) == nokey) { ++nokey; again = true; }
  }
  keys.L = L;
  keys.nokey = nokey;
  for (int l = 0; l < RS_MAX_L; ++l) keys.k[l] = l < L ? host_label_key(values[l], label_dtype, nokey) : nokey;

  const Layout lo = layout_of(L, median);
  char* ws = (char*)workspace;
  double* mean = K ? (double*)(ws + lo.mean) : nullptr;
  uint32_t* prefix = K ? (uint32_t*)(ws + lo.prefix) : nullptr;
  uint32_t* rank = K ? (uint32_t*)(ws + lo.rank) : nullptr;
  uint32_t* kmm = K ? (uint32_t*)(ws + lo.kmm) : nullptr;
  double* part = K ? (double*)(ws + lo.part) : nullptr;
  uint32_t* hist = K && median ? (uint32_t*)(ws + lo.hist) : nullptr;
  const int64_t nhist = hist ? (int64_t)R * RADIX_BINS : 0;
  const unsigned nblk = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(S, RS_TILE), RS_GRID_CAP));

  hipLaunchKernelGGL(rs_init_kernel, dim3((unsigned)std::max<int64_t>(1, ceil_div(nhist, 4 * RS_NT))), dim3(RS_NT), 0, st,
                     count, bounds, L, size3[0], size3[1], size3[2], kmm, hist, nhist);
  hipLaunchKernelGGL(rs_count_kernel, dim3(nblk), dim3(RS_NT), 0, st, labels, label_dtype, S, size3[1], size3[2], keys,
                     count, bounds);
  const int ngroups = (int)ceil_div(R, RS_HG);
  for (int k = 0; k < K; ++k) {
    const void* img = images[k].data;
    const int idt = images[k].dtype, C = images[k].channels;
    hipLaunchKernelGGL(rs_sum_kernel, dim3(nblk), dim3(RS_NT), 0, st, labels, label_dtype, img, idt, C, S, keys, part,
                       kmm);
    hipLaunchKernelGGL(rs_mean_kernel, dim3(R), dim3(64), 0, st, part, (int)nblk, R, count, C, mean, prefix, rank);
    if (median) {
      for (int pass = 0; pass < 3; ++pass) {
        if (pass == 0)
          hipLaunchKernelGGL((rs_scan_kernel<true, true>), dim3(nblk, ngroups), dim3(RS_NT), 0, st, labels, label_dtype,
                             img, idt, C, S, keys, pass, RS_HG, mean, prefix, part, hist);
        else
          hipLaunchKernelGGL((rs_scan_kernel<false, true>), dim3(nblk, ngroups), dim3(RS_NT), 0, st, labels, label_dtype,
                             img, idt, C, S, keys, pass, RS_HG, mean, prefix, part, hist);
        hipLaunchKernelGGL(rs_pick_kernel, dim3(R), dim3(64), 0, st, pass, count, prefix, rank, hist);
      }
    } else {
      hipLaunchKernelGGL((rs_scan_kernel<true, false>), dim3(nblk, 1), dim3(RS_NT), 0, st, labels, label_dtype, img, idt,
                         C, S, keys, 0, R, mean, prefix, part, hist);
    }
    hipLaunchKernelGGL(rs_finalize_kernel, dim3(R), dim3(64), 0, st, part, (int)nblk, R, count, C, mean, prefix, kmm,
                       median, stats, K, k);
  }
  return check_launch("region_stats");
}
