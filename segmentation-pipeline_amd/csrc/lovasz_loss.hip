// Lovasz-softmax criterion (criterions/lovasz_loss.py; Berman et al., CVPR 2018): the convex surrogate of the
// Jaccard index, on the segmented radix sort of segmented_sort.hip.
//
//   segments   per_image == 0: one per channel c over the M = N S voxels of the batch (R = C, element n S + s);
//              per_image != 0: one per (n, c) (R = N C, M = S)
//   element    fg = (t >= 0.5), e = |fg - p| (one fp32 subtraction), key = ~((bits(e) << 1) | fg) & 0x7fffffff: ascending
//              keys are descending errors, e <= 1 means bits(e) < 2^30, so 31 bits hold the key
//   sorted     F(i) = the foreground elements among the first i, G = F(M), I(i) = G - F(i), U(i) = G + i - F(i),
//              J(0) = 0, J(i) = 1 - I(i) / U(i);   L = sum_i e_(i) (J(i) - J(i - 1))
//   ties       the elements of one value of e form a group [lo, hi) and each gets dL/de = (J(hi) - J(lo)) / (hi - lo),
//              which no tie-breaking order can change
//   J(hi) - J(lo) = (I(lo) U(hi) - I(hi) U(lo)) / (U(lo) U(hi)) for lo > 0 and J(hi) for lo = 0: 64-bit integer products,
//              one fp64 division
//
// Forward: one 4-byte memset (the status word), then
//   lv_keys      reads p and t once (row_load), writes the keys segment-major, ORs the status word where a prediction is
//                a NaN or outside [0, 1] (its e is clamped to [0, 1]: every key stays inside 31 bits)
//   the sort     4 passes x 4 launches, 31 bits
//   lv_totals    the foreground count of every tile of LV_TILE sorted keys
//   lv_scan      a block per segment: the exclusive scan of its tile counts, LV_THREADS at a time with a carry; G
//   lv_apply     a block per tile: F (lane: 4 keys, wave, block, the carry over the tile's rounds, the tile's start), the
//                tile's part of L in fp64 (per lane in index order, then the fixed tree of block_sum)
//   lv_finalize  one block: L per segment (its tiles in index order), presence, weights, per-image mean; out2 = {loss,
//                number of segments averaged}; state = R x {G, coefficient dloss/dL_r as fp32}
// Backward, one launch: an element recomputes its key, finds [lo, hi) by two binary searches on key >> 1 in its segment's
// sorted keys, reads F(lo) and F(hi) and writes dx = dloss coefficient sign (J(hi) - J(lo)) / (hi - lo).  The searches are
// what the backward costs (1.14 ms at 1 x 4 x 128^3, 42 lane-divergent loads per element); a first stage over 512 samples
// in LDS and a one-load test for groups of one were measured and were no faster.
//
//   workspace = round_up(4 R M, 256) + m355_segmented_sort_workspace(R, M) + round_up(4 R T, 256) + 8 R T + 8 R + 256 bytes,
//   T = ceil(M / LV_TILE);   kept for the backward: the sorted keys and F, 8 bytes per (class, voxel), and 8 R bytes of state
//
// Deterministic: the sort decides no position by an atomic, the key holds fg, so equal keys are equal elements; the only
// atomic is the OR into the status word.  Every sum has one order.
#include "loss_common.hpp"

namespace m355 {

void segmented_sort_launch(const uint32_t* keys, uint32_t* out, int64_t R, int64_t M, int end_bit, void* workspace,
                           hipStream_t st);
size_t segmented_sort_bytes(int64_t R, int64_t M);

constexpr int LV_TILE = 4096;      // keys per block of the key pass, the scan passes and the backward
constexpr int LV_THREADS = 256;
constexpr int LV_ROUND = LV_THREADS * 4;   // keys of one round of a block: 4 consecutive ones per lane
constexpr int LV_KEY_BITS = 31;

// (key, in range) of one element.  fminf(NaN, 1) = 1: whatever p holds, e is in [0, 1].
__device__ __forceinline__ uint32_t lv_key(float p, float t, bool& ok) {
  const bool fg = t >= 0.5f;
  ok = p >= 0.f && p <= 1.f;
  const float e = fminf(fabsf((fg ? 1.f : 0.f) - p), 1.f);
  return ~((__float_as_uint(e) << 1) | (fg ? 1u : 0u)) & 0x7fffffffu;
}
__device__ __forceinline__ uint32_t lv_fg(uint32_t key) { return ~key & 1u; }
__device__ __forceinline__ float lv_error(uint32_t key) { return __uint_as_float((~key & 0x7fffffffu) >> 1); }

// J(hi) - J(lo), 0 <= lo < hi, from the foreground counts before lo and before hi and the segment's G
__device__ __forceinline__ double lv_jaccard_step(uint32_t lo, uint32_t hi, uint32_t f_lo, uint32_t f_hi, uint32_t G) {
  const uint64_t i_hi = G - f_hi, u_hi = (uint64_t)G + hi - f_hi;   // u_hi >= hi > 0
  if (lo == 0) return (double)(u_hi - i_hi) / (double)u_hi;
  const uint64_t i_lo = G - f_lo, u_lo = (uint64_t)G + lo - f_lo;
  return (double)(int64_t)(i_lo * u_hi - i_hi * u_lo) / (double)(u_lo * u_hi);
}

// where element s of row (n, c) lives: segment and position
struct LvMap {
  int64_t R, M;
  int per_image;
};
static inline LvMap lv_map(int32_t N, int32_t C, int64_t S, int32_t per_image) {
  LvMap m;
  m.per_image = per_image ? 1 : 0;
  m.R = per_image ? (int64_t)N * C : C;
  m.M = per_image ? S : (int64_t)N * S;
  return m;
}
__device__ __forceinline__ void lv_segment(int nc, int C, int64_t S, int per_image, int& r, int64_t& pos0) {
  if (per_image) {
    r = nc;
    pos0 = 0;
  } else {
    r = nc % C;
    pos0 = (int64_t)(nc / C) * S;
  }
}

__global__ __launch_bounds__(LV_THREADS) void lv_keys_kernel(const float* __restrict__ p, const float* __restrict__ t,
                                                             uint32_t* __restrict__ keys, uint32_t* __restrict__ status,
                                                             int C, int64_t S, int64_t M, int per_image) {
  const int nc = blockIdx.y;
  int r;
  int64_t pos0;
  lv_segment(nc, C, S, per_image, r, pos0);
  const float* pr = p + (int64_t)nc * S;
  const float* tr = t + (int64_t)nc * S;
  float* kr = reinterpret_cast<float*>(keys + (int64_t)r * M + pos0);
  bool bad = false;
  for (int64_t b0 = (int64_t)blockIdx.x * LV_TILE; b0 < S; b0 += (int64_t)gridDim.x * LV_TILE) {
    const int64_t end = min(S, b0 + LV_TILE);
    for (int64_t v0 = b0 + threadIdx.x * 4; v0 < end; v0 += LV_ROUND) {
      const int nv = row_valid(v0, end, 4);
      float pv[4], tv[4], kv[4];
      row_load<4>(pr + v0, nv, pv);
      row_load<4>(tr + v0, nv, tv);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bool ok;
        kv[j] = __uint_as_float(lv_key(pv[j], tv[j], ok));
        bad |= (j < nv) && !ok;
      }
      row_store<4>(kr + v0, nv, kv);
    }
  }
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(status, 1u);
}

// the 4 keys of a lane in one round of a tile (keys past the segment's end count as background with e = 0)
__device__ __forceinline__ int lv_load4(const uint32_t* __restrict__ seg, int64_t v0, int64_t M, uint32_t (&k)[4]) {
  const int nv = row_valid(v0, M, 4);
  if (nv == 4 && ((uintptr_t)(seg + v0) & 15) == 0) {
    const uint4 q = *reinterpret_cast<const uint4*>(seg + v0);
    k[0] = q.x; k[1] = q.y; k[2] = q.z; k[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = j < nv ? seg[v0 + j] : 0x7fffffffu;
  }
  return nv;
}

__global__ __launch_bounds__(LV_THREADS) void lv_totals_kernel(const uint32_t* __restrict__ skeys, uint32_t* __restrict__ bt,
                                                               int64_t M, int nblk) {
  __shared__ uint32_t scratch[LV_THREADS / 64];
  const int64_t r = blockIdx.y;
  const uint32_t* seg = skeys + r * M;
  const int64_t begin = (int64_t)blockIdx.x * LV_TILE, end = min(M, begin + LV_TILE);
  uint32_t c = 0;
  for (int64_t v0 = begin + threadIdx.x * 4; v0 < end; v0 += LV_ROUND) {
    uint32_t k[4];
    lv_load4(seg, v0, M, k);
#pragma unroll
    for (int j = 0; j < 4; ++j) c += lv_fg(k[j]);
  }
  const uint32_t s = block_sum<uint32_t, LV_THREADS>(c, scratch);
  if (threadIdx.x == 0) bt[r * nblk + blockIdx.x] = s;
}

// exclusive scan of `v` over the block, `total` in every thread; sh: LV_THREADS / 64 words
__device__ __forceinline__ uint32_t lv_block_excl(uint32_t v, uint32_t& total, uint32_t* sh) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t incl = wave_incl_scan(v);
  __syncthreads();   // sh may still be read from the round before
  if (lane == 63) sh[w] = incl;
  __syncthreads();
  uint32_t base = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < LV_THREADS / 64; ++i) {
    if (i < w) base += sh[i];
    total += sh[i];
  }
  return base + incl - v;
}

__global__ __launch_bounds__(LV_THREADS) void lv_scan_kernel(uint32_t* __restrict__ bt, uint32_t* __restrict__ state,
                                                             int nblk) {
  __shared__ uint32_t sh[LV_THREADS / 64];
  uint32_t* row = bt + (int64_t)blockIdx.x * nblk;
  uint32_t carry = 0;
  for (int b0 = 0; b0 < nblk; b0 += LV_THREADS) {
    const int b = b0 + threadIdx.x;
    const uint32_t v = b < nblk ? row[b] : 0u;
    uint32_t total;
    const uint32_t ex = lv_block_excl(v, total, sh);
    if (b < nblk) row[b] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) state[2 * blockIdx.x] = carry;   // G
}

__global__ __launch_bounds__(LV_THREADS) void lv_apply_kernel(const uint32_t* __restrict__ skeys,
                                                              const uint32_t* __restrict__ bt,
                                                              const uint32_t* __restrict__ state, uint32_t* __restrict__ F,
                                                              double* __restrict__ partial, int64_t M, int nblk) {
  __shared__ uint32_t sh[LV_THREADS / 64];
  __shared__ double scratch[LV_THREADS / 64];
  const int64_t r = blockIdx.y;
  const uint32_t* seg = skeys + r * M;
  uint32_t* fseg = F + r * M;
  const uint32_t G = state[2 * r];
  const int64_t begin = (int64_t)blockIdx.x * LV_TILE, end = min(M, begin + LV_TILE);
  uint32_t carry = bt[r * nblk + blockIdx.x];
  double acc = 0.0;
  for (int64_t r0 = begin; r0 < end; r0 += LV_ROUND) {   // (uniform over the block: the scan's barriers are safe)
    const int64_t v0 = r0 + threadIdx.x * 4;
    uint32_t k[4];
    const int nv = lv_load4(seg, v0, M, k);
    const uint32_t mine = lv_fg(k[0]) + lv_fg(k[1]) + lv_fg(k[2]) + lv_fg(k[3]);
    uint32_t total;
    uint32_t f = carry + lv_block_excl(mine, total, sh);
    carry += total;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nv) {
        const uint32_t i = (uint32_t)(v0 + j), fn = f + lv_fg(k[j]);
        fseg[v0 + j] = f;
        acc += (double)lv_error(k[j]) * lv_jaccard_step(i, i + 1u, f, fn, G);
        f = fn;
      }
  }
  const double s = block_sum<double, LV_THREADS>(acc, scratch);
  if (threadIdx.x == 0) partial[r * nblk + blockIdx.x] = s;
}

// One block.  images = N (per_image) or 1; image i averages its C segments i C .. i C + C - 1.
__global__ __launch_bounds__(LV_THREADS) void lv_finalize_kernel(const double* __restrict__ partial,
                                                                 const uint32_t* __restrict__ status,
                                                                 const float* __restrict__ class_w,
                                                                 double* __restrict__ seg_loss, uint32_t* __restrict__ state,
                                                                 float* __restrict__ out2, int images, int C, int nblk,
                                                                 int all_classes) {
  __shared__ double scratch[LV_THREADS / 64];
  const int R = images * C;
  // a wave per segment: lane l adds the tiles l, l + 64, ... in index order, then the fixed tree of wave_sum
  for (int r = threadIdx.x >> 6; r < R; r += LV_THREADS / 64) {
    double s = 0.0;
    for (int b = threadIdx.x & 63; b < nblk; b += 64) s += partial[(int64_t)r * nblk + b];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) seg_loss[r] = s;
  }
  __syncthreads();
  const bool bad = status[0] != 0u;
  double acc = 0.0, cnt = 0.0;
  for (int i = threadIdx.x; i < images; i += LV_THREADS) {
    double num = 0.0, den = 0.0;
    for (int c = 0; c < C; ++c) {
      const int r = i * C + c;
      const double w = (all_classes || state[2 * r] > 0u) ? (class_w ? (double)class_w[c] : 1.0) : 0.0;
      num += w * seg_loss[r];
      den += w;
      cnt += w != 0.0 ? 1.0 : 0.0;
    }
    const bool any = den > 0.0;
    if (any) acc += num / den;
    for (int c = 0; c < C; ++c) {
      const int r = i * C + c;
      const double w = (all_classes || state[2 * r] > 0u) ? (class_w ? (double)class_w[c] : 1.0) : 0.0;
      const float coef = any ? (float)(w / (den * (double)images)) : 0.f;
      state[2 * r + 1] = __float_as_uint(bad ? __uint_as_float(0x7fc00000u) : coef);
    }
  }
  const double loss = block_sum<double, LV_THREADS>(acc, scratch);
  const double n = block_sum<double, LV_THREADS>(cnt, scratch);
  if (threadIdx.x == 0) {
    out2[0] = bad ? __uint_as_float(0x7fc00000u) : (float)(loss / (double)images);
    out2[1] = (float)n;
  }
}

// The group [lo, hi) of each of 4 queries q = key >> 1 in a segment's sorted keys: lo the first index whose key >> 1 is
// >= q, hi the first whose key >> 1 is > q, both in [0, M].  Branch-free binary searches: the step sizes depend on M only,
// so the 8 searches run in lock-step and their loads overlap.  Every index read is below M.
__device__ __forceinline__ void lv_groups(const uint32_t* __restrict__ seg, uint32_t M, const uint32_t (&q)[4],
                                          uint32_t (&lo)[4], uint32_t (&hi)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) lo[j] = hi[j] = 0u;
  uint32_t n = M;
  while (n > 1) {
    const uint32_t half = n >> 1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t vl = seg[lo[j] + half - 1] >> 1, vh = seg[hi[j] + half - 1] >> 1;
      lo[j] += vl < q[j] ? half : 0u;
      hi[j] += vh <= q[j] ? half : 0u;
    }
    n -= half;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    lo[j] += (seg[lo[j]] >> 1) < q[j] ? 1u : 0u;
    hi[j] += (seg[hi[j]] >> 1) <= q[j] ? 1u : 0u;
  }
}

__global__ __launch_bounds__(LV_THREADS) void lv_bwd_kernel(const float* __restrict__ p, const float* __restrict__ t,
                                                            const uint32_t* __restrict__ skeys, const uint32_t* __restrict__ F,
                                                            const uint32_t* __restrict__ state, const float* __restrict__ dloss,
                                                            float* __restrict__ dx, int C, int64_t S, int64_t M,
                                                            int per_image) {
  const int nc = blockIdx.y;
  int r;
  int64_t pos0;
  lv_segment(nc, C, S, per_image, r, pos0);
  const uint32_t* seg = skeys + (int64_t)r * M;
  const uint32_t* fseg = F + (int64_t)r * M;
  const uint32_t G = state[2 * r];
  const float scale = dloss[0] * __uint_as_float(state[2 * r + 1]);
  const float* pr = p + (int64_t)nc * S;
  const float* tr = t + (int64_t)nc * S;
  float* dr = dx + (int64_t)nc * S;
  for (int64_t b0 = (int64_t)blockIdx.x * LV_TILE; b0 < S; b0 += (int64_t)gridDim.x * LV_TILE) {
    const int64_t end = min(S, b0 + LV_TILE);
    for (int64_t v0 = b0 + threadIdx.x * 4; v0 < end; v0 += LV_ROUND) {
      const int nv = row_valid(v0, end, 4);
      float pv[4], tv[4], o[4];
      row_load<4>(pr + v0, nv, pv);
      row_load<4>(tr + v0, nv, tv);
      uint32_t key[4], q[4], lo[4], hi[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bool ok;
        key[j] = lv_key(pv[j], tv[j], ok);   // (row_load gives p = t = 0 past the row's end: a query like any other)
        q[j] = key[j] >> 1;
      }
      lv_groups(seg, (uint32_t)M, q, lo, hi);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t h = max(hi[j], lo[j] + 1u);   // (its own key is in the group: hi > lo unless the buffers are not this call's)
        const uint32_t f_lo = lo[j] < (uint32_t)M ? fseg[lo[j]] : G, f_hi = h < (uint32_t)M ? fseg[h] : G;
        const double dj = lv_jaccard_step(lo[j], h, f_lo, f_hi, G) / (double)(h - lo[j]);
        o[j] = (lv_fg(key[j]) ? -scale : scale) * (float)dj;
      }
      row_store<4>(dr + v0, nv, o);
    }
  }
}

struct LvLayout {
  int nblk;
  size_t sort, bt, partial, seg_loss, status, bytes;   // byte offsets behind the unsorted keys; the whole
};
static inline LvLayout lv_layout(const LvMap& m) {
  LvLayout l;
  l.nblk = (int)ceil_div(m.M, LV_TILE);
  l.sort = (size_t)round_up(4 * m.R * m.M, 256);
  l.bt = l.sort + (size_t)round_up((int64_t)segmented_sort_bytes(m.R, m.M), 256);
  l.partial = l.bt + (size_t)round_up(4 * m.R * l.nblk, 256);
  l.seg_loss = l.partial + (size_t)8 * m.R * l.nblk;
  l.status = l.seg_loss + (size_t)8 * m.R;
  l.bytes = l.status + 256;
  return l;
}

static int lv_check(const char* what, int32_t N, int32_t C, int64_t S, int32_t per_image) {
  if (int rc = loss_check(what, N, C, S)) return rc;
  M355_REQUIRE(per_image || S <= (int64_t)0x7fffffffll / N, M355_EUNSUPPORTED, "%s: N*S > 2^31 - 1", what);
  M355_REQUIRE(S <= 0x7fffffffll, M355_EUNSUPPORTED, "%s: S > 2^31 - 1", what);
  return M355_OK;
}

}  // namespace m355

using namespace m355;

extern "C" size_t m355_lovasz_loss_workspace(int32_t N, int32_t C, int64_t S, int32_t per_image) {
  if (N <= 0 || C <= 0 || S <= 0) return 0;
  if ((int64_t)N * C > 65535 || S > 0x7fffffffll || (!per_image && S > (int64_t)0x7fffffffll / N)) return 0;
  return lv_layout(lv_map(N, C, S, per_image)).bytes;
}

extern "C" int32_t m355_lovasz_loss_tile(void) { return LV_TILE; }

extern "C" int m355_lovasz_loss_fwd(const float* p, const float* t, int32_t N, int32_t C, int64_t S, int32_t per_image,
                                    int32_t all_classes, const float* class_weights, float* out2, uint32_t* sorted_keys,
                                    uint32_t* F, void* state, void* workspace, size_t workspace_bytes, void* stream) {
  M355_REQUIRE(p && t && out2 && sorted_keys && F && state && workspace, M355_EINVALID_ARG, "lovasz_loss_fwd: null pointer");
  if (int rc = lv_check("lovasz_loss_fwd", N, C, S, per_image)) return rc;
  const LvMap m = lv_map(N, C, S, per_image);
  const LvLayout l = lv_layout(m);
  M355_REQUIRE(workspace_bytes >= l.bytes, M355_EWORKSPACE, "lovasz_loss_fwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  uint32_t* keys = (uint32_t*)ws;
  uint32_t* bt = (uint32_t*)(ws + l.bt);
  double* partial = (double*)(ws + l.partial);
  double* seg_loss = (double*)(ws + l.seg_loss);
  uint32_t* status = (uint32_t*)(ws + l.status);
  if (hipMemsetAsync(status, 0, sizeof(uint32_t), st) != hipSuccess) return check_launch("lovasz_loss_fwd: memset");
  const int NC = N * C;
  hipLaunchKernelGGL(lv_keys_kernel, loss_bwd_grid(S, LV_TILE, NC), dim3(LV_THREADS), 0, st, p, t, keys, status, (int)C, S,
                     m.M, m.per_image);
  segmented_sort_launch(keys, sorted_keys, m.R, m.M, LV_KEY_BITS, ws + l.sort, st);
  const dim3 tiles((unsigned)l.nblk, (unsigned)m.R);
  hipLaunchKernelGGL(lv_totals_kernel, tiles, dim3(LV_THREADS), 0, st, (const uint32_t*)sorted_keys, bt, m.M, l.nblk);
  hipLaunchKernelGGL(lv_scan_kernel, dim3((unsigned)m.R), dim3(LV_THREADS), 0, st, bt, (uint32_t*)state, l.nblk);
  hipLaunchKernelGGL(lv_apply_kernel, tiles, dim3(LV_THREADS), 0, st, (const uint32_t*)sorted_keys, (const uint32_t*)bt,
                     (const uint32_t*)state, F, partial, m.M, l.nblk);
  hipLaunchKernelGGL(lv_finalize_kernel, dim3(1), dim3(LV_THREADS), 0, st, (const double*)partial, (const uint32_t*)status,
                     class_weights, seg_loss, (uint32_t*)state, out2, m.per_image ? (int)N : 1, (int)C, l.nblk,
                     all_classes ? 1 : 0);
  return check_launch("lovasz_loss_fwd");
}

extern "C" int m355_lovasz_loss_bwd(const float* p, const float* t, const uint32_t* sorted_keys, const uint32_t* F,
                                    const void* state, const float* dloss, int32_t N, int32_t C, int64_t S,
                                    int32_t per_image, float* dx, void* stream) {
  M355_REQUIRE(p && t && sorted_keys && F && state && dloss && dx, M355_EINVALID_ARG, "lovasz_loss_bwd: null pointer");
  if (int rc = lv_check("lovasz_loss_bwd", N, C, S, per_image)) return rc;
  const LvMap m = lv_map(N, C, S, per_image);
  hipLaunchKernelGGL(lv_bwd_kernel, loss_bwd_grid(S, LV_TILE, N * C), dim3(LV_THREADS), 0, (hipStream_t)stream, p, t,
                     sorted_keys, F, (const uint32_t*)state, dloss, dx, (int)C, S, m.M, m.per_image);
  return check_launch("lovasz_loss_bwd");
}
