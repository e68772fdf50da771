// Exact Euclidean distance transform and surface distances (post_processing.distance_transform_edt,
// evaluators.SurfaceDistanceEvaluator).
//
//   edt_d_kernel           index distance to the nearest site along D for every voxel, as uint16 (into the workspace)
//   edt_line_kernel        min over a line of (previous pass + (spacing * k)^2): once along H, once along W
//   edt_sqrt_kernel        correctly rounded elementwise square root
//   surface_mask_kernel    the six-neighbour border of (x == value), and its voxel count
//   surface_gather_kernel  sqrt(d2) of the border voxels, compacted
//   sd_sweep_kernel, sd_line_kernel   the batched signed distance of criterions.BoundaryLoss (described where they stand)
//
// A volume is [W, H, D] with D fastest.  The transform is separable: d2[w, h, d] = min_w' ((sw (w - w'))^2 +
// min_h' ((sh (h - h'))^2 + (sd kd[w', h', d])^2)) with kd the index distance to the nearest site of the row.
//
// D sweep.  A wave owns a run of whole rows of at most ED_GROUP voxels and walks it in chunks of 64 consecutive voxels
// (coalesced byte loads, 128-byte stores).  The nearest site to the left of voxel i of the run is the prefix maximum of
// (site ? i : -1), the nearest to the right the suffix minimum of (site ? i : BIG): wave scans by shuffles with a carry
// from chunk to chunk, over the run as ONE sequence -- a site found outside the voxel's own row is discarded afterwards
// by comparing with the row's first and last index.  The left results of the (at most ED_GROUP / 64) chunks wait in
// registers while the right ones are produced back to front.  0xFFFF: the row holds no site.
//
// H and W passes.  A block owns ED_DT consecutive lines (consecutive along D, so every global access of a half wave
// is one contiguous segment) in full: it stages them in LDS, [line position][ED_DT], and then each thread takes
// outputs (p, lane) and searches outwards from p, k = 1, 2, ...: candidates g[p - k] + (s k)^2 and g[p + k] + (s k)^2.
// The search stops as soon as (s k)^2 >= the best value so far: fp32 rounding is monotone and g >= 0, so no candidate
// at that distance or beyond can be smaller -- the pruning is exact, ties included (a tie has the same value).  The
// block reads every line before it writes any, and no other block touches these lines: the W pass runs in place.
//
// Arithmetic.  Every term is __fmul_rn(t, t) with t = __fmul_rn(spacing, (float)k), every sum __fadd_rn: no
// contraction, so the result does not depend on the compiler's choices.  Unit spacing: every intermediate is an integer
// and the result is exact while (W-1)^2 + (H-1)^2 + (D-1)^2 < 2^24.
#include <math.h>
#include "common.hpp"

namespace {

constexpr int ED_NT = 256;
constexpr int ED_GROUP = 1024;                 // voxels of the whole rows a wave owns in the D sweep
constexpr int ED_CHUNKS = ED_GROUP / 64;
constexpr int ED_DT = 32;                      // lines a block of the H / W pass owns
constexpr uint16_t ED_NONE = 0xFFFF;           // kd of a row without a site
static_assert(M355_EDT_MAX_DIM <= ED_GROUP && M355_EDT_MAX_DIM < ED_NONE, "a row fits a wave's run; kd fits uint16");
static_assert((size_t)M355_EDT_MAX_DIM * ED_DT * sizeof(float) <= 65536, "the staged lines fit 64 KiB of LDS");

__global__ __launch_bounds__(ED_NT) void edt_d_kernel(const uint8_t* __restrict__ sites, uint16_t* __restrict__ kd,
                                                      uint32_t rows, uint32_t D, uint32_t rows_per_wave) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * (ED_NT / 64) + (threadIdx.x >> 6);
  const uint32_t r0 = wave * rows_per_wave;          // < rows + ED_NT / 64 * rows_per_wave < 2^32
  if (r0 >= rows) return;                            // (the whole wave: the shuffles below see all 64 lanes or none)
  const uint32_t n = min(rows_per_wave, rows - r0) * D;   // <= ED_GROUP
  const uint32_t base = r0 * D;                      // < 2^31 voxels (checked on the host)
  int left[ED_CHUNKS];
  uint32_t site_bits = 0;
  int carry = -1;
#pragma unroll
  for (int c = 0; c < ED_CHUNKS; ++c) {
    left[c] = -1;
    if ((uint32_t)c * 64 < n) {                      // wave-uniform
      const uint32_t i = c * 64 + lane;
      const bool s = i < n && sites[base + i] != 0;
      int v = s ? (int)i : -1;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(v, off, 64);
        if ((int)lane >= off) v = max(v, o);
      }
      v = max(v, carry);
      carry = __shfl(v, 63, 64);
      left[c] = v;
      site_bits |= (uint32_t)s << c;
    }
  }
  constexpr int BIG = 1 << 30;
  carry = BIG;
#pragma unroll
  for (int c = ED_CHUNKS - 1; c >= 0; --c) {
    if ((uint32_t)c * 64 < n) {
      const uint32_t i = c * 64 + lane;
      int v = (site_bits >> c) & 1 ? (int)i : BIG;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_down(v, off, 64);
        if ((int)lane + off < 64) v = min(v, o);
      }
      v = min(v, carry);
      carry = __shfl(v, 0, 64);
      if (i < n) {
        const int row_first = (int)(i / D * D), row_last = row_first + (int)D - 1;
        const int kl = left[c] >= row_first ? (int)i - left[c] : (int)ED_NONE;
        const int kr = v <= row_last ? v - (int)i : (int)ED_NONE;
        kd[base + i] = (uint16_t)min(kl, kr);
      }
    }
  }
}

// One separable pass over lines of n positions, `line_stride` elements apart.  The lines are numbered (o, j): o < gridDim.y
// slabs `outer_stride` apart, j < inner consecutive elements; block (x, y) owns lines j in [x * ED_DT, x * ED_DT + ED_DT)
// of slab y.  FROM_KD: the input is the D sweep's uint16 index distance and g = (s_in * kd)^2; otherwise the input is
// the previous pass's fp32 (and `in` may be `out`).
template <bool FROM_KD>
__global__ __launch_bounds__(ED_NT) void edt_line_kernel(const void* in, float* out, uint32_t n, uint32_t inner,
                                                         uint32_t line_stride, uint32_t outer_stride, float s_in,
                                                         float s) {
  extern __shared__ float g[];                       // [n][ED_DT]
  const uint32_t lane = threadIdx.x % ED_DT, ty = threadIdx.x / ED_DT;
  const uint32_t j = blockIdx.x * ED_DT + lane;
  const bool live = j < inner;
  const uint32_t at = blockIdx.y * outer_stride + j;   // position 0 of the thread's line; < 2^31 when live
  constexpr uint32_t ROWS = ED_NT / ED_DT;
  for (uint32_t p = ty; p < n; p += ROWS) {
    float v = INFINITY;
    if (live) {
      if (FROM_KD) {
        const uint16_t k = ((const uint16_t*)in)[at + p * line_stride];
        if (k != ED_NONE) {
          const float t = __fmul_rn(s_in, (float)k);
          v = __fmul_rn(t, t);
        }
      } else {
        v = ((const float*)in)[at + p * line_stride];
      }
    }
    g[p * ED_DT + lane] = v;
  }
  __syncthreads();
  if (!live) return;
  for (uint32_t p = ty; p < n; p += ROWS) {
    float m = g[p * ED_DT + lane];
    const uint32_t below = p, above = n - 1 - p, kmax = max(below, above);
    for (uint32_t k = 1; k <= kmax; ++k) {
      const float t = __fmul_rn(s, (float)k);
      const float sq = __fmul_rn(t, t);
      if (!(sq < m)) break;                          // nothing at distance >= k can be smaller (header of this file)
      if (k <= below) m = fminf(m, __fadd_rn(g[(p - k) * ED_DT + lane], sq));
      if (k <= above) m = fminf(m, __fadd_rn(g[(p + k) * ED_DT + lane], sq));
    }
    out[at + p * line_stride] = m;
  }
}

// sqrt in fp64 rounded to fp32 is the correctly rounded fp32 square root (53 >= 2 * 24 + 2 bits), whatever the build's
// fp32 sqrt is.  +inf stays +inf.
__device__ __forceinline__ float sqrt_rn(float v) { return (float)sqrt((double)v); }

__global__ __launch_bounds__(ED_NT) void edt_sqrt_kernel(const float* d2, float* d, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * ED_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * ED_NT) d[i] = sqrt_rn(d2[i]);
}

// Reserves one slot of *counter for every lane with `take`: one atomic per wave, by its first taking lane.  Returns the
// lane's slot (meaningless without `take`).  Integer atomics: the total is exact.
__device__ __forceinline__ int32_t wave_reserve(int32_t* counter, bool take) {
  const uint64_t ballot = __ballot(take);
  if (!ballot) return 0;
  const int lane = threadIdx.x & 63, leader = __ffsll((unsigned long long)ballot) - 1;
  int32_t first = 0;
  if (lane == leader) first = atomicAdd(counter, (int32_t)__popcll(ballot));
  first = __shfl(first, leader, 64);
  return first + (int32_t)__popcll(ballot & ((1ull << lane) - 1));
}

__global__ __launch_bounds__(ED_NT) void surface_mask_kernel(const int32_t* __restrict__ x, int32_t value, uint32_t W,
                                                             uint32_t H, uint32_t D, uint8_t* __restrict__ border,
                                                             int32_t* __restrict__ count) {
  const uint32_t S = W * H * D, HD = H * D;
  const uint32_t steps = (S + gridDim.x * ED_NT - 1) / (gridDim.x * ED_NT);   // the same for every lane (the ballot)
  uint32_t found = 0;                                // border voxels of this wave, the same number in every lane
  for (uint32_t step = 0; step < steps; ++step) {
    const uint32_t v = (step * gridDim.x + blockIdx.x) * ED_NT + threadIdx.x;   // < S + grid * ED_NT < 2^32
    bool b = false;
    if (v < S && x[v] == value) {
      const uint32_t r = v / D, d = v - r * D, w = r / H, h = r - w * H;
      b = d == 0 || d == D - 1 || h == 0 || h == H - 1 || w == 0 || w == W - 1;
      if (!b)
        b = x[v - 1] != value || x[v + 1] != value || x[v - D] != value || x[v + D] != value || x[v - HD] != value ||
            x[v + HD] != value;
    }
    if (v < S) border[v] = b;
    found += (uint32_t)__popcll(__ballot(b));
  }
  // one atomic per wave and launch (one per wave and step serialises on the counter's cache line)
  if ((threadIdx.x & 63) == 0 && found) atomicAdd(count, (int32_t)found);
}

__global__ __launch_bounds__(ED_NT) void surface_gather_kernel(const uint8_t* __restrict__ border,
                                                               const float* __restrict__ d2, int64_t n,
                                                               float* __restrict__ out, int32_t* __restrict__ cursor,
                                                               int32_t capacity) {
  const int64_t stride = (int64_t)gridDim.x * ED_NT, steps = (n + stride - 1) / stride;
  for (int64_t step = 0; step < steps; ++step) {
    const int64_t v = step * stride + (int64_t)blockIdx.x * ED_NT + threadIdx.x;
    const bool b = v < n && border[v] != 0;
    const int32_t slot = wave_reserve(cursor, b);
    if (b && slot >= 0 && slot < capacity) out[slot] = sqrt_rn(d2[v]);
  }
}

// ------------------------------------------------------------------------- batched signed distance
// phi of every (n, c) plane of a target [planes][A0][A1][A2], A2 fastest, in one launch per pass: blockIdx carries the
// plane, and a bit mask in the kernel arguments says which planes are transformed.  A voxel is inside when t > 0.5 (a NaN
// is outside) and needs the distance to the nearest voxel of the OTHER membership only.  At every separable stage one of
// a voxel's two partial distances (to inside, to outside) is zero -- the voxel is a site of its own class -- so one value
// and the membership bit carry both, and the signed transform costs one transform:
//   sd_sweep_kernel   along A2: index distance to the nearest voxel of the other membership in the row, uint16 with the
//                     membership in bit 15; SD_NONE: the row has one membership only.  edt_d_kernel's wave scans, over
//                     run starts and run ends instead of sites: the nearest other voxel to the left of i is the one before
//                     the start of i's run, the nearest to the right the one after its end.
//   sd_line_kernel    along A1, then along A0: the candidate of position q for a target at p is
//                     (m[q] != m[p] ? 0 : g[q]) + (s (p - q))^2.  Effective candidate values are >= 0, so the pruning
//                     argument of this file's header holds unchanged.  g > 0 or +inf for every voxel (a voxel is never
//                     its own opposite), so the fp32 sign bit is free for the membership between the two passes.  The
//                     last pass writes phi: 0 where g is infinite (exactly the planes without a boundary), sqrt_rn(g)
//                     outside, 1 - sqrt_rn(g) inside; and zeros into the planes that are switched off.
// The arithmetic is edt_line_kernel's, term by term: |phi| has the bits of the two-transform formulation through
// m355_edt_sq.
constexpr uint32_t SD_NONE = 0x7FFF;            // no voxel of the other membership in the row
constexpr uint32_t SD_IN = 0x8000;              // membership bit of the sweep's code
constexpr int SD_MASK_PLANES = 1024;            // planes per launch: the mask is 128 bytes of kernel arguments
static_assert(M355_EDT_MAX_DIM <= (int)SD_NONE, "an index distance fits 15 bits");

struct SdPlanes {
  uint32_t on[SD_MASK_PLANES / 32];
};
__device__ __forceinline__ bool sd_on(const SdPlanes& m, uint32_t plane) { return (m.on[plane >> 5] >> (plane & 31)) & 1; }

__global__ __launch_bounds__(ED_NT) void sd_sweep_kernel(const float* __restrict__ target, uint16_t* __restrict__ code,
                                                         SdPlanes planes, size_t S, uint32_t rows, uint32_t D,
                                                         uint32_t rows_per_wave) {
  if (!sd_on(planes, blockIdx.y)) return;
  const float* t = target + blockIdx.y * S;
  uint16_t* kd = code + blockIdx.y * S;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * (ED_NT / 64) + (threadIdx.x >> 6);
  const uint32_t r0 = wave * rows_per_wave;
  if (r0 >= rows) return;                            // (the whole wave, as in edt_d_kernel)
  const uint32_t n = min(rows_per_wave, rows - r0) * D;   // <= ED_GROUP
  const uint32_t base = r0 * D;                      // < 2^31 voxels per plane (checked on the host)
  int run_start[ED_CHUNKS];
  uint32_t in_bits = 0;
  int carry = -1, prev = 0;                          // prev: the membership of the voxel before the chunk
#pragma unroll
  for (int c = 0; c < ED_CHUNKS; ++c) {
    run_start[c] = -1;
    if ((uint32_t)c * 64 < n) {                      // wave-uniform
      const uint32_t i = c * 64 + lane;
      const int m = i < n && t[base + i] > 0.5f;
      int pm = __shfl_up(m, 1, 64);
      if (lane == 0) pm = prev;
      int v = (i == 0 || pm != m) ? (int)i : -1;     // the first voxel of a run of one membership
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(v, off, 64);
        if ((int)lane >= off) v = max(v, o);
      }
      v = max(v, carry);
      carry = __shfl(v, 63, 64);
      prev = __shfl(m, 63, 64);
      run_start[c] = v;
      in_bits |= (uint32_t)m << c;
    }
  }
  constexpr int BIG = 1 << 30;
  carry = BIG;
  int next = 0;                                      // the membership of the voxel after the chunk
#pragma unroll
  for (int c = ED_CHUNKS - 1; c >= 0; --c) {
    if ((uint32_t)c * 64 < n) {
      const uint32_t i = c * 64 + lane;
      const int m = (in_bits >> c) & 1;
      int nm = __shfl_down(m, 1, 64);
      if (lane == 63) nm = next;
      int v = i < n && (i == n - 1 || nm != m) ? (int)i : BIG;   // the last voxel of a run
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_down(v, off, 64);
        if ((int)lane + off < 64) v = min(v, o);
      }
      v = min(v, carry);
      carry = __shfl(v, 0, 64);
      next = __shfl(m, 0, 64);
      if (i < n) {
        // the run is one sequence over the wave's rows: a neighbour found outside the voxel's own row is discarded
        const int row_first = (int)(i / D * D), row_last = row_first + (int)D - 1;
        const int kl = run_start[c] > row_first ? (int)i - run_start[c] + 1 : (int)SD_NONE;
        const int kr = v < row_last ? v + 1 - (int)i : (int)SD_NONE;
        kd[base + i] = (uint16_t)((uint32_t)min(kl, kr) | (m ? SD_IN : 0u));
      }
    }
  }
}

// edt_line_kernel with the membership: lines (o, j) as there, blockIdx.z the plane.  FROM_CODE: the input is the sweep's
// code and g = (s_in * k)^2; otherwise the previous pass's fp32 with the membership in the sign bit (`in` may be `out`).
// LAST: phi is written, and zeros into a plane that is switched off; otherwise such a plane is left alone.
template <bool FROM_CODE, bool LAST>
__global__ __launch_bounds__(ED_NT) void sd_line_kernel(const void* in, float* out, SdPlanes planes, size_t S, uint32_t n,
                                                        uint32_t inner, uint32_t line_stride, uint32_t outer_stride,
                                                        float s_in, float s) {
  extern __shared__ float g[];                       // [n][ED_DT], sign bit: inside
  const uint32_t lane = threadIdx.x % ED_DT, ty = threadIdx.x / ED_DT;
  const uint32_t j = blockIdx.x * ED_DT + lane;
  const bool live = j < inner;
  const uint32_t at = blockIdx.y * outer_stride + j;   // position 0 of the thread's line in its plane; < 2^31 when live
  const size_t plane = blockIdx.z * S;
  constexpr uint32_t ROWS = ED_NT / ED_DT;
  if (!sd_on(planes, blockIdx.z)) {                  // (the whole block)
    if (LAST && live)
      for (uint32_t p = ty; p < n; p += ROWS) out[plane + at + p * line_stride] = 0.f;
    return;
  }
  for (uint32_t p = ty; p < n; p += ROWS) {
    float v = INFINITY;
    if (live) {
      if (FROM_CODE) {
        const uint32_t c = ((const uint16_t*)in)[plane + at + p * line_stride], k = c & SD_NONE;
        if (k != SD_NONE) {
          const float t = __fmul_rn(s_in, (float)k);
          v = __fmul_rn(t, t);
        }
        if (c & SD_IN) v = __uint_as_float(__float_as_uint(v) | 0x80000000u);
      } else {
        v = ((const float*)in)[plane + at + p * line_stride];
      }
    }
    g[p * ED_DT + lane] = v;
  }
  __syncthreads();
  if (!live) return;
  // A line of +inf of one membership offers no candidate (every one is +inf + (s k)^2): its outputs are its inputs, and
  // the search, which would walk the whole line from every position, is skipped.  Most lines of a sparse target are of
  // that kind.  One walk over the line decides, and it ends at the first finite value or change of membership.
  bool search = false;
  const uint32_t first = __float_as_uint(g[lane]);
  for (uint32_t q = 0; q < n && !search; ++q) {
    const uint32_t u = __float_as_uint(g[q * ED_DT + lane]);
    search = (u & 0x7FFFFFFFu) != 0x7F800000u || ((u ^ first) >> 31) != 0;
  }
  for (uint32_t p = ty; p < n; p += ROWS) {
    const uint32_t me = __float_as_uint(g[p * ED_DT + lane]), sign = me & 0x80000000u;
    float m = __uint_as_float(me ^ sign);
    const uint32_t below = p, above = n - 1 - p, kmax = search ? max(below, above) : 0u;
    for (uint32_t k = 1; k <= kmax; ++k) {
      const float t = __fmul_rn(s, (float)k);
      const float sq = __fmul_rn(t, t);
      if (!(sq < m)) break;                          // nothing at distance >= k can be smaller (header of this file)
      if (k <= below) {
        const uint32_t u = __float_as_uint(g[(p - k) * ED_DT + lane]);
        m = fminf(m, (u ^ sign) & 0x80000000u ? sq : __fadd_rn(__uint_as_float(u & 0x7FFFFFFFu), sq));
      }
      if (k <= above) {
        const uint32_t u = __float_as_uint(g[(p + k) * ED_DT + lane]);
        m = fminf(m, (u ^ sign) & 0x80000000u ? sq : __fadd_rn(__uint_as_float(u & 0x7FFFFFFFu), sq));
      }
    }
    if (LAST) out[plane + at + p * line_stride] = isinf(m) ? 0.f : sign ? __fsub_rn(1.f, sqrt_rn(m)) : sqrt_rn(m);
    else out[plane + at + p * line_stride] = __uint_as_float(__float_as_uint(m) | sign);
  }
}

int check_volume(const char* what, const int32_t* s) {
  for (int a = 0; a < 3; ++a) M355_REQUIRE(s[a] >= 1, M355_EINVALID_ARG, "%s: size %d on axis %d", what, s[a], a);
  M355_REQUIRE((int64_t)s[0] * s[1] * s[2] < ((int64_t)1 << 31), M355_EINVALID_ARG, "%s: %lld voxels (fewer than 2^31)",
               what, (long long)((int64_t)s[0] * s[1] * s[2]));
  return M355_OK;
}

int64_t grid_for(int64_t n) { return std::max<int64_t>(1, std::min<int64_t>(m355::ceil_div(n, ED_NT), (int64_t)m355::num_cus() * 16)); }

}  // namespace

extern "C" size_t m355_edt_workspace(const int32_t* size3) {
  if (!size3 || size3[0] < 1 || size3[1] < 1 || size3[2] < 1) return 0;
  const int64_t S = (int64_t)size3[0] * size3[1] * size3[2];
  return (size_t)m355::round_up(S * (int64_t)sizeof(uint16_t), 256);   // the D sweep's index distances
}

extern "C" int m355_edt_sq(const uint8_t* sites, const int32_t* size3, const float* spacing3, float* d2, void* workspace,
                           void* stream) {
  M355_REQUIRE(sites && size3 && spacing3 && d2 && workspace, M355_EINVALID_ARG, "edt_sq: null pointer");
  if (int rc = check_volume("edt_sq", size3)) return rc;
  for (int a = 0; a < 3; ++a)
    M355_REQUIRE(isfinite(spacing3[a]) && spacing3[a] > 0.f, M355_EINVALID_ARG,
                 "edt_sq: spacing %g on axis %d (finite and > 0)", (double)spacing3[a], a);
  for (int a = 0; a < 3; ++a)
    M355_REQUIRE(size3[a] <= M355_EDT_MAX_DIM, M355_EUNSUPPORTED,
                 "edt_sq: size %d on axis %d (at most M355_EDT_MAX_DIM = %d: a line is staged in LDS)", size3[a], a,
                 M355_EDT_MAX_DIM);
  const uint32_t W = size3[0], H = size3[1], D = size3[2], rows = W * H;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t rpw = std::max<uint32_t>(1, ED_GROUP / D);
  const int64_t waves = m355::ceil_div(rows, rpw);
  hipLaunchKernelGGL(edt_d_kernel, dim3((unsigned)m355::ceil_div(waves, ED_NT / 64)), dim3(ED_NT), 0, st, sites,
                     (uint16_t*)workspace, rows, D, rpw);
  if (int rc = m355::check_launch("edt_sq: D sweep")) return rc;
  // along H: slab w, lines (w, d) for d < D, D apart
  hipLaunchKernelGGL(edt_line_kernel<true>, dim3((unsigned)m355::ceil_div(D, ED_DT), W), dim3(ED_NT),
                     (size_t)H * ED_DT * sizeof(float), st, (const void*)workspace, d2, H, D, D, H * D, spacing3[2],
                     spacing3[1]);
  if (int rc = m355::check_launch("edt_sq: H pass")) return rc;
  // along W: the lines are the H * D voxels of plane w = 0, H * D apart
  hipLaunchKernelGGL(edt_line_kernel<false>, dim3((unsigned)m355::ceil_div((int64_t)H * D, ED_DT), 1), dim3(ED_NT),
                     (size_t)W * ED_DT * sizeof(float), st, (const void*)d2, d2, W, H * D, H * D, 0u, 0.f, spacing3[0]);
  return m355::check_launch("edt_sq: W pass");
}

extern "C" size_t m355_signed_distance_workspace(int32_t planes, const int32_t* size3) {
  if (planes < 1 || !size3 || size3[0] < 1 || size3[1] < 1 || size3[2] < 1) return 0;
  const int64_t S = (int64_t)size3[0] * size3[1] * size3[2];
  return (size_t)m355::round_up((int64_t)planes * S * (int64_t)sizeof(uint16_t), 256);   // the sweep's codes
}

extern "C" int m355_signed_distance(const float* target, int32_t planes, const int32_t* size3, const float* spacing3,
                                    const uint8_t* plane_on, float* phi, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  M355_REQUIRE(target && size3 && spacing3 && phi && workspace, M355_EINVALID_ARG, "signed_distance: null pointer");
  M355_REQUIRE(planes >= 1, M355_EINVALID_ARG, "signed_distance: %d planes", planes);
  if (int rc = check_volume("signed_distance", size3)) return rc;
  for (int a = 0; a < 3; ++a)
    M355_REQUIRE(isfinite(spacing3[a]) && spacing3[a] > 0.f, M355_EINVALID_ARG,
                 "signed_distance: spacing %g on axis %d (finite and > 0)", (double)spacing3[a], a);
  for (int a = 0; a < 3; ++a)
    M355_REQUIRE(size3[a] <= M355_EDT_MAX_DIM, M355_EUNSUPPORTED,
                 "signed_distance: size %d on axis %d (at most M355_EDT_MAX_DIM = %d: a line is staged in LDS)", size3[a], a,
                 M355_EDT_MAX_DIM);
  M355_REQUIRE(workspace_bytes >= m355_signed_distance_workspace(planes, size3), M355_EWORKSPACE,
               "signed_distance: workspace of %zu bytes, %zu needed", workspace_bytes,
               m355_signed_distance_workspace(planes, size3));
  const uint32_t A0 = size3[0], A1 = size3[1], A2 = size3[2], rows = A0 * A1;
  const size_t S = (size_t)rows * A2;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t rpw = std::max<uint32_t>(1, ED_GROUP / A2);
  const unsigned sweep_blocks = (unsigned)m355::ceil_div(m355::ceil_div(rows, rpw), ED_NT / 64);
  for (int32_t p0 = 0; p0 < planes; p0 += SD_MASK_PLANES) {
    const int32_t np = std::min<int32_t>(SD_MASK_PLANES, planes - p0);
    SdPlanes mask = {};
    bool any = false;
    for (int32_t i = 0; i < np; ++i)
      if (!plane_on || plane_on[p0 + i]) {
        mask.on[i >> 5] |= 1u << (i & 31);
        any = true;
      }
    const float* t = target + (size_t)p0 * S;
    uint16_t* code = (uint16_t*)workspace + (size_t)p0 * S;
    float* out = phi + (size_t)p0 * S;
    if (any) {
      hipLaunchKernelGGL(sd_sweep_kernel, dim3(sweep_blocks, (unsigned)np), dim3(ED_NT), 0, st, t, code, mask, S, rows, A2,
                         rpw);
      if (int rc = m355::check_launch("signed_distance: sweep")) return rc;
      // along A1: slab a0, lines (a0, a2) for a2 < A2, A2 apart
      hipLaunchKernelGGL((sd_line_kernel<true, false>), dim3((unsigned)m355::ceil_div(A2, ED_DT), A0, (unsigned)np),
                         dim3(ED_NT), (size_t)A1 * ED_DT * sizeof(float), st, (const void*)code, out, mask, S, A1, A2, A2,
                         A1 * A2, spacing3[2], spacing3[1]);
      if (int rc = m355::check_launch("signed_distance: first line pass")) return rc;
    }
    // along A0, in place: the lines are the A1 * A2 voxels of slab a0 = 0, A1 * A2 apart.  Also zeroes the planes that are off.
    hipLaunchKernelGGL((sd_line_kernel<false, true>), dim3((unsigned)m355::ceil_div((int64_t)A1 * A2, ED_DT), 1, (unsigned)np),
                       dim3(ED_NT), (size_t)A0 * ED_DT * sizeof(float), st, (const void*)out, out, mask, S, A0, A1 * A2,
                       A1 * A2, 0u, 0.f, spacing3[0]);
    if (int rc = m355::check_launch("signed_distance: last line pass")) return rc;
  }
  return M355_OK;
}

extern "C" int m355_edt_sqrt(const float* d2, float* d, int64_t n, void* stream) {
  M355_REQUIRE(d2 && d, M355_EINVALID_ARG, "edt_sqrt: null pointer");
  M355_REQUIRE(n >= 1, M355_EINVALID_ARG, "edt_sqrt: %lld elements", (long long)n);
  hipLaunchKernelGGL(edt_sqrt_kernel, dim3((unsigned)grid_for(n)), dim3(ED_NT), 0, (hipStream_t)stream, d2, d, n);
  return m355::check_launch("edt_sqrt");
}

extern "C" int m355_surface_mask(const int32_t* x, int32_t value, const int32_t* size3, uint8_t* border, int32_t* count,
                                 void* stream) {
  M355_REQUIRE(x && size3 && border && count, M355_EINVALID_ARG, "surface_mask: null pointer");
  if (int rc = check_volume("surface_mask", size3)) return rc;
  const int64_t S = (int64_t)size3[0] * size3[1] * size3[2];
  hipLaunchKernelGGL(surface_mask_kernel, dim3((unsigned)grid_for(S)), dim3(ED_NT), 0, (hipStream_t)stream, x, value,
                     (uint32_t)size3[0], (uint32_t)size3[1], (uint32_t)size3[2], border, count);
  return m355::check_launch("surface_mask");
}

extern "C" int m355_surface_gather(const uint8_t* border, const float* d2, int64_t nvox, float* out, int32_t* cursor,
                                   int32_t capacity, void* stream) {
  M355_REQUIRE(border && d2 && out && cursor, M355_EINVALID_ARG, "surface_gather: null pointer");
  M355_REQUIRE(nvox >= 1 && nvox < ((int64_t)1 << 31), M355_EINVALID_ARG, "surface_gather: %lld voxels (1 .. 2^31 - 1)",
               (long long)nvox);
  M355_REQUIRE(capacity >= 0, M355_EINVALID_ARG, "surface_gather: capacity %d", capacity);
  hipLaunchKernelGGL(surface_gather_kernel, dim3((unsigned)grid_for(nvox)), dim3(ED_NT), 0, (hipStream_t)stream, border,
                     d2, nvox, out, cursor, capacity);
  return m355::check_launch("surface_gather");
}
