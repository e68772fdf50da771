// Interesting-slice search and slice mosaics of the contour images (evaluators.py: find_interesting_slices,
// ContourImageEvaluator).
//
//   slice_counts_kernel  foreground voxels per sagittal, coronal and axial slice of every subject of a call, each voxel
//                        read once for all three axes (descriptor table, one grid row per subject)
//   slice_rank_kernel    the slices with a non-zero count by count descending, ties by ascending slice id (rank by
//                        counting, one block per subject and plane)
//   slice_mosaic_kernel  up to three make_grid mosaics of 2-D slices in one launch (a gather)
//
// Counting.  A volume is [W, H, D] with D fastest.  A block owns a contiguous run of tiles of CT_NT * CT_V voxels and
// three LDS counter rows (W, H, D); a lane owns CT_V consecutive voxels (16-byte loads) and reduces them to a CT_V-bit
// foreground mask.  The voxels of a lane up to the end of its first row share one W and one H counter, and so do its
// neighbours: the lanes' popcounts are summed over the wave by row (a segmented shuffle reduction: rows are runs of
// consecutive lanes) and the first lane of a run adds the sum, so a wave issues one LDS atomic per row it touches and
// one per W slab instead of one per lane.  Voxels of a lane past the end of its first row (one lane in D / CT_V, or
// most of them when D < CT_V) and the D counters, which differ from lane to lane, take one LDS atomic per foreground
// voxel.  The block's non-zero counters go out with one global int32 atomic each.  Integer counts: exact and
// independent of the launch geometry and of the order of the atomics.
#include "common.hpp"
#include "ev_load.hpp"

namespace {

using namespace m355::ev;

constexpr int CT_NT = 256;
constexpr int CT_V = 16;                    // voxels per lane and step
constexpr int64_t CT_BLOCK_VOXELS = 65536;  // a block is worth launching for this many voxels

__device__ __forceinline__ int esize(int dt) {
  switch (dt) {
    case M355_EV_I16: case M355_EV_BF16: case M355_EV_F16: return 2;
    case M355_EV_I32: case M355_EV_F32: return 4;
    case M355_EV_I64: return 8;
    default: return 1;
  }
}

// foreground of one label-map element: torch's `data != 0` (a NaN is not equal to 0)
__device__ __forceinline__ bool fg1_map(const void* p, int dt, int64_t i) {
  switch (dt) {
    case M355_EV_I16: return ((const int16_t*)p)[i] != 0;
    case M355_EV_I32: return ((const int32_t*)p)[i] != 0;
    case M355_EV_I64: return ((const int64_t*)p)[i] != 0;
    case M355_EV_F32: return ((const float*)p)[i] != 0.f;
    default: return ((const uint8_t*)p)[i] != 0;
  }
}

// the same for elements [i, i + CT_V), i a multiple of CT_V, the map 16-byte aligned: bit j = element i + j
__device__ __forceinline__ uint32_t fg16_map(const void* p, int dt, int64_t i) {
  uint32_t m = 0;
  switch (dt) {
    case M355_EV_I16: {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint4 r = *(const uint4*)((const int16_t*)p + i + 8 * h);
        const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) m |= (uint32_t)(((w[j >> 1] >> (16 * (j & 1))) & 0xffff) != 0) << (8 * h + j);
      }
      break;
    }
    case M355_EV_I32: {
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const int4 r = *(const int4*)((const int32_t*)p + i + 4 * h);
        m |= ((uint32_t)(r.x != 0) | (uint32_t)(r.y != 0) << 1 | (uint32_t)(r.z != 0) << 2 | (uint32_t)(r.w != 0) << 3)
             << (4 * h);
      }
      break;
    }
    case M355_EV_F32: {
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const float4 r = *(const float4*)((const float*)p + i + 4 * h);
        m |= ((uint32_t)(r.x != 0.f) | (uint32_t)(r.y != 0.f) << 1 | (uint32_t)(r.z != 0.f) << 2 |
              (uint32_t)(r.w != 0.f) << 3) << (4 * h);
      }
      break;
    }
    case M355_EV_I64: {
#pragma unroll
      for (int h = 0; h < 8; ++h) {
        const longlong2 r = *(const longlong2*)((const int64_t*)p + i + 2 * h);
        m |= ((uint32_t)(r.x != 0) | (uint32_t)(r.y != 0) << 1) << (2 * h);
      }
      break;
    }
    default: {   // bool, uint8, int8
      const uint4 r = *(const uint4*)((const uint8_t*)p + i);
      const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int j = 0; j < CT_V; ++j) m |= (uint32_t)(((w[j >> 2] >> (8 * (j & 3))) & 0xff) != 0) << j;
    }
  }
  return m;
}

// foreground of a [C, S] score or one-hot map: argmax over the channels != 0.  Channel 0 stays the argmax unless a
// later channel takes it from channel 0's value (first maximum, a NaN is the maximum): what happens after that does not
// matter.
template <int SD>
__device__ __forceinline__ bool fg1_scores(const void* p, int C, int64_t S, int64_t i) {
  const float best = load_score1<SD>(p, i);
  bool fg = false;
  for (int c = 1; c < C; ++c) fg |= takes(best, load_score1<SD>(p, (int64_t)c * S + i));
  return fg;
}
template <int SD>
__device__ __forceinline__ uint32_t fg16_scores(const void* p, int C, int64_t S, int64_t i) {
  uint32_t m = 0;
#pragma unroll
  for (int h = 0; h < CT_V / SCORE_V; ++h) {
    float best[SCORE_V];
    load_scores8<SD>(p, i + SCORE_V * h, best);
    for (int c = 1; c < C; ++c) {
      float s[SCORE_V];
      load_scores8<SD>(p, (int64_t)c * S + i + SCORE_V * h, s);
#pragma unroll
      for (int j = 0; j < SCORE_V; ++j) m |= (uint32_t)takes(best[j], s[j]) << (SCORE_V * h + j);
    }
  }
  return m;
}

// foreground mask of voxels [i, i + CT_V) of subject d (bits past S are 0); `vec`: the 16-byte loads may be used
__device__ __forceinline__ uint32_t fg_mask(const m355_slice_counts_desc& d, int64_t S, int64_t i, bool vec) {
  if (i >= S) return 0;
  const int C = d.channels;
  if (vec && i + CT_V <= S) {
    if (C == 0) return fg16_map(d.data, d.dtype, i);
    if (d.dtype == M355_EV_F32) return fg16_scores<M355_EV_F32>(d.data, C, S, i);
    if (d.dtype == M355_EV_BF16) return fg16_scores<M355_EV_BF16>(d.data, C, S, i);
    return fg16_scores<M355_EV_F16>(d.data, C, S, i);
  }
  uint32_t m = 0;
  for (int j = 0; j < CT_V && i + j < S; ++j) {
    bool fg;
    if (C == 0) fg = fg1_map(d.data, d.dtype, i + j);
    else if (d.dtype == M355_EV_F32) fg = fg1_scores<M355_EV_F32>(d.data, C, S, i + j);
    else if (d.dtype == M355_EV_BF16) fg = fg1_scores<M355_EV_BF16>(d.data, C, S, i + j);
    else fg = fg1_scores<M355_EV_F16>(d.data, C, S, i + j);
    m |= (uint32_t)fg << j;
  }
  return m;
}

// c[idx] += the sum of v over the run of consecutive lanes that share `key` (keys do not decrease along the wave):
// one LDS atomic per run, by its first lane.  Called by all 64 lanes.
__device__ __forceinline__ void add_by_run(uint32_t* c, uint32_t key, uint32_t idx, uint32_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t ov = __shfl_down(v, off, 64), ok = __shfl_down(key, off, 64);
    if (lane + off < 64 && ok == key) v += ov;
  }
  const uint32_t before = __shfl_up(key, 1, 64);
  if ((lane == 0 || before != key) && v) atomicAdd(&c[idx], v);
}

__global__ __launch_bounds__(CT_NT) void slice_counts_kernel(const m355_slice_counts_desc* __restrict__ descs,
                                                            int32_t* __restrict__ counts) {
  __shared__ uint32_t cnt[3 * M355_SLICE_MAX_DIM];
  const m355_slice_counts_desc d = descs[blockIdx.y];
  const uint32_t W = d.size3[0], H = d.size3[1], D = d.size3[2], T = W + H + D;
  const uint32_t S = W * H * D;   // < 2^31 (checked on the host)
  for (uint32_t k = threadIdx.x; k < T; k += CT_NT) cnt[k] = 0;
  __syncthreads();
  uint32_t* cw = cnt;
  uint32_t* ch = cnt + W;
  uint32_t* cd = cnt + W + H;

  constexpr uint32_t TILE = CT_NT * CT_V;
  const uint32_t tiles = (S + TILE - 1) / TILE, per = (tiles + gridDim.x - 1) / gridDim.x;
  const uint32_t t0 = min(tiles, blockIdx.x * per), t1 = min(tiles, t0 + per);
  const bool vec = ((uintptr_t)d.data & 15) == 0 && (d.channels == 0 || S % SCORE_V == 0);
  // add_by_run shuffles over the whole wave and takes keys that do not decrease along it.  So the trip count is the same
  // for every lane, and a lane past the end of the volume (i >= S) must still reach both add_by_run calls: it brings a
  // zero popcount under a row key above every row of the volume.  No early exit for such lanes.
  for (uint32_t t = t0; t < t1; ++t) {
    const uint32_t i = t * TILE + threadIdx.x * CT_V;   // < S + TILE < 2^32
    const uint32_t mask = fg_mask(d, S, i, vec);
    const uint32_t r0 = i / D, d0 = i - r0 * D;          // the lane's first row w * H + h, and where in it
    const uint32_t w0 = r0 / H, h0 = r0 - w0 * H;
    const uint32_t n0 = min((uint32_t)CT_V, D - d0);     // voxels of the lane inside that row
    const uint32_t first = mask & ((1u << n0) - 1), rest = mask & ~((1u << n0) - 1);
    const uint32_t c0 = __popc(first);
    add_by_run(ch, r0, h0, c0);
    add_by_run(cw, w0, w0, c0);
    for (uint32_t b = first; b; b &= b - 1) atomicAdd(&cd[d0 + (__ffs(b) - 1)], 1u);
    for (uint32_t b = rest; b; b &= b - 1) {
      const uint32_t v = i + (__ffs(b) - 1), r = v / D, w = r / H;
      atomicAdd(&cw[w], 1u);
      atomicAdd(&ch[r - w * H], 1u);
      atomicAdd(&cd[v - r * D], 1u);
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < T; k += CT_NT)
    if (cnt[k]) atomicAdd(&counts[d.counts_offset + k], (int32_t)cnt[k]);
}

__global__ __launch_bounds__(CT_NT) void slice_rank_kernel(const int32_t* __restrict__ counts,
                                                          const m355_slice_seg* __restrict__ segs,
                                                          int32_t* __restrict__ ids, int32_t* __restrict__ ranked,
                                                          int32_t* __restrict__ nums) {
  __shared__ int32_t c[M355_SLICE_MAX_DIM];
  __shared__ int nonzero;
  const m355_slice_seg seg = segs[blockIdx.x];
  const int len = seg.len;
  if (threadIdx.x == 0) nonzero = 0;
  for (int k = threadIdx.x; k < len; k += CT_NT) c[k] = counts[seg.offset + k];
  __syncthreads();
  int mine = 0;
  for (int k = threadIdx.x; k < len; k += CT_NT) {
    const int32_t ck = c[k];
    if (ck <= 0) continue;
    int rank = 0;
    for (int j = 0; j < len; ++j) rank += (c[j] > ck) | ((c[j] == ck) & (j < k));
    ids[seg.offset + rank] = k;
    ranked[seg.offset + rank] = ck;
    ++mine;
  }
  if (mine) atomicAdd(&nonzero, mine);
  __syncthreads();
  for (int p = nonzero + threadIdx.x; p < len; p += CT_NT) {
    ids[seg.offset + p] = -1;
    ranked[seg.offset + p] = 0;
  }
  if (threadIdx.x == 0) nums[blockIdx.x] = nonzero;
}

// ---------------------------------------------------------------------------------------------- mosaics
constexpr int MAX_MOSAICS = 3;
struct MosaicArgs {
  m355_slice_mosaic_desc m[MAX_MOSAICS];
};

__device__ __forceinline__ void store_bits(void* out, int size, int64_t i, uint64_t bits) {
  switch (size) {
    case 1: ((uint8_t*)out)[i] = (uint8_t)bits; break;
    case 2: ((uint16_t*)out)[i] = (uint16_t)bits; break;
    case 4: ((uint32_t*)out)[i] = (uint32_t)bits; break;
    default: ((uint64_t*)out)[i] = bits;
  }
}
__device__ __forceinline__ uint64_t load_bits(const void* p, int size, int64_t i) {
  switch (size) {
    case 1: return ((const uint8_t*)p)[i];
    case 2: return ((const uint16_t*)p)[i];
    case 4: return ((const uint32_t*)p)[i];
    default: return ((const uint64_t*)p)[i];
  }
}
// the pad value in the mosaic's element type
__device__ __forceinline__ uint64_t pad_bits(float pad, int dt) {
  switch (dt) {
    case M355_EV_F32: return __float_as_uint(pad);
    case M355_EV_BF16: return __float_as_uint(pad) >> 16;   // (the pads in use, 0 and -1, are exact)
    case M355_EV_F16: return __half_as_ushort(__float2half(pad));
    case M355_EV_BOOL: return pad != 0.f;
    default: return (uint64_t)(int64_t)pad;
  }
}

__global__ __launch_bounds__(CT_NT) void slice_mosaic_kernel(MosaicArgs a, const m355_slice_tile_desc* __restrict__ tiles) {
  const m355_slice_mosaic_desc m = a.m[blockIdx.y];
  const int64_t cells = (int64_t)m.rows * m.cols;
  const int size = esize(m.dtype);
  const int xmaps = min(m.ncol, m.ntiles), sh = m.tile_h + 1, sw = m.tile_w + 1;
  const uint64_t pad = pad_bits(m.pad, m.dtype);
  for (int64_t cell = blockIdx.x * CT_NT + threadIdx.x; cell < cells; cell += gridDim.x * CT_NT) {
    const int r = (int)(cell / m.cols), c = (int)(cell - (int64_t)r * m.cols);
    int k = -1;
    if (m.ntiles == 1) {
      k = 0;
    } else {
      const int tr = r / sh, tc = c / sw;
      if (r - tr * sh >= 1 && c - tc * sw >= 1 && tc < xmaps && tr * xmaps + tc < m.ntiles) k = tr * xmaps + tc;
    }
    uint64_t bits = pad;
    if (k >= 0) {
      const m355_slice_tile_desc t = tiles[m.first_tile + k];
      bits = 0;
      if (t.src) {
        const int i = r - t.row0, j = c - t.col0, s = t.slice;
        const int64_t H = t.size3[1], D = t.size3[2];
        int64_t at;
        if (t.plane == M355_PLANE_AXIAL) at = (i * H + j) * D + s;
        else if (t.plane == M355_PLANE_CORONAL) at = (j * H + s) * D + (D - 1 - i);
        else at = (s * H + j) * D + (D - 1 - i);
        if (t.dtype == m.dtype) {
          bits = load_bits(t.src, size, at);
        } else {   // a float32 mosaic of 16-bit floats
          const uint16_t h = ((const uint16_t*)t.src)[at];
          bits = t.dtype == M355_EV_BF16 ? (uint32_t)h << 16 : __float_as_uint(__half2float(__ushort_as_half(h)));
        }
      }
    }
    store_bits(m.out, size, cell, bits);
  }
}

bool map_type(int dt) { return dt >= M355_EV_BOOL && dt <= M355_EV_F32; }
bool float_type(int dt) { return dt == M355_EV_F32 || dt == M355_EV_BF16 || dt == M355_EV_F16; }

// size3 of a volume the kernels take: every dimension 1 .. M355_SLICE_MAX_DIM, fewer than 2^31 voxels
int check_size3(const char* what, int i, const int32_t* s) {
  for (int j = 0; j < 3; ++j)
    M355_REQUIRE(s[j] >= 1 && s[j] <= M355_SLICE_MAX_DIM, M355_EINVALID_ARG,
                 "%s: subject %d: size %d on axis %d (1 .. %d: the counters of an axis are one LDS row)", what, i, s[j],
                 j, M355_SLICE_MAX_DIM);
  M355_REQUIRE((int64_t)s[0] * s[1] * s[2] < ((int64_t)1 << 31), M355_EINVALID_ARG,
               "%s: subject %d: %lld voxels (fewer than 2^31)", what, i, (long long)((int64_t)s[0] * s[1] * s[2]));
  return M355_OK;
}

}  // namespace

extern "C" int m355_slice_counts(const m355_slice_counts_desc* descs, int32_t n, void* dev_descs, int32_t* counts,
                                 void* stream) {
  M355_REQUIRE(descs && dev_descs && counts, M355_EINVALID_ARG, "slice_counts: null pointer");
  M355_REQUIRE(n >= 1 && n <= 65535, M355_EINVALID_ARG, "slice_counts: %d subjects (1 .. 65535)", n);
  int64_t total = 0, maxS = 1;
  for (int i = 0; i < n; ++i) {
    const m355_slice_counts_desc& d = descs[i];
    M355_REQUIRE(d.data, M355_EINVALID_ARG, "slice_counts: subject %d: null volume", i);
    if (int rc = check_size3("slice_counts", i, d.size3)) return rc;
    M355_REQUIRE(d.channels >= 0 && d.channels <= M355_EV_MAX_CHANNELS, M355_EINVALID_ARG,
                 "slice_counts: subject %d: %d channels (0: a label map, 1 .. %d: a one-hot or score map)", i, d.channels,
                 M355_EV_MAX_CHANNELS);
    if (d.channels == 0)
      M355_REQUIRE(map_type(d.dtype), M355_EINVALID_ARG, "slice_counts: subject %d: label map element type %d", i, d.dtype);
    else
      M355_REQUIRE(float_type(d.dtype), M355_EINVALID_ARG,
                   "slice_counts: subject %d: one-hot element type %d (float32, bfloat16, float16)", i, d.dtype);
    M355_REQUIRE(d.counts_offset == total, M355_EINVALID_ARG,
                 "slice_counts: subject %d: counts offset %lld, expected %lld (the tables follow one another)", i,
                 (long long)d.counts_offset, (long long)total);
    total += (int64_t)d.size3[0] + d.size3[1] + d.size3[2];
    maxS = std::max<int64_t>(maxS, (int64_t)d.size3[0] * d.size3[1] * d.size3[2]);
  }
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(dev_descs, descs, sizeof(m355_slice_counts_desc) * n, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(counts, 0, sizeof(int32_t) * total, st) != hipSuccess)
    return m355::check_launch("slice_counts: descriptor copy / memset");
  const int64_t cap = std::max<int64_t>(1, (int64_t)m355::num_cus() * 4 / n);
  const dim3 g((unsigned)std::min(cap, m355::ceil_div(maxS, CT_BLOCK_VOXELS)), (unsigned)n);
  hipLaunchKernelGGL(slice_counts_kernel, g, dim3(CT_NT), 0, st, (const m355_slice_counts_desc*)dev_descs, counts);
  return m355::check_launch("slice_counts");
}

extern "C" int m355_slice_rank(const int32_t* counts, const m355_slice_seg* segs, int32_t nseg, void* dev_descs,
                               int32_t* ids, int32_t* ranked, int32_t* nums, void* stream) {
  M355_REQUIRE(counts && segs && dev_descs && ids && ranked && nums, M355_EINVALID_ARG, "slice_rank: null pointer");
  M355_REQUIRE(nseg >= 1 && nseg <= 3 * 65535, M355_EINVALID_ARG, "slice_rank: %d segments (1 .. %d)", nseg, 3 * 65535);
  for (int i = 0; i < nseg; ++i)
    M355_REQUIRE(segs[i].offset >= 0 && segs[i].len >= 1 && segs[i].len <= M355_SLICE_MAX_DIM, M355_EINVALID_ARG,
                 "slice_rank: segment %d: offset %lld, %d slices (1 .. %d)", i, (long long)segs[i].offset, segs[i].len,
                 M355_SLICE_MAX_DIM);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(dev_descs, segs, sizeof(m355_slice_seg) * nseg, hipMemcpyHostToDevice, st) != hipSuccess)
    return m355::check_launch("slice_rank: descriptor copy");
  hipLaunchKernelGGL(slice_rank_kernel, dim3(nseg), dim3(CT_NT), 0, st, counts, (const m355_slice_seg*)dev_descs, ids,
                     ranked, nums);
  return m355::check_launch("slice_rank");
}

extern "C" int m355_slice_mosaic(const m355_slice_mosaic_desc* mosaics, int32_t nmosaics,
                                 const m355_slice_tile_desc* tiles, int32_t ntiles, void* dev_descs, void* stream) {
  M355_REQUIRE(mosaics && tiles && dev_descs, M355_EINVALID_ARG, "slice_mosaic: null pointer");
  M355_REQUIRE(nmosaics >= 1 && nmosaics <= MAX_MOSAICS, M355_EINVALID_ARG, "slice_mosaic: %d mosaics (1 .. %d)",
               nmosaics, MAX_MOSAICS);
  M355_REQUIRE(ntiles >= 1, M355_EINVALID_ARG, "slice_mosaic: %d tiles", ntiles);
  MosaicArgs a{};
  int64_t max_cells = 1;
  int32_t next_tile = 0;
  for (int q = 0; q < nmosaics; ++q) {
    const m355_slice_mosaic_desc& m = mosaics[q];
    M355_REQUIRE(m.out, M355_EINVALID_ARG, "slice_mosaic: mosaic %d: null output", q);
    M355_REQUIRE(m.dtype >= M355_EV_BOOL && m.dtype <= M355_EV_F16, M355_EINVALID_ARG,
                 "slice_mosaic: mosaic %d: element type %d", q, m.dtype);
    M355_REQUIRE(m.ntiles >= 1 && m.ncol >= 1 && m.first_tile == next_tile && (int64_t)next_tile + m.ntiles <= ntiles,
                 M355_EINVALID_ARG, "slice_mosaic: mosaic %d: tiles [%d, %d + %d) of %d in rows of %d", q, m.first_tile,
                 m.first_tile, m.ntiles, ntiles, m.ncol);
    next_tile += m.ntiles;
    M355_REQUIRE(m.tile_h >= 1 && m.tile_w >= 1 && m.tile_h <= M355_SLICE_MAX_DIM && m.tile_w <= M355_SLICE_MAX_DIM,
                 M355_EINVALID_ARG, "slice_mosaic: mosaic %d: tiles of %d x %d", q, m.tile_h, m.tile_w);
    const int64_t xmaps = std::min(m.ncol, m.ntiles), ymaps = m355::ceil_div(m.ntiles, xmaps);
    const bool bare = m.ntiles == 1;
    const int64_t rows = bare ? m.tile_h : ymaps * (m.tile_h + 1) + 1, cols = bare ? m.tile_w : xmaps * (m.tile_w + 1) + 1;
    M355_REQUIRE(m.rows == rows && m.cols == cols && rows * cols < ((int64_t)1 << 31), M355_EINVALID_ARG,
                 "slice_mosaic: mosaic %d: %d x %d cells, %lld x %lld expected (fewer than 2^31)", q, m.rows, m.cols,
                 (long long)rows, (long long)cols);
    for (int k = 0; k < m.ntiles; ++k) {
      const m355_slice_tile_desc& t = tiles[m.first_tile + k];
      const int idx = m.first_tile + k;
      const int row0 = bare ? 0 : (int)(k / xmaps) * (m.tile_h + 1) + 1, col0 = bare ? 0 : (int)(k % xmaps) * (m.tile_w + 1) + 1;
      M355_REQUIRE(t.row0 == row0 && t.col0 == col0, M355_EINVALID_ARG,
                   "slice_mosaic: tile %d at (%d, %d), make_grid puts it at (%d, %d)", idx, t.row0, t.col0, row0, col0);
      if (!t.src) continue;
      if (int rc = check_size3("slice_mosaic", idx, t.size3)) return rc;
      M355_REQUIRE(t.plane >= M355_PLANE_SAGGITAL && t.plane <= M355_PLANE_AXIAL, M355_EINVALID_ARG,
                   "slice_mosaic: tile %d: plane %d", idx, t.plane);
      M355_REQUIRE(t.slice >= 0 && t.slice < t.size3[t.plane], M355_EINVALID_ARG,
                   "slice_mosaic: tile %d: slice %d of %d", idx, t.slice, t.size3[t.plane]);
      const int h = t.plane == M355_PLANE_AXIAL ? t.size3[0] : t.size3[2];
      const int w = t.plane == M355_PLANE_SAGGITAL ? t.size3[1] : t.plane == M355_PLANE_CORONAL ? t.size3[0] : t.size3[1];
      M355_REQUIRE(h == m.tile_h && w == m.tile_w, M355_EINVALID_ARG,
                   "slice_mosaic: tile %d is %d x %d in a mosaic of %d x %d tiles", idx, h, w, m.tile_h, m.tile_w);
      M355_REQUIRE(t.dtype == m.dtype || (m.dtype == M355_EV_F32 && (t.dtype == M355_EV_BF16 || t.dtype == M355_EV_F16)),
                   M355_EINVALID_ARG, "slice_mosaic: tile %d of element type %d in a mosaic of type %d", idx, t.dtype,
                   m.dtype);
    }
    max_cells = std::max(max_cells, rows * cols);
    a.m[q] = m;
  }
  M355_REQUIRE(next_tile == ntiles, M355_EINVALID_ARG, "slice_mosaic: %d tiles given, the mosaics hold %d", ntiles,
               next_tile);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(dev_descs, tiles, sizeof(m355_slice_tile_desc) * ntiles, hipMemcpyHostToDevice, st) != hipSuccess)
    return m355::check_launch("slice_mosaic: descriptor copy");
  const dim3 g((unsigned)std::min<int64_t>(m355::ceil_div(max_cells, CT_NT), (int64_t)m355::num_cus() * 8), (unsigned)nmosaics);
  hipLaunchKernelGGL(slice_mosaic_kernel, g, dim3(CT_NT), 0, st, a, (const m355_slice_tile_desc*)dev_descs);
  return m355::check_launch("slice_mosaic");
}
