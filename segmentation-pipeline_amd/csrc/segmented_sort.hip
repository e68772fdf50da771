// Segmented LSD radix sort of 32-bit keys: R segments of M keys each, ascending, key-only, stable in every
// pass.  Only the bits [0, end_bit) take part; ceil(end_bit / 8) passes of 8-bit digits (the last one may be narrower).
//
// One pass over a segment, tiles of SS_TILE keys, four launches:
//   ss_hist      a block per (tile, segment): the 256 digit counts of its tile -> hist[segment][digit][tile].  LDS integer
//                atomics: they only count.
//   ss_rowsum    a wave per (digit, segment): the digit's count in the segment
//   ss_scan      a wave per (digit, segment): the exclusive prefix sum of hist in (digit, tile) order, which is the order
//                of the output: all keys of digit 0, tile by tile, then digit 1, ...  hist[segment][digit][tile] becomes
//                the first output position of that tile's keys of that digit.
//   ss_scatter   a block per (tile, segment): ranks its keys and writes them.  A key's position is decided without any
//                atomic: wave w owns the keys [w * SS_WAVE_KEYS, (w + 1) * SS_WAVE_KEYS) of the tile, in rounds of 64
//                consecutive keys; in a round the lanes with the same digit find each other by eight 64-bit ballots,
//                the lowest of them reads and advances the wave's count of that digit in LDS, and a lane's rank is that
//                count plus the number of matching lanes below it.  The waves' counts are then added in wave order, the
//                tiles' in tile order (ss_scan): rank order = (tile, wave, round, lane) order = index order, which is what
//                stable means.  The keys go through LDS in their sorted order first, so a block writes runs.
//
// Ping-pong: pass 0 reads `keys`, the last pass writes `out`, the passes between alternate between `out` and a buffer of
// R * M keys in the workspace; `keys` is not written and must not overlap `out`.
//   workspace = round_up(4 R M, 256) + 4 * 256 * R * (ceil(M / SS_TILE) + 1) + 256 bytes
// No allocation, no synchronisation, no host read, no memset: every word that is read was written by the launch before.
#include "common.hpp"

namespace m355 {

constexpr int SS_TILE = 4096;                 // keys of a block
constexpr int SS_THREADS = 256;
constexpr int SS_WAVES = SS_THREADS / 64;
constexpr int SS_WAVE_KEYS = SS_TILE / SS_WAVES;
constexpr int SS_ROUNDS = SS_WAVE_KEYS / 64;  // rounds of 64 keys per wave
constexpr int SS_BINS = 256;

__device__ __forceinline__ uint32_t ss_digit(uint32_t key, int shift, uint32_t mask) { return (key >> shift) & mask; }

__global__ __launch_bounds__(SS_THREADS) void ss_hist_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ hist,
                                                             int64_t M, int nblk, int shift, uint32_t mask) {
  __shared__ uint32_t lh[SS_BINS];
  lh[threadIdx.x] = 0u;
  __syncthreads();
  const int64_t r = blockIdx.y;
  const uint32_t* seg = in + r * M;
  const int64_t begin = (int64_t)blockIdx.x * SS_TILE, end = min(M, begin + SS_TILE);
  for (int64_t i = begin + threadIdx.x; i < end; i += SS_THREADS) atomicAdd(&lh[ss_digit(seg[i], shift, mask)], 1u);
  __syncthreads();
  hist[(r * SS_BINS + threadIdx.x) * nblk + blockIdx.x] = lh[threadIdx.x];
}

// The scan, two launches of one wave per (digit, segment) row of hist: the row's total -> dtot[segment][digit]; then the
// row's start -- the totals of the digits below it -- and the running prefix along the row, 64 tiles at a time.
__global__ __launch_bounds__(64) void ss_rowsum_kernel(const uint32_t* __restrict__ hist, uint32_t* __restrict__ dtot,
                                                       int nblk) {
  const int lane = threadIdx.x, d = blockIdx.x;
  const int64_t r = blockIdx.y;
  const uint32_t* row = hist + (r * SS_BINS + d) * nblk;
  uint32_t s = 0;
  for (int b = lane; b < nblk; b += 64) s += row[b];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += (uint32_t)__shfl_xor((int)s, off, 64);
  if (lane == 0) dtot[r * SS_BINS + d] = s;
}

__global__ __launch_bounds__(64) void ss_scan_kernel(uint32_t* __restrict__ hist, const uint32_t* __restrict__ dtot,
                                                     int nblk) {
  const int lane = threadIdx.x, d = blockIdx.x;
  const int64_t r = blockIdx.y;
  uint32_t run = 0;
  for (int i = lane; i < d; i += 64) run += dtot[r * SS_BINS + i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) run += (uint32_t)__shfl_xor((int)run, off, 64);
  uint32_t* row = hist + (r * SS_BINS + d) * nblk;
  for (int b0 = 0; b0 < nblk; b0 += 64) {
    const int b = b0 + lane;
    const uint32_t v = b < nblk ? row[b] : 0u;
    const uint32_t in = wave_incl_scan(v);
    if (b < nblk) row[b] = run + in - v;
    run += (uint32_t)__shfl((int)in, 63, 64);
  }
}

__global__ __launch_bounds__(SS_THREADS) void ss_scatter_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                                const uint32_t* __restrict__ hist, int64_t M, int nblk,
                                                                int shift, uint32_t mask) {
  __shared__ uint32_t whist[SS_WAVES][SS_BINS];   // a wave's digit counts, then its offset among the waves
  __shared__ uint32_t lkeys[SS_TILE];
  __shared__ uint32_t dstart[SS_BINS];            // where a digit starts in the sorted tile
  __shared__ uint32_t gbase[SS_BINS];             // where this tile's keys of a digit start in the segment
  __shared__ uint32_t wtot[SS_WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r = blockIdx.y;
  const uint32_t* seg = in + r * M;
  const int64_t begin = (int64_t)blockIdx.x * SS_TILE;
  const int ntile = (int)min((int64_t)SS_TILE, M - begin);
#pragma unroll
  for (int i = 0; i < SS_WAVES; ++i) whist[i][threadIdx.x] = 0u;
  __syncthreads();

  uint32_t key[SS_ROUNDS], rank[SS_ROUNDS];
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
#pragma unroll
  for (int i = 0; i < SS_ROUNDS; ++i) {
    const int j = w * SS_WAVE_KEYS + i * 64 + lane;
    const bool valid = j < ntile;
    key[i] = valid ? seg[begin + j] : 0u;
    const uint32_t d = ss_digit(key[i], shift, mask);
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const uint64_t bal = __ballot(bit);
      m &= bit ? bal : ~bal;
    }
    // (a lane outside the tile matches nobody and nobody matches it: it is not in ballot(valid))
    const int leader = valid ? __ffsll((long long)m) - 1 : lane;
    uint32_t before = 0u;
    if (valid && lane == leader) {
      before = whist[w][d];
      whist[w][d] = before + (uint32_t)__popcll(m);
    }
    before = (uint32_t)__shfl((int)before, leader, 64);
    rank[i] = before + (uint32_t)__popcll(m & below);
  }
  __syncthreads();

  // thread d: digit d's counts in wave order -> offsets; the digit's start in the tile; its start in the segment
  uint32_t total = 0;
#pragma unroll
  for (int i = 0; i < SS_WAVES; ++i) {
    const uint32_t c = whist[i][threadIdx.x];
    whist[i][threadIdx.x] = total;
    total += c;
  }
  const uint32_t incl = wave_incl_scan(total);
  if (lane == 63) wtot[w] = incl;
  gbase[threadIdx.x] = hist[(r * SS_BINS + threadIdx.x) * nblk + blockIdx.x];
  __syncthreads();
  uint32_t start = incl - total;
  for (int i = 0; i < w; ++i) start += wtot[i];
  dstart[threadIdx.x] = start;
  __syncthreads();

#pragma unroll
  for (int i = 0; i < SS_ROUNDS; ++i) {
    const int j = w * SS_WAVE_KEYS + i * 64 + lane;
    if (j < ntile) {
      const uint32_t d = ss_digit(key[i], shift, mask);
      lkeys[dstart[d] + whist[w][d] + rank[i]] = key[i];   // < ntile: the ranks of a tile are a permutation of [0, ntile)
    }
  }
  __syncthreads();
  uint32_t* oseg = out + r * M;
  for (int j = threadIdx.x; j < ntile; j += SS_THREADS) {
    const uint32_t k = lkeys[j];
    const uint32_t d = ss_digit(k, shift, mask);
    oseg[gbase[d] + ((uint32_t)j - dstart[d])] = k;
  }
}

struct SsLayout {
  int nblk, passes;
  size_t hist, dtot, bytes;   // the byte offsets of the tiles' and the segments' digit counts behind the second key buffer; the whole
};
static inline SsLayout ss_layout(int64_t R, int64_t M, int end_bit) {
  SsLayout l;
  l.nblk = (int)ceil_div(M, SS_TILE);
  l.passes = (end_bit + 7) / 8;
  l.hist = (size_t)round_up(4 * R * M, 256);
  l.dtot = l.hist + (size_t)4 * SS_BINS * R * l.nblk;
  l.bytes = l.dtot + (size_t)4 * SS_BINS * R + 256;
  return l;
}

static int ss_check(const char* what, int64_t R, int64_t M) {
  M355_REQUIRE(R > 0 && M > 0, M355_EINVALID_ARG, "%s: non-positive size", what);
  M355_REQUIRE(R <= 65535, M355_EUNSUPPORTED, "%s: R > 65535", what);
  M355_REQUIRE(M <= 0x7fffffffll, M355_EUNSUPPORTED, "%s: M > 2^31 - 1", what);
  return M355_OK;
}

// the launches of a checked call (lovasz_loss.hip calls this with its own buffers)
void segmented_sort_launch(const uint32_t* keys, uint32_t* out, int64_t R, int64_t M, int end_bit, void* workspace,
                           hipStream_t st) {
  const SsLayout l = ss_layout(R, M, end_bit);
  uint32_t* tmp = (uint32_t*)workspace;
  uint32_t* hist = (uint32_t*)((char*)workspace + l.hist);
  uint32_t* dtot = (uint32_t*)((char*)workspace + l.dtot);
  const uint32_t* src = keys;
  const dim3 grid((unsigned)l.nblk, (unsigned)R);
  for (int i = 0; i < l.passes; ++i) {
    uint32_t* dst = ((l.passes - 1 - i) & 1) ? tmp : out;
    const int shift = 8 * i, bits = std::min(8, end_bit - shift);
    const uint32_t mask = (1u << bits) - 1u;
    hipLaunchKernelGGL(ss_hist_kernel, grid, dim3(SS_THREADS), 0, st, src, hist, M, l.nblk, shift, mask);
    hipLaunchKernelGGL(ss_rowsum_kernel, dim3(SS_BINS, (unsigned)R), dim3(64), 0, st, (const uint32_t*)hist, dtot, l.nblk);
    hipLaunchKernelGGL(ss_scan_kernel, dim3(SS_BINS, (unsigned)R), dim3(64), 0, st, hist, (const uint32_t*)dtot, l.nblk);
    hipLaunchKernelGGL(ss_scatter_kernel, grid, dim3(SS_THREADS), 0, st, src, dst, (const uint32_t*)hist, M, l.nblk, shift,
                       mask);
    src = dst;
  }
}

size_t segmented_sort_bytes(int64_t R, int64_t M) { return ss_layout(R, M, 32).bytes; }

}  // namespace m355

using namespace m355;

extern "C" size_t m355_segmented_sort_workspace(int64_t R, int64_t M) {
  if (R <= 0 || M <= 0) return 0;
  return segmented_sort_bytes(R, M);
}

extern "C" int32_t m355_segmented_sort_tile(void) { return SS_TILE; }

extern "C" int m355_segmented_sort_u32(const uint32_t* keys, uint32_t* out, int64_t R, int64_t M, int32_t end_bit,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  M355_REQUIRE(keys && out && workspace, M355_EINVALID_ARG, "segmented_sort_u32: null pointer");
  if (int rc = ss_check("segmented_sort_u32", R, M)) return rc;
  M355_REQUIRE(end_bit >= 1 && end_bit <= 32, M355_EINVALID_ARG, "segmented_sort_u32: end_bit outside [1, 32]");
  M355_REQUIRE(keys != out, M355_EINVALID_ARG, "segmented_sort_u32: keys and out overlap");
  M355_REQUIRE(workspace_bytes >= segmented_sort_bytes(R, M), M355_EWORKSPACE, "segmented_sort_u32: workspace too small");
  segmented_sort_launch(keys, out, R, M, end_bit, workspace, (hipStream_t)stream);
  return check_launch("segmented_sort_u32");
}
