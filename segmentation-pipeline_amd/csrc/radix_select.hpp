// Exact order statistics of floats without a sort: the one radix select behind m355_aug_order_stats,
// m355_region_stats (median) and m355_topk_loss_fwd (k-th largest).
//
//   keys        uint32 that order like the floats (f2key)
//   digits      three passes from the top, 11 / 11 / 10 bits (radix_digit); a pass counts the digit of every key whose
//               higher digits equal the prefix found so far
//   histograms  RADIX_BINS counters per query, privatised in LDS with integer atomics and flushed with one global
//               atomic per non-zero bin: integer adds commute, so the counts do not depend on the order
//   pick        between two passes: the bin that holds the rank still to find extends the prefix, the keys in the bins
//               before it come off the rank.  radix_pick_wave: one wave, ascending, 0-based.  radix_pick_block: 256
//               threads, descending, 1-based, and it counts the keys above and in the bin it picks.
// Everything here is inlined into the caller's kernel; which block, wave or launch serves which query is the caller's.
#pragma once
#include "common.hpp"

namespace m355 {

constexpr int RADIX_BINS = 2048;   // bins of one histogram (the last pass uses 1024 of them)

// -nan < -inf < ... < -0 < +0 < ... < +inf < +nan
__device__ __forceinline__ uint32_t bits2key(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ uint32_t f2key(float f) { return bits2key(__float_as_uint(f)); }
__device__ __forceinline__ float key2f(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
constexpr uint32_t KEY_PINF = 0xff800000u;   // f2key(+inf): every larger key is a NaN
constexpr uint32_t KEY_NINF = 0x007fffffu;   // f2key(-inf): every smaller key is a NaN

// digit `pass` of a key is (key >> shift) & mask, one of `bins` values; the digits already fixed are key >> upper
// (pass 0: upper = 32, there are none)
struct RadixDigit {
  int shift, upper, bins;
  uint32_t mask;
};
__host__ __device__ constexpr RadixDigit radix_digit(int pass) {
  const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
  return RadixDigit{shift, shift + (pass == 2 ? 10 : 11), pass == 2 ? 1024 : 2048, pass == 2 ? 1023u : 2047u};
}
__device__ __forceinline__ uint32_t radix_digit_of(uint32_t key, RadixDigit d) { return (key >> d.shift) & d.mask; }

// The histograms of a block of NT threads, `bins` counters in all: the clear (of the LDS copy before a pass, of the global
// one after a pick) and the flush of the LDS copy.  The caller places the barriers: one after the clear, one between the
// block's last LDS atomic and the flush.
template <int NT>
__device__ __forceinline__ void radix_hist_clear(uint32_t* lh, int bins) {
  for (int i = threadIdx.x; i < bins; i += NT) lh[i] = 0u;
}
template <int NT>
__device__ __forceinline__ void radix_hist_flush(const uint32_t* lh, uint32_t* __restrict__ hist, int bins) {
  for (int i = threadIdx.x; i < bins; i += NT) {
    const uint32_t c = lh[i];
    if (c) atomicAdd(&hist[i], c);
  }
}

// One digit by one wave: lane i owns the bins [32 i, 32 i + 32) of h, rank k is 0-based from the smallest key.  True in
// the one lane whose bins hold rank k, and there `digit` is the bin and `rest` the rank inside it; false in every lane
// when the histogram holds k keys or fewer.
__device__ __forceinline__ bool radix_pick_wave(const uint32_t* h, uint32_t k, uint32_t& digit, uint32_t& rest) {
  const int lane = threadIdx.x & 63;
  uint32_t part = 0;
  for (int i = 0; i < 32; ++i) part += h[lane * 32 + i];
  const uint32_t incl = wave_incl_scan(part), excl = incl - part;
  const bool mine = k >= excl && k < incl;
  if (mine) {
    uint32_t cum = excl;
    int d = 0;
    for (; d < 32; ++d) {   // k < incl = excl + the lane's 32 counts: the break is taken at the last bin at the latest
      const uint32_t c = h[lane * 32 + d];
      if (k < cum + c) break;
      cum += c;
    }
    digit = (uint32_t)(lane * 32 + d);
    rest = k - cum;
  }
  return mine;
}

// the descending select so far: the digits found, the 1-based rank among the keys that share them, how many keys lie
// above them and how many are in the bin picked last
struct RadixSel {
  uint32_t prefix, rank, n_eq;
  uint64_t n_gt;
};

// One digit, by every thread of the block (256) with the same result: thread i owns BINS / 256 bins from the top down,
// a scan over the threads finds the one whose bins hold rank `s.rank` counted from the largest key.  sh: 8 words of LDS.
template <int BINS>
__device__ __forceinline__ void radix_pick_block(const uint32_t* __restrict__ hist, int shift, RadixSel& s, uint32_t* sh) {
  constexpr int PER = BINS / 256;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int top = BINS - 1 - (int)threadIdx.x * PER;
  uint32_t c[PER], part = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    c[i] = hist[top - i];
    part += c[i];
  }
  const uint32_t incl = wave_incl_scan(part);
  if (lane == 63) sh[w] = incl;
  if (threadIdx.x == 0) sh[4] = sh[5] = sh[6] = 0u;
  __syncthreads();
  uint32_t cum = incl - part;
  for (int i = 0; i < w; ++i) cum += sh[i];
  if (s.rank > cum && s.rank <= cum + part) {   // exactly one thread
    uint32_t digit = 0, ceq = 0;
    bool found = false;
#pragma unroll
    for (int i = 0; i < PER; ++i)
      if (!found) {
        if (s.rank <= cum + c[i]) {
          found = true;
          digit = (uint32_t)(top - i);
          ceq = c[i];
        } else {
          cum += c[i];
        }
      }
    sh[4] = digit;
    sh[5] = cum;
    sh[6] = ceq;
  }
  __syncthreads();
  s.prefix |= sh[4] << shift;
  s.n_gt += sh[5];
  s.rank -= sh[5];
  s.n_eq = sh[6];
  __syncthreads();   // sh is written again by the next pick
}

}  // namespace m355
