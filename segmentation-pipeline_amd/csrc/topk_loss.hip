// Top-k cross-entropy + Dice criterion (criterions/hybrid_topk_dice_loss.py): the log term averages only the
// k largest per-voxel cross-entropies of the whole batch; the k-th largest is found by the radix select of
// radix_select.hpp (keys, digits, histograms and the descending block pick are there), not a sort.
//
//   e[n, s] = -sum_c w_c t[n,c,s] lp[n,c,s]      PROB    lp = log((x + eps) / (1 + eps)), p = x
//                                                LOGITS  lp = log_softmax(x) over C, p = exp(lp) formed in registers
//   tau = the k-th largest e of the N*S voxels,  n_gt = #{e > tau},  n_eq = #{e == tau}
//   logistic_loss = (sum_{e > tau} e + (k - n_gt) tau) / (C k);   dice_loss: the hybrid loss's, on p
//
// Forward, four launches after one memset of the histograms:
//   tk_fwd_*        voxel-major (focal_tversky_loss.hip's layout): reads x and t once, writes e, the per-(n, c) Dice partial
//                   sums of its chunk and the histogram of the first 11-bit digit of key(e)
//   tk_select<1>    over e: the histogram of the second digit among the keys whose first digit is the k-th largest's
//   tk_select<2>    over e: the histogram of the last 10 bits among the keys whose first 22 are the k-th largest's, and
//                   the sum of every e whose first 22 bits are above them (fp64 partials per chunk)
//   tk_finalize     one block: tau, n_gt, n_eq; the keys that share tau's first 22 bits and lie above it are added from the
//                   last histogram (a key is its value: count * value is their exact sum), so e is read three times
// The pick between two passes is the prologue of the later one: every block repeats it on the finished histograms (a few
// thousand words out of L2), which saves three one-wave launches.  k is a kernel argument or, with k_device, a device
// int64 scalar clamped to [1, N*S]; only the picks and the backward depend on it.
//
// Sums: fp32 per lane in a fixed order, then fp64 across the block and across the chunks in a fixed order; no float atomics.
// Loads and stores go through row_load / row_store, so a misaligned view gives the bits of its aligned clone.
#include "loss_common.hpp"
#include "radix_select.hpp"

#include <cmath>

namespace m355 {

constexpr int TK_CHUNK = 4096;    // voxels per block of the first pass and of the backward, every channel of them
constexpr int TK_CREG = 16;       // most channels whose per-voxel values are held in registers
constexpr int TK_IT = TK_CHUNK / 1024;   // groups of 4 voxels per lane in the kernels that walk the planes
constexpr int TK_ECHUNK = 4096;   // elements of e per block of the two select passes (8192 measured 4 us slower at 1 x 4 x 128^3)
constexpr int TK_K = 3;           // Dice sums per row

// f2key after the two cases a loss has to pin down: every NaN is the largest key, whatever its sign bit, so a NaN is
// selected first as torch.topk does; -0 is +0 (bits2key is f2key on the float's bits, which these cases edit)
__device__ __forceinline__ uint32_t tk_key(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  if (u == 0x80000000u) u = 0u;
  return bits2key(u);
}

// k of this call: the host's, or the device scalar's clamped to [1, M] (whatever it holds, the picks stay inside the
// histograms)
__device__ __forceinline__ int64_t tk_k(const int64_t* __restrict__ k_device, int64_t k_host, int64_t M) {
  const int64_t k = k_device ? k_device[0] : k_host;
  return k < 1 ? 1 : k > M ? M : k;
}

// the first `passes` digits of the k-th largest key from the finished histograms hist[0 .. passes)
__device__ __forceinline__ RadixSel tk_select(const uint32_t* __restrict__ hist, int passes, int64_t k, uint32_t* sh) {
  constexpr RadixDigit D0 = radix_digit(0), D1 = radix_digit(1), D2 = radix_digit(2);
  RadixSel s;
  s.prefix = 0u;
  s.rank = (uint32_t)k;
  s.n_eq = 0u;
  s.n_gt = 0;
  if (passes >= 1) radix_pick_block<D0.bins>(hist, D0.shift, s, sh);
  if (passes >= 2) radix_pick_block<D1.bins>(hist + RADIX_BINS, D1.shift, s, sh);
  if (passes >= 3) radix_pick_block<D2.bins>(hist + 2 * RADIX_BINS, D2.shift, s, sh);
  return s;
}

// ------------------------------------------------------------------------------------------------- forward, pass 1
// Channels in registers: C <= CR.  A block takes TK_CHUNK voxels of one n: C x 3 Dice partials, TK_CHUNK values of e.
template <int CR, int VPL, bool LOGITS>
__global__ __launch_bounds__(256) void tk_fwd_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                     const float* __restrict__ class_w, float* __restrict__ e,
                                                     double* __restrict__ partial, uint32_t* __restrict__ hist, int C,
                                                     int64_t S, int nblk, int square_dice) {
  __shared__ double red[4][CR * TK_K];
  __shared__ uint32_t lh[RADIX_BINS];
  __shared__ float cw[CR];
  radix_hist_clear<256>(lh, RADIX_BINS);
  if ((int)threadIdx.x < CR) cw[threadIdx.x] = (class_w && (int)threadIdx.x < C) ? class_w[threadIdx.x] : 1.f;
  __syncthreads();
  const int b = blockIdx.x;
  const int64_t n = blockIdx.y;
  const float* xn = x + n * C * S;
  const float* tn = t + n * C * S;
  float* en = e + n * S;
  const int64_t begin = (int64_t)b * TK_CHUNK, end = min(S, begin + TK_CHUNK);
  float acc[CR][TK_K];
#pragma unroll
  for (int c = 0; c < CR; ++c)
#pragma unroll
    for (int k = 0; k < TK_K; ++k) acc[c][k] = 0.f;
  for (int64_t v0 = begin + threadIdx.x * VPL; v0 < end; v0 += 256 * VPL) {
    const int nv = row_valid(v0, end, VPL);
    float d[CR][VPL], ex[LOGITS ? CR : 1][VPL], m[VPL], s[VPL], ev[VPL];
#pragma unroll
    for (int c = 0; c < CR; ++c)
      if (c < C) row_load<VPL>(xn + c * S + v0, nv, d[c]);
    if constexpr (LOGITS) {
#pragma unroll
      for (int j = 0; j < VPL; ++j) {
        m[j] = d[0][j];
        s[j] = 0.f;
      }
#pragma unroll
      for (int c = 1; c < CR; ++c)
        if (c < C)
#pragma unroll
          for (int j = 0; j < VPL; ++j) m[j] = fmaxf(m[j], d[c][j]);
#pragma unroll
      for (int c = 0; c < CR; ++c)
        if (c < C)
#pragma unroll
          for (int j = 0; j < VPL; ++j) {
            d[c][j] -= m[j];
            ex[c][j] = expf(d[c][j]);
            s[j] += ex[c][j];
          }
#pragma unroll
      for (int j = 0; j < VPL; ++j) {
        m[j] = logf(s[j]);      // from here on m is log s
        s[j] = 1.f / s[j];      // and s its reciprocal
      }
    }
#pragma unroll
    for (int j = 0; j < VPL; ++j) ev[j] = 0.f;
#pragma unroll
    for (int c = 0; c < CR; ++c)
      if (c < C) {
        float tt[VPL];
        row_load<VPL>(tn + c * S + v0, nv, tt);
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
          if (j >= nv) break;
          float p, lp;
          if constexpr (LOGITS) {
            lp = d[c][j] - m[j];
            p = ex[c][j] * s[j];
          } else {
            p = d[c][j];
            lp = safe_log_prob(p);
          }
          dice_accumulate(p, tt[j], square_dice, acc[c][0], acc[c][1], acc[c][2]);
          ev[j] = fmaf(-(cw[c] * tt[j]), lp, ev[j]);
        }
      }
    row_store<VPL>(en + v0, nv, ev);
#pragma unroll
    for (int j = 0; j < VPL; ++j)
      if (j < nv) atomicAdd(&lh[radix_digit_of(tk_key(ev[j]), radix_digit(0))], 1u);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < CR; ++c)
    if (c < C)
#pragma unroll
      for (int k = 0; k < TK_K; ++k) {
        const double r = wave_sum((double)acc[c][k]);
        if (lane == 0) red[w][c * TK_K + k] = r;
      }
  __syncthreads();
  if ((int)threadIdx.x < C * TK_K) {
    const int c = threadIdx.x / TK_K, k = threadIdx.x % TK_K;
    const double r = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    partial[((n * C + c) * nblk + b) * TK_K + k] = r;
  }
  radix_hist_flush<256>(lh, hist, RADIX_BINS);
}

// C > TK_CREG: the max and the log-sum of every voxel of the chunk first (LOGITS: two reads of the planes, which are in
// L2), then plane by plane; e is summed over the planes in registers
template <bool LOGITS>
__global__ __launch_bounds__(256) void tk_fwd_reread_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                            const float* __restrict__ class_w, float* __restrict__ e,
                                                            double* __restrict__ partial, uint32_t* __restrict__ hist,
                                                            int C, int64_t S, int nblk, int square_dice) {
  __shared__ double scratch[4];
  __shared__ uint32_t lh[RADIX_BINS];
  radix_hist_clear<256>(lh, RADIX_BINS);
  const int b = blockIdx.x;
  const int64_t n = blockIdx.y;
  const float* xn = x + n * C * S;
  const float* tn = t + n * C * S;
  float* en = e + n * S;
  const int64_t begin = (int64_t)b * TK_CHUNK, end = min(S, begin + TK_CHUNK);
  float m[TK_IT][4], ls[TK_IT][4], inv[TK_IT][4], ev[TK_IT][4];
  int nv[TK_IT];
#pragma unroll
  for (int it = 0; it < TK_IT; ++it) {
    const int64_t v0 = begin + (it * 256 + threadIdx.x) * 4;
    nv[it] = row_valid(v0, end, 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) ev[it][j] = 0.f;
    if constexpr (LOGITS) {
      float v[4];
      row_load<4>(xn + v0, nv[it], m[it]);
      for (int c = 1; c < C; ++c) {
        row_load<4>(xn + c * S + v0, nv[it], v);
#pragma unroll
        for (int j = 0; j < 4; ++j) m[it][j] = fmaxf(m[it][j], v[j]);
      }
      float s[4] = {0.f, 0.f, 0.f, 0.f};
      for (int c = 0; c < C; ++c) {
        row_load<4>(xn + c * S + v0, nv[it], v);
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] += expf(v[j] - m[it][j]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ls[it][j] = logf(s[j]);
        inv[it][j] = 1.f / s[j];
      }
    }
  }
  for (int c = 0; c < C; ++c) {
    const float wc = class_w ? class_w[c] : 1.f;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int it = 0; it < TK_IT; ++it) {
      const int64_t v0 = begin + (it * 256 + threadIdx.x) * 4;
      float xx[4], tt[4];
      row_load<4>(xn + c * S + v0, nv[it], xx);
      row_load<4>(tn + c * S + v0, nv[it], tt);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j >= nv[it]) break;
        float p, lp;
        if constexpr (LOGITS) {
          const float dd = xx[j] - m[it][j];
          lp = dd - ls[it][j];
          p = expf(dd) * inv[it][j];
        } else {
          p = xx[j];
          lp = safe_log_prob(p);
        }
        dice_accumulate(p, tt[j], square_dice, s0, s1, s2);
        ev[it][j] = fmaf(-(wc * tt[j]), lp, ev[it][j]);
      }
    }
    const float s[TK_K] = {s0, s1, s2};
    store_block_sums(s, partial, (n * C + c) * nblk + b, scratch);
  }
#pragma unroll
  for (int it = 0; it < TK_IT; ++it) {
    const int64_t v0 = begin + (it * 256 + threadIdx.x) * 4;
    row_store<4>(en + v0, nv[it], ev[it]);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nv[it]) atomicAdd(&lh[radix_digit_of(tk_key(ev[it][j]), radix_digit(0))], 1u);
  }
  __syncthreads();
  radix_hist_flush<256>(lh, hist, RADIX_BINS);
}

// --------------------------------------------------------------------------------------------------- select passes
// PASS 1: digit 1 of the keys whose digit 0 is the k-th largest's.  PASS 2: the last 10 bits of the keys whose first 22
// are the k-th largest's, and esum[block] = the sum of the e whose first 22 bits are above them.
template <int PASS>
__global__ __launch_bounds__(256) void tk_select_kernel(const float* __restrict__ e, int64_t M,
                                                        const int64_t* __restrict__ k_device, int64_t k_host,
                                                        uint32_t* __restrict__ hist, double* __restrict__ esum) {
  __shared__ uint32_t lh[RADIX_BINS];
  __shared__ uint32_t sh[8];
  __shared__ double scratch[4];
  radix_hist_clear<256>(lh, RADIX_BINS);
  const RadixSel sel = tk_select(hist, PASS, tk_k(k_device, k_host, M), sh);   // (its barriers publish the cleared bins)
  constexpr RadixDigit DG = radix_digit(PASS);
  const uint32_t pre = sel.prefix >> DG.upper;
  const int64_t begin = (int64_t)blockIdx.x * TK_ECHUNK, end = min(M, begin + TK_ECHUNK);
  float above = 0.f;
  for (int64_t v0 = begin + threadIdx.x * 4; v0 < end; v0 += 1024) {
    const int nv = row_valid(v0, end, 4);
    float v[4];
    row_load<4>(e + v0, nv, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= nv) break;
      const uint32_t key = tk_key(v[j]), hi = key >> DG.upper;
      if (hi == pre) atomicAdd(&lh[radix_digit_of(key, DG)], 1u);
      else if (PASS == 2 && hi > pre) above += v[j];
    }
  }
  if (PASS == 2) {
    const float s[1] = {above};
    store_block_sums(s, esum, blockIdx.x, scratch);
  }
  __syncthreads();
  radix_hist_flush<256>(lh, hist + PASS * RADIX_BINS, RADIX_BINS);
}

// --------------------------------------------------------------------------------------------------------- finalize
// single block.  The Dice rows as in ft_finalize_kernel: `lanes` (a power of two <= 64) threads share the chunks of one
// row.  state = {tau, r = (k - n_gt) / n_eq, k as two 32-bit words}.
__global__ __launch_bounds__(256) void tk_finalize_kernel(const double* __restrict__ partial, const double* __restrict__ esum,
                                                          const uint32_t* __restrict__ hist,
                                                          const int64_t* __restrict__ k_device, int64_t k_host,
                                                          float* __restrict__ sums, uint32_t* __restrict__ state,
                                                          float* __restrict__ out3, int N, int C, int64_t S, int nblk,
                                                          int lanes, int64_t nsb, float dice_weight) {
  __shared__ double scratch[4];
  __shared__ uint32_t sh[8];
  const int NC = N * C;
  const int64_t k = tk_k(k_device, k_host, (int64_t)N * S);
  const RadixSel sel = tk_select(hist, 3, k, sh);
  const int per = 256 / lanes, sub = threadIdx.x % lanes, slot = threadIdx.x / lanes;
  double dice_acc = 0.0;
  for (int nc0 = 0; nc0 < NC; nc0 += per) {
    const int nc = nc0 + slot;
    double v[TK_K] = {0, 0, 0};
    if (nc < NC)
      for (int b = sub; b < nblk; b += lanes)
        for (int q = 0; q < TK_K; ++q) v[q] += partial[((int64_t)nc * nblk + b) * TK_K + q];
    for (int off = lanes >> 1; off > 0; off >>= 1)
      for (int q = 0; q < TK_K; ++q) v[q] += __shfl_xor(v[q], off, 64);
    if (nc < NC && sub == 0) {
      for (int q = 0; q < TK_K; ++q) sums[nc * TK_K + q] = (float)v[q];
      dice_acc += (double)dice_term(v[0], v[1], v[2]);
    }
  }
  // everything above tau: the chunks' sums in index order per thread, then the keys of tau's last histogram above it
  double top_acc = 0.0;
  for (int64_t i = threadIdx.x; i < nsb; i += 256) top_acc += esum[i];
  constexpr RadixDigit LAST = radix_digit(2);
  const uint32_t digit = sel.prefix & LAST.mask;
  for (uint32_t i = threadIdx.x; i < (uint32_t)LAST.bins; i += 256u)
    if (i > digit) {
      const uint32_t c = hist[2 * RADIX_BINS + i];
      if (c) top_acc += (double)c * (double)key2f((sel.prefix & ~LAST.mask) | i);
    }
  const double dice = block_sum<double, 256>(dice_acc, scratch);
  const double top = block_sum<double, 256>(top_acc, scratch);
  if (threadIdx.x == 0) {
    const float tau = key2f(sel.prefix);
    const double share = (double)((uint64_t)k - sel.n_gt);   // >= 1: the k-th largest itself is not above tau
    const double total = top + share * (double)tau;
    write_out3(out3, dice_weight, (float)(dice / NC), (float)(total / ((double)C * (double)k)));
    state[0] = __float_as_uint(tau);
    state[1] = __float_as_uint((float)(share / (double)sel.n_eq));
    state[2] = (uint32_t)((uint64_t)k & 0xffffffffu);
    state[3] = (uint32_t)((uint64_t)k >> 32);
  }
}

// --------------------------------------------------------------------------------------------------------- backward
// what the backward takes from the saved state: tau as a key, r, and dloss (1 - dice_weight) / (C k)
struct TkBwd {
  uint32_t ktau;
  float r, scale;
};
__device__ __forceinline__ TkBwd tk_bwd_state(const uint32_t* __restrict__ state, float g, float dice_weight, int C) {
  TkBwd s;
  s.ktau = tk_key(__uint_as_float(state[0]));
  s.r = __uint_as_float(state[1]);
  const double k = (double)(((uint64_t)state[3] << 32) | state[2]);
  s.scale = (float)((double)g * (double)(1.f - dice_weight) / ((double)C * k));
  return s;
}
// dloss (1 - dice_weight) sel / (C k) of a voxel: sel = 1 above tau, r on it, 0 below
__device__ __forceinline__ float tk_voxel_scale(float ev, const TkBwd& s) {
  const uint32_t key = tk_key(ev);
  return key > s.ktau ? s.scale : key == s.ktau ? s.scale * s.r : 0.f;
}
// the Dice gradient with respect to p of one element
__device__ __forceinline__ float tk_dice_grad(const DiceBwd& k, float p, float tv, int square_dice) {
  return fmaf(k.kd1, tv, k.kd2 * (square_dice ? 2.f * p : 1.f));
}

// C <= CR.  PROB: dx_c = h_c - kl w_c t_c / (x_c + eps).  LOGITS: dz_c = p_c (h_c - sum_j p_j h_j + kl sum_j w_j t_j)
// - kl w_c t_c, h the Dice gradient with respect to p and kl the voxel's scale.
template <int CR, int VPL, bool LOGITS>
__global__ __launch_bounds__(256) void tk_bwd_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                     const float* __restrict__ e, const float* __restrict__ sums,
                                                     const uint32_t* __restrict__ state, const float* __restrict__ dloss,
                                                     const float* __restrict__ class_w, float* __restrict__ dx, int N, int C,
                                                     int64_t S, float dice_weight, int square_dice) {
  __shared__ DiceBwd coef[CR];
  __shared__ float cw[CR];
  const int64_t n = blockIdx.y;
  const float g = dloss[0];
  if ((int)threadIdx.x < C) {
    coef[threadIdx.x] = dice_bwd_coeffs(sums + (n * C + threadIdx.x) * TK_K, dice_weight, 1.f / (float)(N * C), g);
    cw[threadIdx.x] = class_w ? class_w[threadIdx.x] : 1.f;
  }
  __syncthreads();
  const TkBwd st = tk_bwd_state(state, g, dice_weight, C);
  const float* xn = x + n * C * S;
  const float* tn = t + n * C * S;
  const float* en = e + n * S;
  float* on = dx + n * C * S;
  const int64_t begin = (int64_t)blockIdx.x * TK_CHUNK, end = min(S, begin + TK_CHUNK);
  for (int64_t v0 = begin + threadIdx.x * VPL; v0 < end; v0 += 256 * VPL) {
    const int nv = row_valid(v0, end, VPL);
    float ev[VPL], kl[VPL];
    row_load<VPL>(en + v0, nv, ev);
#pragma unroll
    for (int j = 0; j < VPL; ++j) kl[j] = tk_voxel_scale(ev[j], st);
    if constexpr (!LOGITS) {
#pragma unroll
      for (int c = 0; c < CR; ++c)
        if (c < C) {
          float xx[VPL], tt[VPL], o[VPL];
          row_load<VPL>(xn + c * S + v0, nv, xx);
          row_load<VPL>(tn + c * S + v0, nv, tt);
          const DiceBwd k = coef[c];
#pragma unroll
          for (int j = 0; j < VPL; ++j)
            o[j] = tk_dice_grad(k, xx[j], tt[j], square_dice) - kl[j] * (cw[c] * tt[j]) / (xx[j] + 1e-8f);
          row_store<VPL>(on + c * S + v0, nv, o);
        }
    } else {
      float d[CR][VPL], tt[CR][VPL], m[VPL], s[VPL], sum_ph[VPL], sum_wt[VPL];
#pragma unroll
      for (int c = 0; c < CR; ++c)
        if (c < C) {
          row_load<VPL>(xn + c * S + v0, nv, d[c]);
          row_load<VPL>(tn + c * S + v0, nv, tt[c]);
        }
#pragma unroll
      for (int j = 0; j < VPL; ++j) {
        m[j] = d[0][j];
        s[j] = 0.f;
        sum_ph[j] = 0.f;
        sum_wt[j] = 0.f;
      }
#pragma unroll
      for (int c = 1; c < CR; ++c)
        if (c < C)
#pragma unroll
          for (int j = 0; j < VPL; ++j) m[j] = fmaxf(m[j], d[c][j]);
#pragma unroll
      for (int c = 0; c < CR; ++c)
        if (c < C)
#pragma unroll
          for (int j = 0; j < VPL; ++j) {
            d[c][j] = expf(d[c][j] - m[j]);
            s[j] += d[c][j];
          }
#pragma unroll
      for (int j = 0; j < VPL; ++j) s[j] = 1.f / s[j];
#pragma unroll
      for (int c = 0; c < CR; ++c)
        if (c < C) {
          const DiceBwd k = coef[c];
#pragma unroll
          for (int j = 0; j < VPL; ++j) {
            d[c][j] *= s[j];   // p
            sum_ph[j] = fmaf(d[c][j], tk_dice_grad(k, d[c][j], tt[c][j], square_dice), sum_ph[j]);
            sum_wt[j] = fmaf(cw[c], tt[c][j], sum_wt[j]);
          }
        }
#pragma unroll
      for (int c = 0; c < CR; ++c)
        if (c < C) {
          const DiceBwd k = coef[c];
          float o[VPL];
#pragma unroll
          for (int j = 0; j < VPL; ++j) {
            const float h = tk_dice_grad(k, d[c][j], tt[c][j], square_dice);
            o[j] = fmaf(d[c][j], fmaf(kl[j], sum_wt[j], h - sum_ph[j]), -kl[j] * (cw[c] * tt[c][j]));
          }
          row_store<VPL>(on + c * S + v0, nv, o);
        }
    }
  }
}

// C > TK_CREG, plane by plane.  LOGITS: the planes are read three times more (max, sum of exp, the two sums over c)
// before the pass that writes.
template <bool LOGITS>
__global__ __launch_bounds__(256) void tk_bwd_reread_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                            const float* __restrict__ e, const float* __restrict__ sums,
                                                            const uint32_t* __restrict__ state,
                                                            const float* __restrict__ dloss,
                                                            const float* __restrict__ class_w, float* __restrict__ dx, int N,
                                                            int C, int64_t S, float dice_weight, int square_dice) {
  const int64_t n = blockIdx.y;
  const float g = dloss[0], inv_nc = 1.f / (float)(N * C);
  const TkBwd st = tk_bwd_state(state, g, dice_weight, C);
  const float* xn = x + n * C * S;
  const float* tn = t + n * C * S;
  const float* en = e + n * S;
  float* on = dx + n * C * S;
  const int64_t begin = (int64_t)blockIdx.x * TK_CHUNK, end = min(S, begin + TK_CHUNK);
  float m[TK_IT][4], inv[TK_IT][4], kl[TK_IT][4], sum_ph[TK_IT][4], sum_wt[TK_IT][4];
  int nv[TK_IT];
#pragma unroll
  for (int it = 0; it < TK_IT; ++it) {
    const int64_t v0 = begin + (it * 256 + threadIdx.x) * 4;
    nv[it] = row_valid(v0, end, 4);
    float v[4];
    row_load<4>(en + v0, nv[it], v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      kl[it][j] = tk_voxel_scale(v[j], st);
      sum_ph[it][j] = 0.f;
      sum_wt[it][j] = 0.f;
    }
    if constexpr (LOGITS) {
      row_load<4>(xn + v0, nv[it], m[it]);
      for (int c = 1; c < C; ++c) {
        row_load<4>(xn + c * S + v0, nv[it], v);
#pragma unroll
        for (int j = 0; j < 4; ++j) m[it][j] = fmaxf(m[it][j], v[j]);
      }
      float s[4] = {0.f, 0.f, 0.f, 0.f};
      for (int c = 0; c < C; ++c) {
        row_load<4>(xn + c * S + v0, nv[it], v);
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] += expf(v[j] - m[it][j]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) inv[it][j] = 1.f / s[j];
    }
  }
  for (int pass = LOGITS ? 0 : 1; pass < 2; ++pass)
    for (int c = 0; c < C; ++c) {
      const DiceBwd k = dice_bwd_coeffs(sums + (n * C + c) * TK_K, dice_weight, inv_nc, g);
      const float wc = class_w ? class_w[c] : 1.f;
#pragma unroll
      for (int it = 0; it < TK_IT; ++it) {
        const int64_t v0 = begin + (it * 256 + threadIdx.x) * 4;
        float xx[4], tt[4], o[4];
        row_load<4>(xn + c * S + v0, nv[it], xx);
        row_load<4>(tn + c * S + v0, nv[it], tt);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if constexpr (LOGITS) {
            const float p = expf(xx[j] - m[it][j]) * inv[it][j];
            const float h = tk_dice_grad(k, p, tt[j], square_dice);
            if (pass == 0) {
              sum_ph[it][j] = fmaf(p, h, sum_ph[it][j]);
              sum_wt[it][j] = fmaf(wc, tt[j], sum_wt[it][j]);
            }
            o[j] = fmaf(p, fmaf(kl[it][j], sum_wt[it][j], h - sum_ph[it][j]), -kl[it][j] * (wc * tt[j]));
          } else {
            o[j] = tk_dice_grad(k, xx[j], tt[j], square_dice) - kl[it][j] * (wc * tt[j]) / (xx[j] + 1e-8f);
          }
        }
        if (pass == 1) row_store<4>(on + c * S + v0, nv[it], o);
      }
    }
}

// ------------------------------------------------------------------------------------------------------------- host
struct TkLayout {
  int nblk;          // chunks of a row in pass 1
  int64_t nsb;       // chunks of e in the select passes
  size_t esum, hist, bytes;   // byte offsets of the two regions after the Dice partials; the whole
};
static inline TkLayout tk_layout(int32_t N, int32_t C, int64_t S) {
  TkLayout l;
  l.nblk = (int)ceil_div(S, TK_CHUNK);
  l.nsb = ceil_div((int64_t)N * S, TK_ECHUNK);
  l.esum = (size_t)N * C * l.nblk * TK_K * sizeof(double);
  l.hist = l.esum + (size_t)l.nsb * sizeof(double);
  l.bytes = l.hist + 3 * RADIX_BINS * sizeof(uint32_t) + 256;
  return l;
}

// the sizes: loss_check's, and N*S within the 32-bit counts of the histograms
static int tk_check(const char* what, int32_t N, int32_t C, int64_t S) {
  if (int rc = loss_check(what, N, C, S)) return rc;
  M355_REQUIRE(S <= (int64_t)0xffffffffll / N, M355_EUNSUPPORTED, "%s: N*S > 2^32 - 1", what);
  return M355_OK;
}

using TkFwdK = void (*)(const float*, const float*, const float*, float*, double*, uint32_t*, int, int64_t, int, int);
using TkBwdK = void (*)(const float*, const float*, const float*, const float*, const uint32_t*, const float*, const float*,
                        float*, int, int, int64_t, float, int);

template <bool LOGITS>
static TkFwdK tk_fwd_for(int C) {
  return C <= 4 ? tk_fwd_kernel<4, 4, LOGITS> : C <= 8 ? tk_fwd_kernel<8, 4, LOGITS>
         : C <= TK_CREG ? tk_fwd_kernel<16, 2, LOGITS> : tk_fwd_reread_kernel<LOGITS>;
}
template <bool LOGITS>
static TkBwdK tk_bwd_for(int C) {
  return C <= 4 ? tk_bwd_kernel<4, 4, LOGITS> : C <= 8 ? tk_bwd_kernel<8, 4, LOGITS>
         : C <= TK_CREG ? tk_bwd_kernel<16, 2, LOGITS> : tk_bwd_reread_kernel<LOGITS>;
}

}  // namespace m355

using namespace m355;

extern "C" size_t m355_topk_loss_workspace(int32_t N, int32_t C, int64_t S) {
  if (N <= 0 || C <= 0 || S <= 0) return 0;
  return tk_layout(N, C, S).bytes;
}

extern "C" int m355_topk_loss_fwd(const float* x, const float* t, int32_t N, int32_t C, int64_t S, int64_t k,
                                  const int64_t* k_device, float dice_weight, const float* class_weights,
                                  int32_t square_dice, int32_t from_logits, float* out3, float* sums, float* e, void* state,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  M355_REQUIRE(x && t && out3 && sums && e && state && workspace, M355_EINVALID_ARG, "topk_loss_fwd: null pointer");
  if (int rc = tk_check("topk_loss_fwd", N, C, S)) return rc;
  const int64_t M = (int64_t)N * S;
  M355_REQUIRE(k_device || (k >= 1 && k <= M), M355_EINVALID_ARG, "topk_loss_fwd: k outside [1, N*S]");
  const TkLayout l = tk_layout(N, C, S);
  M355_REQUIRE(workspace_bytes >= l.bytes, M355_EWORKSPACE, "topk_loss_fwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)workspace;
  double* esum = (double*)((char*)workspace + l.esum);
  uint32_t* hist = (uint32_t*)((char*)workspace + l.hist);
  if (hipMemsetAsync(hist, 0, 3 * RADIX_BINS * sizeof(uint32_t), st) != hipSuccess) return check_launch("topk_loss_fwd: memset");
  const TkFwdK k1 = from_logits ? tk_fwd_for<true>(C) : tk_fwd_for<false>(C);
  hipLaunchKernelGGL(k1, dim3((unsigned)l.nblk, (unsigned)N), dim3(256), 0, st, x, t, class_weights, e, partial, hist, (int)C,
                     S, l.nblk, (int)square_dice);
  hipLaunchKernelGGL(tk_select_kernel<1>, dim3((unsigned)l.nsb), dim3(256), 0, st, e, M, k_device, k, hist, esum);
  hipLaunchKernelGGL(tk_select_kernel<2>, dim3((unsigned)l.nsb), dim3(256), 0, st, e, M, k_device, k, hist, esum);
  int lanes = 1;
  while (lanes < 64 && lanes < l.nblk) lanes *= 2;
  hipLaunchKernelGGL(tk_finalize_kernel, dim3(1), dim3(256), 0, st, partial, esum, hist, k_device, k, sums, (uint32_t*)state,
                     out3, (int)N, (int)C, S, l.nblk, lanes, l.nsb, dice_weight);
  return check_launch("topk_loss_fwd");
}

extern "C" int m355_topk_loss_bwd(const float* x, const float* t, const float* e, const float* sums, const void* state,
                                  const float* dloss, int32_t N, int32_t C, int64_t S, float dice_weight,
                                  const float* class_weights, int32_t square_dice, int32_t from_logits, float* dx,
                                  void* stream) {
  M355_REQUIRE(x && t && e && sums && state && dloss && dx, M355_EINVALID_ARG, "topk_loss_bwd: null pointer");
  if (int rc = tk_check("topk_loss_bwd", N, C, S)) return rc;
  const TkBwdK k = from_logits ? tk_bwd_for<true>(C) : tk_bwd_for<false>(C);
  hipLaunchKernelGGL(k, dim3((unsigned)ceil_div(S, TK_CHUNK), (unsigned)N), dim3(256), 0, (hipStream_t)stream, x, t, e, sums,
                     (const uint32_t*)state, dloss, class_weights, dx, (int)N, (int)C, S, dice_weight, (int)square_dice);
  return check_launch("topk_loss_bwd");
}
