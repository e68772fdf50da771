// 3x3x3 / stride 1 / pad 1 convolution with 16-bit operands (M355_COMPUTE_BF16 / M355_COMPUTE_F16) on
// v_mfma_f32_32x32x16_{bf16,f16}: fp32 accumulate, 16x the fp32-MFMA rate.  Forward and data gradient
// (the latter = the same kernel on dy with flipped / transposed packed weights).
//
// Reference ops replaced: nn.Conv3d inside Block3d (models/components.py:36,42,51) and the out conv
// (models/modular_unet.py:83,99) under BASELINE cfg3 ("bf16") / cfg5 ("mixed fp16 with MFMA channel-GEMM
// path"); the reference itself has no reduced-precision path, the fp32 result is the oracle.
//
// GEMM view:  Y[o, v] = sum_{c, tap} Wp[(c, tap), o] * X[c, v + off(tap)],  M = Cout, N = voxels.
// The K-step of 16 is 16 input channels at ONE tap: lanes 0-31 carry channels c..c+7 of voxel (lane & 31),
// lanes 32-63 channels c+8..c+15.  The input arrives in the c8 layout (h16.hpp: [cb][voxel][8 channels],
// one 16-byte item per voxel and channel block), so
//   * a lane's B fragment is ONE item: global -> register -> LDS -> ds_read_b128 -> MFMA, never converted,
//     never transposed (the fp32-input version of this kernel gathered 8 channel planes with 8 scalar loads
//     and 8 conversions per item and was bound by exactly that);
//   * a tap shift is a whole-item offset in the LDS halo tile -- an immediate of the ds_read;
//   * zero padding, tile overhang and channel blocks past the tensor come from the buffer descriptor
//     (out-of-range offset -> the hardware returns 0): no masks, no branches.
// LDS:  xs[half][halo voxel]  (B fragments),  ws[tap][half][32 o]  (A fragments), 16 bytes each, one buffer;
// the next chunk (16 channels: halo tile + 27 taps x 32 output channels of weights) travels global ->
// registers while the current one is multiplied, its loads interleaved into the MFMA stream, and is
// committed to LDS between two barriers.  Two workgroups per CU cover each other's commits.
// With 32 lanes along x (GY = 1) an output row's B fragment for tap row dy is the fragment of input row
// g + dy: the NTW + 2 row fragments of a (dz, dx) pair are read once and used by all 3 * NTW MFMAs of that
// pair (0.75 LDS reads per MFMA at NTW = 4 instead of 1.25) -- LDS bandwidth is what bounds this loop.
// Persistent: one residency of workgroups takes (output tile x 32-channel tile x sample x split) items from
// per-XCD queues, prefetching the first chunk of the next item during the last chunk of the current one.
#include "conv3d_common.hpp"
#include "h16_epilogue.hpp"

namespace m355 {

// ------------------------------------------------------------------ layout conversion
// fp32 NCDHW -> c8: one thread per (voxel, channel block): 8 coalesced plane reads, one 16-byte store.
template <typename HT>
__global__ __launch_bounds__(256) void pack_act16_kernel(const float* __restrict__ x, HT* __restrict__ x16, int C,
                                                         int64_t S, int64_t xbs, int64_t x16bs) {
  using hx8 = typename H16<HT>::x8;
  const int cb = blockIdx.y, n = blockIdx.z;
  const float* xn = x + (int64_t)n * xbs + (int64_t)cb * 8 * S;
  hx8* dst = reinterpret_cast<hx8*>(x16 + (int64_t)n * x16bs) + (int64_t)cb * S;
  const int nc = min(8, C - cb * 8);
  for (int64_t s = blockIdx.x * 256ll + threadIdx.x; s < S; s += gridDim.x * 256ll) {
    hx8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (HT)(j < nc ? xn[(int64_t)j * S + s] : 0.f);
    dst[s] = v;
  }
}

template <typename HT>
__global__ __launch_bounds__(256) void unpack_act16_kernel(const HT* __restrict__ x16, float* __restrict__ x, int C,
                                                           int64_t S, int64_t x16bs, int64_t xbs) {
  using hx8 = typename H16<HT>::x8;
  const int cb = blockIdx.y, n = blockIdx.z;
  float* xn = x + (int64_t)n * xbs + (int64_t)cb * 8 * S;
  const hx8* src = reinterpret_cast<const hx8*>(x16 + (int64_t)n * x16bs) + (int64_t)cb * S;
  const int nc = min(8, C - cb * 8);
  for (int64_t s = blockIdx.x * 256ll + threadIdx.x; s < S; s += gridDim.x * 256ll) {
    const hx8 v = src[s];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < nc) xn[(int64_t)j * S + s] = (float)v[j];
  }
}

int launch_pack_act16(const float* x, void* x16, int N, int C, int64_t S, int64_t xbs, int64_t x16bs, int compute,
                      hipStream_t st) {
  dim3 grid((unsigned)std::min<int64_t>(ceil_div(S, 256 * 4), 4096), (unsigned)c8_blocks(C), (unsigned)N);
  if (compute == M355_COMPUTE_BF16)
    hipLaunchKernelGGL(pack_act16_kernel<__bf16>, grid, dim3(256), 0, st, x, (__bf16*)x16, C, S, xbs, x16bs);
  else
    hipLaunchKernelGGL(pack_act16_kernel<_Float16>, grid, dim3(256), 0, st, x, (_Float16*)x16, C, S, xbs, x16bs);
  return check_launch("pack_act16");
}

int launch_unpack_act16(const void* x16, float* x, int N, int C, int64_t S, int64_t x16bs, int64_t xbs, int compute,
                        hipStream_t st) {
  dim3 grid((unsigned)std::min<int64_t>(ceil_div(S, 256 * 4), 4096), (unsigned)c8_blocks(C), (unsigned)N);
  if (compute == M355_COMPUTE_BF16)
    hipLaunchKernelGGL(unpack_act16_kernel<__bf16>, grid, dim3(256), 0, st, (const __bf16*)x16, x, C, S, x16bs, xbs);
  else
    hipLaunchKernelGGL(unpack_act16_kernel<_Float16>, grid, dim3(256), 0, st, (const _Float16*)x16, x, C, S, x16bs, xbs);
  return check_launch("unpack_act16");
}

// ------------------------------------------------------------------ weight pack
// wpb[(((ch*27 + tap)*2 + half)*mout_pad + m)*8 + j], channel = ch*16 + half*8 + j; zero rows / columns past
// the tensor.  transpose: the data-gradient filter (flipped taps, channels swapped).  Also zeroes the work
// queues of the persistent kernel (every launch of it is preceded by this pack on the same stream).
template <typename HT>
__device__ __forceinline__ void pack_w3_h16_body(const float* __restrict__ w, HT* __restrict__ wp, int Cout, int Cin,
                                                 int nchunks, int mout_pad, int transpose, int64_t bid, int64_t nblk) {
  const int64_t total = (int64_t)nchunks * 27 * 2 * mout_pad * 8;
  for (int64_t i = bid * (int64_t)blockDim.x + threadIdx.x; i < total; i += nblk * blockDim.x) {
    const int j = (int)(i & 7);
    int64_t r = i >> 3;
    const int m = (int)(r % mout_pad);
    r /= mout_pad;
    const int half = (int)(r & 1);
    r >>= 1;
    const int tap = (int)(r % 27);
    const int kc = (int)(r / 27) * 16 + half * 8 + j;
    float v = 0.f;
    if (!transpose) {
      if (kc < Cin && m < Cout) v = w[((int64_t)m * Cin + kc) * 27 + tap];
    } else {
      if (kc < Cout && m < Cin) v = w[((int64_t)kc * Cin + m) * 27 + (26 - tap)];
    }
    wp[i] = (HT)v;
  }
}

template <typename HT>
__global__ void pack_w3_h16_kernel(const float* __restrict__ w, HT* __restrict__ wp, int Cout,
                                   int Cin, int nchunks, int mout_pad, int transpose, int* __restrict__ counter) {
  if (counter && blockIdx.x == 0 && threadIdx.x < 16) counter[threadIdx.x] = 0;
  pack_w3_h16_body<HT>(w, wp, Cout, Cin, nchunks, mout_pad, transpose, blockIdx.x, gridDim.x);
}

// All stale packed weights of a model in ONE launch (m355_conv3d_pack_batch).  The single-tensor kernels above gather
// (each lane reads another row of w: ~1.3 TB/s of useful traffic); here every block moves one TILE through LDS so that
// both the reads of w and the writes of the packed form are contiguous runs:
//   fp32 forward   : a plain 2-D transpose  w[m][r] -> wp[r][m]         (r = c*27 + tap), 32 x 32 tiles
//   fp32 transposed: per K-channel kc,      w[kc][m][tap] -> wp[kc][26-tap][m], tiles of 32 m x 27 taps
//   16-bit forms   : per 16-channel chunk ch and 32 rows m, the (16 x 27)- resp. (32 x 27)-float runs of w
//                    -> wp[ch][tap][half][m][8] (one 512-byte run per (tap, half))
// Pure copies / one rounding per element, the same expressions as above: the packed bytes are identical (tested).
// Every entry owns a run of blocks (its tile count), found by a scan of the <= 64 entries in the kernel arguments.
constexpr int PACK_MT = 8;                       // rows m per tile of the 16-bit forms
constexpr int PACK_LDS_H16 = 16 * (PACK_MT * 27 + 1);   // floats (>= PACK_MT * (16 * 27 + 1)): 13.9 KB, 8+ blocks per CU
constexpr int PACK_LDS_F32 = 32 * 33;

__device__ __forceinline__ void pack_tile_f32(const PackEntry& e, int bid, float* __restrict__ t) {
  const float* __restrict__ w = e.w;
  float* __restrict__ wp = (float*)e.wp;
  const int tid = threadIdx.x;
  const int ta = (e.mout_pad + 31) >> 5;
  if (!e.transpose) {
    // src[m][r], R = Cin*27 per row; dst[r][m], rows r < kdim*27, cols m < mout_pad
    const int R = e.Cin * 27, Rp = e.kdim * 27;
    const int a0 = (bid % ta) * 32, b0 = (bid / ta) * 32;
    const int col = tid & 31, row = tid >> 5;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int a = a0 + row + 8 * p, b = b0 + col;
      t[(row + 8 * p) * 33 + col] = (a < e.Cout && b < R) ? w[(int64_t)a * R + b] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int b = b0 + row + 8 * p, a = a0 + col;
      if (b < Rp && a < e.mout_pad) wp[(int64_t)b * e.mout_pad + a] = t[col * 33 + row + 8 * p];
    }
  } else {
    // kc = z over the weight's Cout (padded to kdim), m over its Cin (padded to mout_pad):
    // src[(z*Cin + m)*27 + tap] -> dst[(z*27 + 26 - tap)*mout_pad + m]
    const int z = bid / ta, a0 = (bid % ta) * 32;
    const int na = min(32, e.Cin - a0);               // valid rows m of this tile (may be <= 0)
    const float* src = w + ((int64_t)z * e.Cin + a0) * 27;
    for (int i = tid; i < 32 * 27; i += 256) t[i] = (z < e.Cout && i < na * 27) ? src[i] : 0.f;
    __syncthreads();
    for (int i = tid; i < 27 * 32; i += 256) {
      const int tp = i >> 5, aa = i & 31;             // destination tap row, column m
      if (a0 + aa < e.mout_pad) wp[((int64_t)z * 27 + tp) * e.mout_pad + a0 + aa] = t[aa * 27 + (26 - tp)];
    }
  }
}

template <typename HT>
__device__ __forceinline__ void pack_tile_h16(const PackEntry& e, int bid, float* __restrict__ t) {
  const float* __restrict__ w = e.w;
  HT* __restrict__ wp = (HT*)e.wp;
  const int tid = threadIdx.x;
  const int ta = (e.mout_pad + PACK_MT - 1) / PACK_MT;
  const int ch = bid / ta, m0 = (bid % ta) * PACK_MT;
  constexpr int RS = 16 * 27 + 1;        // forward: t[mm][cc*27 + tap]
  constexpr int KS = PACK_MT * 27 + 1;   // transposed: t[kk][mm*27 + tap]
  if (!e.transpose) {
    // rows m (weight's Cout), K-channels c = ch*16 + half*8 + j (weight's Cin), cc = c - ch*16
    const int nc = max(0, min(16, e.Cin - ch * 16));
    for (int i = tid; i < PACK_MT * 16 * 27; i += 256) {
      const int r = i / (16 * 27), q = i - r * (16 * 27);
      const int m = m0 + r;
      t[r * RS + q] = (m < e.Cout && q < nc * 27) ? w[((int64_t)m * e.Cin + ch * 16) * 27 + q] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < 54 * PACK_MT * 8; i += 256) {   // (tap, half, mm, j): runs of PACK_MT * 8 elements
      const int j = i & 7, mm = (i >> 3) % PACK_MT, th = i / (PACK_MT * 8);
      const int tap = th >> 1, half = th & 1;
      if (m0 + mm < e.mout_pad)
        wp[((((int64_t)ch * 27 + tap) * 2 + half) * e.mout_pad + m0 + mm) * 8 + j] = (HT)t[mm * RS + (half * 8 + j) * 27 + tap];
    }
  } else {
    // K-channels kc = ch*16 + kk (weight's Cout), rows m (weight's Cin)
    const int nm = max(0, min(PACK_MT, e.Cin - m0));
    for (int i = tid; i < 16 * PACK_MT * 27; i += 256) {
      const int kk = i / (PACK_MT * 27), q = i - kk * (PACK_MT * 27);
      const int kc = ch * 16 + kk;
      t[kk * KS + q] = (kc < e.Cout && q < nm * 27) ? w[((int64_t)kc * e.Cin + m0) * 27 + q] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < 54 * PACK_MT * 8; i += 256) {
      const int j = i & 7, mm = (i >> 3) % PACK_MT, th = i / (PACK_MT * 8);
      const int tap = th >> 1, half = th & 1;
      if (m0 + mm < e.mout_pad)
        wp[((((int64_t)ch * 27 + tap) * 2 + half) * e.mout_pad + m0 + mm) * 8 + j] =
            (HT)t[(half * 8 + j) * KS + mm * 27 + (26 - tap)];
    }
  }
}

// KIND 0: fp32 entries; 1: 16-bit entries (bf16 / fp16 per entry)
template <int KIND>
__global__ __launch_bounds__(256) void pack_w3_batch_kernel(const PackBatch b) {
  __shared__ float t[KIND == 0 ? PACK_LDS_F32 : PACK_LDS_H16];
  int k = 0;
  while (k + 1 < b.n && (int)blockIdx.x >= b.e[k + 1].blk0) ++k;
  const PackEntry& e = b.e[k];
  const int bid = (int)blockIdx.x - e.blk0;
  if (bid == 0 && threadIdx.x < 16) e.counter[threadIdx.x] = 0;
  if constexpr (KIND == 0) {
    pack_tile_f32(e, bid, t);
  } else {
    if (e.kind == 1)
      pack_tile_h16<__bf16>(e, bid, t);
    else
      pack_tile_h16<_Float16>(e, bid, t);
  }
}

// entries of one launch share the kind class (fp32 / 16-bit): the caller (m355_conv3d_pack_batch) flushes on a change
void launch_pack_batch(PackBatch& b, int n, hipStream_t st) {
  int blocks = 0;
  for (int i = 0; i < n; ++i) {
    PackEntry& e = b.e[i];
    e.blk0 = blocks;
    if (e.kind == 0) {
      const int ta = (e.mout_pad + 31) / 32;
      e.nblk = e.transpose ? e.kdim * ta : (int)ceil_div((int64_t)e.kdim * 27, 32) * ta;
    } else {
      e.nblk = e.kdim * (int)ceil_div(e.mout_pad, PACK_MT);   // (chunk, PACK_MT-row tile)
    }
    blocks += e.nblk;
  }
  b.n = n;
  if (b.e[0].kind == 0)
    hipLaunchKernelGGL(pack_w3_batch_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, st, b);
  else
    hipLaunchKernelGGL(pack_w3_batch_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, b);
}

// c8 output of a split-K plan: y16[n][cb][s] = bias + sum_ks slab[ks][n][o][s] (fixed order), rounded once.
// `stat` (optional): the statistics partials of the normalisation that follows, as the conv epilogue of the
// unsplit plans emits them -- (sum, sum of squares) of the fp32 values per channel, one slot per block:
// stat[((n * gridDim.x + blockIdx.x) * Cout + c) * 2 + {0,1}].  Saves the separate pass over the c8 tensor.
template <typename HT>
__global__ __launch_bounds__(256) void splitk_reduce_c8_kernel(const float* __restrict__ slab,
                                                               const float* __restrict__ bias, HT* __restrict__ y16,
                                                               int Cout, int64_t S, int ksplit, int64_t slab_stride,
                                                               int64_t ybs16, float* __restrict__ stat,
                                                               int* __restrict__ oflag) {
  using hx8 = typename H16<HT>::x8;
  __shared__ float red[4][16];
  bool sat = false;
  const int cb = blockIdx.y, n = blockIdx.z;
  const int c0 = cb * 8, nc = min(8, Cout - c0);
  const float* sp = slab + ((int64_t)n * Cout + c0) * S;
  hx8* dst = reinterpret_cast<hx8*>(y16 + (int64_t)n * ybs16) + (int64_t)cb * S;
  float bv[8], s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    bv[j] = (bias && j < nc) ? bias[c0 + j] : 0.f;
    s1[j] = s2[j] = 0.f;
  }
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < S; i += gridDim.x * 256ll) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = j < nc ? sp[(int64_t)j * S + i] : 0.f;
    int k = 1;
    for (; k + 4 <= ksplit; k += 4) {   // four splits' loads in flight together; summed in split order all the same
      float t[4][8];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) t[u][j] = j < nc ? sp[(int64_t)(k + u) * slab_stride + (int64_t)j * S + i] : 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += t[u][j];
    }
    for (; k < ksplit; ++k) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < nc) v[j] += sp[(int64_t)k * slab_stride + (int64_t)j * S + i];
    }
    hx8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float t = j < nc ? v[j] + bv[j] : 0.f;
      o[j] = to_h16_sat<HT>(t, sat);
      s1[j] += t;
      s2[j] = fmaf(t, t, s2[j]);
    }
    dst[i] = o;
  }
  report_saturation(sat, oflag);
  if (!stat) return;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    s1[j] = wave_sum(s1[j]);
    s2[j] = wave_sum(s2[j]);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[w][j] = s1[j];
      red[w][8 + j] = s2[j];
    }
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    const int j = threadIdx.x & 7, k = threadIdx.x >> 3;
    const float t = ((red[0][k * 8 + j] + red[1][k * 8 + j]) + red[2][k * 8 + j]) + red[3][k * 8 + j];
    if (j < nc) stat[(((int64_t)n * gridDim.x + blockIdx.x) * Cout + c0 + j) * 2 + k] = t;
  }
}

// Output conv of the network (Cout <= 4) with nn.Softmax(dim=1) as its epilogue (models/modular_unet.py:83-84,99-100):
// rows 0..3 of the 32-row tile -- all channels of a voxel -- are registers 0..3 of the lower lane half, so the
// softmax is in-register arithmetic and the logits never travel to HBM (same expressions as softmax_fwd_kernel).
template <int NTW, int GY>
__device__ __forceinline__ void store_conv_tile_softmax(const f32x16 (&acc)[NTW], float* __restrict__ dst,
                                                        const float* __restrict__ bias, int Cout, int z, int y0, int xg,
                                                        int ly, int half, int D, int H, int W, bool lane_ok) {
  const int64_t HW = (int64_t)H * W, DHW = HW * D;
  float bb[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) bb[c] = (bias && c < Cout) ? bias[c] : 0.f;
#pragma unroll
  for (int g = 0; g < NTW; ++g) {
    const int yg = y0 + g * GY + ly;
    if (!(lane_ok && half == 0 && yg < H)) continue;
    float v[4], mx = -INFINITY, sum = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      v[c] = acc[g][c] + bb[c];
      if (c < Cout) mx = fmaxf(mx, v[c]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < Cout) sum += expf(v[c] - mx);
    const float inv = 1.f / sum;
    const int64_t base = (int64_t)z * HW + (int64_t)yg * W + xg;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < Cout) dst[base + (int64_t)c * DHW] = expf(v[c] - mx) * inv;
  }
}

// ... and with nn.Sigmoid (M355_CONV_SIGMOID): sigmoid_f32 of bias + accumulator per channel, the bits of m355_sigmoid_fwd.
template <int NTW, int GY>
__device__ __forceinline__ void store_conv_tile_sigmoid(const f32x16 (&acc)[NTW], float* __restrict__ dst,
                                                        const float* __restrict__ bias, int Cout, int z, int y0, int xg,
                                                        int ly, int half, int D, int H, int W, bool lane_ok) {
  const int64_t HW = (int64_t)H * W, DHW = HW * D;
  float bb[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) bb[c] = (bias && c < Cout) ? bias[c] : 0.f;
#pragma unroll
  for (int g = 0; g < NTW; ++g) {
    const int yg = y0 + g * GY + ly;
    if (!(lane_ok && half == 0 && yg < H)) continue;
    const int64_t base = (int64_t)z * HW + (int64_t)yg * W + xg;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < Cout) dst[base + (int64_t)c * DHW] = sigmoid_f32(acc[g][c] + bb[c]);
  }
}

// ------------------------------------------------------------------ the kernel
#ifdef M355_H16_STAMPS
// Diagnostic build only (tools/h16_stamps.py): per-workgroup cycle sums of the phases of a chunk, wave 0.
__device__ unsigned long long m355_h16_stamps[1024][8];
#define STAMP(var) unsigned long long var = __builtin_amdgcn_s_memtime()
#else
#define STAMP(var)
#endif
// OUT16: the output tile is written as c8 items into y16 (ybs in ELEMENTS of it); otherwise fp32 NCDHW into y.
// NW: waves per workgroup = z slices of the tile.  NW = 4: one LDS buffer (commit between two barriers), two
// workgroups per CU cover each other's commits.  NW = 8: ONE workgroup of 8 waves per CU (two waves per SIMD)
// with the tile 8 x NTW rows x 32 and DOUBLE-buffered LDS (2 x (x tile + weights) = 142 KB at NTW = 2): the next
// chunk is written into the other buffer as soon as its loads have landed, while the other waves keep issuing
// MFMAs, and a chunk costs one barrier -- the structure of the fp32 kernel (conv3d.hip), which the 16-bit
// chunks (16x shorter in MFMA time) need even more.
// ONE: one item per workgroup (grid = items), no queue and no prefetch across items.  For items of one or two chunks
// the chain ticket -> loads -> commit -> MFMAs -> stores of a persistent workgroup is mostly latency (a single-chunk
// item has ~1 us of MFMAs but costs ~8 us), and what hides latency there is simply MORE independent workgroups:
// two resident per CU, the next one dispatched by the hardware the moment one retires.
// SIGMOID: the head epilogue (`head` != 0) is nn.Sigmoid instead of nn.Softmax(dim=1).  Instantiations of their own,
// launched for M355_CONV_SIGMOID alone: with the choice made at run time six of the existing instantiations gained
// registers and one lost an occupancy step (profiles/sigmoid_head_resources.txt).
template <int NTW, int GX, typename HT, bool OUT16, int NW = 4, bool ONE = false, bool SIGMOID = false>
__global__ __launch_bounds__(NW * 64, (NW == 8 ? 1 : (NTW <= 4 ? 2 : 1))) void conv3_h16_kernel(
    const HT* __restrict__ x16, const HT* __restrict__ wp, const float* __restrict__ bias,
    const float* __restrict__ add, float* __restrict__ y, float* __restrict__ slab, int CB, int Cout, int D, int H,
    int W, int cout_pad, int tz_tiles, int ty_tiles, int tx_tiles, int otiles, int nchunks, int ksplit, int nbatch,
    int64_t xbs16, int64_t ybs, int64_t slab_stride, float* __restrict__ stat, int* __restrict__ work_counter,
    int stagger, int head, int order, int* __restrict__ oflag) {
  using T = FwdTile<NTW, GX>;
  using hx8 = typename H16<HT>::x8;
  constexpr int GY = T::GY, TZ = NW, TY = T::TY, TX = T::TX, RS = T::RS, PS = T::PS, HV = (TZ + 2) * PS;
  constexpr int NT = NW * 64;                    // threads
  constexpr bool DB = NW == 8;                   // double-buffered LDS
  constexpr bool REUSE = GX == 32;               // row-fragment reuse across (output row, tap row), see the header
  constexpr int XI = 2 * HV;                     // (half, halo voxel) items of 16 bytes
  constexpr int XPER = (XI + NT - 1) / NT;
  constexpr int WI = 27 * 2 * 32;                // (tap, half, o) items of 16 bytes
  constexpr int WPER = (WI + NT - 1) / NT;
  constexpr int NSTEP = REUSE ? 9 : 27;          // MFMA steps per chunk: (dx, dz) pairs, or single taps
  __shared__ __attribute__((aligned(16))) hx8 xs[DB ? 2 : 1][XI];
  __shared__ __attribute__((aligned(16))) hx8 ws[DB ? 2 : 1][WI];
  __shared__ int next_item_s;
  bool sat = false;                              // an fp16 c8 output value was clamped (store_conv_tile_c8)

#ifdef M355_H16_STAMPS
  const unsigned long long r_entry = __builtin_amdgcn_s_memrealtime();
#endif
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int l32 = lane & 31;
  const int ly = l32 / GX, lx = l32 % GX;
  const int iHW = H * W;
  const int S = D * iHW;

  const int sp_tiles = tz_tiles * ty_tiles * tx_tiles;
  const int total = sp_tiles * otiles * nbatch * ksplit;
  const int cps = (nchunks + ksplit - 1) / ksplit;

  struct Item {
    int z0, y0, x0, o0, n, ks, ch_begin, ch_end, sp;
  };
  auto decode = [&](int it) {
    Item q;
    // order bit 1: the output-channel tile is the fastest index (the items sharing an input tile are adjacent in
    // time and on one XCD); bit 0: the (y, z) tiles are walked in 4x4 cubes (z-halos shared in L2 as well)
    const int ot = (order & 2) ? it % otiles : (it / sp_tiles) % otiles;
    int sp = (order & 2) ? (it / otiles) % sp_tiles : it % sp_tiles, r = it / (otiles * sp_tiles);
    const int txt = sp % tx_tiles;
    sp /= tx_tiles;
    int tyt, tzt;
    if ((order & 1) && (ty_tiles & 3) == 0 && (tz_tiles & 3) == 0) {
      const int ty_lo = sp & 3, tz_lo = (sp >> 2) & 3, hi = sp >> 4;
      const int tyh = ty_tiles >> 2;
      tyt = (hi % tyh) * 4 + ty_lo;
      tzt = (hi / tyh) * 4 + tz_lo;
    } else {
      tyt = sp % ty_tiles;
      tzt = sp / ty_tiles;
    }
    q.sp = (tzt * ty_tiles + tyt) * tx_tiles + txt;   // canonical tile index (statistics slot)
    q.x0 = txt * TX;
    q.y0 = tyt * TY;
    q.z0 = tzt * TZ;
    q.o0 = ot * 32;
    q.ks = r % ksplit;
    q.n = r / ksplit;
    q.ch_begin = q.ks * cps;
    q.ch_end = min(nchunks, q.ch_begin + cps);
    return q;
  };

  // byte offsets of this thread's halo items from the first channel block of a chunk; zero padding, items
  // past the tile and the missing second block of an odd block count lie outside the descriptor -> 0
  constexpr unsigned OOB = 0x80000000u;
  unsigned goff[XPER];
  auto compute_goff = [&](const Item& q) {
#pragma unroll
    for (int i = 0; i < XPER; ++i) {
      const int e = tid + NT * i;
      const int h = e / HV, r = e - h * HV;
      const int zz = r / PS, r2 = r - zz * PS;
      const int yy = r2 / RS, xx = r2 - yy * RS;
      const int gz = q.z0 + zz - 1, gy = q.y0 + yy - 1, gx = q.x0 + xx - 1;
      const bool ok = e < XI && (unsigned)gz < (unsigned)D && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
      goff[i] = ok ? (unsigned)(h * S + gz * iHW + gy * W + gx) * 16u : OOB;
    }
  };

  f32x4 xr[XPER], wr[WPER];
  __amdgpu_buffer_rsrc_t rx;
  const f32x4* wsrc = reinterpret_cast<const f32x4*>(wp);
  auto chunk_setup = [&](const Item& q, int ch, bool live) {  // !live: zero-sized descriptor, no memory traffic
    const int nb = min(2, CB - 2 * ch);
    rx = __builtin_amdgcn_make_buffer_rsrc((void*)(x16 + (int64_t)q.n * xbs16 + (int64_t)(2 * ch) * S * 8), 0,
                                           live ? nb * S * 16 : 0, 0x00020000);
    wsrc = reinterpret_cast<const f32x4*>(wp) + (int64_t)ch * 54 * cout_pad + q.o0;
  };
  auto fetch_x = [&](int k) {  // k is a compile-time constant wherever this is called
    xr[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, goff[k], 0, 0));
  };
  auto fetch_w = [&](int k) {
    const int idx = tid + NT * k;
    const int idc = idx < WI ? idx : WI - 1;  // clamp: keeps the array fully scalarised
    wr[k] = wsrc[(int64_t)(idc >> 5) * cout_pad + (idc & 31)];
  };
  // Prefetch items issued during MFMA step s.  ALL of them go out in the first quarter of the chunk (halo items
  // first: HBM / L2 latency; then the L2-resident weight items): a load issued late in the chunk lands a
  // full memory round trip after the last MFMA, and with one LDS buffer the commit (and so the next chunk) waits
  // for it -- spreading the loads over the whole chunk, as the 16x longer fp32 chunks can afford, made every
  // chunk cost MFMA time + memory latency (measured: 43 % of the MFMA rate on 12-chunk items).
  constexpr int ESTEPS = NSTEP / 4 > 0 ? NSTEP / 4 : 1;          // steps that carry halo loads (and as many for weights)
  constexpr int XPS = (XPER + ESTEPS - 1) / ESTEPS, WPS = (WPER + ESTEPS - 1) / ESTEPS;
  constexpr int VPS = XPS > WPS ? XPS : WPS;                     // most prefetch loads in one step
  auto fetch_step = [&](int s) {
#pragma unroll
    for (int k = 0; k < XPER; ++k)
      if (k / XPS == s) fetch_x(k);
#pragma unroll
    for (int k = 0; k < WPER; ++k)
      if (ESTEPS + k / WPS == s) fetch_w(k);
  };
  auto commit = [&](int b) {
#pragma unroll
    for (int i = 0; i < XPER; ++i)
      if (tid + NT * i < XI) reinterpret_cast<f32x4*>(xs[b])[tid + NT * i] = xr[i];
#pragma unroll
    for (int j = 0; j < WPER; ++j)
      if (tid + NT * j < WI) reinterpret_cast<f32x4*>(ws[b])[tid + NT * j] = wr[j];
  };

  // ---- work queue (see conv3_mfma_fwd_p_kernel in conv3d.hip): eight contiguous item regions, one per XCD
  // label (blockIdx % 8), each with an atomic ticket counter; a workgroup whose region is empty steals.
  const int G = (int)gridDim.x;
  const int xl = blockIdx.x & 7;
  const int cpx = (total + 7) >> 3;
  auto region_size = [&](int r) { return max(0, min(cpx, total - r * cpx)); };
  auto region_static = [&](int r) { return min(region_size(r), (G - r + 7) >> 3); };
  auto steal = [&]() {  // thread 0; `total` = nothing left anywhere
    // One 32-byte read of all eight ticket counters first: when every region is drained (what every
    // workgroup finds once, at the end of its life) that is one memory round trip instead of seven
    // dependent atomics (~15-40k cycles, a quarter of the lifetime of a short 16-bit launch).
    int seen[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) seen[r] = __hip_atomic_load(work_counter + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int a = 1; a < 8; ++a) {
      const int r = (xl + a) & 7;
      if (region_static(r) + seen[r] >= region_size(r)) continue;  // nothing dynamic left there (counters only grow)
      const int k = region_static(r) + atomicAdd(work_counter + r, 1);
      if (k < region_size(r)) return r * cpx + k;
    }
    return total;
  };
  auto resolve = [&](int taken) {
    const int k = region_static(xl) + taken;
    return k < region_size(xl) ? xl * cpx + k : steal();
  };
  // (ONE: XCD-aware placement -- blocks b and b + 8 share an XCD and its L2, so every XCD gets a contiguous run of
  // items and the halos that neighbouring tiles share hit in that L2)
  int it = xl * cpx + (int)(blockIdx.x >> 3);
  if constexpr (ONE) {
    const int q = G >> 3, r = G & 7;
    it = stagger ? (xl < r ? xl * (q + 1) : r * (q + 1) + (xl - r) * q) + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  }
  if (!ONE && (int)(blockIdx.x >> 3) >= region_size(xl)) {  // more workgroups than items in this region (uniform)
    if (tid == 0) next_item_s = steal();
    __syncthreads();
    it = next_item_s;
    __syncthreads();
    if (it >= total) {
      queue_leave(work_counter);
      return;
    }
  }
  Item cur = decode(it);
  compute_goff(cur);
  chunk_setup(cur, cur.ch_begin, true);
#pragma unroll
  for (int s = 0; s < NSTEP; ++s) fetch_step(s);
  commit(0);
  __syncthreads();
  int buf = 0;

  const int xoff = half * HV + wave * PS + ly * RS + lx;
  const int woff = half * 32 + l32;

  // Two workgroups share a CU (one wave of each per SIMD) and start together with identical work: left alone they
  // run in lockstep -- both in their MFMA phase (sharing the matrix pipe), then both at the barriers / LDS commit
  // with the pipe idle (SQ counters: pipe busy 54 %, and a wave's non-MFMA time never overlapped its partner's
  // MFMAs).  The workgroup in the odd hardware wave slot starts half a chunk late; equal periods keep the offset.
  if (!DB && stagger > 0) {
    const unsigned wave_slot = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 4);  // HW_REG_HW_ID.WAVE_ID
    if (wave_slot & 1u) {
      for (int i = 0; i < stagger; ++i) __builtin_amdgcn_s_sleep(16);               // 16 x 64 cycles each
    }
  }

#ifdef M355_H16_STAMPS
  unsigned long long ph_mfma = 0, ph_b1 = 0, ph_commit = 0, ph_b2 = 0, ph_epi = 0, ph_n = 0;
  const unsigned long long t_begin = __builtin_amdgcn_s_memtime();
#endif
  f32x16 acc[NTW];
  while (true) {
    int pending = 0;
    if constexpr (!ONE) {
      if (tid == 0) pending = atomicAdd(work_counter + xl, 1);
      if (cur.ch_end - cur.ch_begin == 1) {  // single-chunk items: no chunk to hide the ticket's round trip behind
        if (tid == 0) next_item_s = resolve(pending);
        __syncthreads();
      }
    }
#pragma unroll
    for (int g = 0; g < NTW; ++g)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[g][r] = 0.f;
    Item nxt = cur;
    int nit = total;
    for (int ch = cur.ch_begin; ch < cur.ch_end; ++ch) {
      if (ch + 1 < cur.ch_end) {
        chunk_setup(cur, ch + 1, true);
      } else {  // last chunk of this item: prefetch the first chunk of the next one
        if constexpr (ONE) {
          nit = total;
          chunk_setup(cur, cur.ch_begin, false);   // zero-sized descriptor: the unconditional prefetch moves nothing
        } else {
          nit = next_item_s;
          const bool live = nit < total;
          nxt = decode(live ? nit : it);
          compute_goff(nxt);
          chunk_setup(nxt, nxt.ch_begin, live);
        }
      }
      STAMP(t0);
      const hx8* xb = xs[buf] + xoff;
      const hx8* wb = ws[buf] + woff;
      if constexpr (REUSE) {
        // step s = (dx, dz): rows j = 0 .. NTW+1 of plane wave + dz at column offset dx; MFMA (g, dy) uses
        // row g + dy and the weights of tap (dz, dy, dx).  MFMAs run row by row, so a row fragment dies early;
        // the fragments of step s+1 are requested in the order step s+1 consumes them, one per MFMA from the
        // point where step s has freed enough registers (NR reads behind 3*NTW MFMAs).
        constexpr int NR = NTW + 5;                       // fragment reads per step
        constexpr int NM = 3 * NTW;                       // MFMAs per step
        constexpr int BARE = NM > NR ? NM - NR : 0;       // leading MFMAs without a read behind them
        hx8 fa[2][3], fb[2][NTW + 2];
        auto lds_step = [&](int s, int slot) {
          const int dx = s / 3, dz = s % 3;
          const hx8* wt = wb + (dz * 9 + dx) * 64;        // + dy * 3 * 64
          const hx8* xt = xb + dz * PS + dx;              // + j * RS
          fa[slot][0] = wt[0];
          fb[slot][0] = xt[0];
          fb[slot][1] = xt[RS];
          fa[slot][1] = wt[3 * 64];
          fb[slot][2] = xt[2 * RS];
          fa[slot][2] = wt[6 * 64];
#pragma unroll
          for (int j = 3; j < NTW + 2; ++j) fb[slot][j] = xt[j * RS];
        };
        lds_step(0, 0);
#pragma unroll
        for (int s = 0; s < NSTEP; ++s) {
          if (s + 1 < NSTEP) lds_step(s + 1, (s + 1) & 1);
          fetch_step(s);
#pragma unroll
          for (int j = 0; j < NTW + 2; ++j)
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
              const int g = j - dy;
              if (g >= 0 && g < NTW) acc[g] = H16<HT>::mfma(fa[s & 1][dy], fb[s & 1][j], acc[g]);
            }
#pragma unroll
          for (int m = 0; m < NM; ++m) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                       // MFMA
            if (m >= BARE) __builtin_amdgcn_sched_group_barrier(0x100, (NR + NM - BARE - 1) / (NM - BARE), 0);  // DS read
            if (m < VPS) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                          // one prefetch load
          }
          __builtin_amdgcn_sched_group_barrier(0x020, VPS, 0);  // (more loads than MFMAs in a step: tiny tiles)
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
        hx8 fa[2], fb[2][NTW];
        auto lds_step = [&](int s, int slot) {
          const int dz = s / 9, dy = (s / 3) % 3, dx = s % 3;
          fa[slot] = wb[s * 64];
#pragma unroll
          for (int g = 0; g < NTW; ++g) fb[slot][g] = xb[dz * PS + (g * GY + dy) * RS + dx];
        };
        lds_step(0, 0);
#pragma unroll
        for (int s = 0; s < NSTEP; ++s) {
          if (s + 1 < NSTEP) lds_step(s + 1, (s + 1) & 1);
          fetch_step(s);
#pragma unroll
          for (int g = 0; g < NTW; ++g) acc[g] = H16<HT>::mfma(fa[s & 1], fb[s & 1][g], acc[g]);
#pragma unroll
          for (int g = 0; g < NTW; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // DS read
            __builtin_amdgcn_sched_group_barrier(0x020, (VPS + NTW - 1) / NTW, 0);  // prefetch loads
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if constexpr (!ONE) {
        if (ch == cur.ch_begin && cur.ch_end - cur.ch_begin > 1 && tid == 0) next_item_s = resolve(pending);
      }
      STAMP(t1);
      if constexpr (DB) {
        STAMP(t2);
        commit(buf ^ 1);   // the other buffer: last read a chunk ago, and every wave has passed that chunk's barrier
        STAMP(t3);
        __syncthreads();
        buf ^= 1;
#ifdef M355_H16_STAMPS
        {
          STAMP(t4);
          ph_mfma += t1 - t0; ph_b1 += t2 - t1; ph_commit += t3 - t2; ph_b2 += t4 - t3; ph_n += 1;
        }
#endif
      } else {
      __syncthreads();  // every wave has read its last fragment of this chunk
      STAMP(t2);
      commit(0);
      STAMP(t3);
      __syncthreads();
#ifdef M355_H16_STAMPS
      {
        STAMP(t4);
        ph_mfma += t1 - t0; ph_b1 += t2 - t1; ph_commit += t3 - t2; ph_b2 += t4 - t3; ph_n += 1;
      }
#endif
      }
    }
    STAMP(te0);

    // ---- output tile of `cur` ----
    {
      const int z = cur.z0 + wave;
      const int xg = cur.x0 + lx;
      const bool lane_ok = z < D && xg < W;
      if (ksplit == 1) {
        float* st = stat ? stat + (((int64_t)cur.n * sp_tiles + cur.sp) * NW + wave) * Cout * 2 : nullptr;
        if constexpr (OUT16)
          store_conv_tile_c8<NTW, GY, HT>(acc, reinterpret_cast<HT*>(y) + (int64_t)cur.n * ybs, bias, cur.o0, Cout, z,
                                          cur.y0, xg, ly, half, H, W, (int64_t)S, lane_ok, st, sat);
        else if (head && SIGMOID)
          store_conv_tile_sigmoid<NTW, GY>(acc, y + (int64_t)cur.n * ybs, bias, Cout, z, cur.y0, xg, ly, half, D, H, W,
                                           lane_ok);
        else if (head)   // (host: Cout <= 4, one channel tile, no residual, no statistics)
          store_conv_tile_softmax<NTW, GY>(acc, y + (int64_t)cur.n * ybs, bias, Cout, z, cur.y0, xg, ly, half, D, H, W,
                                           lane_ok);
        else
          store_conv_tile<NTW, GY>(acc, y + (int64_t)cur.n * ybs, add ? add + (int64_t)cur.n * ybs : nullptr, bias,
                                   cur.o0, Cout, z, cur.y0, xg, ly, half, D, H, W, lane_ok, st);
      } else {
        store_conv_tile<NTW, GY>(acc, slab + (int64_t)cur.ks * slab_stride + (int64_t)cur.n * Cout * S, nullptr,
                                 nullptr, cur.o0, Cout, z, cur.y0, xg, ly, half, D, H, W, lane_ok, nullptr);
      }
    }
#ifdef M355_H16_STAMPS
    ph_epi += __builtin_amdgcn_s_memtime() - te0;
#endif
    if (nit >= total) break;
    it = nit;
    cur = nxt;
  }
#ifdef M355_H16_STAMPS
  if (tid == 0 && blockIdx.x < 1024) {
    unsigned long long* o = m355_h16_stamps[blockIdx.x];
    o[0] = ph_mfma; o[1] = ph_b1; o[2] = ph_commit; o[3] = ph_b2; o[4] = ph_epi; o[5] = ph_n;
    o[6] = __builtin_amdgcn_s_memtime() - t_begin;
    o[7] = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);
    // (timeline probe: tools/h16_timeline.py) 100 MHz ticks at kernel entry / exit of this workgroup, XCC id in the top bits
    o[3] = r_entry;
    o[4] = __builtin_amdgcn_s_memrealtime();
    o[7] |= (unsigned long long)__builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) << 32;   // HW_REG_XCC_ID
  }
#endif
  if constexpr (OUT16) report_saturation(sat, oflag);
  if constexpr (!ONE) queue_leave(work_counter);
}

// ---- K-channels <= 4: the first conv of a network (Cin = 4: d0.c0) and the data gradient of its output conv (dy has
// Cout = 3 channels) ----
// The kernel above spends a whole k-step of 16 on ONE tap of a 16-channel chunk: with <= 4 real channels 3/4 of every
// MFMA multiplies zeros, 27 MFMAs per 32-voxel group where 7 suffice -- and the single-chunk item is all fixed cost
// (d0.c0 forward 0.135 ms against 0.02 ms of bytes).  Here a k-step is FOUR taps x 4 channels: the B fragment of a lane
// is two 8-byte LDS reads (channels 0..3 of the voxel at tap 4s + 2h and at tap 4s + 2h + 1), the A fragments are
// gathered once per workgroup from the ordinary packed weights (wp[(tap*2 + half)*cout_pad + m][8], half 0, j < 4), so
// nothing changes for the weight caches.  One output tile (4 x NTW x 32 voxels, one 32-channel tile) per workgroup, c8
// output through store_conv_tile_c8 with the same statistics slots as the generic plan.
template <int NTW, typename HT>
__global__ __launch_bounds__(256, 2) void conv3_c4_h16_kernel(
    const HT* __restrict__ x16, const HT* __restrict__ wp, const float* __restrict__ bias, HT* __restrict__ y16, int Cout,
    int D, int H, int W, int cout_pad, int tz_tiles, int ty_tiles, int tx_tiles, int otiles, int64_t xbs16, int64_t ybs16,
    float* __restrict__ stat, int* __restrict__ oflag) {
  using hx8 = typename H16<HT>::x8;
  constexpr int TZ = 4, TY = NTW, RS = 34, PS = (TY + 2) * RS, HV = (TZ + 2) * PS;
  __shared__ __attribute__((aligned(16))) uint2 xs[HV];        // channels 0..3 of every halo voxel
  __shared__ __attribute__((aligned(16))) uint4 ws[7 * 2 * 32];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l32 = lane & 31;
  const int sp_tiles = tz_tiles * ty_tiles * tx_tiles;
  int it = blockIdx.x;
  const int ot = it % otiles;
  it /= otiles;
  const int sp = it % sp_tiles, n = it / sp_tiles;
  const int txt = sp % tx_tiles, tyt = (sp / tx_tiles) % ty_tiles, tzt = sp / (tx_tiles * ty_tiles);
  const int z0 = tzt * TZ, y0 = tyt * TY, x0 = txt * 32;
  const int iHW = H * W;
  const int64_t S = (int64_t)D * iHW;
  {
    const uint4* xin = reinterpret_cast<const uint4*>(x16 + (int64_t)n * xbs16);   // block 0 only
    for (int e = tid; e < HV; e += 256) {
      const int zz = e / PS, r = e - zz * PS;
      const int yy = r / RS, xx = r - yy * RS;
      const int gz = z0 + zz - 1, gy = y0 + yy - 1, gx = x0 + xx - 1;
      uint2 v = make_uint2(0u, 0u);
      if (gz >= 0 && gz < D && gy >= 0 && gy < H && gx >= 0 && gx < W)
        v = *reinterpret_cast<const uint2*>(xin + ((int64_t)gz * iHW + gy * W + gx));
      xs[e] = v;
    }
    HT* w16 = reinterpret_cast<HT*>(ws);
    for (int i = tid; i < 7 * 2 * 32 * 8; i += 256) {
      const int j = i & 7, m = (i >> 3) & 31, h = (i >> 8) & 1, s = i >> 9;
      const int tap = 4 * s + 2 * h + (j >> 2);
      w16[i] = tap < 27 ? wp[((int64_t)(tap * 2) * cout_pad + ot * 32 + m) * 8 + (j & 3)] : (HT)0.f;
    }
  }
  __syncthreads();
  f32x16 acc[NTW];
#pragma unroll
  for (int g = 0; g < NTW; ++g)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[g][r] = 0.f;
  const uint2* xb = xs + wave * PS + l32;
#pragma unroll
  for (int s = 0; s < 7; ++s) {
    const hx8 a = __builtin_bit_cast(hx8, ws[(s * 2 + half) * 32 + l32]);
    const int ta = 4 * s + 2 * half, tb = min(ta + 1, 26);   // "tap 27" (s = 6, upper half): zero weights, any valid row
    const int offa = (ta / 9) * PS + ((ta / 3) % 3) * RS + ta % 3;
    const int offb = (tb / 9) * PS + ((tb / 3) % 3) * RS + tb % 3;
#pragma unroll
    for (int g = 0; g < NTW; ++g) {
      const uint2 lo = xb[g * RS + offa], hi = xb[g * RS + offb];
      const uint4 bv = make_uint4(lo.x, lo.y, hi.x, hi.y);
      acc[g] = H16<HT>::mfma(a, __builtin_bit_cast(hx8, bv), acc[g]);
    }
  }
  const int z = z0 + wave, xg = x0 + l32;
  float* st = stat ? stat + (((int64_t)n * sp_tiles + sp) * 4 + wave) * Cout * 2 : nullptr;
  bool sat = false;
  store_conv_tile_c8<NTW, 1, HT>(acc, y16 + (int64_t)n * ybs16, bias, ot * 32, Cout, z, y0, xg, 0, half, H, W, S,
                                 z < D && xg < W, st, sat);
  report_saturation(sat, oflag);
}

// ---- M-channels <= 4: the output convolution of a network (Cout = 3: out conv + softmax of cfg2) ----
// conv3_h16_kernel spends a 32-row MFMA tile on 3 useful rows: 27 taps x 2 k-halves = 54 MFMAs per 32 voxels and chunk, 0.10 ms
// for 0.02 ms of bytes (round-3 review, item 3).  Here the tap row dy moves from the K side to the M side: row m = 8 dy + o
// of the A fragment holds W[o][c][dz][dy][dx], so ONE MFMA per (dz, dx) and INPUT row j produces the partial sums of the
// three output rows j - dy it contributes to,
//     P_j[8 dy + o][x] = sum_c W[o, c, dz, dy, dx] * X[c, z + dz - 1, y0 - 1 + j, x + dx - 1]      j = 0 .. NTW + 1
// and the output row g is an in-lane sum of three accumulator registers: out[o][g] = P_g[o] + P_{g+1}[8 + o] + P_{g+2}[16 + o]
// (rows 0..3, 8..11, 16..19 all sit in the LOWER lane half of the 32x32 C/D layout: registers o, 4 + o, 8 + o).
// 9 x (NTW + 2) = 54 MFMAs per chunk and wave instead of 108, 9 A fragments instead of 27, the halo tile and its
// row-fragment reads exactly as in conv3_h16_kernel's REUSE loop.  fp32 NCDHW output with bias and (optionally)
// nn.Softmax(dim=1) in registers (models/modular_unet.py:99-100).  One item per workgroup, two workgroups per CU.
template <int NTW, typename HT>
__global__ __launch_bounds__(256, 2) void conv3_cout4_h16_kernel(
    const HT* __restrict__ x16, const HT* __restrict__ wp, const float* __restrict__ bias, float* __restrict__ y, int CB,
    int Cout, int D, int H, int W, int cout_pad, int tz_tiles, int ty_tiles, int tx_tiles, int nchunks, int64_t xbs16,
    int64_t ybs, int head) {   // head: 0 none, 1 softmax, 2 sigmoid (wave-uniform)
  using T = FwdTile<NTW, 32>;
  using hx8 = typename H16<HT>::x8;
  constexpr int TZ = 4, TY = T::TY, RS = T::RS, PS = T::PS, HV = (TZ + 2) * PS;
  constexpr int XI = 2 * HV, XPER = (XI + 255) / 256;      // (half, halo voxel) items of 16 bytes
  constexpr int WI = 9 * 64, WPER = (WI + 255) / 256;      // ((dz, dx), lane) A-fragment items
  __shared__ __attribute__((aligned(16))) hx8 xs[XI];
  __shared__ __attribute__((aligned(16))) hx8 ws[WI];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l32 = lane & 31;
  const int iHW = H * W, S = D * iHW;
  int it = blockIdx.x;
  const int sp_tiles = tz_tiles * ty_tiles * tx_tiles;
  const int sp = it % sp_tiles, n = it / sp_tiles;
  const int txt = sp % tx_tiles, tyt = (sp / tx_tiles) % ty_tiles, tzt = sp / (tx_tiles * ty_tiles);
  const int z0 = tzt * TZ, y0 = tyt * TY, x0 = txt * 32;

  constexpr unsigned OOB = 0x80000000u;
  unsigned goff[XPER];
#pragma unroll
  for (int i = 0; i < XPER; ++i) {
    const int e = tid + 256 * i;
    const int h = e / HV, r = e - h * HV;
    const int zz = r / PS, r2 = r - zz * PS;
    const int yy = r2 / RS, xx = r2 - yy * RS;
    const int gz = z0 + zz - 1, gy = y0 + yy - 1, gx = x0 + xx - 1;
    const bool ok = e < XI && (unsigned)gz < (unsigned)D && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
    goff[i] = ok ? (unsigned)(h * S + gz * iHW + gy * W + gx) * 16u : OOB;
  }
  // this thread's A-fragment items: item (s = (dz, dx), lane' = (m, half')) <- packed weight item of tap (dz, dy = m >> 3, dx),
  // output channel o = m & 7 (zero rows: o >= Cout or dy > 2)
  int woff[WPER];
#pragma unroll
  for (int k = 0; k < WPER; ++k) {
    const int idx = tid + 256 * k;
    const int sidx = idx >> 6, ln = idx & 63, m = ln & 31, hh = ln >> 5;
    const int o = m & 7, dy = m >> 3, dz = sidx / 3, dx = sidx - 3 * dz;
    woff[k] = (idx < WI && o < Cout && dy < 3) ? ((dz * 9 + dy * 3 + dx) * 2 + hh) * cout_pad + o : -1;
  }
  f32x4 xr[XPER], wr[WPER];
  auto fetch = [&](int ch, bool live) {
    const int nb = min(2, CB - 2 * ch);
    __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(x16 + (int64_t)n * xbs16 + (int64_t)(2 * ch) * S * 8), 0,
                                                                  live ? nb * S * 16 : 0, 0x00020000);
#pragma unroll
    for (int i = 0; i < XPER; ++i) xr[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, goff[i], 0, 0));
    const f32x4* wsrc = reinterpret_cast<const f32x4*>(wp) + (int64_t)ch * 54 * cout_pad;
#pragma unroll
    for (int k = 0; k < WPER; ++k) wr[k] = (live && woff[k] >= 0) ? wsrc[woff[k]] : f32x4{0.f, 0.f, 0.f, 0.f};
  };
  auto commit = [&]() {
#pragma unroll
    for (int i = 0; i < XPER; ++i)
      if (tid + 256 * i < XI) reinterpret_cast<f32x4*>(xs)[tid + 256 * i] = xr[i];
#pragma unroll
    for (int k = 0; k < WPER; ++k)
      if (tid + 256 * k < WI) reinterpret_cast<f32x4*>(ws)[tid + 256 * k] = wr[k];
  };
  fetch(0, true);
  commit();
  __syncthreads();
  f32x16 acc[NTW + 2];
#pragma unroll
  for (int j = 0; j < NTW + 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  const hx8* xb = xs + half * HV + wave * PS + l32;
  for (int ch = 0; ch < nchunks; ++ch) {
    fetch(ch + 1, ch + 1 < nchunks);          // (zero-sized descriptor after the last chunk: the loads move nothing)
    // software-pipelined by one step, as conv3_h16_kernel's loop: the 1 + (NTW + 2) fragments of step s + 1 are requested
    // between the MFMAs of step s (left alone, hipcc sinks every ds_read in front of its MFMA with lgkmcnt(0))
    {
      hx8 fa[2], fb[2][NTW + 2];
      auto lds_step = [&](int st, int slot) {
        const int dz = st / 3, dx = st % 3;
        fa[slot] = ws[st * 64 + lane];
        const hx8* xt = xb + dz * PS + dx;
#pragma unroll
        for (int j = 0; j < NTW + 2; ++j) fb[slot][j] = xt[j * RS];
      };
      lds_step(0, 0);
#pragma unroll
      for (int st = 0; st < 9; ++st) {
        if (st + 1 < 9) lds_step(st + 1, (st + 1) & 1);
#pragma unroll
        for (int j = 0; j < NTW + 2; ++j) acc[j] = H16<HT>::mfma(fa[st & 1], fb[st & 1][j], acc[j]);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                 // MFMA
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                                 // A + first B fragment of the next step
#pragma unroll
        for (int m = 1; m < NTW + 2; ++m) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                               // MFMA
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                               // one more B fragment
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();
    if (ch + 1 < nchunks) commit();
    __syncthreads();
  }
  // ---- output rows: fold the three tap rows, bias, softmax over the <= 4 channels, fp32 NCDHW ----
  if (half == 0) {
    const int z = z0 + wave, xg = x0 + l32;
    const int64_t DHW = (int64_t)S;
    float bb[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) bb[c] = (bias && c < Cout) ? bias[c] : 0.f;
    float* dst = y + (int64_t)n * ybs;
#pragma unroll
    for (int g = 0; g < NTW; ++g) {
      const int yg = y0 + g;
      if (!(z < D && xg < W && yg < H)) continue;
      float v[4], mx = -INFINITY, sum = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        v[c] = ((acc[g][c] + acc[g + 1][4 + c]) + acc[g + 2][8 + c]) + bb[c];
        if (c < Cout) mx = fmaxf(mx, v[c]);
      }
      const int64_t base = (int64_t)z * iHW + (int64_t)yg * W + xg;
      if (head == 1) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < Cout) sum += expf(v[c] - mx);
        const float inv = 1.f / sum;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < Cout) dst[base + (int64_t)c * DHW] = expf(v[c] - mx) * inv;
      } else if (head == 2) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < Cout) dst[base + (int64_t)c * DHW] = sigmoid_f32(v[c]);
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < Cout) dst[base + (int64_t)c * DHW] = v[c];
      }
    }
  }
}

template <typename HT>
static void pack_w3_h16_t(const FwdPlan& p, const float* w, HT* wpb, int Cout_w, int Cin_w, bool transpose, hipStream_t st) {
  const int64_t total = (int64_t)p.nchunks * 27 * 2 * p.mout_pad * 8;
  const int blocks = (int)std::min<int64_t>(ceil_div(total, 256), 2048);
  hipLaunchKernelGGL(pack_w3_h16_kernel<HT>, dim3(blocks), dim3(256), 0, st, w, wpb, Cout_w, Cin_w, p.nchunks,
                     p.mout_pad, transpose ? 1 : 0, (int*)((char*)wpb + p.wp_bytes - 256));
}

void launch_pack_w3_h16(const FwdPlan& p, int compute, const float* w, void* wp, int Cout_w, int Cin_w, bool transpose,
                        hipStream_t st) {
  if (compute == M355_COMPUTE_BF16)
    pack_w3_h16_t<__bf16>(p, w, (__bf16*)wp, Cout_w, Cin_w, transpose, st);
  else
    pack_w3_h16_t<_Float16>(p, w, (_Float16*)wp, Cout_w, Cin_w, transpose, st);
}

// The kernel of a 16-bit route.  The generic kernel's argument list is spelled once: `kern` is the instantiation.
template <int NTW, int GX, typename HT>
static void launch_h16(const ConvRoute& r, const ConvCall& c, const HT* x16, const HT* wp, const float* bias, const float* add,
                       float* slab, float* stat, int* work_counter) {
  const FwdPlan& p = r.plan;
  const m355_conv3d_desc* d = c.d;
  const int N = d->N, D = d->D, H = d->H, W = d->W;
  const bool out16 = r.out16 && p.ksplit == 1;   // a split plan writes fp32 slabs; its reduction writes the c8 output
  if (r.kind == ConvKind::H16C4) {
    if constexpr (GX == 32)
      hipLaunchKernelGGL((conv3_c4_h16_kernel<NTW, HT>), r.grid, dim3(256), 0, c.st, x16, wp, bias, (HT*)c.out, r.mout, D, H, W,
                         p.mout_pad, p.tz_tiles, p.ty_tiles, p.tx_tiles, p.otiles, r.in16_bs, r.out_bs, stat, c.oflag);
    return;
  }
  if (r.kind == ConvKind::H16Cout4) {
    if constexpr (GX == 32 && NTW == 4)
      hipLaunchKernelGGL((conv3_cout4_h16_kernel<4, HT>), r.grid, dim3(256), 0, c.st, x16, wp, bias, c.out, (int)c8_blocks(r.kin),
                         r.mout, D, H, W, p.mout_pad, p.tz_tiles, p.ty_tiles, p.tx_tiles, p.nchunks, r.in16_bs, r.out_bs,
                         r.head);
    return;
  }
  const auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, r.grid, dim3(r.block), 0, c.st, x16, wp, bias, add, c.out, slab, (int)c8_blocks(r.kin), r.mout, D, H,
                       W, p.mout_pad, p.tz_tiles, p.ty_tiles, p.tx_tiles, p.otiles, p.nchunks, p.ksplit, N, r.in16_bs, r.out_bs,
                       (int64_t)N * r.mout * D * H * W, stat, work_counter, r.sched, r.head, r.order, c.oflag);
  };
  if (r.sigmoid) {   // (check_conv: fp32 output, unsplit plan) the instantiations with the sigmoid epilogue
    if (r.kind == ConvKind::H16OneShot) return launch(conv3_h16_kernel<NTW, GX, HT, false, 4, true, true>);
    if constexpr (NTW == 2 && GX == 32)
      if (r.kind == ConvKind::H16Queue8) return launch(conv3_h16_kernel<NTW, GX, HT, false, 8, false, true>);
    return launch(conv3_h16_kernel<NTW, GX, HT, false, 4, false, true>);
  }
  with_bool(out16, [&](auto O) {
    constexpr bool OUT16 = decltype(O)::value;
    if (r.kind == ConvKind::H16OneShot) return launch(conv3_h16_kernel<NTW, GX, HT, OUT16, 4, true>);   // one item per workgroup
    if constexpr (NTW == 2 && GX == 32)
      if (r.kind == ConvKind::H16Queue8) return launch(conv3_h16_kernel<NTW, GX, HT, OUT16, 8>);   // 8-wave double-buffered variant
    launch(conv3_h16_kernel<NTW, GX, HT, OUT16>);
  });
}

template <typename HT>
static int launch_h16_conv_t(const ConvRoute& r, const ConvCall& c, int* oflag) {
  // r.out16: c.out is a c8 tensor of the same 16-bit type (r.out_bs in elements of it)
  // oflag: the overflow word the c8 stores report a saturated fp16 value to (null: saturate silently)
  const FwdPlan& p = r.plan;
  const m355_conv3d_desc* d = c.d;
  hipStream_t st = c.st;
  const int64_t S = (int64_t)d->D * d->H * d->W;
  int* work_counter = queue_state(st);   // per (device, stream): concurrent launches over one model never share it
  M355_REQUIRE(work_counter, M355_ELAUNCH, "conv3d(16-bit operands): could not allocate the work-queue state");
  const HT* in16 = (const HT*)c.in16;
  if (r.aux & AUX_PACK_IN) {
    // fp32 NCDHW input: one conversion pass into the c8 layout (the model path hands over c8 tensors that its
    // normalisation / pooling passes wrote, m355_conv3d_fwd_h16)
    void* stage = (char*)c.ws + r.stage_off;
    if (int rc = launch_pack_act16(c.in, stage, d->N, r.kin, S, r.in_bs, r.in16_bs, d->compute, st)) return rc;
    in16 = (const HT*)stage;
  }
  HT* wpb = r.prepacked ? (HT*)c.w : (HT*)c.ws;
  float* slab = (float*)((char*)c.ws + r.slab_off);
  if (r.aux & AUX_PACK_W) pack_w3_h16_t<HT>(p, c.w, wpb, d->Cout, d->Cin, r.transpose, st);
  const bool split = (r.aux & AUX_SPLITK) != 0;   // bias, residual and statistics then come from the reduction pass
  ConvCall k = c;
  k.oflag = oflag;
#define M355_H16_CASE(NTW, GX)                                                                                   \
  if (p.ntw == NTW && p.gx == GX) {                                                                              \
    launch_h16<NTW, GX, HT>(r, k, in16, wpb, split ? nullptr : c.bias, split ? nullptr : c.add, slab,            \
                            split ? nullptr : c.stat, work_counter);                                             \
  } else
  M355_H16_CASE(4, 32) M355_H16_CASE(2, 32) M355_H16_CASE(1, 32)
  M355_H16_CASE(4, 16) M355_H16_CASE(2, 16) M355_H16_CASE(1, 16)
  M355_H16_CASE(2, 8) M355_H16_CASE(1, 8) {
    set_error("conv3d(16-bit operands): no kernel for ntw=%d gx=%d", p.ntw, p.gx);
    return M355_EUNSUPPORTED;
  }
#undef M355_H16_CASE
  if (r.kind == ConvKind::H16C4) return check_launch("conv3_c4_h16");
  if (r.kind == ConvKind::H16Cout4) return check_launch("conv3_cout4_h16");
  if (split && r.out16)
    hipLaunchKernelGGL(splitk_reduce_c8_kernel<HT>, r.reduce_grid, dim3(256), 0, st, slab, c.bias, (HT*)c.out, r.mout, S,
                       p.ksplit, (int64_t)d->N * r.mout * S, r.out_bs, c.stat, oflag);
  else if (split)
    hipLaunchKernelGGL(splitk_reduce_kernel, r.reduce_grid, dim3(256), 0, st, slab, c.bias, c.add, c.out, d->N, r.mout, S,
                       p.ksplit, (int64_t)d->N * r.mout * S, r.out_bs);
  return check_launch("conv3d_h16");
}

int launch_h16_conv(const ConvRoute& r, const ConvCall& c) {
  if (c.d->compute == M355_COMPUTE_BF16) return launch_h16_conv_t<__bf16>(r, c, nullptr);   // bf16 neither clamps nor reports
  return launch_h16_conv_t<_Float16>(r, c, c.oflag);
}


// ------------------------------------------------ weight gradient from c8 operands (16-bit training flow)
// dW[o,c,tap] = sum_v dy[o,v] * x[c,v+off(tap)] with BOTH operands handed over in the c8 layout (h16.hpp) -- the
// tensors the forward / data-gradient convolutions of the same layer consume anyway, so nothing is converted here
// and the bytes per voxel are half of the fp32 kernel above.  LDS keeps the tiles VOXEL-major, [voxel][32 channels]
// (64-byte rows = four c8 items, copied 16 bytes at a time straight from global memory): a tap is then a whole-row
// offset for every (dz, dy, dx) -- no pre-shifted copies -- and the MFMA fragments (k = 16 x-adjacent voxels of one
// channel) come out of `ds_read_b64_tr_b16`, the hardware transpose read: per 16-lane group a block of 4 voxels x
// 16 channels, delivered channel-per-lane.  The four rows a half-wave reads are 256 contiguous bytes: conflict-free
// for every tap.  Tile = 2 x 4 x 32 voxels (halo 4 x 6 x 34): 68.6 KB of LDS, two workgroups per CU; each wave
// owns 7 of the 27 taps (as the fp32 kernels).  Out-of-volume halo voxels, ragged tiles and channel blocks past the
// tensor are zero-filled by the buffer descriptor.
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
template <typename HT>
__device__ __forceinline__ typename H16<HT>::x8 tr_frag(const unsigned char* p) {
  // two transposed 4-voxel blocks -> the 8 k-values of this lane's half
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 256));
  const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(typename H16<HT>::x8, v);
}

template <typename HT>
__global__ __launch_bounds__(256, 2) void conv3_bww_c8_kernel(
    const HT* __restrict__ x16, const HT* __restrict__ dy16, float* __restrict__ slab, int N, int CBin, int CBout,
    int Cin, int Cout, int D, int H, int W, int tz_tiles, int ty_tiles, int tx_tiles, int nsplit, int ctiles,
    int otiles, int64_t xbs16, int64_t ybs16) {
  constexpr int TZ = 2, TY = 4, TX = 32, NV = TZ * TY * TX;          // 256 voxels
  constexpr int HR = TX + 2, HP = (TY + 2) * HR;                       // 34, 204 halo voxels per row / plane
  constexpr int HV2 = 2 * HP;                                          // a PAIR of halo planes: 408 voxels
  constexpr int XI2 = HV2 * 4, XPER2 = (XI2 + 255) / 256;              // 16-byte items of a plane pair: 1632 -> 7
  constexpr int DI = NV * 4, DPER = DI / 256;                          // of the dy tile: 1024 -> 4
  constexpr unsigned OOB = 0x80000000u;
  // The x halo tile (4 planes) is a RING of four plane slots: a workgroup walks its tiles along z, consecutive tiles
  // share two of their four halo planes, and only the two new ones are fetched (26 KB instead of 52 KB per tile; with
  // the dy tile 42 KB instead of 68 KB).  The kernel is bound by what a CU can miss per clock (~10 B/clk, DESIGN 4.5:
  // 68 KB per tile and workgroup = 2x its MFMA time), so the bytes are the time.  Absolute halo plane z0 - 1 + zz of
  // the tile at z0 = 2 * tzt lives in slot (2 * (tzt & 1) + zz) & 3.
  __shared__ __attribute__((aligned(16))) uint4 xs[4 * HP * 4];   // [slot][halo row][halo column][channel block of the tile]
  __shared__ __attribute__((aligned(16))) uint4 ds[DI];           // [voxel][channel block]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l32 = lane & 31;
  int vid;  // XCD-aware placement, (c-tile, o-tile) pair fastest: see conv3_mfma_bww2_kernel
  {
    const int nwg = (int)gridDim.x, bid = (int)blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    vid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int pairs = ctiles * otiles;
  const int pair = vid % pairs, split = vid / pairs;
  const int ctile = pair % ctiles, otile = pair / ctiles;
  const int iHW = H * W, S = D * iHW;

  // tile-invariant part of the staging: item e of a plane pair = (channel block e / HV2, pair voxel e % HV2)
  int xrel[XPER2], xdst[XPER2];
  unsigned xcode[XPER2];
#pragma unroll
  for (int k = 0; k < XPER2; ++k) {
    const int e = tid + 256 * k;
    const int cbl = e / HV2, hv = e - cbl * HV2;
    const int zz = hv / HP, r = hv - zz * HP;
    const int yy = r / HR, xx = r - yy * HR;
    xrel[k] = cbl * S + zz * iHW + yy * W + xx;
    xdst[k] = hv * 4 + cbl;                                                 // within the pair's two slots
    xcode[k] = e < XI2 ? (1u << zz) | (1u << (8 + yy)) | ((unsigned)xx << 16) : 0xffffu;  // past the end: never valid
  }
  const int dv = tid, dvz = dv / (TY * TX), dvy = (dv / TX) % TY, dvx = dv % TX;  // dy item k: (block k, voxel tid)

  // tiles: z fastest inside a (sample, y tile, x tile) column; split s owns the contiguous range [s * per, (s + 1) * per)
  const int ntiles = N * tz_tiles * ty_tiles * tx_tiles;
  const int per = ntiles / nsplit, rem = ntiles - per * nsplit;       // the first `rem` splits take one tile more
  const int t_begin = split * per + min(split, rem), t_end = t_begin + per + (split < rem ? 1 : 0);
  __amdgpu_buffer_rsrc_t rxu, rxl, rd;
  unsigned zymask_u = 0u, zymask_l = 0u;
  int xbase_u = 0, xbase_l = 0, dbase = 0, xlim = 0, slot_u = 0, slot_l = 0;
  bool dok = false, cold = false;
  auto tile_setup = [&](int tile, bool live) {   // staging state of the tile that is fetched next
    const int tzt = tile % tz_tiles;
    int col = tile / tz_tiles;
    const int txt = col % tx_tiles;
    col /= tx_tiles;
    const int tyt = col % ty_tiles, n = col / ty_tiles;
    const int z0 = tzt * TZ, y0 = tyt * TY, x0 = txt * TX;
    cold = tzt == 0 || tile == t_begin;          // nothing of this column is in the ring yet: both plane pairs
    const int nbx = min(4, CBin - 4 * ctile), nbd = min(4, CBout - 4 * otile);
    const void* xb = x16 + (int64_t)n * xbs16 + (int64_t)(4 * ctile) * S * 8;
    rxu = __builtin_amdgcn_make_buffer_rsrc((void*)xb, 0, live ? nbx * S * 16 : 0, 0x00020000);
    rxl = rxu;
    rd = __builtin_amdgcn_make_buffer_rsrc((void*)(dy16 + (int64_t)n * ybs16 + (int64_t)(4 * otile) * S * 8), 0,
                                           live ? nbd * S * 16 : 0, 0x00020000);
    unsigned ym = 0u;
    for (int yy = 0; yy < TY + 2; ++yy)
      if (y0 + yy - 1 >= 0 && y0 + yy - 1 < H) ym |= 1u << (8 + yy);
    zymask_l = ym, zymask_u = ym;                // lower pair: planes z0 - 1, z0; upper pair: z0 + 1, z0 + 2
    if (z0 - 1 >= 0) zymask_l |= 1u;
    if (z0 < D) zymask_l |= 2u;
    if (z0 + 1 < D) zymask_u |= 1u;
    if (z0 + 2 < D) zymask_u |= 2u;
    xbase_l = (z0 - 1) * iHW + (y0 - 1) * W + x0 - 1;
    xbase_u = xbase_l + 2 * iHW;
    xlim = x0 - 1;                                   // halo column xx is inside the volume iff 0 <= xlim + xx < W
    slot_l = (2 * (tzt & 1)) & 3;
    slot_u = (slot_l + 2) & 3;
    const int gz = z0 + dvz, gy = y0 + dvy, gx = x0 + dvx;
    dok = gz < D && gy < H && gx < W;
    dbase = gz * iHW + gy * W + gx;
  };
  uint4 xr[XPER2], dr[DPER];
  auto fetch = [&]() {   // the two NEW halo planes of the next tile + its dy tile (in flight during this tile's MFMAs)
#pragma unroll
    for (int k = 0; k < XPER2; ++k) {
      const int xx = (int)(xcode[k] >> 16);
      const bool ok = ((xcode[k] & 0xffffu) & ~zymask_u) == 0u && (unsigned)(xlim + xx) < (unsigned)W;
      xr[k] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rxu, ok ? (unsigned)(xbase_u + xrel[k]) * 16u : OOB, 0, 0));
    }
#pragma unroll
    for (int k = 0; k < DPER; ++k)
      dr[k] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rd, dok ? (unsigned)(k * S + dbase) * 16u : OOB, 0, 0));
  };
  auto commit = [&]() {
    uint4* xu = xs + slot_u * HP * 4;
#pragma unroll
    for (int k = 0; k < XPER2; ++k)
      if (tid + 256 * k < XI2) xu[xdst[k]] = xr[k];
#pragma unroll
    for (int k = 0; k < DPER; ++k) ds[dv * 4 + k] = dr[k];
    if (cold) {   // (uniform) start of a column / of this split's range: the other two planes, loaded here and now -- once
                  // per ~16-64 tiles, not worth 28 staging registers held through every MFMA phase
      uint4* xl = xs + slot_l * HP * 4;
#pragma unroll
      for (int k = 0; k < XPER2; ++k) {
        const int xx = (int)(xcode[k] >> 16);
        const bool ok = ((xcode[k] & 0xffffu) & ~zymask_l) == 0u && (unsigned)(xlim + xx) < (unsigned)W;
        xr[k] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rxl, ok ? (unsigned)(xbase_l + xrel[k]) * 16u : OOB, 0, 0));
      }
#pragma unroll
      for (int k = 0; k < XPER2; ++k)
        if (tid + 256 * k < XI2) xl[xdst[k]] = xr[k];
    }
  };

  // transposed-read bases: lane 4q + p of a 16-lane group addresses voxel row q, channels 4p .. 4p+3 of its
  // group's 16-channel half; groups 2, 3 (the upper MFMA half) take the voxels 8 .. 15 of the k-step
  const int grp = lane >> 4, tq = (lane & 15) >> 2, tp = lane & 3;
  const int lb = (8 * (grp >> 1) + tq) * 64 + (grp & 1) * 32 + tp * 8;
  const unsigned char* db = reinterpret_cast<const unsigned char*>(ds) + lb;
  int tdz[7], tyx[7];   // this wave's taps: plane offset dz, byte offset of (dy, dx) inside a plane
#pragma unroll
  for (int t = 0; t < 7; ++t) {
    const int tap = min(wave * 7 + t, 26);
    tdz[t] = tap / 9;
    tyx[t] = (((tap / 3) % 3) * HR + tap % 3) * 64;
  }

  f32x16 acc[7];
#pragma unroll
  for (int t = 0; t < 7; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  if (t_begin < t_end) {
    tile_setup(t_begin, true);
    fetch();
    commit();
  }
  __syncthreads();
#ifdef M355_H16_STAMPS
  unsigned long long ph_mfma = 0, ph_b1 = 0, ph_commit = 0, ph_b2 = 0, ph_n = 0;
  const unsigned long long t_life = __builtin_amdgcn_s_memtime();
#endif
  for (int tile = t_begin; tile < t_end; ++tile) {
    STAMP(t0);
    // fragment bases of THIS tile: voxel plane z, tap plane dz -> ring slot (2 * parity + z + dz) & 3
    const int par2 = 2 * ((tile % tz_tiles) & 1);
    const unsigned char* xt[7][2];
#pragma unroll
    for (int t = 0; t < 7; ++t)
#pragma unroll
      for (int z = 0; z < 2; ++z)
        xt[t][z] = reinterpret_cast<const unsigned char*>(xs) + lb + tyx[t] + ((par2 + z + tdz[t]) & 3) * (HP * 64);
    const bool more = tile + 1 < t_end;
    tile_setup(more ? tile + 1 : tile, more);
    fetch();   // unconditional (zero-sized descriptors after the last tile): keeps the loop one basic block
    // 16 k-steps (voxel row r = (z, y), x half xk) x 7 taps = 112 MFMAs per wave, software-pipelined by one k-step: the
    // A fragment and the 7 B fragments of step g + 1 are requested between the MFMAs of step g (left to the compiler
    // every MFMA waited lgkmcnt(0) for its own fragment: ~70 cycles per MFMA instead of 32).  A scheduling barrier per
    // step keeps the compiler from regrouping the stream by accumulator.
    {
      using hx8 = typename H16<HT>::x8;
      auto afrag = [&](int g) {
        const int r = g >> 1, xk = g & 1, z = r / TY, y = r % TY;
        return tr_frag<HT>(db + ((z * TY + y) * TX + 16 * xk) * 64);
      };
      auto bfrag = [&](int g, int t) {
        const int r = g >> 1, xk = g & 1, z = r / TY, y = r % TY;
        return tr_frag<HT>(xt[t][z] + (y * HR + 16 * xk) * 64);
      };
      hx8 aq[2], bq[2][7];
      aq[0] = afrag(0);
#pragma unroll
      for (int t = 0; t < 7; ++t) bq[0][t] = bfrag(0, t);
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        if (g + 1 < 16) aq[(g + 1) & 1] = afrag(g + 1);
#pragma unroll
        for (int t = 0; t < 7; ++t) {
          if (g + 1 < 16) bq[(g + 1) & 1][t] = bfrag(g + 1, t);
          acc[t] = H16<HT>::mfma(aq[g & 1], bq[g & 1][t], acc[t]);
        }
        if (g + 1 < 16) {
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);      // A fragment of the next step
#pragma unroll
          for (int t = 0; t < 7; ++t) {
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);    // B fragment (next step, tap t)
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);    // MFMA (this step, tap t)
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    STAMP(t1);
    __syncthreads();  // every wave is done reading this tile
    STAMP(t2);
    if (more) commit();
    STAMP(t3);
    __syncthreads();
#ifdef M355_H16_STAMPS
    {
      STAMP(t4);
      ph_mfma += t1 - t0; ph_b1 += t2 - t1; ph_commit += t3 - t2; ph_b2 += t4 - t3; ph_n += 1;
    }
#endif
  }
#ifdef M355_H16_STAMPS
  if (tid == 0 && blockIdx.x < 1024) {
    unsigned long long* o = m355_h16_stamps[blockIdx.x];
    o[0] = ph_mfma; o[1] = ph_b1; o[2] = ph_commit; o[3] = ph_b2; o[4] = 0; o[5] = ph_n;
    o[6] = __builtin_amdgcn_s_memtime() - t_life;
    o[7] = 0;
  }
#endif

  // partial dW -> slab[split][27][Cout][Cin] (lane = input channel: 32 consecutive floats per store)
  float* sl = slab + (int64_t)split * 27 * Cout * Cin;
  const int c = ctile * 32 + l32;
#pragma unroll
  for (int t = 0; t < 7; ++t) {
    const int tap = wave * 7 + t;
    if (tap < 27 && c < Cin) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = otile * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (o < Cout) sl[((int64_t)tap * Cout + o) * Cin + c] = acc[t][r];
      }
    }
  }
}

// ---- the two EDGE layers of a network: Cin <= 4 (first conv) or Cout <= 4 (output conv) ----
// conv3_bww_c8_kernel pads the narrow side to a 32-column MFMA tile: 27 MFMAs per k-step of which 1/8 of the columns
// are real (d0.c0 / out conv of cfg2: 0.22 ms each against 0.03 ms of bytes).  Here the narrow channel AND the tap share
// the column index, as in the fp32 kernel conv3_mfma_bww_small_kernel: column n = 4 * tau + q (tau = one of 8 taps of a
// wave, q = narrow channel 0..3), so ONE MFMA per k-step and wave covers 8 taps and the four waves cover all 27:
//     G[p, (tau, q)] = sum_v P[p, v] * Q[q, v + off(tau)]
//   swap = 0 (Cin <= 4):  P = dy (wide = Cout), Q = x,                                  dW[o = p][c = q][tau]
//   swap = 1 (Cout <= 4): P = x (wide = Cin),   Q = dy at v - off(tau) = v + off(26 - tau),  dW[o = q][c = p][tau]
// Both operands arrive as c8.  P sits in LDS voxel-major with 64-byte rows (ds_read_b64_tr_b16 fragments as in the
// kernel above); Q's halo tile keeps its 16-byte items, and the transposed read takes a PER-LANE address: lane (row r,
// piece tp) of a 16-lane group points at voxel r + off(tau_tp) -- the hardware hands element e of piece tp to lane
// 4 * tp + e, which is exactly column (tau_tp, q = e).  Channels 4..7 of Q's block are never read.
template <typename HT>
__global__ __launch_bounds__(256, 2) void conv3_bww_c8_small_kernel(
    const HT* __restrict__ P16, const HT* __restrict__ Q16, float* __restrict__ slab, int N, int CBp, int CP, int CQ, int D,
    int H, int W, int tz_tiles, int ty_tiles, int tx_tiles, int nsplit, int ptiles, int64_t pbs16, int64_t qbs16, int swap,
    int Cin, int Cout) {
  constexpr int TZ = 2, TY = 4, TX = 32, NV = TZ * TY * TX;          // 256 voxels
  constexpr int HR = TX + 2, HP = (TY + 2) * HR, HVX = (TZ + 2) * HP;  // 34, 204, 816 halo voxels
  constexpr int QPER = (HVX + 255) / 256, PPER = NV * 4 / 256;        // 16-byte items per thread: 4 and 4
  constexpr unsigned OOB = 0x80000000u;
  __shared__ __attribute__((aligned(16))) uint4 qs[HVX + 8];  // [halo voxel]  (block 0 of Q; + slack for the dummy taps)
  __shared__ __attribute__((aligned(16))) uint4 ps[NV * 4];   // [voxel][channel block of the tile]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l32 = lane & 31;
  int vid;
  {
    const int nwg = (int)gridDim.x, bid = (int)blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    vid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int ptile = vid % ptiles, split = vid / ptiles;
  const int iHW = H * W, S = D * iHW;
  // staging geometry of the Q halo tile: item e = halo voxel e
  int qrel[QPER];
  unsigned qcode[QPER];
#pragma unroll
  for (int k = 0; k < QPER; ++k) {
    const int hv = tid + 256 * k;
    const int zz = hv / HP, r = hv - zz * HP;
    const int yy = r / HR, xx = r - yy * HR;
    qrel[k] = zz * iHW + yy * W + xx;
    qcode[k] = hv < HVX ? (1u << zz) | (1u << (8 + yy)) | ((unsigned)xx << 16) : 0xffffu;
  }
  const int dvz = tid / (TY * TX), dvy = (tid / TX) % TY, dvx = tid % TX;   // P item k: (block k, voxel tid)
  const int tiles_per_n = tz_tiles * ty_tiles * tx_tiles;
  const int ntiles = N * tiles_per_n;
  __amdgpu_buffer_rsrc_t rp, rq;
  unsigned zymask = 0u;
  int qbase = 0, pbase = 0, xlim = 0;
  bool pok = false;
  auto tile_setup = [&](int tile, bool live) {
    int t = tile;
    const int n = t / tiles_per_n;
    t -= n * tiles_per_n;
    const int txt = t % tx_tiles;
    t /= tx_tiles;
    const int tyt = t % ty_tiles, tzt = t / ty_tiles;
    const int z0 = tzt * TZ, y0 = tyt * TY, x0 = txt * TX;
    const int nbp = min(4, CBp - 4 * ptile);
    rp = __builtin_amdgcn_make_buffer_rsrc((void*)(P16 + (int64_t)n * pbs16 + (int64_t)(4 * ptile) * S * 8), 0,
                                           live ? nbp * S * 16 : 0, 0x00020000);
    rq = __builtin_amdgcn_make_buffer_rsrc((void*)(Q16 + (int64_t)n * qbs16), 0, live ? S * 16 : 0, 0x00020000);
    zymask = 0u;
    for (int zz = 0; zz < TZ + 2; ++zz)
      if (z0 + zz - 1 >= 0 && z0 + zz - 1 < D) zymask |= 1u << zz;
    for (int yy = 0; yy < TY + 2; ++yy)
      if (y0 + yy - 1 >= 0 && y0 + yy - 1 < H) zymask |= 1u << (8 + yy);
    qbase = (z0 - 1) * iHW + (y0 - 1) * W + x0 - 1;
    xlim = x0 - 1;
    const int gz = z0 + dvz, gy = y0 + dvy, gx = x0 + dvx;
    pok = gz < D && gy < H && gx < W;
    pbase = gz * iHW + gy * W + gx;
  };
  uint4 qr[QPER], pr[PPER];
  auto fetch = [&]() {
#pragma unroll
    for (int k = 0; k < QPER; ++k) {
      const int xx = (int)(qcode[k] >> 16);
      const bool ok = ((qcode[k] & 0xffffu) & ~zymask) == 0u && (unsigned)(xlim + xx) < (unsigned)W;
      qr[k] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rq, ok ? (unsigned)(qbase + qrel[k]) * 16u : OOB, 0, 0));
    }
#pragma unroll
    for (int k = 0; k < PPER; ++k)
      pr[k] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rp, pok ? (unsigned)(k * S + pbase) * 16u : OOB, 0, 0));
  };
  auto commit = [&]() {
#pragma unroll
    for (int k = 0; k < QPER; ++k) {
      const int hv = tid + 256 * k;
      if (hv < HVX) qs[hv] = qr[k];
    }
#pragma unroll
    for (int k = 0; k < PPER; ++k) ps[tid * 4 + k] = pr[k];
  };
  // fragment bases.  A (P tile): as conv3_bww_c8_kernel.  B (Q halo tile): this lane's piece is tap tau = 8 wave +
  // 4 (grp & 1) + tp at voxel row 8 (grp >> 1) + tq; swap reads the mirrored tap.
  const int grp = lane >> 4, tq = (lane & 15) >> 2, tp = lane & 3;
  const int lb = (8 * (grp >> 1) + tq) * 64 + (grp & 1) * 32 + tp * 8;
  const unsigned char* pb = reinterpret_cast<const unsigned char*>(ps) + lb;
  const int tau = min(wave * 8 + 4 * (grp & 1) + tp, 26);
  const int tsrc = swap ? 26 - tau : tau;
  const unsigned char* qb = reinterpret_cast<const unsigned char*>(qs) +
                            ((tsrc / 9) * HP + ((tsrc / 3) % 3) * HR + tsrc % 3 + 8 * (grp >> 1) + tq) * 16;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  if (tid < 8) qs[HVX + tid] = make_uint4(0u, 0u, 0u, 0u);
  if (split < ntiles) {
    tile_setup(split, true);
    fetch();
    commit();
  }
  __syncthreads();
  for (int tile = split; tile < ntiles; tile += nsplit) {
    const bool more = tile + nsplit < ntiles;
    tile_setup(more ? tile + nsplit : tile, more);
    fetch();
#pragma unroll
    for (int r = 0; r < TZ * TY; ++r) {
      const int z = r / TY, y = r % TY;
#pragma unroll
      for (int xk = 0; xk < 2; ++xk) {
        const typename H16<HT>::x8 a = tr_frag<HT>(pb + ((z * TY + y) * TX + 16 * xk) * 64);
        // two transposed 4-voxel pieces of this lane's tap: rows r .. r+3 and r+4 .. r+7 of its k-half (16 bytes a row)
        typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
        const unsigned char* q0 = qb + (z * HP + y * HR + 16 * xk) * 16;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(q0));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(q0 + 64));
        const s16x8 bv = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        acc = H16<HT>::mfma(a, __builtin_bit_cast(typename H16<HT>::x8, bv), acc);
      }
    }
    __syncthreads();
    if (more) commit();
    __syncthreads();
  }
  // partial dW -> slab[split][tap][Cout][Cin]: column l32 = (tap of this wave l32 >> 2, narrow channel l32 & 3)
  float* sl = slab + (int64_t)split * 27 * Cout * Cin;
  const int tap = wave * 8 + (l32 >> 2), q = l32 & 3;
  if (tap < 27 && q < CQ) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int pch = ptile * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (pch < CP) {
        const int o = swap ? q : pch, c = swap ? pch : q;
        sl[((int64_t)tap * Cout + o) * Cin + c] = acc[r];
      }
    }
  }
}

// weight gradient from c8 operands (tile 2 x 4 x 32 voxels); slab[split][27][Cout][Cin], summed by slab_reduce_t_kernel.
// C8Small, an edge layer (Cin <= 4 or Cout <= 4): narrow channel and tap share the MFMA column
void launch_bww_c8(const BwwRoute& r, const void* x16, const void* dy16, float* slab, const m355_conv3d_desc* d, hipStream_t st) {
  const int Cin = d->Cin, Cout = d->Cout;
  const int tz = (int)ceil_div(d->D, 2), ty = (int)ceil_div(d->H, 4), tx = (int)ceil_div(d->W, 32);
  with_h16(d->compute, [&](auto T) {
    typedef typename decltype(T)::type HT;
    if (r.kind == BwwKind::C8Small) {
      const int swap = Cin <= 4 ? 0 : 1;
      const int CP = swap ? Cin : Cout, CQ = swap ? Cout : Cin;
      hipLaunchKernelGGL(conv3_bww_c8_small_kernel<HT>, r.grid, dim3(256), 0, st, (const HT*)(swap ? x16 : dy16),
                         (const HT*)(swap ? dy16 : x16), slab, d->N, (int)c8_blocks(CP), CP, CQ, d->D, d->H, d->W, tz, ty, tx,
                         r.nsplit, (int)ceil_div(CP, 32), swap ? r.xbs : r.ybs, swap ? r.ybs : r.xbs, swap, Cin, Cout);
    } else {
      hipLaunchKernelGGL(conv3_bww_c8_kernel<HT>, r.grid, dim3(256), 0, st, (const HT*)x16, (const HT*)dy16, slab, d->N,
                         (int)c8_blocks(Cin), (int)c8_blocks(Cout), Cin, Cout, d->D, d->H, d->W, tz, ty, tx, r.nsplit,
                         (int)ceil_div(Cin, 32), (int)ceil_div(Cout, 32), r.xbs, r.ybs);
    }
  });
}

#ifdef M355_H16_STAMPS
}  // namespace m355
extern "C" int m355_debug_h16_stamps(unsigned long long* host_out) {
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(m355::m355_h16_stamps), sizeof(m355::m355_h16_stamps)) == hipSuccess ? 0 : -3;
}
namespace m355 {
#endif
}  // namespace m355
