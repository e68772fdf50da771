// nn.Upsample(scale_factor=2) in the two conventions next to align_corners=True (elementwise.hip): mode='nearest'
// (= 'nearest-exact' at this factor) and mode='trilinear' with align_corners=False, the half-pixel convention ("hp").
// fp32 NCDHW and the c8 layout of the 16-bit flows (h16.hpp), forward and gather-form backward.  HBM-write bound
// (1 read, 8 writes), grid-stride, one pass each.
//
// Reference op replaced: upsample_class=nn.Upsample of ModularUNet (models/modular_unet.py:20-21,72-81,96) with
// upsample_params other than the default.
//
// Index maps (aten/src/ATen/native/UpSample.h at scale 2):
//   nearest     y[2i + a] = x[i], a in {0, 1}: the forward moves bits, the backward sums the 2x2x2 block.
//   half-pixel  src = 0.5 * (dst + 0.5) - 0.5 clamped below at 0, i1 = min(i0 + 1, n - 1), per axis:
//                 y[2i]     = 0.25 * x[max(i - 1, 0)] + 0.75 * x[i]
//                 y[2i + 1] = 0.75 * x[i] + 0.25 * x[min(i + 1, n - 1)]
//               The weights are constants, and as fma(0.75, b, 0.25 * a) a clamped tap (a == b) returns b exactly.
//               Transposed: x[i] collects 0.25, 0.75, 0.75, 0.25 from outputs 2i - 1 .. 2i + 2 with the OUTPUT index
//               clamped to [0, 2n - 1] -- the tap that falls off the volume lands on the border output, which is the
//               output that read x[i] a second time through its clamped neighbour (n = 1: both outputs with weight 1).
// A thread owns an input voxel (VEC: an x pair) and the 2x2x2 outputs above it, so the forward reads the clamped
// 3x3x3 neighbourhood once per block, and every store of the VEC variants is a float4 of one output row.
#include "resample_host.hpp"

namespace m355 {

struct UpIdx {
  int n, c, z, y, x;
};
// i -> position in an [N][C][D][H][WV] index space; 32-bit divisions wherever the index fits (a 64-bit division is
// ~100 instructions, and there are four per thread)
__device__ __forceinline__ UpIdx up_split(int64_t i, int WV, int H, int D, int C) {
  UpIdx v;
  if (((uint64_t)i >> 32) == 0) {
    unsigned r = (unsigned)i;
    v.x = (int)(r % (unsigned)WV); r /= (unsigned)WV;
    v.y = (int)(r % (unsigned)H);  r /= (unsigned)H;
    v.z = (int)(r % (unsigned)D);  r /= (unsigned)D;
    v.c = (int)(r % (unsigned)C);
    v.n = (int)(r / (unsigned)C);
  } else {
    v.x = (int)(i % WV);
    int64_t r = i / WV;
    v.y = (int)(r % H); r /= H;
    v.z = (int)(r % D); r /= D;
    v.c = (int)(r % C);
    v.n = (int)(r / C);
  }
  return v;
}

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }
// 0.75 * near + 0.25 * far, exact for near == far
__device__ __forceinline__ float hp_mix(float near, float far) { return fmaf(0.75f, near, 0.25f * far); }

// ------------------------------------------------------------------ nearest, fp32
template <bool VEC>
__global__ __launch_bounds__(256) void nearest2_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int C,
                                                           int D, int H, int W, int64_t xbs, int64_t ybs) {
  const int OH = 2 * H, OW = 2 * W, WV = VEC ? W / 2 : W;
  const int64_t S = (int64_t)D * H * W;
  const int64_t total = (int64_t)N * C * D * H * WV;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll) {
    const UpIdx v = up_split(i, WV, H, D, C);
    const float* xp = x + (int64_t)v.n * xbs + (int64_t)v.c * S + ((int64_t)v.z * H + v.y) * W;
    float* yp = y + (int64_t)v.n * ybs + (int64_t)v.c * S * 8 + ((int64_t)(2 * v.z) * OH + 2 * v.y) * OW;
    if (VEC) {
      const float a = xp[2 * v.x], b = xp[2 * v.x + 1];
      const float4 o = make_float4(a, a, b, b);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<float4*>(yp + ((int64_t)(q >> 1) * OH + (q & 1)) * OW + 4 * v.x) = o;
    } else {
      const float a = xp[v.x];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float* o = yp + ((int64_t)(q >> 1) * OH + (q & 1)) * OW + 2 * v.x;
        o[0] = a;
        o[1] = a;
      }
    }
  }
}

// the eight gradients of the block, summed in (z, y, x) order
template <bool VEC>
__global__ __launch_bounds__(256) void nearest2_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int N, int C,
                                                           int D, int H, int W, int64_t dybs, int64_t dxbs) {
  const int OH = 2 * H, OW = 2 * W, WV = VEC ? W / 2 : W;
  const int64_t S = (int64_t)D * H * W;
  const int64_t total = (int64_t)N * C * D * H * WV;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll) {
    const UpIdx v = up_split(i, WV, H, D, C);
    const float* dp = dy + (int64_t)v.n * dybs + (int64_t)v.c * S * 8 + ((int64_t)(2 * v.z) * OH + 2 * v.y) * OW;
    float* o = dx + (int64_t)v.n * dxbs + (int64_t)v.c * S + ((int64_t)v.z * H + v.y) * W;
    if (VEC) {
      float s0 = 0.f, s1 = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 g = *reinterpret_cast<const float4*>(dp + ((int64_t)(q >> 1) * OH + (q & 1)) * OW + 4 * v.x);
        s0 += g.x + g.y;
        s1 += g.z + g.w;
      }
      *reinterpret_cast<float2*>(o + 2 * v.x) = make_float2(s0, s1);
    } else {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float* g = dp + ((int64_t)(q >> 1) * OH + (q & 1)) * OW + 2 * v.x;
        s += g[0] + g[1];
      }
      o[v.x] = s;
    }
  }
}

// ------------------------------------------------------------------ half-pixel trilinear, fp32
// separable: x, then y, then z -- three weight products and seven additions per output, each stage a convex combination
template <bool VEC>
__global__ __launch_bounds__(256) void trilinear2_hp_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int N,
                                                                int C, int D, int H, int W, int64_t xbs, int64_t ybs) {
  constexpr int XP = VEC ? 2 : 1;   // inputs along x per thread, 2 * XP outputs per row
  const int OH = 2 * H, OW = 2 * W, WV = VEC ? W / 2 : W;
  const int64_t S = (int64_t)D * H * W;
  const int64_t total = (int64_t)N * C * D * H * WV;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll) {
    const UpIdx v = up_split(i, WV, H, D, C);
    const float* xp = x + (int64_t)v.n * xbs + (int64_t)v.c * S;
    const int x0 = XP * v.x;
    int cx[XP + 2];
#pragma unroll
    for (int k = 0; k < XP + 2; ++k) cx[k] = clampi(x0 - 1 + k, W - 1);
    float pl[3][2][2 * XP];   // per input plane: the two output rows
#pragma unroll
    for (int kz = 0; kz < 3; ++kz) {
      float rx[3][2 * XP];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const float* row = xp + ((int64_t)clampi(v.z - 1 + kz, D - 1) * H + clampi(v.y - 1 + ky, H - 1)) * W;
        float t[XP + 2];
#pragma unroll
        for (int k = 0; k < XP + 2; ++k) t[k] = row[cx[k]];
#pragma unroll
        for (int p = 0; p < XP; ++p) {
          rx[ky][2 * p] = hp_mix(t[p + 1], t[p]);
          rx[ky][2 * p + 1] = hp_mix(t[p + 1], t[p + 2]);
        }
      }
#pragma unroll
      for (int k = 0; k < 2 * XP; ++k) {
        pl[kz][0][k] = hp_mix(rx[1][k], rx[0][k]);
        pl[kz][1][k] = hp_mix(rx[1][k], rx[2][k]);
      }
    }
    float* yp = y + (int64_t)v.n * ybs + (int64_t)v.c * S * 8 + ((int64_t)(2 * v.z) * OH + 2 * v.y) * OW + 2 * x0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float o[2 * XP];
#pragma unroll
      for (int k = 0; k < 2 * XP; ++k) o[k] = hp_mix(pl[1][q & 1][k], pl[(q >> 1) ? 2 : 0][q & 1][k]);
      float* dst = yp + ((int64_t)(q >> 1) * OH + (q & 1)) * OW;
      if (VEC) {
        *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2 * XP - 2], o[2 * XP - 1]);
      } else {
        dst[0] = o[0];
        dst[1] = o[1];
      }
    }
  }
}

__device__ __forceinline__ float hp_tap_weight(int k) { return (k == 0 || k == 3) ? 0.25f : 0.75f; }

// gather-form transpose (deterministic, no atomics): 4 x 4 x 4 taps with the output index clamped, fp32 sums
template <bool VEC>
__global__ __launch_bounds__(256) void trilinear2_hp_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int N,
                                                                int C, int D, int H, int W, int64_t dybs, int64_t dxbs) {
  const int OD = 2 * D, OH = 2 * H, OW = 2 * W, WV = VEC ? W / 2 : W;
  const int64_t S = (int64_t)D * H * W;
  const int64_t total = (int64_t)N * C * D * H * WV;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll) {
    const UpIdx v = up_split(i, WV, H, D, C);
    const float* dp = dy + (int64_t)v.n * dybs + (int64_t)v.c * S * 8;
    float* o = dx + (int64_t)v.n * dxbs + (int64_t)v.c * S + ((int64_t)v.z * H + v.y) * W;
    float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
    for (int kz = 0; kz < 4; ++kz) {
      const int oz = clampi(2 * v.z - 1 + kz, OD - 1);
#pragma unroll
      for (int ky = 0; ky < 4; ++ky) {
        const float* row = dp + ((int64_t)oz * OH + clampi(2 * v.y - 1 + ky, OH - 1)) * OW;
        const float w = hp_tap_weight(kz) * hp_tap_weight(ky);
        if (VEC) {   // inputs 2x, 2x + 1: outputs 4x - 1 .. 4x + 4, the middle four as one float4
          const float4 q = *reinterpret_cast<const float4*>(row + 4 * v.x);
          const float l = row[max(4 * v.x - 1, 0)], r = row[min(4 * v.x + 4, OW - 1)];
          const float r0 = fmaf(0.25f, q.z, fmaf(0.75f, q.y, fmaf(0.75f, q.x, 0.25f * l)));
          const float r1 = fmaf(0.25f, r, fmaf(0.75f, q.w, fmaf(0.75f, q.z, 0.25f * q.y)));
          acc0 = fmaf(w, r0, acc0);
          acc1 = fmaf(w, r1, acc1);
        } else {
          float r0 = 0.f;
#pragma unroll
          for (int k = 0; k < 4; ++k) r0 = fmaf(hp_tap_weight(k), row[clampi(2 * v.x - 1 + k, OW - 1)], r0);
          acc0 = fmaf(w, r0, acc0);
        }
      }
    }
    if (VEC) *reinterpret_cast<float2*>(o + 2 * v.x) = make_float2(acc0, acc1);
    else o[v.x] = acc0;
  }
}

// ------------------------------------------------------------------ c8 (one thread: the 8 channels of an item)
// nearest forward: the input item, eight times
template <typename HT>
__global__ __launch_bounds__(256) void nearest2_fwd_c8_kernel(const HT* __restrict__ x16, HT* __restrict__ y16, int N, int CB,
                                                              int D, int H, int W, int64_t xbs, int64_t ybs) {
  using hx8 = typename H16<HT>::x8;
  const int OH = 2 * H, OW = 2 * W;
  const int64_t S = (int64_t)D * H * W;
  const int64_t total = (int64_t)N * CB * S;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll) {
    const UpIdx v = up_split(i, W, H, D, CB);
    const hx8 a = (reinterpret_cast<const hx8*>(x16 + (int64_t)v.n * xbs) + (int64_t)v.c * S)[((int64_t)v.z * H + v.y) * W + v.x];
    hx8* yp = reinterpret_cast<hx8*>(y16 + (int64_t)v.n * ybs) + (int64_t)v.c * S * 8 + ((int64_t)(2 * v.z) * OH + 2 * v.y) * OW +
              2 * v.x;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      hx8* o = yp + ((int64_t)(q >> 1) * OH + (q & 1)) * OW;
      o[0] = a;
      o[1] = a;
    }
  }
}

// nearest backward: fp32 sum of the block's eight gradients, one rounding (saturating for fp16: eight loss-scaled
// gradients can leave its range)
template <typename HT>
__global__ __launch_bounds__(256) void nearest2_bwd_c8_kernel(const HT* __restrict__ dy16, HT* __restrict__ dx16, int N, int CB,
                                                              int D, int H, int W, int64_t dybs, int64_t dxbs,
                                                              int* __restrict__ oflag) {
  using hx8 = typename H16<HT>::x8;
  bool sat = false;
  const int OH = 2 * H, OW = 2 * W;
  const int64_t S = (int64_t)D * H * W;
  const int64_t total = (int64_t)N * CB * S;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll) {
    const UpIdx v = up_split(i, W, H, D, CB);
    const hx8* dp = reinterpret_cast<const hx8*>(dy16 + (int64_t)v.n * dybs) + (int64_t)v.c * S * 8 +
                    ((int64_t)(2 * v.z) * OH + 2 * v.y) * OW + 2 * v.x;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const hx8* g = dp + ((int64_t)(q >> 1) * OH + (q & 1)) * OW;
      const hx8 g0 = g[0], g1 = g[1];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += (float)g0[j] + (float)g1[j];
    }
    hx8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = to_h16_sat<HT>(acc[j], sat);
    (reinterpret_cast<hx8*>(dx16 + (int64_t)v.n * dxbs) + (int64_t)v.c * S)[((int64_t)v.z * H + v.y) * W + v.x] = o;
  }
  report_saturation(sat, oflag);
}

// half-pixel forward: a thread owns input column ix of OUTPUT row (oz, oy) and writes the two adjacent output items
// above it -- 12 item loads (2 z x 2 y x 3 x), z and y combined first, then x; fp32, one rounding
template <typename HT>
__global__ __launch_bounds__(256) void trilinear2_hp_fwd_c8_kernel(const HT* __restrict__ x16, HT* __restrict__ y16, int N,
                                                                   int CB, int D, int H, int W, int64_t xbs, int64_t ybs) {
  using hx8 = typename H16<HT>::x8;
  const int OD = 2 * D, OH = 2 * H, OW = 2 * W;
  const int64_t S = (int64_t)D * H * W;
  const int64_t total = (int64_t)N * CB * OD * OH * W;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll) {
    const UpIdx v = up_split(i, W, OH, OD, CB);   // (z, y): the output row
    const int zn = v.z >> 1, yn = v.y >> 1;       // the near input plane / row (0.75) and the far one (0.25)
    const int zf = (v.z & 1) ? min(zn + 1, D - 1) : max(zn - 1, 0), yf = (v.y & 1) ? min(yn + 1, H - 1) : max(yn - 1, 0);
    const hx8* xp = reinterpret_cast<const hx8*>(x16 + (int64_t)v.n * xbs) + (int64_t)v.c * S;
    const hx8* rows[4] = {xp + ((int64_t)zn * H + yn) * W, xp + ((int64_t)zn * H + yf) * W, xp + ((int64_t)zf * H + yn) * W,
                          xp + ((int64_t)zf * H + yf) * W};
    const int cx[3] = {max(v.x - 1, 0), v.x, min(v.x + 1, W - 1)};
    float t[3][8];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const hx8 nn = rows[0][cx[k]], nf = rows[1][cx[k]], fn = rows[2][cx[k]], ff = rows[3][cx[k]];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        t[k][j] = hp_mix(hp_mix((float)nn[j], (float)nf[j]), hp_mix((float)fn[j], (float)ff[j]));
    }
    hx8 o0, o1;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      o0[j] = (HT)hp_mix(t[1][j], t[0][j]);
      o1[j] = (HT)hp_mix(t[1][j], t[2][j]);
    }
    hx8* o = reinterpret_cast<hx8*>(y16 + (int64_t)v.n * ybs) + (int64_t)v.c * S * 8 + ((int64_t)v.z * OH + v.y) * OW + 2 * v.x;
    o[0] = o0;
    o[1] = o1;
  }
}

// half-pixel backward: the 4 x 4 x 4 clamped taps of trilinear2_hp_bwd_kernel on c8 gradients
template <typename HT>
__global__ __launch_bounds__(256) void trilinear2_hp_bwd_c8_kernel(const HT* __restrict__ dy16, HT* __restrict__ dx16, int N,
                                                                   int CB, int D, int H, int W, int64_t dybs, int64_t dxbs,
                                                                   int* __restrict__ oflag) {
  using hx8 = typename H16<HT>::x8;
  bool sat = false;
  const int OD = 2 * D, OH = 2 * H, OW = 2 * W;
  const int64_t S = (int64_t)D * H * W;
  const int64_t total = (int64_t)N * CB * S;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll) {
    const UpIdx v = up_split(i, W, H, D, CB);
    const hx8* dp = reinterpret_cast<const hx8*>(dy16 + (int64_t)v.n * dybs) + (int64_t)v.c * S * 8;
    int ox[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) ox[k] = clampi(2 * v.x - 1 + k, OW - 1);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kz = 0; kz < 4; ++kz) {
      const int oz = clampi(2 * v.z - 1 + kz, OD - 1);
#pragma unroll
      for (int ky = 0; ky < 4; ++ky) {
        const hx8* row = dp + ((int64_t)oz * OH + clampi(2 * v.y - 1 + ky, OH - 1)) * OW;
        const float wzy = hp_tap_weight(kz) * hp_tap_weight(ky);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const hx8 g = row[ox[k]];
          const float w = wzy * hp_tap_weight(k);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] = fmaf(w, (float)g[j], acc[j]);
        }
      }
    }
    hx8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = to_h16_sat<HT>(acc[j], sat);
    (reinterpret_cast<hx8*>(dx16 + (int64_t)v.n * dxbs) + (int64_t)v.c * S)[((int64_t)v.z * H + v.y) * W + v.x] = o;
  }
  report_saturation(sat, oflag);
}

}  // namespace m355

using namespace m355;

// one body for the four fp32 entry points: `a` reads, `b` is written (forward: x, y; backward: dy, dx)
static int upsample2x_fp32(ResampleOp op, const float* a, float* b, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                           int64_t abs_, int64_t bbs, void* stream) {
  const ResampleArgs args = {N, C, D, H, W, 0, {abs_, bbs, 0}, {(uintptr_t)a, (uintptr_t)b, 0, 0}};
  if (int rc = validate_resample(op, args)) return rc;
  const ResamplePlan p = plan_resample(op, args);
  const hipStream_t st = (hipStream_t)stream;
  with_bool(p.variant == RS_VECTOR, [&](auto V) {
    constexpr bool vec = decltype(V)::value;
    switch (op) {
      case RS_NEAR_FWD: hipLaunchKernelGGL(nearest2_fwd_kernel<vec>, p.grid, dim3(256), 0, st, a, b, N, C, D, H, W, p.bs[0], p.bs[1]); break;
      case RS_NEAR_BWD: hipLaunchKernelGGL(nearest2_bwd_kernel<vec>, p.grid, dim3(256), 0, st, a, b, N, C, D, H, W, p.bs[0], p.bs[1]); break;
      case RS_HP_FWD: hipLaunchKernelGGL(trilinear2_hp_fwd_kernel<vec>, p.grid, dim3(256), 0, st, a, b, N, C, D, H, W, p.bs[0], p.bs[1]); break;
      default: hipLaunchKernelGGL(trilinear2_hp_bwd_kernel<vec>, p.grid, dim3(256), 0, st, a, b, N, C, D, H, W, p.bs[0], p.bs[1]);
    }
  });
  return check_launch(RESAMPLE_ROWS[op].name);
}

static int upsample2x_c8(ResampleOp op, const void* a, void* b, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                         int64_t abs_, int64_t bbs, int32_t compute, void* stream) {
  const ResampleArgs args = {N, C, D, H, W, compute, {abs_, bbs, 0}, {(uintptr_t)a, (uintptr_t)b, 0, 0}};
  if (int rc = validate_resample(op, args)) return rc;
  const ResamplePlan p = plan_resample(op, args);
  const hipStream_t st = (hipStream_t)stream;
  const int CB = (int)c8_blocks(C);
  with_h16(compute, [&](auto T) {
    typedef typename decltype(T)::type HT;
    const HT* src = (const HT*)a;
    HT* dst = (HT*)b;
    switch (op) {
      case RS_NEAR_FWD_H16: hipLaunchKernelGGL(nearest2_fwd_c8_kernel<HT>, p.grid, dim3(256), 0, st, src, dst, N, CB, D, H, W, p.bs[0], p.bs[1]); break;
      case RS_NEAR_BWD_H16: hipLaunchKernelGGL(nearest2_bwd_c8_kernel<HT>, p.grid, dim3(256), 0, st, src, dst, N, CB, D, H, W, p.bs[0], p.bs[1], overflow_flag()); break;
      case RS_HP_FWD_H16: hipLaunchKernelGGL(trilinear2_hp_fwd_c8_kernel<HT>, p.grid, dim3(256), 0, st, src, dst, N, CB, D, H, W, p.bs[0], p.bs[1]); break;
      default: hipLaunchKernelGGL(trilinear2_hp_bwd_c8_kernel<HT>, p.grid, dim3(256), 0, st, src, dst, N, CB, D, H, W, p.bs[0], p.bs[1], overflow_flag());
    }
  });
  return check_launch(RESAMPLE_ROWS[op].name);
}

#define M355_UPSAMPLE2X_FP32(name, op)                                                                                      \
  extern "C" int name(const float* a, float* b, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W, int64_t a_batch_stride, \
                      int64_t b_batch_stride, void* stream) {                                                               \
    return upsample2x_fp32(op, a, b, N, C, D, H, W, a_batch_stride, b_batch_stride, stream);                                \
  }
#define M355_UPSAMPLE2X_C8(name, op)                                                                                        \
  extern "C" int name(const void* a, void* b, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W, int64_t a_batch_stride,  \
                      int64_t b_batch_stride, int32_t compute, void* stream) {                                              \
    return upsample2x_c8(op, a, b, N, C, D, H, W, a_batch_stride, b_batch_stride, compute, stream);                         \
  }
M355_UPSAMPLE2X_FP32(m355_upsample_nearest2x_fwd, RS_NEAR_FWD)
M355_UPSAMPLE2X_FP32(m355_upsample_nearest2x_bwd, RS_NEAR_BWD)
M355_UPSAMPLE2X_FP32(m355_upsample_trilinear2x_hp_fwd, RS_HP_FWD)
M355_UPSAMPLE2X_FP32(m355_upsample_trilinear2x_hp_bwd, RS_HP_BWD)
M355_UPSAMPLE2X_C8(m355_upsample_nearest2x_fwd_h16, RS_NEAR_FWD_H16)
M355_UPSAMPLE2X_C8(m355_upsample_nearest2x_bwd_h16, RS_NEAR_BWD_H16)
M355_UPSAMPLE2X_C8(m355_upsample_trilinear2x_hp_fwd_h16, RS_HP_FWD_H16)
M355_UPSAMPLE2X_C8(m355_upsample_trilinear2x_hp_bwd_h16, RS_HP_BWD_H16)

// how entry point (mode, direction, c8) would serve this call: the same checks, the same code, no launch
extern "C" int m355_upsample2x_plan(int32_t mode, int32_t direction, int32_t c8, int32_t N, int32_t C, int32_t D, int32_t H,
                                    int32_t W, const int64_t* strides3, const uint64_t* pointers4, int32_t compute,
                                    int64_t* out8) {
  M355_REQUIRE(strides3 && pointers4 && out8, M355_EINVALID_ARG, "upsample2x_plan: null pointer");
  M355_REQUIRE((mode == 0 || mode == 1) && (direction == 0 || direction == 1) && (c8 == 0 || c8 == 1), M355_EINVALID_ARG,
               "upsample2x_plan: no entry point (mode %d, direction %d, c8 %d)", mode, direction, c8);
  return resample_plan_query((ResampleOp)(RS_NEAR_FWD + 4 * c8 + 2 * mode + direction), N, C, D, H, W, strides3, pointers4,
                             compute, out8);
}
