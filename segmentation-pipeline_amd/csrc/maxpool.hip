// nn.MaxPool3d(kernel_size=2, stride=2): forward with a route byte per pooled element, backward as a pure gather --
// fp32 NCDHW and the c8 layout of the 16-bit flows (h16.hpp).  HBM-bound, grid-stride, one pass each.
//
// Reference op replaced: downsample_class=nn.MaxPool3d of ModularUNet (models/modular_unet.py:22,56-65,92).
//
// Semantics are torch's (aten/src/ATen/native/cpu/MaxPoolKernel.cpp, identical on its device path): the window is
// scanned in (d, h, w) order from max = -inf, index = first element, with the update rule `v > max || isnan(v)`.
// Hence a tie goes to the FIRST maximum, a window that holds a NaN returns NaN and routes to its LAST NaN, an
// all -inf window routes to element 0, and [-0.0, +0.0, ...] returns -0.0.  The output is the selected element's
// bits.  The route is the window position 0..7 = (dd * 2 + dh) * 2 + dw, one uint8 per pooled element; the backward
// reads it instead of x, writes every dx element exactly once and needs no atomics.
#include "resample_host.hpp"

namespace m355 {

__device__ __forceinline__ void mp_scan(float v, int q, float& m, int& k) {
  if (v > m || v != v) {
    m = v;
    k = q;
  }
}

// ------------------------------------------------------------------ fp32 forward
// VEC: two outputs per thread from four 16-byte loads; needs W % 4 == 0 and the alignment the host proves.  The skip
// slice of a concat buffer whose base is only 4- or 8-byte aligned takes the scalar path.
template <bool VEC>
__global__ __launch_bounds__(256) void maxpool2_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                           uint8_t* __restrict__ idx, int N, int C, int D, int H,
                                                           int W, int64_t xbs, int64_t ybs) {
  const int OD = D / 2, OH = H / 2, OW = W / 2;
  const int OWV = VEC ? OW / 2 : OW;
  const int64_t OS = (int64_t)OD * OH * OW;
  const int64_t total = (int64_t)N * C * OD * OH * OWV;
  const float ninf = -__builtin_huge_valf();
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll) {
    const int ox = (int)(i % OWV);
    int64_t r = i / OWV;
    const int oy = (int)(r % OH);
    r /= OH;
    const int oz = (int)(r % OD);
    r /= OD;
    const int c = (int)(r % C);
    const int n = (int)(r / C);
    const float* xp = x + (int64_t)n * xbs + (int64_t)c * D * H * W;
    float* yp = y + (int64_t)n * ybs + (int64_t)c * OS;
    const int64_t r00 = ((int64_t)(2 * oz) * H + 2 * oy) * W;
    const int64_t r01 = r00 + W, r10 = r00 + (int64_t)H * W, r11 = r10 + W;
    const int64_t ov = ((int64_t)oz * OH + oy) * OW;
    if (VEC) {
      const float4 a = *reinterpret_cast<const float4*>(xp + r00 + 4 * ox);
      const float4 b = *reinterpret_cast<const float4*>(xp + r01 + 4 * ox);
      const float4 cc = *reinterpret_cast<const float4*>(xp + r10 + 4 * ox);
      const float4 d = *reinterpret_cast<const float4*>(xp + r11 + 4 * ox);
      float m0 = ninf, m1 = ninf;
      int k0 = 0, k1 = 0;
      mp_scan(a.x, 0, m0, k0); mp_scan(a.y, 1, m0, k0); mp_scan(b.x, 2, m0, k0); mp_scan(b.y, 3, m0, k0);
      mp_scan(cc.x, 4, m0, k0); mp_scan(cc.y, 5, m0, k0); mp_scan(d.x, 6, m0, k0); mp_scan(d.y, 7, m0, k0);
      mp_scan(a.z, 0, m1, k1); mp_scan(a.w, 1, m1, k1); mp_scan(b.z, 2, m1, k1); mp_scan(b.w, 3, m1, k1);
      mp_scan(cc.z, 4, m1, k1); mp_scan(cc.w, 5, m1, k1); mp_scan(d.z, 6, m1, k1); mp_scan(d.w, 7, m1, k1);
      *reinterpret_cast<float2*>(yp + ov + 2 * ox) = make_float2(m0, m1);
      if (idx)
        *reinterpret_cast<uchar2*>(idx + ((int64_t)n * C + c) * OS + ov + 2 * ox) =
            make_uchar2((unsigned char)k0, (unsigned char)k1);
    } else {
      const int xi = 2 * ox;
      float m = ninf;
      int k = 0;
      mp_scan(xp[r00 + xi], 0, m, k); mp_scan(xp[r00 + xi + 1], 1, m, k);
      mp_scan(xp[r01 + xi], 2, m, k); mp_scan(xp[r01 + xi + 1], 3, m, k);
      mp_scan(xp[r10 + xi], 4, m, k); mp_scan(xp[r10 + xi + 1], 5, m, k);
      mp_scan(xp[r11 + xi], 6, m, k); mp_scan(xp[r11 + xi + 1], 7, m, k);
      yp[ov + ox] = m;
      if (idx) idx[((int64_t)n * C + c) * OS + ov + ox] = (uint8_t)k;
    }
  }
}

// ------------------------------------------------------------------ fp32 backward (+ skip gradient)
// one thread per x pair (VEC: per two pairs, 16-byte dx / add accesses); the pair is one window's dw = 0, 1
template <bool VEC>
__global__ __launch_bounds__(256) void maxpool2_bwd_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ idx,
                                                           const float* __restrict__ add, float* __restrict__ dx, int N,
                                                           int C, int D, int H, int W, int64_t dybs, int64_t abs_,
                                                           int64_t dxbs) {
  const int OD = D / 2, OH = H / 2, OW = W / 2;
  const int WV = VEC ? W / 4 : W / 2;
  const int64_t OS = (int64_t)OD * OH * OW;
  const int64_t total = (int64_t)N * C * D * H * WV;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll) {
    const int xv = (int)(i % WV);
    int64_t r = i / WV;
    const int iy = (int)(r % H);
    r /= H;
    const int iz = (int)(r % D);
    r /= D;
    const int c = (int)(r % C);
    const int n = (int)(r / C);
    const int q0 = ((iz & 1) * 2 + (iy & 1)) * 2;   // window position of the pair's first element
    const int64_t orow = ((int64_t)(iz / 2) * OH + iy / 2) * OW;
    const float* gp = dy + (int64_t)n * dybs + (int64_t)c * OS + orow;
    const uint8_t* kp = idx + ((int64_t)n * C + c) * OS + orow;
    const int64_t sp = (int64_t)c * D * H * W + ((int64_t)iz * H + iy) * W;
    if (VEC) {
      const float2 g = *reinterpret_cast<const float2*>(gp + 2 * xv);
      const uchar2 k = *reinterpret_cast<const uchar2*>(kp + 2 * xv);
      float4 o;
      o.x = k.x == q0 ? g.x : 0.f;
      o.y = k.x == q0 + 1 ? g.x : 0.f;
      o.z = k.y == q0 ? g.y : 0.f;
      o.w = k.y == q0 + 1 ? g.y : 0.f;
      if (add) {
        const float4 a = *reinterpret_cast<const float4*>(add + (int64_t)n * abs_ + sp + 4 * xv);
        o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w;
      }
      *reinterpret_cast<float4*>(dx + (int64_t)n * dxbs + sp + 4 * xv) = o;
    } else {
      const float g = gp[xv];
      const int k = kp[xv];
      float o0 = k == q0 ? g : 0.f, o1 = k == q0 + 1 ? g : 0.f;
      if (add) {
        const float* a = add + (int64_t)n * abs_ + sp + 2 * xv;
        o0 += a[0];
        o1 += a[1];
      }
      float* o = dx + (int64_t)n * dxbs + sp + 2 * xv;
      o[0] = o0;
      o[1] = o1;
    }
  }
}

// ------------------------------------------------------------------ c8 forward
// one thread per pooled voxel and channel block, as avgpool2_c8_kernel: eight 16-byte items in, one out, and the eight
// route bytes of the item as one 8-byte store.  The comparison runs on the 16-bit values converted to float (exact),
// the output lane is the selected element itself.  Lanes past C are written as zero (value and route).
template <typename HT>
__global__ __launch_bounds__(256) void maxpool2_c8_kernel(const HT* __restrict__ x16, HT* __restrict__ y16,
                                                          uint8_t* __restrict__ idx8, int C, int CB, int D, int H, int W,
                                                          int64_t xbs, int64_t ybs, int N) {
  using hx8 = typename H16<HT>::x8;
  const int OD = D / 2, OH = H / 2, OW = W / 2;
  const int64_t OS = (int64_t)OD * OH * OW, S = (int64_t)D * H * W;
  const int64_t total = (int64_t)N * CB * OS;
  const float ninf = -__builtin_huge_valf();
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll) {
    const int64_t ov = i % OS;
    const int64_t r = i / OS;
    const int cb = (int)(r % CB), n = (int)(r / CB);
    const int nc = min(8, C - cb * 8);
    const int ox = (int)(ov % OW), oy = (int)((ov / OW) % OH), oz = (int)(ov / ((int64_t)OW * OH));
    const hx8* src = reinterpret_cast<const hx8*>(x16 + (int64_t)n * xbs) + (int64_t)cb * S;
    hx8 v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q)
      v[q] = src[((int64_t)(2 * oz + (q >> 2)) * H + 2 * oy + ((q >> 1) & 1)) * W + 2 * ox + (q & 1)];
    hx8 o = v[0];
    float m[8];
    uint32_t k[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      m[j] = ninf;
      k[j] = 0;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = (float)v[q][j];
        const bool take = f > m[j] || f != f;
        m[j] = take ? f : m[j];
        k[j] = take ? (uint32_t)q : k[j];
        o[j] = take ? v[q][j] : o[j];
      }
    }
    uint32_t klo = 0, khi = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j >= nc) {
        o[j] = (HT)0.f;
        k[j] = 0;
      }
      if (j < 4) klo |= k[j] << (8 * j);
      else khi |= k[j] << (8 * (j - 4));
    }
    (reinterpret_cast<hx8*>(y16 + (int64_t)n * ybs) + (int64_t)cb * OS)[ov] = o;
    if (idx8) reinterpret_cast<uint2*>(idx8)[((int64_t)n * CB + cb) * OS + ov] = make_uint2(klo, khi);
  }
}

// ------------------------------------------------------------------ c8 backward (+ skip gradient)
// one thread per un-pooled voxel and channel block, as avgpool2_bwd_c8_kernel; the sum with the skip gradient is
// rounded once and saturates into the overflow word like every c8 gradient (the routing itself cannot overflow)
template <typename HT>
__global__ __launch_bounds__(256) void maxpool2_bwd_c8_kernel(const HT* __restrict__ dp16, const uint8_t* __restrict__ idx8,
                                                              const HT* __restrict__ dskip16, HT* __restrict__ dx16, int C,
                                                              int CB, int D, int H, int W, int64_t pbs16, int64_t sbs16,
                                                              int64_t xbs16, int N, int* __restrict__ oflag) {
  using hx8 = typename H16<HT>::x8;
  const int OH = H / 2, OW = W / 2;
  const int64_t S = (int64_t)D * H * W, OS = S >> 3;
  const int64_t total = (int64_t)N * CB * S;
  bool sat = false;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll) {
    const int64_t v = i % S;
    const int64_t r = i / S;
    const int cb = (int)(r % CB), n = (int)(r / CB);
    const int nc = min(8, C - cb * 8);
    const int ix = (int)(v % W), iy = (int)((v / W) % H), iz = (int)(v / ((int64_t)W * H));
    const uint32_t q = (uint32_t)(((iz & 1) * 2 + (iy & 1)) * 2 + (ix & 1));
    const int64_t ov = ((int64_t)(iz >> 1) * OH + (iy >> 1)) * OW + (ix >> 1);
    const hx8 g = (reinterpret_cast<const hx8*>(dp16 + (int64_t)n * pbs16) + (int64_t)cb * OS)[ov];
    const uint2 k = reinterpret_cast<const uint2*>(idx8)[((int64_t)n * CB + cb) * OS + ov];
    hx8 s{};
    if (dskip16) s = (reinterpret_cast<const hx8*>(dskip16 + (int64_t)n * sbs16) + (int64_t)cb * S)[v];
    hx8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t kj = ((j < 4 ? k.x : k.y) >> (8 * (j & 3))) & 0xffu;
      float f = kj == q ? (float)g[j] : 0.f;
      if (dskip16) f += (float)s[j];
      o[j] = j < nc ? to_h16_sat<HT>(f, sat) : (HT)0.f;
    }
    (reinterpret_cast<hx8*>(dx16 + (int64_t)n * xbs16) + (int64_t)cb * S)[v] = o;
  }
  report_saturation(sat, oflag);
}

}  // namespace m355

using namespace m355;

extern "C" int m355_maxpool3d_2x_fwd(const float* x, float* y, uint8_t* idx, int32_t N, int32_t C, int32_t D, int32_t H,
                                     int32_t W, int64_t x_batch_stride, int64_t y_batch_stride, void* stream) {
  const ResampleArgs a = {N, C, D, H, W, 0, {x_batch_stride, y_batch_stride, 0}, {(uintptr_t)x, (uintptr_t)y, 0, (uintptr_t)idx}};
  if (int rc = validate_resample(RS_MAX_FWD, a)) return rc;
  const ResamplePlan p = plan_resample(RS_MAX_FWD, a);
  with_bool(p.variant == RS_VECTOR, [&](auto V) {
    hipLaunchKernelGGL(maxpool2_fwd_kernel<decltype(V)::value>, p.grid, dim3(256), 0, (hipStream_t)stream, x, y, idx, N, C, D,
                       H, W, p.bs[0], p.bs[1]);
  });
  return check_launch("maxpool3d_2x_fwd");
}

extern "C" int m355_maxpool3d_2x_bwd(const float* dy, const uint8_t* idx, const float* add, float* dx, int32_t N, int32_t C,
                                     int32_t D, int32_t H, int32_t W, int64_t dy_batch_stride, int64_t add_batch_stride,
                                     int64_t dx_batch_stride, void* stream) {
  const ResampleArgs a = {N, C, D, H, W, 0, {dy_batch_stride, add_batch_stride, dx_batch_stride},
                          {(uintptr_t)dy, (uintptr_t)add, (uintptr_t)dx, (uintptr_t)idx}};
  if (int rc = validate_resample(RS_MAX_BWD, a)) return rc;
  const ResamplePlan p = plan_resample(RS_MAX_BWD, a);
  with_bool(p.variant == RS_VECTOR, [&](auto V) {
    hipLaunchKernelGGL(maxpool2_bwd_kernel<decltype(V)::value>, p.grid, dim3(256), 0, (hipStream_t)stream, dy, idx, add, dx, N,
                       C, D, H, W, p.bs[0], p.bs[1], p.bs[2]);
  });
  return check_launch("maxpool3d_2x_bwd");
}

extern "C" int m355_maxpool3d_2x_fwd_h16(const void* x16, void* y16, uint8_t* idx8, int32_t N, int32_t C, int32_t D,
                                         int32_t H, int32_t W, int64_t x16_batch_stride, int64_t y16_batch_stride,
                                         int32_t compute, void* stream) {
  const ResampleArgs a = {N, C, D, H, W, compute, {x16_batch_stride, y16_batch_stride, 0},
                          {(uintptr_t)x16, (uintptr_t)y16, 0, (uintptr_t)idx8}};
  if (int rc = validate_resample(RS_MAX_FWD_H16, a)) return rc;
  const ResamplePlan p = plan_resample(RS_MAX_FWD_H16, a);
  with_h16(compute, [&](auto T) {
    typedef typename decltype(T)::type HT;
    hipLaunchKernelGGL(maxpool2_c8_kernel<HT>, p.grid, dim3(256), 0, (hipStream_t)stream, (const HT*)x16, (HT*)y16, idx8, C,
                       (int)c8_blocks(C), D, H, W, p.bs[0], p.bs[1], N);
  });
  return check_launch("maxpool3d_2x_fwd_h16");
}

extern "C" int m355_maxpool3d_2x_bwd_h16(const void* dpool16, const uint8_t* idx8, const void* dskip16, void* dx16, int32_t N,
                                         int32_t C, int32_t D, int32_t H, int32_t W, int64_t dpool16_batch_stride,
                                         int64_t dskip16_batch_stride, int64_t dx16_batch_stride, int32_t compute,
                                         void* stream) {
  const ResampleArgs a = {N, C, D, H, W, compute, {dpool16_batch_stride, dskip16_batch_stride, dx16_batch_stride},
                          {(uintptr_t)dpool16, (uintptr_t)dskip16, (uintptr_t)dx16, (uintptr_t)idx8}};
  if (int rc = validate_resample(RS_MAX_BWD_H16, a)) return rc;
  const ResamplePlan p = plan_resample(RS_MAX_BWD_H16, a);
  with_h16(compute, [&](auto T) {
    typedef typename decltype(T)::type HT;
    hipLaunchKernelGGL(maxpool2_bwd_c8_kernel<HT>, p.grid, dim3(256), 0, (hipStream_t)stream, (const HT*)dpool16, idx8,
                       (const HT*)dskip16, (HT*)dx16, C, (int)c8_blocks(C), D, H, W, p.bs[0], p.bs[1], p.bs[2], N,
                       overflow_flag());
  });
  return check_launch("maxpool3d_2x_bwd_h16");
}
