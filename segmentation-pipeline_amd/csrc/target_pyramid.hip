// Target pyramid of deep supervision (ops.target_pyramid, criterions/deep_supervision_loss.py): one launch
// reads an fp32 target y[N, C, D, H, W] once and writes its L coarser levels, level j of size (D, H, W) / 2^j.
//
//   AREA     out_j = mean of the 2^j cube.  Level 1 is summed in registers from four rows, level j from the eight level
//            j-1 cells of its block's LDS tile -- the pairwise tree ((x0 + x1) + (y ..)) + (z ..), times 0.125.  Every
//            partial sum of a one-hot target is an integer <= 4096 and every scale a power of two: exact.
//   NEAREST  out_j[z, y, x] = y[z 2^j, y 2^j, x 2^j]: only the even rows are read, level j picks cell (0, 0, 0) of level j-1.
//
// A work-group owns whole 2^L cubes of one (n, c) plane: one cube index along z, `YC` consecutive ones along y and a chunk
// of `XT` input floats along x (a multiple of 2^L; the last chunk of a row may be shorter).  A level-1 item is 4 consecutive
// floats of a row (the last item of a row with W % 4 == 2 has 2): a 16-byte load where the address allows it, 4-byte loads
// otherwise; it yields 2 level-1 cells, stored as one 8-byte access where the address allows it.  The higher levels are a
// few per cent of the bytes; their stores are 4 bytes per lane, consecutive lanes on consecutive x.
// No atomics, one summation order whatever the alignment, no workspace: a call repeats bit for bit and can be captured.
#include "common.hpp"

namespace m355 {

constexpr int PYR_MAX_LEVELS = 4;
constexpr int PYR_ITEMS = 512;   // level-1 items a work-group aims for; one y cube of the 4-level kernel has up to 1024

struct PyrArgs {
  int64_t off[PYR_MAX_LEVELS];   // element offset of level j + 1 in `out`
  int D, H, W;
  int XT, YC;                    // chunk of a row (input floats), y cubes per work-group
  int nxc, nyg;                  // chunks per row, groups of YC y cubes
};

// widest chunk of a row per number of levels: (2^L / 2)^2 * XT / 4 level-1 items per y cube = 512, 512, 512, 1024
static inline int pyr_xt_max(int levels) { return levels == 1 ? 2048 : levels == 2 ? 512 : levels == 3 ? 128 : 64; }

__device__ __forceinline__ void pyr_load4(const float* __restrict__ p, int nv, float (&v)[4]) {
  if (nv >= 4 && ((uintptr_t)p & 15) == 0) {
    const float4 r = *reinterpret_cast<const float4*>(p);
    v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < nv ? p[j] : 0.f;
  }
}

// level J (2 <= J <= L) of the block's tile from level J - 1 in LDS; `src` rows are XT >> (J - 1) wide
template <int L, int MODE, int J>
__device__ __forceinline__ void pyr_level(const PyrArgs& a, const float* __restrict__ src, float* __restrict__ dst,
                                          float* __restrict__ out, int64_t nc, int zc, int yc0, int nyc, int x0, int xw) {
  constexpr int HJ = (1 << L) >> J, HP = HJ * 2;   // cells per cube edge at level J and at level J - 1
  const int XJ = a.XT >> J, XP = XJ * 2, xwj = xw >> J;
  const int64_t Dj = a.D >> J, Hj = a.H >> J, Wj = a.W >> J;
  const int items = nyc * HJ * HJ * xwj;
  __syncthreads();
  for (int it = threadIdx.x; it < items; it += 256) {
    const int x = it % xwj;
    int r = it / xwj;
    const int yj = r % HJ;
    r /= HJ;
    const int zj = r % HJ, yc = r / HJ;
    const float* s = src + ((yc * HP + 2 * zj) * HP + 2 * yj) * XP + 2 * x;
    float v;
    if (MODE == M355_PYRAMID_AREA) {
      const float* t = s + HP * XP;
      v = (((s[0] + s[1]) + (s[XP] + s[XP + 1])) + ((t[0] + t[1]) + (t[XP] + t[XP + 1]))) * 0.125f;
    } else {
      v = s[0];
    }
    out[a.off[J - 1] + ((nc * Dj + (zc * HJ + zj)) * Hj + ((yc0 + yc) * HJ + yj)) * Wj + (x0 >> J) + x] = v;
    if (J < L) dst[((yc * HJ + zj) * HJ + yj) * XJ + x] = v;
  }
}

template <int L, int MODE>
__global__ __launch_bounds__(256) void target_pyramid_kernel(const float* __restrict__ y, float* __restrict__ out, PyrArgs a) {
  constexpr int B = 1 << L, H1 = B / 2;   // input voxels and level-1 cells per cube edge
  // level-1, -2 and -3 tiles [y cube][z][y][x]: 2 * items, / 8, / 64 floats
  __shared__ float s1[L > 1 ? 2048 : 1];
  __shared__ float s2[L > 2 ? 256 : 1];
  __shared__ float s3[L > 3 ? 32 : 1];
  int64_t bid = blockIdx.x;
  const int xc = (int)(bid % a.nxc);
  bid /= a.nxc;
  const int yg = (int)(bid % a.nyg);
  bid /= a.nyg;
  const int zc = (int)(bid % (a.D >> L));
  const int64_t nc = bid / (a.D >> L);
  const int x0 = xc * a.XT, xw = min(a.XT, a.W - x0);
  const int yc0 = yg * a.YC, nyc = min(a.YC, (a.H >> L) - yc0);
  const int nx4 = (xw + 3) >> 2, X1 = a.XT >> 1;
  const int64_t D1 = a.D >> 1, H1g = a.H >> 1, W1 = a.W >> 1;
  const int items = nyc * H1 * H1 * nx4;
  for (int it = threadIdx.x; it < items; it += 256) {
    const int x4 = it % nx4;
    int r = it / nx4;
    const int y1 = r % H1;
    r /= H1;
    const int z1 = r % H1, yc = r / H1;
    const int nv = min(4, xw - 4 * x4);   // 4, or 2 at the end of a row with W % 4 == 2
    const int64_t zi = (int64_t)zc * B + 2 * z1, yi = (int64_t)(yc0 + yc) * B + 2 * y1;
    const float* p = y + ((nc * a.D + zi) * a.H + yi) * a.W + x0 + 4 * x4;
    float v0, v1;
    if (MODE == M355_PYRAMID_AREA) {
      float r0[4], r1[4], r2[4], r3[4];
      const float* q = p + (int64_t)a.H * a.W;
      pyr_load4(p, nv, r0);
      pyr_load4(p + a.W, nv, r1);
      pyr_load4(q, nv, r2);
      pyr_load4(q + a.W, nv, r3);
      v0 = (((r0[0] + r0[1]) + (r1[0] + r1[1])) + ((r2[0] + r2[1]) + (r3[0] + r3[1]))) * 0.125f;
      v1 = (((r0[2] + r0[3]) + (r1[2] + r1[3])) + ((r2[2] + r2[3]) + (r3[2] + r3[3]))) * 0.125f;
    } else {
      float r0[4];
      pyr_load4(p, nv, r0);
      v0 = r0[0];
      v1 = r0[2];
    }
    float* o = out + a.off[0] + ((nc * D1 + (zc * H1 + z1)) * H1g + ((yc0 + yc) * H1 + y1)) * W1 + (x0 >> 1) + 2 * x4;
    if (nv == 4 && ((uintptr_t)o & 7) == 0) {
      *reinterpret_cast<float2*>(o) = make_float2(v0, v1);
    } else {
      o[0] = v0;
      if (nv == 4) o[1] = v1;
    }
    if (L > 1) {
      float* s = s1 + ((yc * H1 + z1) * H1 + y1) * X1 + 2 * x4;
      s[0] = v0;
      if (nv == 4) s[1] = v1;
    }
  }
  if constexpr (L >= 2) pyr_level<L, MODE, 2>(a, s1, s2, out, nc, zc, yc0, nyc, x0, xw);
  if constexpr (L >= 3) pyr_level<L, MODE, 3>(a, s2, s3, out, nc, zc, yc0, nyc, x0, xw);
  if constexpr (L >= 4) pyr_level<L, MODE, 4>(a, s3, s3, out, nc, zc, yc0, nyc, x0, xw);
}

using PyrK = void (*)(const float*, float*, PyrArgs);
template <int MODE>
static PyrK pyr_kernel(int levels) {
  return levels == 1 ? target_pyramid_kernel<1, MODE> : levels == 2 ? target_pyramid_kernel<2, MODE>
         : levels == 3 ? target_pyramid_kernel<3, MODE> : target_pyramid_kernel<4, MODE>;
}

}  // namespace m355

using namespace m355;

extern "C" int64_t m355_target_pyramid_elems(int32_t N, int32_t C, int32_t D, int32_t H, int32_t W, int32_t levels) {
  if (N <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0 || levels < 1 || levels > PYR_MAX_LEVELS) return 0;
  const int m = (1 << levels) - 1;
  if ((D & m) || (H & m) || (W & m)) return 0;
  int64_t total = 0;
  for (int j = 1; j <= levels; ++j) total += (int64_t)N * C * (D >> j) * (H >> j) * (W >> j);
  return total;
}

extern "C" int m355_target_pyramid(const float* y, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W, int32_t levels,
                                   int32_t mode, float* out, void* stream) {
  M355_REQUIRE(y && out, M355_EINVALID_ARG, "target_pyramid: null pointer");
  M355_REQUIRE(N > 0 && C > 0 && D > 0 && H > 0 && W > 0, M355_EINVALID_ARG, "target_pyramid: non-positive size");
  M355_REQUIRE(levels >= 1 && levels <= PYR_MAX_LEVELS, M355_EINVALID_ARG, "target_pyramid: levels %d outside 1..%d",
               (int)levels, PYR_MAX_LEVELS);
  M355_REQUIRE(mode == M355_PYRAMID_AREA || mode == M355_PYRAMID_NEAREST, M355_EINVALID_ARG,
               "target_pyramid: mode %d is neither M355_PYRAMID_AREA (0) nor M355_PYRAMID_NEAREST (1)", (int)mode);
  const int B = 1 << levels;
  M355_REQUIRE(D % B == 0, M355_EUNSUPPORTED, "target_pyramid: D = %d is not divisible by %d (2^levels)", (int)D, B);
  M355_REQUIRE(H % B == 0, M355_EUNSUPPORTED, "target_pyramid: H = %d is not divisible by %d (2^levels)", (int)H, B);
  M355_REQUIRE(W % B == 0, M355_EUNSUPPORTED, "target_pyramid: W = %d is not divisible by %d (2^levels)", (int)W, B);
  PyrArgs a;
  int64_t off = 0;
  for (int j = 1; j <= PYR_MAX_LEVELS; ++j) {
    a.off[j - 1] = off;
    off += (int64_t)N * C * (D >> j) * (H >> j) * (W >> j);
  }
  a.D = D; a.H = H; a.W = W;
  a.XT = std::min<int>(W, pyr_xt_max(levels));
  a.nxc = (int)ceil_div(W, a.XT);
  const int per_cube = (B / 2) * (B / 2) * (int)ceil_div(a.XT, 4);   // level-1 items of one y cube: <= 1024
  a.YC = std::max(1, std::min(H / B, PYR_ITEMS / per_cube));
  a.nyg = (int)ceil_div(H / B, a.YC);
  const int64_t blocks = (int64_t)N * C * (D / B) * a.nyg * a.nxc;
  M355_REQUIRE(blocks <= 0x7fffffffll, M355_EUNSUPPORTED, "target_pyramid: %lld work-groups exceed the grid limit",
               (long long)blocks);
  const PyrK k = mode == M355_PYRAMID_AREA ? pyr_kernel<M355_PYRAMID_AREA>(levels) : pyr_kernel<M355_PYRAMID_NEAREST>(levels);
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, y, out, a);
  return check_launch("target_pyramid");
}
