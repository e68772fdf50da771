// Training augmentation on the device: the per-voxel work of the torchio chains of the reference's production configs
// (research/dmri_hippo/configs/main_config.py:86-100, research/msseg2/msseg2.py:44-57).  The random parameters are drawn
// on the host (augmentation.py); every kernel here is deterministic given them.
//
//   aug_resample_kernel   spatial transforms: output voxel p reads the input at q = M p + t + B d(p), d = cubic B-spline
//                         displacement of a control grid held in LDS; nearest / trilinear / cubic B-spline, element
//                         sizes 1 / 4 / 8 (nearest only for 1 and 8), pad value per channel from device memory
//   aug_prefilter_kernel  cubic B-spline coefficients, in place, one thread per line (scipy spline_filter, mode mirror)
//   aug_hist_kernel       exact order statistics by the radix select of radix_select.hpp: up to RADIX_Q ranks at once,
//   aug_pick_kernel       one wave of the one-workgroup pick per rank; or one min / max pass
//   aug_intensity_kernel  fused intensity program: bias field, clip + rescale, gamma, noise (Philox4x32-10)
//   aug_blur_kernel       one axis of the separable Gaussian (scipy gaussian_filter, mode reflect), program epilogue
//   aug_otsu_kernel       Otsu border pad value, one workgroup per channel
//   aug_channel_minmax_kernel  per-channel min or max (the 'minimum' pad value) of all channels in one pass
// Statistics a stage needs (percentile cutoffs, min / max) are written to device memory by the select kernels and read
// there by the kernel that applies the stage: no host round trip.  Only integer atomics: results are deterministic.
#include "radix_select.hpp"

namespace m355 {

constexpr int AUG_NT = 256;
constexpr int AUG_MAX_GRID = 4096;       // floats of the control grid in LDS (7x7x4x3 = 588)
constexpr int RADIX_Q = 4;               // keys selected at once: floor / ceil rank of two percentiles
constexpr int OTSU_BINS = 128;
constexpr int OTSU_NT = 1024;
constexpr int BLUR_MAX_RADIUS = 512;

enum { AUG_NEAREST = 0, AUG_LINEAR = 1, AUG_BSPLINE = 2 };

struct Program {
  m355_aug_stage s[M355_AUG_MAX_STAGES];
  int n;
  int size[3];
  int64_t S;
};

// ------------------------------------------------------------------------------------------------ helpers
__device__ __forceinline__ void philox_round(uint32_t c[4], uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
  const uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
  const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
  c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
}

// standard normal of element i of the stream `seed`: Philox4x32-10 of counter (i_lo, i_hi, 0, 0), Box-Muller of words 0, 1
__device__ __forceinline__ float philox_normal(uint64_t seed, uint64_t i) {
  uint32_t c[4] = {(uint32_t)i, (uint32_t)(i >> 32), 0u, 0u};
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  const float u1 = ((float)c[0] + 1.0f) * 2.3283064365386963e-10f;   // (0, 1]
  const float u2 = (float)c[1] * 2.3283064365386963e-10f;            // [0, 1)
  return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
}

// torchio's normalised bias-field coordinate of index i on an axis of n voxels: (2i - (n - 1)) / (n - 1), 0 when n == 1
__device__ __forceinline__ float bias_coord(int i, int n) { return n > 1 ? (float)(2 * i - (n - 1)) / (float)(n - 1) : 0.f; }

// value of element i (channel c) after stages [0, upto) of the program
__device__ float run_program(float v, int64_t i, const Program& P, int upto) {
  const int64_t c = i / P.S, s = i - c * P.S;
  for (int k = 0; k < upto; ++k) {
    const m355_aug_stage& st = P.s[k];
    switch (st.op) {
      case M355_AUG_BIAS: {
        const int64_t hw = (int64_t)P.size[1] * P.size[2];
        const int z = (int)(s / hw), r = (int)(s - z * hw), y = r / P.size[2], x = r - y * P.size[2];
        const float cx = bias_coord(z, P.size[0]), cy = bias_coord(y, P.size[1]), cz = bias_coord(x, P.size[2]);
        float acc = 0.f, px = 1.f;
        int j = 0;
        for (int a = 0; a <= st.order; ++a, px *= cx) {
          float py = 1.f;
          for (int b = 0; b <= st.order - a; ++b, py *= cy) {
            float pz = 1.f;
            for (int e = 0; e <= st.order - a - b; ++e, pz *= cz) acc += st.vec[j++] * px * py * pz;
          }
        }
        v = v * expf(acc);
        break;
      }
      case M355_AUG_RESCALE: {
        const float lo = (float)st.stats[0], hi = (float)st.stats[1], rng = hi - lo;
        if (rng == 0.f) break;   // constant image: unchanged (torchio)
        v = fminf(fmaxf(v, lo), hi);
        v = __fsub_rn(v, lo);
        v = __fdiv_rn(v, rng);
        v = __fmul_rn(v, st.b - st.a);
        v = __fadd_rn(v, st.a);
        break;
      }
      case M355_AUG_GAMMA: {
        const float g = st.vec[c];
        const float m = powf(fabsf(v), g);
        v = v > 0.f ? m : v < 0.f ? -m : 0.f * m;
        break;
      }
      case M355_AUG_NOISE:
        v = v + (st.a + st.b * philox_normal(st.seed, (uint64_t)i));
        break;
      default: break;
    }
  }
  return v;
}

static unsigned grid_of(int64_t n, int64_t cap = 8192) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, AUG_NT), cap));
}

// ------------------------------------------------------------------------------------------------ resample
struct ResampleArgs {
  float m[9];        // r = m (p - cout) + t0, q = r + cin: coordinates relative to the volume centres
  float t0[3];
  float b[9];        // displacement into input index space
  float cin[3], cout[3];
  int in[3], out[3];
  int kc[3];         // control points per axis (kc[0] == 0: no displacement)
  float gscale[3];   // (K - 3) / Vout
  int C, interp, elem;
  double pad_const;
};

__device__ __forceinline__ int mirror_idx(int i, int n) {
  if (n == 1) return 0;
  const int period = 2 * n - 2;
  i = i < 0 ? -i : i;
  i %= period;
  return i >= n ? period - i : i;
}
__device__ __forceinline__ void bspline_w(float f, float w[4]) {
  const float f2 = f * f, f3 = f2 * f, g = 1.f - f;
  w[0] = g * g * g * (1.f / 6.f);
  w[1] = (3.f * f3 - 6.f * f2 + 4.f) * (1.f / 6.f);
  w[2] = (-3.f * f3 + 3.f * f2 + 3.f * f + 1.f) * (1.f / 6.f);
  w[3] = f3 * (1.f / 6.f);
}

__global__ __launch_bounds__(AUG_NT) void aug_resample_kernel(const void* __restrict__ x, void* __restrict__ y,
                                                              ResampleArgs a, const float* __restrict__ grid,
                                                              const double* __restrict__ pad) {
  extern __shared__ float lgrid[];
  const int ng = a.kc[0] * a.kc[1] * a.kc[2] * 3;
  for (int i = threadIdx.x; i < ng; i += AUG_NT) lgrid[i] = grid[i];
  __syncthreads();
  const int64_t So = (int64_t)a.out[0] * a.out[1] * a.out[2], Si = (int64_t)a.in[0] * a.in[1] * a.in[2];
  const int64_t ohw = (int64_t)a.out[1] * a.out[2];
  for (int64_t v = blockIdx.x * (int64_t)AUG_NT + threadIdx.x; v < So; v += (int64_t)gridDim.x * AUG_NT) {
    const int p0 = (int)(v / ohw), rr = (int)(v - p0 * ohw), p1 = rr / a.out[2], p2 = rr - p1 * a.out[2];
    const float d0 = p0 - a.cout[0], d1 = p1 - a.cout[1], d2 = p2 - a.cout[2];
    float r[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) r[j] = a.m[3 * j] * d0 + a.m[3 * j + 1] * d1 + a.m[3 * j + 2] * d2 + a.t0[j];
    if (ng) {
      const int p[3] = {p0, p1, p2};
      int base[3];
      float w[3][4];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float u = ((float)p[j] + 0.5f) * a.gscale[j];
        int i0 = (int)floorf(u);
        i0 = min(max(i0, 0), a.kc[j] - 4);
        base[j] = i0;
        bspline_w(u - (float)i0, w[j]);
      }
      float disp[3] = {0.f, 0.f, 0.f};
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
          const float wij = w[0][i] * w[1][j];
          const float* row = &lgrid[(((base[0] + i) * a.kc[1] + base[1] + j) * a.kc[2] + base[2]) * 3];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float wk = wij * w[2][k];
            disp[0] += wk * row[3 * k];
            disp[1] += wk * row[3 * k + 1];
            disp[2] += wk * row[3 * k + 2];
          }
        }
#pragma unroll
      for (int j = 0; j < 3; ++j) r[j] += a.b[3 * j] * disp[0] + a.b[3 * j + 1] * disp[1] + a.b[3 * j + 2] * disp[2];
    }
    float q[3];
    bool inside = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      q[j] = r[j] + a.cin[j];
      inside &= q[j] >= -0.5f && q[j] < (float)a.in[j] - 0.5f;
    }
    if (a.elem != 4 || a.interp == AUG_NEAREST) {
      int64_t src = -1;
      if (inside) {
        int id[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) id[j] = min(max((int)floorf(q[j] + 0.5f), 0), a.in[j] - 1);
        src = ((int64_t)id[0] * a.in[1] + id[1]) * a.in[2] + id[2];
      }
      for (int c = 0; c < a.C; ++c) {
        const int64_t o = c * So + v;
        if (a.elem == 1) ((uint8_t*)y)[o] = src < 0 ? (uint8_t)0 : ((const uint8_t*)x)[c * Si + src];
        else if (a.elem == 8) ((int64_t*)y)[o] = src < 0 ? (int64_t)0 : ((const int64_t*)x)[c * Si + src];
        else ((float*)y)[o] = src < 0 ? (float)(pad ? pad[c] : a.pad_const) : ((const float*)x)[c * Si + src];
      }
      continue;
    }
    const float* xf = (const float*)x;
    float* yf = (float*)y;
    if (!inside) {
      for (int c = 0; c < a.C; ++c) yf[c * So + v] = (float)(pad ? pad[c] : a.pad_const);
      continue;
    }
    if (a.interp == AUG_LINEAR) {
      int i0[3], i1[3];
      float f[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float fl = floorf(q[j]);
        f[j] = q[j] - fl;
        i0[j] = min(max((int)fl, 0), a.in[j] - 1);
        i1[j] = min(max((int)fl + 1, 0), a.in[j] - 1);
      }
      const int64_t h = a.in[2], dz = (int64_t)a.in[1] * a.in[2];
      for (int c = 0; c < a.C; ++c) {
        const float* xc = xf + c * Si;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
              const float w = (i ? f[0] : 1.f - f[0]) * (j ? f[1] : 1.f - f[1]) * (k ? f[2] : 1.f - f[2]);
              acc += w * xc[(i ? i1[0] : i0[0]) * dz + (j ? i1[1] : i0[1]) * h + (k ? i1[2] : i0[2])];
            }
        yf[c * So + v] = acc;
      }
    } else {
      int id[3][4];
      float w[3][4];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float fl = floorf(q[j]);
        bspline_w(q[j] - fl, w[j]);
#pragma unroll
        for (int k = 0; k < 4; ++k) id[j][k] = mirror_idx((int)fl - 1 + k, a.in[j]);
      }
      const int64_t h = a.in[2], dz = (int64_t)a.in[1] * a.in[2];
      for (int c = 0; c < a.C; ++c) {
        const float* xc = xf + c * Si;
        float acc = 0.f;
        for (int i = 0; i < 4; ++i)
          for (int j = 0; j < 4; ++j) {
            const float* row = xc + id[0][i] * dz + id[1][j] * h;
            const float wij = w[0][i] * w[1][j];
            acc += wij * (w[2][0] * row[id[2][0]] + w[2][1] * row[id[2][1]] + w[2][2] * row[id[2][2]] +
                          w[2][3] * row[id[2][3]]);
          }
        yf[c * So + v] = acc;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ B-spline prefilter
// scipy ni_splines.c for order 3 (one pole z = sqrt(3) - 2), mirror boundary: exact causal initialisation over the line
__global__ __launch_bounds__(AUG_NT) void aug_prefilter_kernel(float* __restrict__ x, int C, int D, int H, int W, int axis) {
  const int n = axis == 0 ? D : axis == 1 ? H : W;
  const int64_t stride = axis == 0 ? (int64_t)H * W : axis == 1 ? W : 1;
  const int64_t lines = (int64_t)C * D * H * W / n;
  const float z = -0.2679491924311228f;   // sqrt(3) - 2
  const float gain = (1.f - z) * (1.f - 1.f / z);
  for (int64_t l = blockIdx.x * (int64_t)AUG_NT + threadIdx.x; l < lines; l += (int64_t)gridDim.x * AUG_NT) {
    int64_t base;
    if (axis == 0) {
      const int64_t hw = (int64_t)H * W, c = l / hw;
      base = c * D * hw + (l - c * hw);
    } else if (axis == 1) {
      const int64_t c = l / ((int64_t)D * W), r = l - c * D * W, zz = r / W;
      base = (c * D + zz) * (int64_t)H * W + (r - zz * W);
    } else {
      base = l * W;
    }
    float* p = x + base;
    for (int i = 0; i < n; ++i) p[i * stride] *= gain;
    // causal init (mirror)
    const float zn1 = powf(z, (float)(n - 1));
    float c0 = p[0] + zn1 * p[(n - 1) * stride];
    float zi = z;
    for (int i = 1; i < n - 1; ++i) {
      c0 += zi * (p[i * stride] + zn1 * p[(n - 1 - i) * stride]);
      zi *= z;
    }
    c0 /= 1.f - zn1 * zn1;
    p[0] = c0;
    float prev = c0;
    for (int i = 1; i < n; ++i) {
      prev = p[i * stride] + z * prev;
      p[i * stride] = prev;
    }
    // anticausal init (mirror)
    float last = (z * p[(n - 2) * stride] + p[(n - 1) * stride]) * z / (z * z - 1.f);
    p[(n - 1) * stride] = last;
    for (int i = n - 2; i >= 0; --i) {
      last = z * (last - p[i * stride]);
      p[i * stride] = last;
    }
  }
}

// ------------------------------------------------------------------------------------------------ order statistics
// workspace: RadixState, then hist[RADIX_Q][RADIX_BINS] (uint32)
struct RadixState {
  uint32_t prefix[RADIX_Q];
  uint32_t rank[RADIX_Q];    // rank still to find inside the current prefix bucket
  uint32_t minmax[2];        // max(~key), max(key)
  uint32_t pad[6];
};
constexpr size_t RADIX_WS = sizeof(RadixState) + sizeof(uint32_t) * RADIX_Q * RADIX_BINS;

// max of two keys over the workgroup (AUG_NT threads), result in thread 0: one global atomic per workgroup, since
// same-address atomics from every wave serialise
__device__ __forceinline__ void block_max2(uint32_t& a, uint32_t& b) {
  __shared__ uint32_t red[2][AUG_NT / 64];
  for (int off = 32; off > 0; off >>= 1) {
    a = max(a, (uint32_t)__shfl_xor((int)a, off, 64));
    b = max(b, (uint32_t)__shfl_xor((int)b, off, 64));
  }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < AUG_NT / 64; ++w) { a = max(a, red[0][w]); b = max(b, red[1][w]); }
}

// pass < 0: min / max only.  pass 0..2: digit `pass` of every key whose higher digits equal prefix[j]
__global__ __launch_bounds__(AUG_NT) void aug_hist_kernel(const float* __restrict__ x, int64_t n, Program P, int upto,
                                                          int pass, int nq, RadixState* __restrict__ st,
                                                          uint32_t* __restrict__ hist) {
  __shared__ uint32_t lh[RADIX_Q][RADIX_BINS];
  const RadixDigit dg = radix_digit(pass);
  if (pass >= 0) {
    radix_hist_clear<AUG_NT>(&lh[0][0], RADIX_Q * RADIX_BINS);
    __syncthreads();
  }
  uint32_t pre[RADIX_Q];
  for (int j = 0; j < RADIX_Q; ++j) pre[j] = pass > 0 && j < nq ? st->prefix[j] >> dg.upper : 0u;
  uint32_t kmin = 0u, kmax = 0u;
  for (int64_t i = blockIdx.x * (int64_t)AUG_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * AUG_NT) {
    const uint32_t key = f2key(run_program(x[i], i, P, upto));
    if (pass < 0) {
      kmin = max(kmin, ~key);
      kmax = max(kmax, key);
      continue;
    }
    const uint32_t hi = pass == 0 ? 0u : key >> dg.upper;
    const uint32_t d = radix_digit_of(key, dg);
    for (int j = 0; j < nq; ++j)
      if (hi == pre[j]) atomicAdd(&lh[j][d], 1u);
  }
  if (pass < 0) {
    block_max2(kmin, kmax);
    if (threadIdx.x == 0) {
      atomicMax(&st->minmax[0], kmin);
      atomicMax(&st->minmax[1], kmax);
    }
    return;
  }
  __syncthreads();
  radix_hist_flush<AUG_NT>(&lh[0][0], hist, nq * RADIX_BINS);
}

// numpy's _lerp: a + (b - a) t, or b - (b - a)(1 - t) when t >= 0.5
__device__ __forceinline__ double np_lerp(double a, double b, double t) {
  const double d = b - a;
  return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}

struct PickArgs {
  int64_t ks[RADIX_Q / 2];
  double fr[RADIX_Q / 2];
};

// one workgroup, one wave per query: find the bucket of rank[j], extend prefix[j], clear the histogram.  After the last
// pass out[q] = lerp(key(ks[q]), key(ks[q] + 1), fr[q]).
__global__ __launch_bounds__(AUG_NT) void aug_pick_kernel(int pass, int nq, RadixState* __restrict__ st,
                                                          uint32_t* __restrict__ hist, PickArgs pa, double* out,
                                                          int nout) {
  const int w = threadIdx.x >> 6;
  if (w < nq) {
    uint32_t digit, rest;
    if (radix_pick_wave(hist + w * RADIX_BINS, st->rank[w], digit, rest)) {   // exactly one lane
      st->prefix[w] |= digit << radix_digit(pass).shift;
      st->rank[w] = rest;
    }
  }
  __syncthreads();
  radix_hist_clear<AUG_NT>(hist, nq * RADIX_BINS);
  if (pass == 2 && threadIdx.x == 0) {
    for (int q = 0; q < nout; ++q)
      out[q] = np_lerp((double)key2f(st->prefix[2 * q]), (double)key2f(st->prefix[2 * q + 1]), pa.fr[q]);
  }
}

struct Ranks {
  uint32_t r[RADIX_Q];
};
__global__ void aug_rank_init_kernel(RadixState* st, Ranks r) {
  for (int j = 0; j < RADIX_Q; ++j) st->rank[j] = r.r[j];
}

__global__ void aug_minmax_out_kernel(const RadixState* st, double* out, int want_min, int want_max) {
  int o = 0;
  if (want_min) out[o++] = (double)key2f(~st->minmax[0]);
  if (want_max) out[o++] = (double)key2f(st->minmax[1]);
}

// per-channel min / max: grid (blocks per channel, C); keys[c] = {max(~key), max(key)} (zeroed), then out[c] = min or max
__global__ __launch_bounds__(AUG_NT) void aug_channel_minmax_kernel(const float* __restrict__ x, int64_t S,
                                                                    uint32_t* __restrict__ keys) {
  const int c = blockIdx.y;
  const float* xc = x + (int64_t)c * S;
  uint32_t kmin = 0u, kmax = 0u;
  for (int64_t i = blockIdx.x * (int64_t)AUG_NT + threadIdx.x; i < S; i += (int64_t)gridDim.x * AUG_NT) {
    const uint32_t key = f2key(xc[i]);
    kmin = max(kmin, ~key);
    kmax = max(kmax, key);
  }
  block_max2(kmin, kmax);
  if (threadIdx.x == 0) {
    atomicMax(&keys[2 * c], kmin);
    atomicMax(&keys[2 * c + 1], kmax);
  }
}

__global__ void aug_channel_minmax_out_kernel(const uint32_t* __restrict__ keys, int C, int which, double* __restrict__ out) {
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < C; c += gridDim.x * blockDim.x)
    out[c] = which == 0 ? (double)key2f(~keys[2 * c]) : (double)key2f(keys[2 * c + 1]);
}

// ------------------------------------------------------------------------------------------------ intensity program
// x == y is allowed (in place): every thread reads and writes only its own elements, so no __restrict__
__global__ __launch_bounds__(AUG_NT) void aug_intensity_kernel(const float* x, float* y, int64_t n,
                                                               Program P) {
  for (int64_t i = blockIdx.x * (int64_t)AUG_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * AUG_NT)
    y[i] = run_program(x[i], i, P, P.n);
}

// ------------------------------------------------------------------------------------------------ Gaussian blur
__device__ __forceinline__ int reflect_idx(int i, int n) {   // scipy 'reflect' (d c b a | a b c d | d c b a), repeated
  const int period = 2 * n;
  i %= period;
  if (i < 0) i += period;
  return i >= n ? period - 1 - i : i;
}

__global__ __launch_bounds__(AUG_NT) void aug_blur_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n,
                                                          int axis, float sigma, int radius, Program P) {
  __shared__ float wts[2 * BLUR_MAX_RADIUS + 1];
  __shared__ double tot;
  if (threadIdx.x == 0) {   // normalise in a fixed order
    double s = 0.0;
    for (int k = 0; k <= 2 * radius; ++k) s += exp(-0.5 / ((double)sigma * sigma) * (double)(k - radius) * (k - radius));
    tot = s;
  }
  __syncthreads();
  for (int k = threadIdx.x; k <= 2 * radius; k += AUG_NT) {
    const double d = k - radius;
    wts[k] = (float)(exp(-0.5 / ((double)sigma * sigma) * d * d) / tot);
  }
  __syncthreads();
  const int len = P.size[axis];
  const int64_t stride = axis == 0 ? (int64_t)P.size[1] * P.size[2] : axis == 1 ? P.size[2] : 1;
  for (int64_t i = blockIdx.x * (int64_t)AUG_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * AUG_NT) {
    const int pos = (int)((i / stride) % len);
    const float* line = x + (i - pos * stride);
    float acc = 0.f;
    for (int k = -radius; k <= radius; ++k) acc += wts[k + radius] * line[reflect_idx(pos + k, len) * stride];
    y[i] = run_program(acc, i, P, P.n);
  }
}

// ------------------------------------------------------------------------------------------------ Otsu pad value
// face voxels in torchio's order (x[0], x[-1], x[:,0], x[:,-1], x[:,:,0], x[:,:,-1]; edges and corners repeat)
__device__ __forceinline__ float face_voxel(const float* xc, int D, int H, int W, int64_t f) {
  const int64_t hw = (int64_t)H * W, dw = (int64_t)D * W;
  int z, yy, xx;
  if (f < 2 * hw) { z = f < hw ? 0 : D - 1; f %= hw; yy = (int)(f / W); xx = (int)(f % W); }
  else if ((f -= 2 * hw) < 2 * dw) { yy = f < dw ? 0 : H - 1; f %= dw; z = (int)(f / W); xx = (int)(f % W); }
  else { f -= 2 * dw; const int64_t dh = (int64_t)D * H; xx = f < dh ? 0 : W - 1; f %= dh; z = (int)(f / H); yy = (int)(f % H); }
  return xc[((int64_t)z * H + yy) * W + xx];
}

__global__ __launch_bounds__(OTSU_NT) void aug_otsu_kernel(const float* __restrict__ x, int D, int H, int W,
                                                           double* __restrict__ pad) {
  __shared__ uint32_t hist[OTSU_BINS];
  __shared__ float red[2][OTSU_NT / 64];
  __shared__ double dred[2][OTSU_NT / 64];
  __shared__ int best;
  const int c = blockIdx.x;
  const float* xc = x + (int64_t)c * D * H * W;
  const int64_t nf = 2 * ((int64_t)H * W + (int64_t)D * W + (int64_t)D * H);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float mn = INFINITY, mx = -INFINITY;
  for (int64_t f = threadIdx.x; f < nf; f += OTSU_NT) {
    const float v = face_voxel(xc, D, H, W, f);
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  for (int off = 32; off > 0; off >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, off, 64));
    mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  }
  if (lane == 0) { red[0][wv] = mn; red[1][wv] = mx; }
  for (int i = threadIdx.x; i < OTSU_BINS; i += OTSU_NT) hist[i] = 0u;
  __syncthreads();
  mn = red[0][0]; mx = red[1][0];
  for (int i = 1; i < OTSU_NT / 64; ++i) { mn = fminf(mn, red[0][i]); mx = fmaxf(mx, red[1][i]); }
  const float scale = mx > mn ? (float)OTSU_BINS / (mx - mn) : 0.f;
  for (int64_t f = threadIdx.x; f < nf; f += OTSU_NT) {
    const int b = max(0, min((int)((face_voxel(xc, D, H, W, f) - mn) * scale), OTSU_BINS - 1));
    atomicAdd(&hist[b], 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0) {   // maximise the between-class variance over the split after bin t (bin centres)
    double tot = 0.0, totm = 0.0;
    for (int b = 0; b < OTSU_BINS; ++b) { tot += hist[b]; totm += hist[b] * (b + 0.5); }
    double w0 = 0.0, m0 = 0.0, bv = -1.0;
    int bt = OTSU_BINS - 1;
    for (int t = 0; t < OTSU_BINS - 1; ++t) {
      w0 += hist[t];
      m0 += hist[t] * (t + 0.5);
      const double w1 = tot - w0;
      if (w0 == 0.0 || w1 == 0.0) continue;
      const double d = m0 / w0 - (totm - m0) / w1;
      const double var = w0 * w1 * d * d;
      if (var > bv) { bv = var; bt = t; }
    }
    best = bt;
  }
  __syncthreads();
  const int bt = best;
  double s_lo = 0.0, n_lo = 0.0, s_all = 0.0;
  for (int64_t f = threadIdx.x; f < nf; f += OTSU_NT) {
    const float v = face_voxel(xc, D, H, W, f);
    const int b = max(0, min((int)((v - mn) * scale), OTSU_BINS - 1));
    s_all += v;
    if (b <= bt && bt < OTSU_BINS - 1) { s_lo += v; n_lo += 1.0; }
  }
  for (int off = 32; off > 0; off >>= 1) {
    s_lo += __shfl_xor(s_lo, off, 64);
    n_lo += __shfl_xor(n_lo, off, 64);
    s_all += __shfl_xor(s_all, off, 64);
  }
  __syncthreads();
  if (lane == 0) { dred[0][wv] = s_lo; dred[1][wv] = s_all; red[0][wv] = (float)n_lo; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0, k = 0.0;
    for (int i = 0; i < OTSU_NT / 64; ++i) { a += dred[0][i]; b += dred[1][i]; k += red[0][i]; }
    pad[c] = k > 0.0 ? a / k : b / (double)nf;
  }
}

// ------------------------------------------------------------------------------------------------ host side
static int check_size3(const char* who, const int32_t* s) {
  M355_REQUIRE(s, M355_EINVALID_ARG, "%s: null size", who);
  M355_REQUIRE(s[0] > 0 && s[1] > 0 && s[2] > 0, M355_EINVALID_ARG, "%s: non-positive size %d x %d x %d", who, s[0],
               s[1], s[2]);
  M355_REQUIRE((int64_t)s[0] * s[1] * s[2] < ((int64_t)1 << 31), M355_EINVALID_ARG,
               "%s: %d x %d x %d has 2^31 voxels or more", who, s[0], s[1], s[2]);
  return M355_OK;
}

static int make_program(const char* who, Program& P, const m355_aug_stage* stages, int32_t nstages, int32_t C,
                        const int32_t* size3) {
  M355_REQUIRE(nstages >= 0 && nstages <= M355_AUG_MAX_STAGES, M355_EINVALID_ARG, "%s: %d stages (0 .. %d)", who, nstages,
               M355_AUG_MAX_STAGES);
  M355_REQUIRE(nstages == 0 || stages, M355_EINVALID_ARG, "%s: null stage list", who);
  P = Program{};
  P.n = nstages;
  for (int j = 0; j < 3; ++j) P.size[j] = size3[j];
  P.S = (int64_t)size3[0] * size3[1] * size3[2];
  for (int k = 0; k < nstages; ++k) {
    const m355_aug_stage& s = stages[k];
    switch (s.op) {
      case M355_AUG_BIAS:
        M355_REQUIRE(s.vec && s.order >= 0 && s.order <= 8, M355_EINVALID_ARG,
                     "%s: stage %d: bias field needs coefficients and an order in 0 .. 8", who, k);
        break;
      case M355_AUG_RESCALE:
        M355_REQUIRE(s.stats, M355_EINVALID_ARG, "%s: stage %d: rescale needs its statistics", who, k);
        break;
      case M355_AUG_GAMMA:
        M355_REQUIRE(s.vec, M355_EINVALID_ARG, "%s: stage %d: gamma needs per-channel exponents", who, k);
        break;
      case M355_AUG_NOISE: break;
      default: M355_REQUIRE(false, M355_EINVALID_ARG, "%s: stage %d: unknown op %d", who, k, s.op);
    }
    P.s[k] = s;
  }
  (void)C;
  return M355_OK;
}

}  // namespace m355

using namespace m355;

extern "C" int m355_aug_resample(const void* x, void* y, int32_t C, const int32_t* in3, const int32_t* out3,
                                 int32_t elem_bytes, int32_t interp, const double* mat12, const double* disp9,
                                 const float* grid, const int32_t* grid3, const double* pad, double pad_const,
                                 void* stream) {
  if (int rc = check_size3("aug_resample: input", in3)) return rc;
  if (int rc = check_size3("aug_resample: output", out3)) return rc;
  M355_REQUIRE(x && y && mat12 && x != y, M355_EINVALID_ARG, "aug_resample: null pointer, or x == y");
  M355_REQUIRE(C > 0 && (int64_t)C * in3[0] * in3[1] * in3[2] < ((int64_t)1 << 40), M355_EINVALID_ARG,
               "aug_resample: %d channels", C);
  M355_REQUIRE(elem_bytes == 1 || elem_bytes == 4 || elem_bytes == 8, M355_EINVALID_ARG,
               "aug_resample: element size %d not in {1, 4, 8}", elem_bytes);
  M355_REQUIRE(interp >= AUG_NEAREST && interp <= AUG_BSPLINE, M355_EINVALID_ARG, "aug_resample: interpolation %d",
               interp);
  M355_REQUIRE(elem_bytes == 4 || interp == AUG_NEAREST, M355_EINVALID_ARG,
               "aug_resample: %d-byte elements are labels: nearest interpolation only", elem_bytes);
  ResampleArgs a{};
  a.C = C; a.interp = interp; a.elem = elem_bytes; a.pad_const = pad_const;
  for (int j = 0; j < 3; ++j) {
    a.in[j] = in3[j]; a.out[j] = out3[j];
    a.cin[j] = (float)(0.5 * (in3[j] - 1));
    a.cout[j] = (float)(0.5 * (out3[j] - 1));
  }
  for (int j = 0; j < 3; ++j) {   // t0 = M cout + t - cin, in double
    double t = mat12[4 * j + 3] - 0.5 * (in3[j] - 1);
    for (int k = 0; k < 3; ++k) {
      a.m[3 * j + k] = (float)mat12[4 * j + k];
      t += mat12[4 * j + k] * 0.5 * (out3[k] - 1);
    }
    a.t0[j] = (float)t;
    for (int k = 0; k < 3; ++k) a.b[3 * j + k] = disp9 ? (float)disp9[3 * j + k] : (j == k ? 1.f : 0.f);
  }
  size_t lds = 0;
  if (grid) {
    M355_REQUIRE(grid3 && grid3[0] >= 4 && grid3[1] >= 4 && grid3[2] >= 4, M355_EINVALID_ARG,
                 "aug_resample: a control grid needs >= 4 points per axis");
    const int64_t ng = (int64_t)grid3[0] * grid3[1] * grid3[2] * 3;
    M355_REQUIRE(ng <= AUG_MAX_GRID, M355_EINVALID_ARG, "aug_resample: control grid of %lld floats > %d", (long long)ng,
                 AUG_MAX_GRID);
    for (int j = 0; j < 3; ++j) {
      a.kc[j] = grid3[j];
      a.gscale[j] = (float)((double)(grid3[j] - 3) / out3[j]);
    }
    lds = (size_t)ng * sizeof(float);
  }
  const int64_t So = (int64_t)out3[0] * out3[1] * out3[2];
  hipLaunchKernelGGL(aug_resample_kernel, dim3(grid_of(So)), dim3(AUG_NT), lds, (hipStream_t)stream, x, y, a, grid, pad);
  return check_launch("aug_resample");
}

extern "C" int m355_aug_prefilter(float* x, int32_t C, const int32_t* size3, void* stream) {
  if (int rc = check_size3("aug_prefilter", size3)) return rc;
  M355_REQUIRE(x && C > 0, M355_EINVALID_ARG, "aug_prefilter: null pointer or %d channels", C);
  const int64_t nvox = (int64_t)C * size3[0] * size3[1] * size3[2];
  for (int axis = 0; axis < 3; ++axis) {
    if (size3[axis] < 2) continue;   // a one-voxel line is its own coefficient
    hipLaunchKernelGGL(aug_prefilter_kernel, dim3(grid_of(nvox / size3[axis])), dim3(AUG_NT), 0, (hipStream_t)stream, x,
                       C, size3[0], size3[1], size3[2], axis);
  }
  return check_launch("aug_prefilter");
}

extern "C" size_t m355_aug_workspace(void) { return RADIX_WS; }

extern "C" int m355_aug_order_stats(const float* x, int32_t C, const int32_t* size3, const m355_aug_stage* stages,
                                    int32_t nstages, int32_t nq, const int64_t* ks, const double* fracs, double* out,
                                    void* workspace, size_t ws_bytes, void* stream) {
  if (int rc = check_size3("aug_order_stats", size3)) return rc;
  M355_REQUIRE(x && out && ks && fracs && workspace && C > 0, M355_EINVALID_ARG, "aug_order_stats: null pointer");
  M355_REQUIRE(nq == 1 || nq == 2, M355_EINVALID_ARG, "aug_order_stats: %d queries (1 or 2)", nq);
  M355_REQUIRE(ws_bytes >= RADIX_WS, M355_EWORKSPACE, "aug_order_stats: workspace %zu < %zu bytes", ws_bytes, RADIX_WS);
  Program P;
  if (int rc = make_program("aug_order_stats", P, stages, nstages, C, size3)) return rc;
  const int64_t n = (int64_t)C * P.S;
  M355_REQUIRE(n < ((int64_t)1 << 32), M355_EINVALID_ARG, "aug_order_stats: %lld values (ranks are 32-bit)", (long long)n);
  PickArgs pa{};
  for (int q = 0; q < nq; ++q) {
    M355_REQUIRE(ks[q] >= 0 && ks[q] < n && fracs[q] >= 0.0 && fracs[q] <= 1.0, M355_EINVALID_ARG,
                 "aug_order_stats: rank %lld / fraction %g outside [0, %lld) x [0, 1]", (long long)ks[q], fracs[q],
                 (long long)n);
    pa.ks[q] = ks[q];
    pa.fr[q] = fracs[q];
  }
  hipStream_t st = (hipStream_t)stream;
  RadixState* rs = (RadixState*)workspace;
  uint32_t* hist = (uint32_t*)((char*)workspace + sizeof(RadixState));
  if (hipMemsetAsync(workspace, 0, RADIX_WS, st) != hipSuccess) return check_launch("aug_order_stats: memset");
  const unsigned grid = grid_of(n, 2048);
  bool minmax = true;   // ranks 0 and n-1 only, no interpolation: one min / max pass
  for (int q = 0; q < nq; ++q) minmax &= (ks[q] == 0 || ks[q] == n - 1) && fracs[q] == 0.0;
  if (minmax) {
    hipLaunchKernelGGL(aug_hist_kernel, dim3(grid), dim3(AUG_NT), 0, st, x, n, P, P.n, -1, 0, rs, hist);
    if (nq == 2 && ks[0] == 0 && ks[1] == n - 1) {
      hipLaunchKernelGGL(aug_minmax_out_kernel, dim3(1), dim3(1), 0, st, rs, out, 1, 1);
    } else {
      for (int q = 0; q < nq; ++q)
        hipLaunchKernelGGL(aug_minmax_out_kernel, dim3(1), dim3(1), 0, st, rs, out + q, ks[q] == 0, ks[q] != 0);
    }
    return check_launch("aug_order_stats");
  }
  // ranks 2q and 2q+1 of the select: ks[q] and ks[q] + 1 (capped), interpolated with fracs[q]; they go in by a kernel
  // argument, so no host buffer is read after this call returns
  Ranks rk{};
  for (int q = 0; q < nq; ++q) {
    rk.r[2 * q] = (uint32_t)ks[q];
    rk.r[2 * q + 1] = (uint32_t)std::min<int64_t>(ks[q] + 1, n - 1);
  }
  hipLaunchKernelGGL(aug_rank_init_kernel, dim3(1), dim3(1), 0, st, rs, rk);
  const int nsel = 2 * nq;
  for (int pass = 0; pass < 3; ++pass) {
    hipLaunchKernelGGL(aug_hist_kernel, dim3(grid), dim3(AUG_NT), 0, st, x, n, P, P.n, pass, nsel, rs, hist);
    hipLaunchKernelGGL(aug_pick_kernel, dim3(1), dim3(AUG_NT), 0, st, pass, nsel, rs, hist, pa, out, nq);
  }
  return check_launch("aug_order_stats");
}

extern "C" int m355_aug_intensity(const float* x, float* y, int32_t C, const int32_t* size3, const m355_aug_stage* stages,
                                  int32_t nstages, void* stream) {
  if (int rc = check_size3("aug_intensity", size3)) return rc;
  M355_REQUIRE(x && y && C > 0, M355_EINVALID_ARG, "aug_intensity: null pointer or %d channels", C);
  Program P;
  if (int rc = make_program("aug_intensity", P, stages, nstages, C, size3)) return rc;
  const int64_t n = (int64_t)C * P.S;
  hipLaunchKernelGGL(aug_intensity_kernel, dim3(grid_of(n)), dim3(AUG_NT), 0, (hipStream_t)stream, x, y, n, P);
  return check_launch("aug_intensity");
}

extern "C" int m355_aug_blur(const float* x, float* y, int32_t C, const int32_t* size3, int32_t axis, double sigma,
                             const m355_aug_stage* stages, int32_t nstages, void* stream) {
  if (int rc = check_size3("aug_blur", size3)) return rc;
  M355_REQUIRE(x && y && x != y && C > 0, M355_EINVALID_ARG, "aug_blur: null pointer, x == y or %d channels", C);
  M355_REQUIRE(axis >= 0 && axis <= 2, M355_EINVALID_ARG, "aug_blur: axis %d", axis);
  M355_REQUIRE(sigma > 0.0 && sigma * 4.0 + 0.5 <= BLUR_MAX_RADIUS, M355_EINVALID_ARG,
               "aug_blur: sigma %g voxels outside (0, %g]", sigma, (BLUR_MAX_RADIUS - 0.5) / 4.0);
  Program P;
  if (int rc = make_program("aug_blur", P, stages, nstages, C, size3)) return rc;
  for (int k = 0; k < nstages; ++k)
    M355_REQUIRE(stages[k].op != M355_AUG_RESCALE, M355_EINVALID_ARG,
                 "aug_blur: a rescale stage needs statistics of the blurred image: not an epilogue");
  const int radius = (int)(4.0 * sigma + 0.5);   // scipy: int(truncate * sd + 0.5)
  const int64_t n = (int64_t)C * P.S;
  hipLaunchKernelGGL(aug_blur_kernel, dim3(grid_of(n)), dim3(AUG_NT), 0, (hipStream_t)stream, x, y, n, axis, (float)sigma,
                     radius, P);
  return check_launch("aug_blur");
}

extern "C" int m355_aug_otsu_pad(const float* x, int32_t C, const int32_t* size3, double* pad, void* stream) {
  if (int rc = check_size3("aug_otsu_pad", size3)) return rc;
  M355_REQUIRE(x && pad && C > 0 && C <= 65535, M355_EINVALID_ARG, "aug_otsu_pad: null pointer or %d channels", C);
  hipLaunchKernelGGL(aug_otsu_kernel, dim3(C), dim3(OTSU_NT), 0, (hipStream_t)stream, x, size3[0], size3[1], size3[2], pad);
  return check_launch("aug_otsu_pad");
}

extern "C" int m355_aug_channel_minmax(const float* x, int32_t C, const int32_t* size3, int32_t which, double* out,
                                       void* workspace, size_t ws_bytes, void* stream) {
  if (int rc = check_size3("aug_channel_minmax", size3)) return rc;
  M355_REQUIRE(x && out && workspace && C > 0 && C <= 65535, M355_EINVALID_ARG,
               "aug_channel_minmax: null pointer or %d channels", C);
  M355_REQUIRE(which == 0 || which == 1, M355_EINVALID_ARG, "aug_channel_minmax: which %d not in {0 (min), 1 (max)}",
               which);
  const size_t need = (size_t)C * 2 * sizeof(uint32_t);
  M355_REQUIRE(ws_bytes >= need, M355_EWORKSPACE, "aug_channel_minmax: workspace %zu < %zu bytes", ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(workspace, 0, need, st) != hipSuccess) return check_launch("aug_channel_minmax: memset");
  const int64_t S = (int64_t)size3[0] * size3[1] * size3[2];
  // >= 16 elements per thread, <= 1024 workgroups in all
  const unsigned per = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(S, AUG_NT * 16), std::max(1, 1024 / C)));
  hipLaunchKernelGGL(aug_channel_minmax_kernel, dim3(per, C), dim3(AUG_NT), 0, st, x, S, (uint32_t*)workspace);
  hipLaunchKernelGGL(aug_channel_minmax_out_kernel, dim3(grid_of(C, 64)), dim3(AUG_NT), 0, st, (const uint32_t*)workspace,
                     C, which, out);
  return check_launch("aug_channel_minmax");
}
