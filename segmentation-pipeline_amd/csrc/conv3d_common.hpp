// Shared pieces of the 3x3x3 convolution code: device helpers of the kernels (conv3d.hip: fp32 kernels and the launchers;
// conv3d_f32x3.hip: split kernels; conv3d_h16.hip: bf16 / fp16 operand kernels) and what the host layer (conv3d_host.hip:
// every extern "C" entry point) hands the launchers: a route (conv3d_route.hpp: planners, routes, checks) and a call.
#pragma once
#include "common.hpp"
#include "h16.hpp"
#include "conv3d_route.hpp"

namespace m355 {


// Opaque copy: stops LICM from hoisting per-element address decode out of a loop (which
// would keep hundreds of loop-invariant registers alive and spill).
__device__ __forceinline__ int opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

// Work-queue state of the persistent kernels: counter[0..7] = tickets of the eight item regions, counter[8] =
// workgroups that have left.  The LAST workgroup to leave zeroes the state, so a packed-weight buffer (which
// holds it) can be reused launch after launch without a memset; the weight-pack kernels zero it initially.
__device__ __forceinline__ void queue_leave(int* __restrict__ counter) {
  if (threadIdx.x == 0) {
    if (atomicAdd(counter + 8, 1) == (int)gridDim.x - 1) {
#pragma unroll
      for (int r = 0; r < 9; ++r) counter[r] = 0;
    }
  }
}

// ------------------------------------------------------------ MFMA fwd kernel
template <int NTW, int GX>
struct FwdTile {
  static constexpr int GY = 32 / GX;
  static constexpr int TZ = 4;  // one z slice per wave
  static constexpr int TY = NTW * GY;
  static constexpr int TX = GX;
  static constexpr int RS = TX + 2;
  static constexpr int PS = (TY + 2) * RS;
  static constexpr int CS = (TZ + 2) * PS;
  static constexpr int CC = 4;  // input channels per LDS chunk (even: MFMA k-pair)
  static constexpr int NROWS = CC * (TZ + 2) * (TY + 2);
};

// Output tile of one wave: C/D layout col = lane&31 (voxel), row = (r&3) + 8*(r>>2) + 4*(lane>>5).
// The bias / residual values of all 16 rows are loaded as one batch (one wait) and the row offsets
// k*DHW are uniform, so the 16*NTW stores go out back to back.  (Written the obvious way --
// `if (o < Cout) { v = acc; if (bias) v += bias[o]; if (add) v += add[idx]; y[idx] = v; }` per
// element -- hipcc emits a branch, a load and a vmcnt(0) per element: ~10 us per tile with the
// matrix core idle.)
template <int NTW, int GY>
__device__ __forceinline__ void store_conv_tile(const f32x16 (&acc)[NTW], float* __restrict__ dst,
                                                const float* __restrict__ addp, const float* __restrict__ bias,
                                                int o0, int Cout, int z, int y0, int xg, int ly, int half,
                                                int D, int H, int W, bool lane_ok, float* __restrict__ stat) {
  // lane_ok: this lane's (z, x) column lies inside the volume.  Every lane stays active to the end
  // (the statistics below are reduced with cross-lane shuffles).
  // stat (may be null): (sum, sum of squares) of the values this WAVE stores, per output channel ->
  // stat[o*2 + {0,1}]; the normalisation that follows the conv sums these partials instead of
  // reading y again (m355_conv3d_fwd_stats / m355_norm_stats_from_partials).
  const int64_t HW = (int64_t)H * W, DHW = HW * D;
  const int ob = o0 + 4 * half;  // this lane's first output channel; row r is channel ob + (r&3) + 8*(r>>2)
  float bb[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) bb[r] = 0.f;
  if (bias) {
#pragma unroll
    for (int r = 0; r < 16; ++r) bb[r] = bias[min(ob + (r & 3) + 8 * (r >> 2), Cout - 1)];
  }
  float s1[16], s2[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) s1[r] = s2[r] = 0.f;
#pragma unroll
  for (int g = 0; g < NTW; ++g) {
    const int yg = y0 + g * GY + ly;
    const bool ok = lane_ok && yg < H;
    const int64_t base = ok ? (int64_t)ob * DHW + (int64_t)z * HW + (int64_t)yg * W + xg : 0;
    float v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = acc[g][r] + bb[r];
    if (addp) {
      float aa[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = (r & 3) + 8 * (r >> 2);
        aa[r] = addp[(ok && ob + k < Cout) ? base + (int64_t)k * DHW : 0];
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) v[r] += aa[r];
    }
    if (stat) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float t = ok ? v[r] : 0.f;
        s1[r] += t;
        s2[r] = fmaf(t, t, s2[r]);
      }
    }
    if (ok) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = (r & 3) + 8 * (r >> 2);
        if (ob + k < Cout) dst[base + (int64_t)k * DHW] = v[r];
      }
    }
  }
  if (stat) {
    // reduce-scatter over the 32 lanes of each half (xor < 32 stays inside the half): 32 values
    // (16 rows x {sum, sumsq}) are summed over 32 lanes with 16+8+4+2+1 shuffles; lane l ends up
    // holding value index l & 31 = q*16 + r.  Fixed order -> bit-reproducible.
    float a[32];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      a[r] = s1[r];
      a[16 + r] = s2[r];
    }
    // (opaque: the lane-derived values of this once-per-item tail are RECOMPUTED here -- hoisted out of the persistent
    // kernels' item loop they sat in registers through every MFMA chunk, and conv3_mfma_fwd_p_kernel<4, 32> at the
    // 256-register limit spilled them to scratch: 5 VGPR spills, 16 B of scratch, round-3 review)
    const int l32 = opaque((int)threadIdx.x) & 31;
#pragma unroll
    for (int h = 16; h >= 1; h >>= 1) {
      const bool up = (l32 & h) != 0;
#pragma unroll
      for (int i = 0; i < h; ++i) {
        const float send = up ? a[i] : a[i + h];
        const float keep = up ? a[i + h] : a[i];
        a[i] = keep + __shfl_xor(send, h, 64);
      }
    }
    const int r = l32 & 15, q = l32 >> 4;
    const int o = o0 + 4 * (opaque((int)threadIdx.x >> 5) & 1) + (r & 3) + 8 * (r >> 2);
    if (o < Cout) stat[(int64_t)o * 2 + q] = a[0];
  }
}


// ---- 16-row output tile (v_mfma_f32_16x16x4_f32) for the remainder of channel counts that are no multiple of
// 32 (the reference's real widths are 40 / 80 / 120: research/msseg2/msseg2.py:87, main_config.py:123-127;
// a 32-row tile for 8 remaining channels is 75 % padding).  Same flop rate as the 32x32x2 form; the K-step of 4
// is exactly one 4-channel LDS chunk at a tap.  C/D layout: col = lane & 15 (voxel), row = 4 * (lane >> 4) + reg.
// A 32-voxel group is two MFMAs (x-halves h2); acc[g][h2] holds 4 channels of one voxel per lane.
typedef float f32x4v __attribute__((ext_vector_type(4)));
template <int NTW, int GX>
__device__ __forceinline__ void store_conv_tile16(const f32x4v (&acc)[NTW][2], float* __restrict__ dst,
                                                  const float* __restrict__ addp, const float* __restrict__ bias,
                                                  int o0, int Cout, int z, int y0, int x0, int lane, int D, int H, int W,
                                                  float* __restrict__ stat) {
  constexpr int GY = 32 / GX;
  const int64_t HW = (int64_t)H * W, DHW = HW * D;
  const int ob = o0 + 4 * (lane >> 4);
  float bb[4], s1[4], s2[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    bb[r] = (bias && ob + r < Cout) ? bias[ob + r] : 0.f;
    s1[r] = s2[r] = 0.f;
  }
#pragma unroll
  for (int g = 0; g < NTW; ++g)
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2) {
      const int vox = 16 * h2 + (lane & 15);
      const int yg = y0 + g * GY + vox / GX, xg = x0 + vox % GX;
      const bool ok = z < D && yg < H && xg < W;
      const int64_t base = ok ? (int64_t)ob * DHW + (int64_t)z * HW + (int64_t)yg * W + xg : 0;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[g][h2][r] + bb[r];
      if (addp) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += addp[(ok && ob + r < Cout) ? base + (int64_t)r * DHW : 0];
      }
      if (stat) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float t = ok ? v[r] : 0.f;
          s1[r] += t;
          s2[r] = fmaf(t, t, s2[r]);
        }
      }
      if (ok) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (ob + r < Cout) dst[base + (int64_t)r * DHW] = v[r];
      }
    }
  if (stat) {  // sum over the 16 lanes (voxels) of each channel quad, fixed order
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int off = 8; off >= 1; off >>= 1) {
        s1[r] += __shfl_xor(s1[r], off, 64);
        s2[r] += __shfl_xor(s2[r], off, 64);
      }
    }
    if ((lane & 15) == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (ob + r < Cout) {
          stat[(int64_t)(ob + r) * 2] = s1[r];
          stat[(int64_t)(ob + r) * 2 + 1] = s2[r];
        }
    }
  }
}

// ConvTranspose3d k2 s2 forward on the split (conv3d_f32x3.hip; caller: convt.hip)
int convt_fwd_x3_nvt(int Cin);
void launch_convt_fwd_x3(int nvt, dim3 grid, const float* x, const float* w, const float* bias, float* y, int Cin, int Cout,
                         int D, int H, int W, int64_t xbs, int64_t ybs, int mt_per_wg, hipStream_t st);
// ... and its weight gradient (slabs, bias partials, then their fixed-order reduce); grid.x = the voxel-range splits
void launch_convt_bww_x3(int mt, dim3 grid, const float* x, const float* dy, float* dw, float* dbias, float* slab, double* bslab,
                         int N, int Cin, int Cout, int D, int H, int W, int64_t xbs, int64_t ybs, hipStream_t st);

// ConvTranspose3d (convt.hip): the same contract.  `kind` names the kernel family of the call, the numbers are that
// family's launch; the byte counts hold for every kind, so one workspace serves whichever side the pointers pick.
enum class ConvtKind {
  Direct,       // convt_direct_*_kernel: not k2 s2 p0, >= 2^31 elements per sample, or a y side the MFMA kernels cannot take
  MfmaF32,      // convt_k2s2_{fwd,bwd_data,bwd_weight}_mfma_kernel
  X3,           // convt_k2s2_fwd_x3_kernel (M355_COMPUTE_F32X3 forward)
  C8,           // convt_k2s2_fwd_c8_kernel, convt_k2s2_bww_c8_kernel
  H16,          // convt_k2s2_fwd_h16_kernel, convt_k2s2_bwd_data_h16_kernel
  Unsupported   // c8 entry points only: M355_EUNSUPPORTED
};
struct ConvtRoute {
  ConvtKind kind;
  int nvt;                    // voxels per workgroup tile (forward, fp32 data gradient)
  int mt;                     // 32-channel tiles per workgroup: fp32 gradients (2 | 4), c8 weight gradient (ct: 1 | 2 | 4)
  int mt_per_wg;              // m-tiles a workgroup walks (C8 forward: m-tile pairs) or stages (H16)
  int ks_n, ng;               // H16 forward: 16-channel K steps, 128-voxel groups per tile
  dim3 grid;
  size_t lds;
  int split, o_per_split;     // data gradient: splits of K = 8 * Cout and output channels of each; weight gradient: voxel-range splits
  size_t slab_bytes;          // split partials, at the head of the workspace
  size_t dbias_offset, dbias_bytes;   // the bias gradient's scratch (weight gradient)
  size_t workspace_bytes;
  int32_t plan_code[4];       // m355_conv_transpose3d_plan
};
// which: 0 forward, 1 data gradient, 2 weight gradient.  y_side_ok: even y batch stride and 8-byte aligned y / dy -- the
// one fact that is neither in the descriptor nor in the tuning (the queries pass true: the upper bound)
ConvtRoute route_convt(const m355_conv3d_desc* d, int which, bool y_side_ok);
ConvtRoute route_convt_c8(const m355_conv3d_desc* d, int which);   // the c8 entry points (*_h16)

// ------------------------------------------------------------------ launchers
// The pointers of one forward / data-gradient call; everything else is in its route.
struct ConvCall {
  const m355_conv3d_desc* d;
  const float* in;            // fp32 NCDHW input ...
  const void* in16;           // ... or c8 (null: the 16-bit kinds round `in` into the staging copy first)
  const float* w;             // weight tensor, or with M355_CONV_W_PACKED the buffer m355_conv3d_pack filled for this route
  const float* bias;
  const float* add;
  float* out;                 // fp32 NCDHW, or (route.out16) a c8 tensor
  float* stat;                // fused statistics partials (null: none)
  int* oflag;                 // overflow word of a c8 data gradient (fp16: the stores saturate and report there)
  void* ws;
  hipStream_t st;
};
// every kind but the 16-bit ones (conv3d.hip): weight pack unless prepacked, the kernel, the split-K reduction
int launch_f32_conv(const ConvRoute& r, const ConvCall& c);
// the 16-bit kinds (conv3d_h16.hip): operand pack of an fp32 input, weight pack unless prepacked, the kernel, the reduction
int launch_h16_conv(const ConvRoute& r, const ConvCall& c);
// packed weights of every kind with a packed form (m355_conv3d_pack)
void launch_pack_weights(const ConvRoute& r, const m355_conv3d_desc* d, bool transpose, const float* w, void* packed,
                         hipStream_t st);
void launch_pack_w3_h16(const FwdPlan& p, int compute, const float* w, void* wp, int Cout_w, int Cin_w, bool transpose,
                        hipStream_t st);
// M355_COMPUTE_F32X3 (conv3d_f32x3.hip): split + fragment-ordered weights, and the main and 16-row launches of an X3 route
void launch_pack_w3_x3(const FwdPlan& p, const float* w, void* wp, int Cout_w, int Cin_w, bool transpose, hipStream_t st);
int launch_x3_conv(const ConvRoute& r, const float* in, const void* wp, const float* bias, const float* add, float* out,
                   float* slab, const m355_conv3d_desc* d, hipStream_t st, float* stat);

// The pointers of one weight-gradient call.
struct BwwCall {
  const m355_conv3d_desc* d;
  const void* x;              // fp32 NCDHW or c8, as the entry point takes them
  const void* dy;
  const float* dy32;          // the fp32 dy of the bias gradient (c8-only flow: none, it reads the c8 dy)
  float* dw;
  float* dbias;
  float grad_unscale;         // c8-only flow: the loss scale removed in the fp32 epilogues
  void* ws;
  hipStream_t st;
};
// ONE weight-gradient launcher (conv3d.hip): operand packs, the kernel of r.kind, the slab reduction, the bias gradient
int launch_bww(const BwwRoute& r, const BwwCall& c);
// ... and the typed launchers of the other two files it switches to: slabs into `slab`
void launch_bww_x3(const BwwRoute& r, const float* x, const float* dy, float* slab, const m355_conv3d_desc* d, hipStream_t st);
void launch_bww_c8(const BwwRoute& r, const void* x16, const void* dy16, float* slab, const m355_conv3d_desc* d, hipStream_t st);

// One entry of a batched weight pack (m355_conv3d_pack_batch): after optimizer.step every conv weight of a model is
// re-packed (forward + data-gradient form), ~37 launches of 5-15 us each on the critical path of a train step; the batch
// kernel does them in one launch, blockIdx.y = entry.  kind: 0 = fp32 MFMA layout, 1 = bf16, 2 = fp16 (c8 chunks).
struct PackEntry {
  const float* w;
  void* wp;
  int* counter;       // work queue in the tail of the packed region, zeroed like the single pack kernels do
  int Cout, Cin;      // of the weight tensor
  int kdim;           // fp32: kin_pad; 16-bit: nchunks
  int mout_pad;
  int transpose, kind;
  int blk0, nblk;     // this entry's blocks [blk0, blk0 + nblk) of the launch: proportional to its element count
};
constexpr int PACK_BATCH = 64;   // 64 x 56 B of kernel arguments (< 4 KB)
struct PackBatch {
  PackEntry e[PACK_BATCH];
  int n;
};
void launch_pack_batch(PackBatch& b, int n, hipStream_t st);
// ... and of the split-kernel forms (M355_COMPUTE_F32X3, conv3d_f32x3.hip)
struct X3PackEntry {
  const float* w;
  void* wq;
  int Cout, Cin;      // of the weight tensor
  int nchunks, otiles, tile16, transpose;
  int blk0, nblk;
};
struct X3PackBatch {
  X3PackEntry e[PACK_BATCH];
  int n;
};
void launch_pack_x3_batch(X3PackBatch& b, int n, hipStream_t st);

// fp32 MFMA weight layout (see pack_w3_kernel): block `bid` of `nblk` of one tensor
__device__ __forceinline__ void pack_w3_body(const float* __restrict__ w, float* __restrict__ wp, int Cout, int Cin,
                                             int kin_pad, int mout_pad, int transpose, int64_t bid, int64_t nblk) {
  const int64_t total = (int64_t)kin_pad * 27 * mout_pad;
  for (int64_t i = bid * (int64_t)blockDim.x + threadIdx.x; i < total; i += nblk * blockDim.x) {
    const int m = (int)(i % mout_pad);
    const int64_t r = i / mout_pad;
    const int tap = (int)(r % 27);
    const int kc = (int)(r / 27);
    float v = 0.f;
    if (!transpose) {
      if (kc < Cin && m < Cout) v = w[((int64_t)m * Cin + kc) * 27 + tap];
    } else {
      if (kc < Cout && m < Cin) v = w[((int64_t)kc * Cin + m) * 27 + (26 - tap)];
    }
    wp[i] = v;
  }
}
// y[n,o,s] = bias[o] + add[n,o,s] + sum_ks slab[ks][n,o,s]   (fixed order)
__global__ void splitk_reduce_kernel(const float* __restrict__ slab, const float* __restrict__ bias,
                                     const float* __restrict__ add, float* __restrict__ y, int N,
                                     int Cout, int64_t S, int ksplit, int64_t slab_stride,
                                     int64_t ybs);

}  // namespace m355

// dbias through the shared two-stage reduction; `ws` holds Cout * ceil(S / DBIAS_CHUNK) doubles
int launch_dbias(const float* dy, float* dbias, int N, int Cout, int64_t S, int64_t ybs, void* ws, hipStream_t st);
