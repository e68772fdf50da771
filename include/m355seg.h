/*
 * m355seg.h — C ABI of libm355seg.so: the MI355X (gfx950) 3D U-Net hot path.
 *
 * This is the drop-in boundary for the efirdc/Segmentation-Pipeline hot path
 * (SURVEY.md §8b).  The reference has no native code: every entry point below
 * replaces a stock torch.nn op the reference calls from Python, and the comment
 * on each one cites the reference call site (paths relative to the reference
 * repo root) it stands in for.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no C++/torch types.
 *  - All tensors are float32 (M355_F32), NCDHW, spatial dims dense
 *    (stride of W == 1, H == W, D == H*W, C == D*H*W).  The batch stride is
 *    explicit (in elements) wherever a tensor may be a channel slice of a
 *    larger concat buffer; 0 means dense (C*D*H*W).  An fp32 tensor that
 *    carries a batch stride needs no alignment beyond its element size, and
 *    any stride is legal (the vector kernels are chosen from the pointers and
 *    strides at hand), except where an entry point states a requirement and
 *    rejects what misses it.  Everything else (weights, bias, statistics,
 *    workspace, packed weights) is expected as an allocator hands it out:
 *    16-byte aligned.  c8 tensors are made of 16-byte items: 16-byte aligned,
 *    strides % 8 == 0.
 *  - Caller owns every buffer, including workspace.  The library never
 *    frees device memory and keeps no pointer to a tensor or workspace after a
 *    call returns.  The ONE piece of device state it keeps is the work-queue
 *    pool of the queue-driven conv kernels (256 KB per device: 4096 slots of
 *    eight ticket counters + an exit counter, all zero between launches).  A
 *    caller that hands that pool over with m355_queue_pool_set() before its
 *    first conv launch on a device -- the Python host does, from torch's
 *    allocator -- gets a library that makes no device allocation at all;
 *    otherwise the pool is hipMalloc'ed + hipMemset on first use (never inside
 *    a stream capture) and lives until the process exits.
 *  - Workspace and output contents on entry are irrelevant unless an entry
 *    point says "zeroed by the CALLER": the library initialises what it reads.
 *  - Every call only ENQUEUES work on `stream` (a hipStream_t passed as
 *    void*); no implicit synchronisation.
 *  - Return 0 (M355_OK) or a negative status; never throws, never aborts.
 *    m355_last_error() returns a thread-local message for the last failure.
 */
#ifndef M355SEG_H
#define M355SEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: m355_conv3d_desc.reserved became `flags` (packed weights, fused softmax); c8 / 16-bit entry points; ensembles;
 * padded sliding window; weight standardisation
 * 3: c8-only training flow (norm / pool / conv-transpose / trilinear / dropout / space-to-depth backward on c8 tensors,
 *    loss-scaled pack / unpack), device-side sampler, one-pass grid aggregation, caller-provided work-queue pool
 *    (m355_queue_pool_*), fused norm-backward tail */
#define M355_ABI_VERSION 3

enum {
  M355_OK = 0,
  M355_EINVALID_ARG = -1,
  M355_EUNSUPPORTED = -2,
  M355_ELAUNCH = -3,
  M355_EWORKSPACE = -4
};

enum { M355_F32 = 0 };

/* arithmetic of the 3x3x3 convolutions:
 *   M355_COMPUTE_F32  exact fp32: v_mfma_f32_32x32x2_f32, a k-ordered fp32 fma chain (default)
 *   M355_COMPUTE_BF16 operands rounded to bf16 (round-to-nearest-even), v_mfma_f32_32x32x16_bf16 with
 *                     fp32 accumulation (BASELINE cfg3).
 *   M355_COMPUTE_F16  the same with IEEE fp16 operands, v_mfma_f32_32x32x16_f16 (BASELINE cfg5:
 *                     "mixed fp16 with MFMA channel-GEMM path"); values beyond +-65504 become inf.
 *   M355_COMPUTE_F32X3 fp32 tensors in and out, fp32 results, bf16 matrix pipe: every operand is split EXACTLY into
 *                     three bf16 values (x = hi + mid + lo, 8 + 8 + 8 significant bits; each step exact in fp32) and
 *                     six of the nine plane products -- all but the three below 2^-24 of the product -- run on
 *                     v_mfma_f32_32x32x16_bf16 with fp32 accumulation (conv3d_f32x3.hip): 6 MFMAs of K = 16 stand for
 *                     8 fp32 MFMAs of K = 2 at a sixteenth of the cost per K.  Measured against fp64 the results are
 *                     as accurate as fp32 arithmetic is: max error 2e-7 .. 1.5e-6 of max |result| on the BASELINE
 *                     layers, within 2.5x of the fp32 MFMA kernels' (profiles/r04_f32x3_accuracy.txt; both carry the
 *                     error of an fp32 accumulation).  Applies to the 3x3x3 / stride 1 / pad 1 forward and data gradient of
 *                     layers with >= 8 K-channels and > 4 M-channels, and to the weight gradient of layers with > 4
 *                     channels on both sides, at least two z planes and < 2^24 voxels per sample, and to the forward of
 *                     the k = 2 / stride 2 conv-transpose (m355_conv_transpose3d_fwd); every other descriptor and entry
 *                     point treats it as M355_COMPUTE_F32.  This is what the host side's
 *                     default precision "fp32" passes (ops.py); "fp32_mfma" passes M355_COMPUTE_F32.
 * The 16-bit modes apply to conv3d fwd, bwd_data and bwd_weight (the edge layers' weight gradient runs in exact fp32).
 * In the 16-bit modes the convolution kernels read their input in the "c8" layout
 *     x16[n][cb][voxel][8]   cb = channel block of 8 (zero-padded past C), 16-bit elements,
 * i.e. the 8 channels of a voxel are one aligned 16-byte item = one MFMA operand fragment (h16.hpp).
 * The *_h16 entry points take such tensors directly (the normalisation / pooling passes of the model
 * path write them, m355_norm_act_fwd_h16 ...); the plain entry points accept fp32 NCDHW and convert
 * into their workspace first. */
enum { M355_COMPUTE_F32 = 0, M355_COMPUTE_BF16 = 1, M355_COMPUTE_F16 = 2, M355_COMPUTE_F32X3 = 3 };

/* activation fused into the normalise pass (components.py:26,54-55).  3..6 are the smooth ones, evaluated in fp32 in every
 * flow: nn.ELU(alpha), nn.GELU() (erf), nn.GELU(approximate='tanh'), nn.SiLU().  7 is not a code. */
enum { M355_ACT_NONE = 0, M355_ACT_RELU = 1, M355_ACT_LEAKY_RELU = 2, M355_ACT_ELU = 3, M355_ACT_GELU = 4,
       M355_ACT_GELU_TANH = 5, M355_ACT_SILU = 6 };

int m355_version(void);
const char* m355_last_error(void);
/* The M355_* tuning overrides (test / sweep hooks: M355_CONV_NTW, M355_CONV_KSPLIT, M355_CONV_SLOTS, ...) are
 * read from the environment once, when the library is loaded; call this after changing them. */
void m355_reload_tuning(void);
/* Work-queue pool (see "Conventions"): `zeroed_device_buffer` = m355_queue_pool_bytes() bytes of zero-filled device
 * memory on `device`, 64-byte aligned, owned by the caller and kept alive (and otherwise untouched) for as long as the
 * library is used on that device.  Call before the first conv launch on the device; M355_EUNSUPPORTED once a different
 * pool is in use there.  Every queue-driven launch takes a 64-byte slot keyed by (device, stream, capture id): launches
 * on different streams, and launch sequences captured into different hipGraphs, never share one. */
size_t m355_queue_pool_bytes(void);
int m355_queue_pool_set(void* zeroed_device_buffer, size_t bytes, int32_t device);
/* fp16 training flow (loss-scaled activation gradients, "grad_scale" below): `device_word` = a zeroed 4-byte device word
 * owned by the caller (NULL: off).  From then on, on that device, every kernel that rounds a loss-scaled gradient to fp16
 * ORs bit 0 into it when it had to clamp a value to +-65504 (the gradient was clipped: the scale is too large), and every
 * epilogue that removes the loss scale from a parameter gradient (grad_unscale != 1) ORs bit 1 when its result is not
 * finite.  The host reads and clears the word after a backward pass and, when it is non-zero, skips the optimizer step and
 * lowers the scale (segmentation_pipeline_amd.ops.fp16_overflow(); the reference has no reduced-precision path). */
int m355_overflow_flag_set(void* device_word, int32_t device);

/* ------------------------------------------------------------------ conv3d
 * Replaces nn.Conv3d as used by Block3d (models/components.py:36,42,51) and the
 * out conv (models/modular_unet.py:83,99), and the strided F.conv3d of
 * BlurConv3d (components.py:119).  Cubic kernel k, isotropic stride / zero pad.
 *   y[n,o,z,y,x] = bias[o] + add[n,o,z,y,x]
 *                + sum_{c,dz,dy,dx} w[o,c,dz,dy,dx] * x[n,c,z*s+dz-p, ...]
 * `bias` and `add` may be NULL.  `add` has y's layout (residual branch fusion,
 * components.py:67-68).  Weight layout [Cout,Cin,k,k,k] (torch).
 */
typedef struct m355_conv3d_desc {
  int32_t N, Cin, Cout;
  int32_t D, H, W;          /* INPUT spatial size of the forward op */
  int32_t k, stride, pad;
  int32_t out_pad;          /* conv-transpose only */
  int64_t x_batch_stride;   /* elements; 0 = dense */
  int64_t y_batch_stride;   /* elements; 0 = dense */
  int32_t compute;          /* M355_COMPUTE_* (3x3x3 / s1 / p1; M355_COMPUTE_F32X3 also k2 s2 conv-transpose fwd; ignored elsewhere) */
  int32_t flags;            /* M355_CONV_* bits, 0 by default */
} m355_conv3d_desc;

/* desc->flags */
enum {
  /* the `w` argument of m355_conv3d_fwd(_stats|_h16) / m355_conv3d_bwd_data(_h16) points at weights packed by
   * m355_conv3d_pack for THIS descriptor (same shapes, compute mode and direction) instead of the torch-layout
   * filter: the per-launch repacking kernel is skipped.  Weights only change at optimizer.step, so a caller
   * packs once per parameter version.  The buffer is read-only for the conv kernels: any number of launches, on any
   * streams, may share it concurrently (the work-queue state of the queue-driven kernels lives in a per-(stream,
   * capture) slot of the work-queue pool, see "Conventions" above and m355_queue_pool_set). */
  M355_CONV_W_PACKED = 1,
  /* forward only: nn.Softmax(dim=1) over the Cout output channels applied in the conv epilogue (the out conv +
   * hypothesis of ModularUNet, models/modular_unet.py:99-100); allowed when m355_conv3d_fuses_softmax(desc) != 0
   * (the fp32 Cout <= 4 kernel, where a voxel's channels sit in one thread's registers).  Same bits as
   * m355_conv3d_fwd followed by m355_softmax_fwd. */
  M355_CONV_SOFTMAX = 2,
  /* forward only: nn.Sigmoid applied per element in the conv epilogue (hypothesis_class=nn.Sigmoid: binary and multi-label
   * heads); allowed when m355_conv3d_fuses_sigmoid(desc) != 0, which holds exactly where m355_conv3d_fuses_softmax does
   * (one epilogue slot, one tuning switch).  Same bits as m355_conv3d_fwd followed by m355_sigmoid_fwd.  Setting both
   * head flags is M355_EINVALID_ARG; a head flag on a descriptor that does not fuse it is M355_EUNSUPPORTED. */
  M355_CONV_SIGMOID = 4
};
int32_t m355_conv3d_fuses_softmax(const m355_conv3d_desc* d);
int32_t m355_conv3d_fuses_sigmoid(const m355_conv3d_desc* d);
/* which: 0 = forward, 1 = data gradient.  0 bytes = this descriptor has no packed form (generic direct kernels). */
size_t m355_conv3d_packed_bytes(const m355_conv3d_desc* d, int32_t which);
int m355_conv3d_pack(const m355_conv3d_desc* d, int32_t which, const float* w, void* packed, void* stream);
/* The same for many weights in one launch: after optimizer.step (segmentation_trainer.py:259) every conv weight of a
 * model needs its forward and data-gradient forms again -- ~37 packs of 5-15 us each, back to back on the critical
 * path of a cfg2 train step.  Each item is packed exactly as m355_conv3d_pack(&item.desc, item.which, item.w,
 * item.packed) would (identical bytes); `packed` must hold m355_conv3d_packed_bytes(&item.desc, item.which). */
typedef struct m355_pack_item {
  m355_conv3d_desc desc;
  int32_t which;
  const float* w;
  void* packed;
} m355_pack_item;
int m355_conv3d_pack_batch(const m355_pack_item* items, int32_t n, void* stream);

size_t m355_conv3d_fwd_workspace(const m355_conv3d_desc* d);
int m355_conv3d_fwd(const m355_conv3d_desc* d, const float* x, const float* w,
                    const float* bias, const float* add, float* y,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Forward with the statistics of the following normalisation fused into the epilogue
 * (Block3d: conv -> norm, models/components.py:51-53): besides y the kernel writes, per sample n,
 * slot p and output channel o, the (sum, sum of squares) of the y values one wave stored:
 *   stat_partials[((n * P + p) * Cout + o) * 2 + {0,1}],   P = m355_conv3d_stats_slots(desc)
 * (every slot of every channel is written; slots of waves that lie outside the volume hold zeros).
 * m355_norm_stats_from_partials() turns them into mean / rstd without reading y again.
 * P == 0 means this descriptor has no fused statistics (not 3x3x3 s1 p1, the fp32 Cout <= 4 kernel, or a
 * split-K plan): call m355_conv3d_fwd + m355_norm_stats instead. */
int64_t m355_conv3d_stats_slots(const m355_conv3d_desc* d);
int m355_conv3d_fwd_stats(const m355_conv3d_desc* d, const float* x, const float* w,
                          const float* bias, const float* add, float* y, float* stat_partials,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- c8 tensors (16-bit compute modes) ----
 * bytes of a dense c8 tensor; conversion fp32 NCDHW <-> c8 (round-to-nearest-even; batch strides in
 * ELEMENTS of the respective tensor, 0 = dense). */
size_t m355_act16_bytes(int32_t N, int32_t C, int64_t S);
int m355_act16_pack(const float* x, void* x16, int32_t N, int32_t C, int64_t S, int64_t x_batch_stride,
                    int64_t x16_batch_stride, int32_t compute, void* stream);
int m355_act16_unpack(const void* x16, float* x, int32_t N, int32_t C, int64_t S, int64_t x16_batch_stride,
                      int64_t x_batch_stride, int32_t compute, void* stream);
/* conv3d forward / data gradient (3x3x3 s1 p1, desc->compute = BF16 | F16) on a c8 input: x16 holds
 * desc->Cin channels (fwd), dy16 desc->Cout channels (bwd_data); outputs are fp32 NCDHW exactly as in
 * m355_conv3d_fwd(_stats) / m355_conv3d_bwd_data (stat_partials may be NULL).  Workspace:
 * m355_conv3d_h16_workspace(desc, which) bytes, which = 0 forward, 1 data gradient. */
size_t m355_conv3d_h16_workspace(const m355_conv3d_desc* d, int32_t which);
int m355_conv3d_fwd_h16(const m355_conv3d_desc* d, const void* x16, int64_t x16_batch_stride, const float* w,
                        const float* bias, const float* add, float* y, float* stat_partials, void* workspace,
                        size_t workspace_bytes, void* stream);
/* forward whose OUTPUT is c8 as well (written by the epilogue: lanes exchange channel halves and store whole
 * 16-byte items): the pre-norm tensor of conv -> norm/act -> conv never exists in fp32.  No fused `add`. */
/* statistics slots of m355_conv3d_fwd_h16_c8 (differs from m355_conv3d_stats_slots for split-K plans, whose
 * reduction pass emits the partials: one slot per block of that pass) */
int64_t m355_conv3d_stats_slots_c8(const m355_conv3d_desc* d);
int m355_conv3d_fwd_h16_c8(const m355_conv3d_desc* d, const void* x16, int64_t x16_batch_stride, const float* w,
                           const float* bias, void* y16, int64_t y16_batch_stride, float* stat_partials,
                           void* workspace, size_t workspace_bytes, void* stream);
int m355_conv3d_bwd_data_h16(const m355_conv3d_desc* d, const void* dy16, int64_t dy16_batch_stride, const float* w,
                             float* dx, void* workspace, size_t workspace_bytes, void* stream);
/* weight gradient of the 3x3x3 / stride 1 / padding 1 conv with BOTH operands in c8: x16 = the packed conv input the
 * forward pass consumed, dy16 = the packed output gradient the data gradient consumes (so the 16-bit training flow
 * converts each tensor once).  dw fp32 [Cout][Cin][3][3][3]; dbias (may be NULL) is reduced from the fp32 `dy`
 * (NCDHW, desc->y_batch_stride; may be NULL when dbias is).  Replaces the reference's autograd conv weight
 * gradient under `torch.cuda.amp.autocast` (segmentation_pipeline/segmentation_trainer.py:203-227).  Volumes
 * below 2^25 voxels per sample. */
size_t m355_conv3d_bwd_weight_h16_workspace(const m355_conv3d_desc* d);
int m355_conv3d_bwd_weight_h16(const m355_conv3d_desc* d, const void* x16, int64_t x16_batch_stride, const void* dy16,
                               int64_t dy16_batch_stride, const float* dy, float* dw, float* dbias, void* workspace,
                               size_t workspace_bytes, void* stream);

/* Introspection for profiling: which kernel variant a 3x3x3 conv dispatches to.
 * which: 0 = forward, 1 = data gradient, 2 = weight gradient (of m355_conv3d_bwd_weight).  out[0] = kernel family:
 * 0 generic direct kernel, 1 MFMA implicit GEMM (one output tile per workgroup), 3 the same as a persistent kernel
 * (workgroups walk several tiles), 2 the small-Cout forward (Cout <= 4: the packed-FMA kernel conv3_valu_smallcout_kernel, or
 * with M355_SMALLCOUT_VALU=0 the z-Toeplitz MFMA kernel), 4 the 16-bit operand kernel (persistent), 5 its
 * 8-wave double-buffered variant, 6 its one-item-per-workgroup variant, 7 the split kernel of M355_COMPUTE_F32X3
 * (conv3_f32x3_kernel); weight gradient: 8 conv3_bww_x3_kernel, 9 conv3_mfma_bww2(c)_kernel, 10 the edge-layer kernel
 * conv3_mfma_bww_small_kernel, 11 the c8 kernel behind an operand pack (16-bit modes).  out[1] = voxel groups per wave
 * (NTW), out[2] = lanes along x per group (GX; weight gradient: tile width), out[3] = split-K factor (weight gradient:
 * voxel-range splits).  Pure host function. */
int m355_conv3d_plan(const m355_conv3d_desc* d, int32_t which, int32_t* out4);

/* Introspection, as m355_resample_plan: what ONE call of a launching conv entry point would start.  entry: 0 conv3d_fwd,
 * 1 _fwd_stats, 2 _bwd_data, 3 _bwd_weight, 4 _fwd_h16, 5 _fwd_h16_c8, 6 _bwd_data_h16, 7 _bwd_data_h16_c8,
 * 8 _bwd_weight_h16, 9 _bwd_weight_c8.  batch_strides[2]: the entry point's stride ARGUMENTS (c8 entry points: first
 * operand, then c8 output | dy16; 0 = dense; the fp32 strides are the descriptor's).  pointers[7]: the entry point's
 * pointers as integers -- compared with zero and masked, never followed: [0] first operand (x | dy | x16 | dy16),
 * [1] w (weight gradients: the second operand dy | dy16), [2] bias (m355_conv3d_bwd_weight_h16: its fp32 dy), [3] add,
 * [4] output (y | dx | dw), [5] statistics partials (weight gradients: dbias), [6] workspace.  Runs the entry point's
 * argument checks in its order and returns its code; on M355_OK out[0..11] =
 *   [0] kernel variant.  Forward / data gradient: 0 direct, 1 conv3_mfma_fwd_kernel, 2 conv3_mfma_fwd_p_kernel, 3 packed-FMA
 *       small-Cout (conv3_valu_smallcout_kernel), 4 Toeplitz small-Cout (conv3_mfma_fwd_smallcout_kernel), 5 conv3_f32x3_kernel,
 *       conv3_h16_kernel 6 queue-driven with 4 waves / 7 with 8 waves / 8 one-shot, 9 conv3_c4_h16_kernel,
 *       10 conv3_cout4_h16_kernel.  Weight gradient: 0 direct, conv3_mfma_bww_kernel 1 vector / 2 scalar,
 *       3 conv3_mfma_bww2_kernel, 4 conv3_mfma_bww2c_kernel, 5 conv3_mfma_bww_small_kernel, 6 conv3_bww_x3_kernel,
 *       7 conv3_bww_x3c_kernel, 8 conv3_bww_c8_kernel, 9 conv3_bww_c8_small_kernel
 *   [1..3] grid x, y, z of the main launch (x = 0: none, a <= 16 channel output runs on the 16-row tile alone), [4] its block size
 *   [5], [6] grid x and z of the 16-row tile launch (0: none)
 *   [7] the auxiliary launches, a bit mask: 1 weight pack, 2 operand pack (fp32 -> c8) of the first operand, 4 of the second,
 *       8 16-row tile, 16 split-K reduction, 32 ... that emits the statistics, slab reduction 64 transposed / 128 per tap /
 *       256 plain, bias gradient 512 from the fp32 dy / 1024 from the c8 dy
 *   [8] the workspace bytes the call was checked against, [9] grid x of the split-K / slab reduction (0: none)
 *   [10], [11] workspace offsets: forward / data gradient the split-K slabs and the c8 staging copy (packed weights at 0);
 *       weight gradient the bias gradient's scratch and the first c8 operand copy (slabs at 0).
 * Pure host function. */
int m355_conv3d_launch_plan(int32_t entry, const m355_conv3d_desc* d, const int64_t* batch_strides, const uint64_t* pointers,
                            size_t workspace_bytes, int64_t* out12);

/* dx = conv-transpose of dy with w (autograd of the op above w.r.t. x).
 * desc describes the FORWARD op; dx has x's shape and x_batch_stride,
 * dy has y's shape and y_batch_stride. */
size_t m355_conv3d_bwd_data_workspace(const m355_conv3d_desc* d);
int m355_conv3d_bwd_data(const m355_conv3d_desc* d, const float* dy, const float* w,
                         float* dx, void* workspace, size_t workspace_bytes, void* stream);

/* dw[o,c,taps] = sum_{n,voxels} dy * shifted x;  dbias[o] = sum dy (NULL to skip).
 * Deterministic (fixed-order two-stage reduction). */
size_t m355_conv3d_bwd_weight_workspace(const m355_conv3d_desc* d);
int m355_conv3d_bwd_weight(const m355_conv3d_desc* d, const float* x, const float* dy,
                           float* dw, float* dbias,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------- conv-transpose3d
 * Replaces nn.ConvTranspose3d(kernel_size=2, stride=2) reached through the
 * upsample_class hook (models/modular_unet.py:20-21,72-81,96) and the
 * F.conv_transpose3d of BlurConvTranspose3d (components.py:152).
 * desc: N, Cin, Cout, D/H/W = INPUT spatial, k, stride, pad, out_pad.
 * Weight layout [Cin,Cout,k,k,k] (torch).  Output spatial =
 * (D-1)*stride - 2*pad + k + out_pad.
 */
size_t m355_conv_transpose3d_workspace(const m355_conv3d_desc* d);
int m355_conv_transpose3d_fwd(const m355_conv3d_desc* d, const float* x, const float* w,
                              const float* bias, float* y,
                              void* workspace, size_t workspace_bytes, void* stream);
int m355_conv_transpose3d_bwd_data(const m355_conv3d_desc* d, const float* dy, const float* w,
                                   float* dx, void* workspace, size_t workspace_bytes,
                                   void* stream);
int m355_conv_transpose3d_bwd_weight(const m355_conv3d_desc* d, const float* x, const float* dy,
                                     float* dw, float* dbias,
                                     void* workspace, size_t workspace_bytes, void* stream);

/* Introspection, as m355_conv3d_plan: the route a conv-transpose call takes.  which: 0 / 1 / 2 = forward / data gradient /
 * weight gradient of the fp32 entry points above, 3 / 4 / 5 = the same of the c8 entry points (*_h16).  y_side (fp32
 * entry points only): the y / dy pointer the call would get; the MFMA kernels need it 8-byte aligned and an even
 * y_batch_stride.  NULL = aligned, which is what m355_conv_transpose3d_workspace assumes.  out[0] = kernel family:
 * 0 the generic direct kernels, 1 the fp32-MFMA k2s2 kernels, 2 the split forward of M355_COMPUTE_F32X3
 * (convt_k2s2_fwd_x3_kernel), 3 convt_k2s2_fwd_c8_kernel / convt_k2s2_bww_c8_kernel, 4 convt_k2s2_fwd_h16_kernel /
 * convt_k2s2_bwd_data_h16_kernel, 5 none: the c8 entry point returns M355_EUNSUPPORTED.  out[1..3] by which and family
 * (all 0 for families 0 and 5):
 *   0: voxel tile NVT, m-tiles per workgroup, 0          1: voxel tile NVT, channel tiles MT, splits of K = 8 * Cout
 *   2: channel tiles MT, voxel-range splits, 0           3, family 3: voxel tile NVT, m-tile pairs per workgroup, 0
 *   3, family 4: K steps KS (4 | 8), voxel groups NG, m-tiles staged per workgroup
 *   4: m-tiles staged per workgroup MTW, grid.x, 0       5: channel tiles CT, voxel-range splits, 0
 * Pure host function. */
int m355_conv_transpose3d_plan(const m355_conv3d_desc* d, int32_t which, const void* y_side, int32_t* out4);

/* The gradients of the k = 2 / stride 2 conv-transpose on the bf16 matrix pipe through the exact three-way operand split
 * of M355_COMPUTE_F32X3 (fp32 tensors, fp32 accumulation, nothing rounded to 16 bits): entry points and queries of their
 * own, with the argument meaning of m355_conv_transpose3d_bwd_data / _bwd_weight.  The three fp32 entry points above, their
 * plan and their workspace query do not change with them.
 * m355_conv_transpose3d_x3_bwd_supported(desc, y_side): bit 0 = the data gradient, bit 1 = the weight gradient has a split
 * kernel for this descriptor and this dy pointer (NULL = aligned).  The weight gradient (convt_k2s2_bwd_weight_x3_kernel)
 * needs desc->compute == M355_COMPUTE_F32X3, k 2 / stride 2 / pad 0 / out_pad 0, below 2^31 elements per sample, W even, dy
 * 16-byte aligned with y_batch_stride a multiple of 4, x_batch_stride even, at least 512 voxels in the batch (the
 * smallest level measured; smaller ones stay on the fp32-MFMA kernel), and M355_F32X3 / M355_F32X3_CONVT_BWD not 0.  The data
 * gradient has no split kernel: bit 0 is never set.  A gradient whose bit is clear gets M355_EUNSUPPORTED from its entry
 * point before any launch (so does an x pointer off an 8-byte boundary); the caller then takes the fp32 entry point.
 * m355_conv_transpose3d_x3_bwd_workspace(desc): bytes for the supported gradients (slabs [split][Cin][Cout][8] fp32, then
 * the bias partials [split][Cout] double, each rounded up to 256), 0 when none is.
 * m355_conv_transpose3d_x3_bwd_plan(desc, which = 1 | 2, y_side, out4): out[0] = 2 (the split family of
 * m355_conv_transpose3d_plan) or 5 (none: M355_EUNSUPPORTED); which = 2: out[1] = channel tiles MT (2 | 4) of
 * convt_k2s2_bwd_weight_x3_kernel<MT>, out[2] = voxel-range splits (grid.x, slabs), out[3] = 0.  Pure host functions. */
int32_t m355_conv_transpose3d_x3_bwd_supported(const m355_conv3d_desc* d, const void* y_side);
size_t m355_conv_transpose3d_x3_bwd_workspace(const m355_conv3d_desc* d);
int m355_conv_transpose3d_x3_bwd_plan(const m355_conv3d_desc* d, int32_t which, const void* y_side, int32_t* out4);
int m355_conv_transpose3d_bwd_data_x3(const m355_conv3d_desc* d, const float* dy, const float* w, float* dx,
                                      void* workspace, size_t workspace_bytes, void* stream);
int m355_conv_transpose3d_bwd_weight_x3(const m355_conv3d_desc* d, const float* x, const float* dy, float* dw, float* dbias,
                                        void* workspace, size_t workspace_bytes, void* stream);

/* nn.ConvTranspose3d(kernel_size=2, stride=2) c8 -> c8 for the 16-bit modes (fp32 weights and arithmetic: the op
 * is HBM-bound): the output lands directly in its slot of the decoder's c8 concat buffer
 * (models/modular_unet.py:96-97).  Other geometries: M355_EUNSUPPORTED (unpack / fp32 / pack instead). */
int m355_conv_transpose3d_fwd_h16(const m355_conv3d_desc* d, const void* x16, int64_t x16_batch_stride,
                                  const float* w, const float* bias, void* y16, int64_t y16_batch_stride,
                                  int32_t compute, void* stream);

/* --------------------------------------------------- normalisation (+ act)
 * Replaces normalization_class(out_channels) + activation_class() inside
 * Block3d (components.py:52-55): nn.BatchNorm3d (default) or nn.GroupNorm via
 * functools.partial.  One descriptor covers both:
 *   groups == 0 : BatchNorm — one statistic per channel over (N, voxels)
 *   groups  > 0 : GroupNorm — one statistic per (n, group) over (C/groups, voxels)
 * y = act((x - mean) * rstd * gamma[c] + beta[c]) (+ add, the residual branch).
 */
typedef struct m355_norm_desc {
  int32_t N, C;
  int64_t S;                /* voxels per channel (D*H*W) */
  int32_t groups;           /* 0 = batch norm */
  int32_t act;              /* M355_ACT_* */
  float eps;
  float act_slope;          /* the activation's parameter: LeakyReLU negative slope, ELU alpha; ignored by codes 0, 1, 4-6 */
  int64_t x_batch_stride;   /* elements; 0 = dense */
  int64_t y_batch_stride;
  int64_t add_batch_stride; /* batch stride of the fused residual `add` (0 = dense C*S) */
} m355_norm_desc;

/* number of statistics: C for BN, N*groups for GN */
int64_t m355_norm_num_stats(const m355_norm_desc* d);
size_t m355_norm_workspace(const m355_norm_desc* d);

/* Introspection, as m355_conv3d_plan: how a normalisation pass of this descriptor is launched.  which = the pass:
 *   0 statistics (m355_norm_stats, m355_norm_sums)    1 forward fp32      2 forward fp32 -> c8 (m355_norm_act_fwd_h16)
 *   3 forward c8 -> c8     4 forward with pooled second output     5 / 6 backward pass 1 / pass 2, fp32
 *   7 backward pass 2 with a c8 twin of dx (m355_norm_act_bwd_h16)        8 / 9 backward pass 1 / pass 2, c8
 * out[0] = 1 when the pass takes its vector kernel (float4 rows; which = 2: four voxels per thread in flight; 0 where the
 * pass has one kernel only), judged with every pointer 16-byte aligned -- a call on a pointer that is not takes the scalar
 * kernel; out[1] = chunks per statistic (which = 0) or per channel (5, 8) of the first-stage partial sums, else 0;
 * out[2] = grid.x; out[3] = byte offset of stat_m[num_stats][2] (float) behind the backward's partials in the workspace
 * (which >= 5, else 0; saturates at INT32_MAX): m355_norm_workspace(desc) covers the largest such offset + 8 * num_stats.
 * Returns M355_EINVALID_ARG for a null desc / out4, an unknown pass or a descriptor the pass's entry point rejects with that
 * code, M355_EUNSUPPORTED where that entry point would (N or C > 65535 on the fp32 passes).  The descriptor carries no
 * D, H, W, so which = 4 answers for any S, although m355_norm_act_pool_fwd itself needs D * H * W == S, all even.
 * Pure host function. */
int m355_norm_plan(const m355_norm_desc* d, int32_t which, int32_t* out4);

/* Pass 1: mean[s], rstd[s] (biased variance, 1/sqrt(var+eps)).  For BN in
 * training mode running_mean/running_var (may be NULL) are updated in place
 * with `momentum` and the UNBIASED variance, as torch does. */
int m355_norm_stats(const m355_norm_desc* d, const float* x, float* mean, float* rstd,
                    float* running_mean, float* running_var, float momentum,
                    void* workspace, size_t workspace_bytes, void* stream);
/* The same statistics from the partials of m355_conv3d_fwd_stats (x is not read).  `slots` = P of
 * the producing conv; desc->C must be that conv's Cout and desc->S its output voxel count.
 * Workspace: m355_norm_workspace(desc) bytes.  Fixed summation order (double), bit-reproducible. */
int m355_norm_stats_from_partials(const m355_norm_desc* d, const float* stat_partials, int64_t slots,
                                  float* mean, float* rstd, float* running_mean, float* running_var,
                                  float momentum, void* workspace, size_t workspace_bytes, void* stream);
/* BN eval mode: derive mean/rstd from the running statistics. */
int m355_norm_stats_from_running(const m355_norm_desc* d, const float* running_mean,
                                 const float* running_var, float* mean, float* rstd,
                                 void* stream);
/* Pass 2: normalise + affine + activation (+ add).  gamma/beta/add may be NULL. */
int m355_norm_act_fwd(const m355_norm_desc* d, const float* x, const float* mean,
                      const float* rstd, const float* gamma, const float* beta,
                      const float* add, float* y, void* stream);
/* Backward.  x is the SAVED PRE-NORM input; the activation mask and x_hat are
 * recomputed from it.  Produces dx (x's layout), dgamma[C], dbeta[C] (either may
 * be NULL when gamma is NULL).  `training` = 0 for BN eval mode (statistics are
 * constants, no mean-subtraction terms). */
/* normalise + activation with nn.AvgPool3d(2, 2) of the result as a second output (an encoder block's output
 * continues into the skip connection and, pooled, into the next level: models/modular_unet.py:90-92).  y as in
 * m355_norm_act_fwd (no residual add); pooled: fp32 [N, C, D/2, H/2, W/2] with its own batch stride (0 = dense).
 * D * H * W must equal desc->S, all even.  Bit-identical to m355_norm_act_fwd followed by m355_avgpool3d_2x_fwd.
 * Alignment: x and y 8-byte aligned, desc->x_batch_stride and desc->y_batch_stride even (the kernel moves x pairs);
 * M355_EINVALID_ARG otherwise, nothing is launched.  Channel slices of an aligned concat buffer always qualify (S is a
 * multiple of 8). */
int m355_norm_act_pool_fwd(const m355_norm_desc* d, const float* x, const float* mean, const float* rstd,
                           const float* gamma, const float* beta, float* y, float* pooled, int64_t pooled_batch_stride,
                           int32_t D, int32_t H, int32_t W, void* stream);
int m355_norm_act_bwd(const m355_norm_desc* d, const float* x, const float* dy,
                      const float* mean, const float* rstd, const float* gamma,
                      const float* beta, float* dx, float* dgamma, float* dbeta,
                      int training, void* workspace, size_t workspace_bytes, void* stream);
/* The backward of m355_norm_act_pool_fwd: the gradient of the activated tensor is dskip (fp32 [N, C, D, H, W] with its
 * own batch stride, 0 = dense; NULL: the skip path carries no gradient) + the un-pooled dpool (fp32 [N, C, D/2, H/2, W/2],
 * own batch stride, 0 = dense), summed inside both passes of the normalisation backward: the pass of
 * m355_avgpool3d_2x_bwd[_add] that writes the sum, and its re-read, do not happen.  x and dx share desc->x_batch_stride;
 * desc->y_batch_stride is not used.  D * H * W must equal desc->S (M355_EINVALID_ARG), all even (M355_EUNSUPPORTED).
 * dx, dgamma and dbeta are bit-identical to m355_avgpool3d_2x_bwd[_add] into a dense tensor followed by
 * m355_norm_act_bwd.  No pointer needs more than 4-byte alignment.  Workspace: m355_norm_workspace(desc) bytes. */
int m355_norm_act_bwd_pool(const m355_norm_desc* d, const float* x, const float* dskip, int64_t dskip_batch_stride,
                           const float* dpool, int64_t dpool_batch_stride, int32_t D, int32_t H, int32_t W,
                           const float* mean, const float* rstd, const float* gamma, const float* beta, float* dx,
                           float* dgamma, float* dbeta, int training, void* workspace, size_t workspace_bytes,
                           void* stream);
/* The same with dx ALSO written as a c8 tensor (h16 layout above) by the second pass: in the 16-bit training flow dx
 * is the output gradient of the convolution in front of the normalisation, and that convolution's data- and
 * weight-gradient kernels read it as c8 (m355_conv3d_bwd_data_h16 / m355_conv3d_bwd_weight_h16). */
int m355_norm_act_bwd_h16(const m355_norm_desc* d, const float* x, const float* dy, const float* mean,
                          const float* rstd, const float* gamma, const float* beta, float* dx, float* dgamma,
                          float* dbeta, int training, void* dx16, int64_t dx16_batch_stride, int32_t compute,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Synchronised batch norm: BatchNorm3d statistics over the batch of ALL ranks of a data-parallel job, so that a model
 * trained with its batch sharded over GPUs normalises exactly as the reference's single-process run of the whole batch
 * (models/nested_residual_unet.py:19-23 is BatchNorm; segmentation_trainer.py:189-262 is one process).  The library
 * provides the local halves, the caller all-reduces (SUM, RCCL) between them:
 *   forward : m355_norm_sums -> all-reduce(sums) -> m355_norm_stats_from_sums
 *   backward: m355_norm_act_bwd_reduce(total_count = &sums[2C]) -> all-reduce(stat_m) -> m355_norm_act_bwd_apply
 * sums: double[2*C + 1] = {sum x, sum x^2} per channel, then the element count (N*S) that went into them; from x or from
 * the producing conv's epilogue partials (stat_partials != NULL, x unused).  desc->groups must be 0.
 * m355_norm_act_bwd_reduce divides by *total_count (device pointer; NULL = the local count), so the SUM over ranks of
 * stat_m[C][2] is the global mean; dgamma / dbeta stay local sums (the gradient all-reduce averages them like any
 * other parameter gradient).  m355_norm_act_bwd_apply: dx (and, dx16 != NULL, its c8 twin as m355_norm_act_bwd_h16). */
int m355_norm_sums(const m355_norm_desc* d, const float* x, const float* stat_partials, int64_t slots, double* sums,
                   void* workspace, size_t workspace_bytes, void* stream);
int m355_norm_stats_from_sums(const m355_norm_desc* d, const double* sums, float* mean, float* rstd,
                              float* running_mean, float* running_var, float momentum, void* stream);
int m355_norm_act_bwd_reduce(const m355_norm_desc* d, const float* x, const float* dy, const float* mean,
                             const float* rstd, const float* gamma, const float* beta, float* dgamma, float* dbeta,
                             int training, const double* total_count, float* stat_m, void* workspace,
                             size_t workspace_bytes, void* stream);
int m355_norm_act_bwd_apply(const m355_norm_desc* d, const float* x, const float* dy, const float* mean,
                            const float* rstd, const float* gamma, const float* beta, const float* stat_m, float* dx,
                            void* dx16, int64_t dx16_batch_stride, int32_t compute, void* stream);

/* The passes that WRITE c8 tensors in the 16-bit modes (so that conv -> norm/act -> conv never converts):
 * m355_norm_act_fwd with a c8 output y16 (the layout transposer: reads the fp32 NCDHW conv output) and,
 * when y != NULL, the usual fp32 NCDHW output as well (desc->y_batch_stride) for non-conv consumers;
 * nn.AvgPool3d(2, 2) (models/modular_unet.py:22,41,64,92) c8 -> c8 (fp32 sums, one rounding). */
int m355_norm_act_fwd_h16(const m355_norm_desc* d, const float* x, const float* mean, const float* rstd,
                          const float* gamma, const float* beta, const float* add, float* y, void* y16,
                          int64_t y16_batch_stride, int32_t compute, void* stream);
/* normalise + activation (+ residual add16) c8 -> c8, for a pre-norm tensor produced by m355_conv3d_fwd_h16_c8;
 * statistics of such a tensor when its conv had none fused (split-K plans): per-channel (sum, sum of squares)
 * partials [N][P][C][2], P = m355_act16_partials_slots(S), fed to m355_norm_stats_from_partials. */
int m355_norm_act_fwd_c8(const m355_norm_desc* d, const void* x16, int64_t x16_batch_stride, const float* mean,
                         const float* rstd, const float* gamma, const float* beta, const void* add16,
                         int64_t add16_batch_stride, void* y16, int64_t y16_batch_stride, int32_t compute,
                         void* stream);
int64_t m355_act16_partials_slots(int64_t S);
int m355_act16_channel_partials(const void* x16, int64_t x16_batch_stride, int32_t N, int32_t C, int64_t S,
                                int32_t compute, float* stat_partials, void* stream);
int m355_avgpool3d_2x_fwd_h16(const void* x16, void* y16, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                              int64_t x16_batch_stride, int64_t y16_batch_stride, int32_t compute, void* stream);

/* ---- the c8-only TRAINING flow of the 16-bit modes (round 3) ----
 * With autograd on, activations and activation gradients of the conv -> norm/act -> conv -> pool / conv-transpose ->
 * concat chain exist only as c8 tensors, as they already do under no_grad; these are the backward halves.  They replace
 * the reference's autograd under `torch.cuda.amp.autocast` (segmentation_pipeline/segmentation_trainer.py:203-227) for
 * Block3d (models/components.py:62-73), nn.AvgPool3d and nn.ConvTranspose3d(2, 2) (models/modular_unet.py:64,72-81,92,96).
 *
 * grad_scale / grad_unscale: the fp16 mode carries activation gradients multiplied by a power of two (at full size the
 * gradient of a mean over ~2e6 voxels is ~1e-7, below the fp16 normal range).  The scale is applied where a gradient
 * first becomes c8 (m355_act16_pack_scaled; values past the fp16 range saturate) and removed in the fp32 epilogue of
 * every PARAMETER gradient (`grad_unscale` = 1 / scale); activation gradients keep it.  bf16: 1. */
int m355_act16_pack_scaled(const float* x, void* x16, int32_t N, int32_t C, int64_t S, int64_t x_batch_stride,
                           int64_t x16_batch_stride, int32_t compute, float scale, void* stream);
int m355_act16_unpack_scaled(const void* x16, float* x, int32_t N, int32_t C, int64_t S, int64_t x16_batch_stride,
                             int64_t x_batch_stride, int32_t compute, float scale, void* stream);
/* data gradient of the 3x3x3 conv, c8 in -> c8 out (dx16 holds desc->Cin channels); workspace:
 * m355_conv3d_h16_workspace(desc, 1).  Same arithmetic as m355_conv3d_bwd_data_h16 followed by one rounding. */
int m355_conv3d_bwd_data_h16_c8(const m355_conv3d_desc* d, const void* dy16, int64_t dy16_batch_stride, const float* w,
                                void* dx16, int64_t dx16_batch_stride, void* workspace, size_t workspace_bytes,
                                void* stream);
/* weight gradient from c8 operands as m355_conv3d_bwd_weight_h16, with the bias gradient (may be NULL) reduced from
 * the c8 dy16 itself and both multiplied by grad_unscale in their fp32 epilogues. */
size_t m355_conv3d_bwd_weight_c8_workspace(const m355_conv3d_desc* d);
int m355_conv3d_bwd_weight_c8(const m355_conv3d_desc* d, const void* x16, int64_t x16_batch_stride, const void* dy16,
                              int64_t dy16_batch_stride, float* dw, float* dbias, float grad_unscale, void* workspace,
                              size_t workspace_bytes, void* stream);
/* normalisation + activation backward on c8 operands: x16 = the saved PRE-NORM tensor, the incoming gradient is
 * dy16 (may be NULL when dpool16 is given) + un-pooled dpool16 (may be NULL; then D, H, W are ignored): an encoder
 * block's output continues into the skip connection AND, through nn.AvgPool3d(2, 2), into the next level, and the sum
 * of the two gradients is formed inside this pass.  dx16: c8, same shape as x16.  dgamma / dbeta (may be NULL) fp32,
 * multiplied by grad_unscale.  Workspace: m355_norm_workspace(desc).  Expressions as m355_norm_act_bwd. */
int m355_norm_act_bwd_c8(const m355_norm_desc* d, const void* x16, int64_t x16_batch_stride, const void* dy16,
                         int64_t dy16_batch_stride, const void* dpool16, int64_t dpool16_batch_stride, int32_t D,
                         int32_t H, int32_t W, const float* mean, const float* rstd, const float* gamma,
                         const float* beta, void* dx16, int64_t dx16_batch_stride, float* dgamma, float* dbeta,
                         int training, float grad_unscale, int32_t compute, void* workspace, size_t workspace_bytes,
                         void* stream);
/* The same backward as its two halves around an exchange (synchronised BatchNorm on the c8 flow -- the reference's
 * dmri_hippo model is BatchNorm, models/nested_residual_unet.py:19-23, and a batch sharded over ranks must normalise
 * with the statistics of the whole batch): _reduce = first pass + per-statistic sums divided by `total_count[0]` (a
 * device double: the element count per statistic over ALL ranks) -> stat_m[2 * num_stats] (this rank's share of the
 * two gradient means) and the local dgamma / dbeta; the host all-reduces stat_m (SUM); _apply = second pass with the
 * reduced stat_m.  With total_count = this rank's own count the pair equals m355_norm_act_bwd_c8 bit for bit. */
int m355_norm_act_bwd_c8_reduce(const m355_norm_desc* d, const void* x16, int64_t x16_batch_stride, const void* dy16,
                                int64_t dy16_batch_stride, const void* dpool16, int64_t dpool16_batch_stride, int32_t D,
                                int32_t H, int32_t W, const float* mean, const float* rstd, const float* gamma,
                                const float* beta, float* dgamma, float* dbeta, int training, const double* total_count,
                                float grad_unscale, float* stat_m, int32_t compute, void* workspace, size_t workspace_bytes,
                                void* stream);
int m355_norm_act_bwd_c8_apply(const m355_norm_desc* d, const void* x16, int64_t x16_batch_stride, const void* dy16,
                               int64_t dy16_batch_stride, const void* dpool16, int64_t dpool16_batch_stride, int32_t D,
                               int32_t H, int32_t W, const float* mean, const float* rstd, const float* gamma,
                               const float* beta, const float* stat_m, void* dx16, int64_t dx16_batch_stride,
                               int32_t compute, void* stream);
/* nn.AvgPool3d(2, 2) backward c8 -> c8, optionally adding the gradient of the un-pooled tensor's other consumer
 * (dskip16, may be NULL): dx16[v] = dskip16[v] + dpool16[v / 2] / 8.  D, H, W: the UN-pooled size (even). */
int m355_avgpool3d_2x_bwd_h16(const void* dpool16, const void* dskip16, void* dx16, int32_t N, int32_t C, int32_t D,
                              int32_t H, int32_t W, int64_t dpool16_batch_stride, int64_t dskip16_batch_stride,
                              int64_t dx16_batch_stride, int32_t compute, void* stream);
/* nn.Upsample(scale_factor=2, mode='trilinear', align_corners=True) c8 -> c8 and its (gather-form, deterministic)
 * backward: the `up` of NestedResUNet (segmentation_pipeline/models/nested_residual_unet.py:74,92-101) in the c8
 * flow.  D, H, W: the LOW-resolution size; fp32 interpolation with ATen's align_corners weights, one rounding. */
int m355_upsample_trilinear2x_fwd_h16(const void* x16, void* y16, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                                      int64_t x16_batch_stride, int64_t y16_batch_stride, int32_t compute, void* stream);
int m355_upsample_trilinear2x_bwd_h16(const void* dy16, void* dx16, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                                      int64_t dy16_batch_stride, int64_t dx16_batch_stride, int32_t compute,
                                      void* stream);
/* space-to-depth / depth-to-space by 2 on c8 activations: the rearrangement around the stride-1 3x3x3 form of
 * BlurConv3d / BlurConvTranspose3d (segmentation_pipeline/models/components.py:91-154) in the 16-bit flows.  N, C, D, H,
 * W describe the FULL-resolution tensor (C channels, even sizes); the packed tensor has 8 * C channels (channel
 * c * 8 + pz * 4 + py * 2 + px = element of c8 block c) at half the resolution.  Each is the other's backward. */
int m355_space_to_depth2_h16(const void* x16, void* y16, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                             int64_t x16_batch_stride, int64_t y16_batch_stride, int32_t compute, void* stream);
int m355_depth_to_space2_h16(const void* x16, void* y16, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                             int64_t x16_batch_stride, int64_t y16_batch_stride, int32_t compute, void* stream);
/* y16[n][c][s] = x16[n][c][s] * scale[n * C + c]: nn.Dropout3d on a c8 activation (nested_residual_unet.py:43-44,
 * components.py:70-71) and its backward (the same call on the gradient); saturating for fp16. */
int m355_act16_channel_scale(const void* x16, const float* scale, void* y16, int32_t N, int32_t C, int64_t S,
                             int64_t x16_batch_stride, int64_t y16_batch_stride, int32_t compute, void* stream);
/* nn.ConvTranspose3d(kernel_size=2, stride=2) backward from c8 operands on the 16-bit matrix core (operands rounded to
 * the 16-bit type, fp32 accumulate): dx16 (desc->Cin channels, c8) from dy16 (desc->Cout channels at twice the
 * resolution); dw fp32 [Cin][Cout][2][2][2] and dbias (may be NULL), both multiplied by grad_unscale.
 * m355_conv_transpose3d_h16_bwd_supported(desc) == 0: unpack / m355_conv_transpose3d_bwd_* / pack instead (other
 * geometries, Cout > 128). */
int32_t m355_conv_transpose3d_h16_bwd_supported(const m355_conv3d_desc* d);
size_t m355_conv_transpose3d_h16_bwd_workspace(const m355_conv3d_desc* d);
int m355_conv_transpose3d_bwd_data_h16(const m355_conv3d_desc* d, const void* dy16, int64_t dy16_batch_stride,
                                       const float* w, void* dx16, int64_t dx16_batch_stride, int32_t compute,
                                       void* stream);
int m355_conv_transpose3d_bwd_weight_h16(const m355_conv3d_desc* d, const void* x16, int64_t x16_batch_stride,
                                         const void* dy16, int64_t dy16_batch_stride, float* dw, float* dbias,
                                         float grad_unscale, int32_t compute, void* workspace, size_t workspace_bytes,
                                         void* stream);

/* --------------------------------------------------------------- pooling
 * nn.AvgPool3d(kernel_size=2, stride=2, count_include_pad=False)
 * (models/modular_unet.py:22,41,64,92).  Input D,H,W must be even.
 */
int m355_avgpool3d_2x_fwd(const float* x, float* y, int32_t N, int32_t C,
                          int32_t D, int32_t H, int32_t W,
                          int64_t x_batch_stride, int64_t y_batch_stride, void* stream);
int m355_avgpool3d_2x_bwd(const float* dy, float* dx, int32_t N, int32_t C,
                          int32_t D, int32_t H, int32_t W, /* INPUT size of fwd */
                          int64_t dy_batch_stride, int64_t dx_batch_stride, void* stream);

/* dx = add + pool-backward(dy): the encoder block's output feeds the pool AND the skip connection
 * (models/modular_unet.py:90-92), so its gradient is the sum of two; `add` (dx's shape, own batch stride) is the
 * skip gradient -- one pass instead of a pool-backward pass plus a separate elementwise add. */
int m355_avgpool3d_2x_bwd_add(const float* dy, const float* add, float* dx, int32_t N, int32_t C,
                              int32_t D, int32_t H, int32_t W, /* INPUT size of fwd */
                              int64_t dy_batch_stride, int64_t add_batch_stride, int64_t dx_batch_stride,
                              void* stream);

/* nn.MaxPool3d(kernel_size=2, stride=2) (downsample_class of ModularUNet): D, H, W even (M355_EUNSUPPORTED otherwise,
 * as m355_avgpool3d_2x_fwd).  torch's semantics: the 2x2x2 window is scanned in (d, h, w) order from max = -inf,
 * index = first, updating on `v > max || isnan(v)` -- ties go to the first maximum, a NaN window returns NaN and
 * routes to its last NaN; y holds the selected element's bits.
 * idx: the route, uint8 [N, C, D/2, H/2, W/2] dense, window position 0..7 = (dd * 2 + dh) * 2 + dw; may be NULL
 * (inference).  Batch strides in elements, 0 = dense.  Wide accesses only where pointers and strides prove the
 * alignment; any 4-byte aligned channel slice is accepted. */
int m355_maxpool3d_2x_fwd(const float* x, float* y, uint8_t* idx, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                          int64_t x_batch_stride, int64_t y_batch_stride, void* stream);
/* dx[v] = (idx[v/2] == position of v in its window ? dy[v/2] : 0) + (add ? add[v] : 0); D, H, W: the UN-pooled size.
 * A pure gather: x is not read, every dx element is written exactly once, no atomics (deterministic).  `add` (may be
 * NULL): the skip gradient, as in m355_avgpool3d_2x_bwd_add. */
int m355_maxpool3d_2x_bwd(const float* dy, const uint8_t* idx, const float* add, float* dx, int32_t N, int32_t C,
                          int32_t D, int32_t H, int32_t W, int64_t dy_batch_stride, int64_t add_batch_stride,
                          int64_t dx_batch_stride, void* stream);
/* c8 -> c8; idx8: uint8 [N, ceil(C/8), S/8, 8] dense (8-byte aligned), may be NULL.  The comparison runs on the 16-bit
 * values; lanes past C are written as zero. */
int m355_maxpool3d_2x_fwd_h16(const void* x16, void* y16, uint8_t* idx8, int32_t N, int32_t C, int32_t D, int32_t H,
                              int32_t W, int64_t x16_batch_stride, int64_t y16_batch_stride, int32_t compute, void* stream);
/* dx16[v] = dskip16[v] (may be NULL) + routed dpool16, rounded once; fp16 saturates into the overflow word (bit 0) as
 * m355_avgpool3d_2x_bwd_h16 does.  D, H, W: the UN-pooled size. */
int m355_maxpool3d_2x_bwd_h16(const void* dpool16, const uint8_t* idx8, const void* dskip16, void* dx16, int32_t N,
                              int32_t C, int32_t D, int32_t H, int32_t W, int64_t dpool16_batch_stride,
                              int64_t dskip16_batch_stride, int64_t dx16_batch_stride, int32_t compute, void* stream);

/* ------------------------------------------------------------- upsampling
 * nn.Upsample(scale_factor=2, mode='trilinear', align_corners=True)
 * (models/modular_unet.py:20,39,80,96).  D,H,W = input size; output = 2x.
 */
int m355_upsample_trilinear2x_fwd(const float* x, float* y, int32_t N, int32_t C,
                                  int32_t D, int32_t H, int32_t W,
                                  int64_t x_batch_stride, int64_t y_batch_stride, void* stream);
int m355_upsample_trilinear2x_bwd(const float* dy, float* dx, int32_t N, int32_t C,
                                  int32_t D, int32_t H, int32_t W,
                                  int64_t dy_batch_stride, int64_t dx_batch_stride, void* stream);

/* nn.Upsample(scale_factor=2) in its other two conventions (csrc/upsample.hip), with the argument lists of their
 * m355_upsample_trilinear2x_* counterparts: N, C, D, H, W describe the INPUT (any positive size, odd and 1 included),
 * the output is 2x; batch strides in elements, 0 = dense; the output may be a channel slice of a wider buffer and only
 * 4-byte aligned (16-byte rows are a variant the host picks, see m355_upsample2x_plan).
 *   nearest   mode='nearest' (= 'nearest-exact' at factor 2): y[2z+a, 2y+b, 2x+c] = x[z, y, x].  The forward moves bits
 *             (NaN payloads, signed zeros, infinities and denormals come out unchanged); the backward is the sum of the
 *             block's eight gradients in gather form, deterministic.
 *   hp        mode='trilinear', align_corners=False (half-pixel): per axis y[2i] = 0.25 x[max(i-1, 0)] + 0.75 x[i],
 *             y[2i+1] = 0.75 x[i] + 0.25 x[min(i+1, n-1)]; the backward is the gather-form transpose (4 taps per axis,
 *             the tap past an edge folded onto the border output), fp32 sums, deterministic. */
int m355_upsample_nearest2x_fwd(const float* x, float* y, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                                int64_t x_batch_stride, int64_t y_batch_stride, void* stream);
int m355_upsample_nearest2x_bwd(const float* dy, float* dx, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                                int64_t dy_batch_stride, int64_t dx_batch_stride, void* stream);
int m355_upsample_trilinear2x_hp_fwd(const float* x, float* y, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                                     int64_t x_batch_stride, int64_t y_batch_stride, void* stream);
int m355_upsample_trilinear2x_hp_bwd(const float* dy, float* dx, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                                     int64_t dy_batch_stride, int64_t dx_batch_stride, void* stream);
/* The same c8 -> c8 (compute: M355_COMPUTE_BF16 or M355_COMPUTE_F16; 16-byte aligned items): fp32 arithmetic, one
 * rounding.  The nearest forward copies items.  The backward kernels round with saturation in fp16 and OR bit 0 into the
 * overflow word (m355_overflow_flag_set) when a sum left the fp16 range. */
int m355_upsample_nearest2x_fwd_h16(const void* x16, void* y16, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                                    int64_t x16_batch_stride, int64_t y16_batch_stride, int32_t compute, void* stream);
int m355_upsample_nearest2x_bwd_h16(const void* dy16, void* dx16, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                                    int64_t dy16_batch_stride, int64_t dx16_batch_stride, int32_t compute, void* stream);
int m355_upsample_trilinear2x_hp_fwd_h16(const void* x16, void* y16, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                                         int64_t x16_batch_stride, int64_t y16_batch_stride, int32_t compute,
                                         void* stream);
int m355_upsample_trilinear2x_hp_bwd_h16(const void* dy16, void* dx16, int32_t N, int32_t C, int32_t D, int32_t H,
                                         int32_t W, int64_t dy16_batch_stride, int64_t dx16_batch_stride, int32_t compute,
                                         void* stream);
/* Introspection, as m355_resample_plan, for the eight entry points above: mode 0 nearest, 1 hp; direction 0 forward,
 * 1 backward; c8 0 fp32, 1 the _h16 one.  strides3 / pointers4: the two tensors in the entry point's argument order (the
 * rest is ignored).  Runs the entry point's argument checks and returns its code; on M355_OK out8 as there:
 *   out8[0] = 0 scalar / the only kernel, 1 vector (fp32: float4 stores / loads of the 2x tensor's rows; the backward also
 *             stores float2);   out8[1..3] = grid;   out8[4] = 0;   out8[5..7] = the batch strides, dense ones resolved.
 * Pure host function, launches nothing. */
int m355_upsample2x_plan(int32_t mode, int32_t direction, int32_t c8, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                         const int64_t* strides3, const uint64_t* pointers4, int32_t compute, int64_t* out8);

/* Introspection, as m355_norm_plan: how an entry point of the factor-2 resampling family serves a call.  op:
 *   0 avgpool3d_2x_fwd   1 avgpool3d_2x_bwd   2 avgpool3d_2x_bwd_add   3 upsample_trilinear2x_fwd   4 upsample_trilinear2x_bwd
 *   5 space_to_depth2    6 depth_to_space2    7 maxpool3d_2x_fwd       8 maxpool3d_2x_bwd
 *   9 avgpool3d_2x_fwd_h16   10 avgpool3d_2x_bwd_h16   11 upsample_trilinear2x_fwd_h16   12 upsample_trilinear2x_bwd_h16
 *   13 space_to_depth2_h16   14 depth_to_space2_h16    15 maxpool3d_2x_fwd_h16           16 maxpool3d_2x_bwd_h16
 * N .. W and compute as that entry point takes them (compute is ignored by the fp32 ones); strides3: its batch strides in
 * its own argument order; pointers4: the addresses of its tensors in the order of strides3, then the max-pool route
 * bytes (0 for a NULL); entries the entry point has no argument for are ignored.  The addresses are compared with 0 and
 * masked, never read.  Runs the entry point's argument checks and returns its code; on M355_OK
 *   out8[0] = kernel variant: 0 scalar / the only kernel, 1 vector (fp32 pools: 16-byte rows) or quads (trilinear forward),
 *             2 the LDS-tiled trilinear forward;   out8[1..3] = grid x, y, z;   out8[4] = dynamic LDS bytes;
 *   out8[5..7] = the batch strides, dense ones resolved (0 for an unused one).
 * Pure host function, launches nothing. */
int m355_resample_plan(int32_t op, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W, const int64_t* strides3,
                       const uint64_t* pointers4, int32_t compute, int64_t* out8);

/* ---------------------------------------------------------------- softmax
 * nn.Softmax(dim=1) (models/modular_unet.py:26,46,84,100) and the softmax of
 * StochasticMatrix (components.py:170-185): x viewed as [N, C, inner, S] with
 * softmax over C; inner = 1 for the plain case, C for the stochastic matrix.
 * diag_bias is added to x[n, i, i, :] first when inner == C (0 to disable).
 */
int m355_softmax_fwd(const float* x, float* y, int32_t N, int32_t C, int32_t inner,
                     int64_t S, float diag_bias, void* stream);
int m355_softmax_bwd(const float* y, const float* dy, float* dx, int32_t N, int32_t C,
                     int32_t inner, int64_t S, void* stream);

/* ---------------------------------------------------------------- sigmoid
 * nn.Sigmoid as hypothesis_class (models/modular_unet.py:26-27,84,100): y = 1 / (1 + expf(-x)) over n dense fp32
 * elements, and its gradient dx = dy * (y * (1 - y)) from the saved y.  The stand-alone form of the M355_CONV_SIGMOID
 * epilogue (same expression, same bits), for output convolutions that do not fuse it.  float4 accesses when every
 * pointer is 16-byte aligned, scalar otherwise.
 */
int m355_sigmoid_fwd(const float* x, float* y, int64_t n, void* stream);
int m355_sigmoid_bwd(const float* y, const float* dy, float* dx, int64_t n, void* stream);

/* ------------------------------------------------------- hybrid dice loss
 * HybridLogisticDiceLoss.forward (criterions/hybrid_logistic_dice_loss.py:13-43).
 * prediction p and one-hot target t: dense [N, C, S].
 * out[0] = loss, out[1] = dice_loss, out[2] = logistic_loss.
 * sums (workspace kept for backward): [N*C*4] = {sum p*t, sum_p, sum_t, sum t*log p_safe}
 * where sum_p/sum_t are of squares when square_dice != 0.
 */
size_t m355_hybrid_loss_workspace(int32_t N, int32_t C, int64_t S);
int m355_hybrid_loss_fwd(const float* p, const float* t, int32_t N, int32_t C, int64_t S,
                         float dice_weight, const float* class_weights /* [C] or NULL */,
                         int32_t square_dice, float* out3, float* sums,
                         void* workspace, size_t workspace_bytes, void* stream);
/* dp = dloss * d(loss)/dp, closed form from the saved sums. */
int m355_hybrid_loss_bwd(const float* p, const float* t, const float* sums,
                         const float* dloss /* device scalar */, int32_t N, int32_t C, int64_t S,
                         float dice_weight, const float* class_weights, int32_t square_dice,
                         float* dp, void* stream);

/* ------------------------------------------------ binary cross-entropy + dice loss
 * HybridBinaryLogisticDiceLoss (criterions/hybrid_binary_logistic_dice_loss.py): the loss of a sigmoid
 * head, every channel a binary problem of its own.  x and the target t (values in [0, 1], soft targets allowed):
 * dense fp32 [N, C, S], rows at nc * S for any S (no alignment requirement).  eps = 1e-8.
 *   from_logits == 0   x = p (probabilities): q = 1 - p, lp = log((p + eps) / (1 + eps)), lq = log((q + eps) / (1 + eps));
 *                      no expf is evaluated
 *   from_logits != 0   x = z (logits): p = 1 / (1 + expf(-z)), the bits of m355_sigmoid_fwd; lp = -softplus(-z),
 *                      lq = -softplus(z), softplus(v) = max(v, 0) + log1p(exp(-|v|)); no eps
 *   dice_nc     = 2 sum(p t) / (sum p^2 + sum t^2 + eps)                (sum p + sum t without square_dice)
 *   logistic_nc = cw[c] * (pw[c] * sum(t lp) + sum((1 - t) lq)) / S     (cw = class_weights, pw = pos_weight, or 1)
 *   out3 = {loss, dice_loss, logistic_loss} = {(1 - w) logistic_loss + w dice_loss, mean(1 - dice_nc), mean(-logistic_nc)}
 * sums (kept for backward): [N*C*5] = {sum p t, sum p(^2), sum t(^2), sum t lp, sum (1 - t) lq}, unweighted.
 * The Dice sums and expressions are those of m355_hybrid_loss_fwd: without from_logits, out3[1] has its bits.
 * Deterministic (fp64 block and cross-chunk sums in a fixed order, no float atomics).  Errors as m355_hybrid_loss_*:
 * null pointer / non-positive size M355_EINVALID_ARG, N*C > 65535 M355_EUNSUPPORTED, workspace M355_EWORKSPACE; nothing
 * is launched then.  m355_binary_loss_workspace is 0 for a non-positive size.
 */
size_t m355_binary_loss_workspace(int32_t N, int32_t C, int64_t S);
int m355_binary_loss_fwd(const float* x, const float* t, int32_t N, int32_t C, int64_t S, float dice_weight,
                         const float* class_weights /* [C] or NULL */, const float* pos_weight /* [C] or NULL */,
                         int32_t square_dice, int32_t from_logits, float* out3, float* sums /* [N*C*5] */,
                         void* workspace, size_t workspace_bytes, void* stream);
/* dx = dloss * d(loss)/dx in one pass, closed form from the saved sums: the gradient with respect to p, or with
 * from_logits to z directly (log part cw (-pw t sigmoid(-z) + (1 - t) sigmoid(z)) / (N C S), Dice part times
 * p sigmoid(-z)), which stays alive where a sigmoid's own backward multiplies by p (1 - p) = 0.  Writes dx[0, N*C*S). */
int m355_binary_loss_bwd(const float* x, const float* t, const float* sums, const float* dloss /* device scalar */,
                         int32_t N, int32_t C, int64_t S, float dice_weight, const float* class_weights,
                         const float* pos_weight, int32_t square_dice, int32_t from_logits, float* dx, void* stream);

/* ------------------------------------------------ focal Tversky loss
 * HybridFocalTverskyLoss (criterions/hybrid_focal_tversky_loss.py): a Tversky term that weighs false
 * positives (alpha) and false negatives (beta) separately, raised to a power, plus a focal cross-entropy on the positive
 * half.  x and the target t (values in [0, 1], soft targets allowed): dense fp32 [N, C, S], rows at nc * S for any S (no
 * alignment requirement).  eps = 1e-8.
 *   from_logits == 0   x = p (probabilities): q = 1 - p, lp = log((p + eps) / (1 + eps)); no expf is evaluated
 *   from_logits != 0   x = z (logits), the log-softmax over the C channels of a voxel is taken here: m = max_c z_c,
 *                      s = sum_c exp(z_c - m), lp_c = (z_c - m) - log s, p_c = exp(z_c - m) / s, q_c = -expm1(lp_c); no eps
 *   TP = sum p t, FP = sum p (1 - t), FN = sum q t, each accumulated directly
 *   TI = TP / (TP + alpha FP + beta FN + eps/2),  u = max(0, 1 - TI),  tversky_nc = v[c] * u^e   (e = tversky_power;
 *        v = tversky_class_weights or 1; no powf for e == 1)
 *   focal_nc = w[c] * sum(t q^gamma lp) / S   (w = focal_class_weights or 1; gamma = focal_gamma: 0 -- the factor is
 *        exactly 1 --, 1, 2, 3 by multiplication, any other value >= 1 by powf, 0 at q == 0)
 *   out3 = {loss, tversky_loss, focal_loss} = {(1 - tw) focal_loss + tw tversky_loss, mean(tversky_nc), mean(-focal_nc)}
 * With alpha = beta = 0.5, e = 1, gamma = 0 and from_logits == 0 this is m355_hybrid_loss_fwd without square_dice.
 * sums (kept for backward): [N*C*4] = {TP, FP, FN, sum t q^gamma lp}, unweighted.
 * Deterministic (fp32 per lane, then fp64 block and cross-chunk sums in a fixed order, no float atomics); a misaligned
 * view gives the bits of its aligned copy.  Errors: null pointer, non-positive size, alpha or beta negative or not
 * finite, tversky_power <= 0, focal_gamma outside {0} u [1, inf) M355_EINVALID_ARG; N*C > 65535 M355_EUNSUPPORTED (no
 * limit on C of its own); workspace M355_EWORKSPACE; nothing is launched then.  m355_focal_tversky_workspace is 0 for a
 * non-positive size.
 */
size_t m355_focal_tversky_workspace(int32_t N, int32_t C, int64_t S);
int m355_focal_tversky_fwd(const float* x, const float* t, int32_t N, int32_t C, int64_t S,
                           float tversky_weight, float alpha, float beta, float tversky_power, float focal_gamma,
                           const float* focal_class_weights /* [C] or NULL */, const float* tversky_class_weights /* [C] or NULL */,
                           int32_t from_logits, float* out3, float* sums /* [N*C*4] */,
                           void* workspace, size_t workspace_bytes, void* stream);
/* dx = dloss * d(loss)/dx in one pass, closed form from the saved sums (the Tversky part is 0 where u == 0, for e < 1
 * too): the gradient with respect to p, or with from_logits to z directly,
 *   dz_k = g_k - p_k sum_c g_c + p_k (h_k - sum_c p_c h_c),   g the focal and h the Tversky gradient per channel,
 * which stays alive at a voxel saturated on the wrong class, where a softmax's own backward multiplies by p_k = 0.
 * Up to 16 channels the per-voxel values stay in registers between the sums over c and their use; above that the planes
 * are read again.  Writes dx[0, N*C*S). */
int m355_focal_tversky_bwd(const float* x, const float* t, const float* sums, const float* dloss /* device scalar */,
                           int32_t N, int32_t C, int64_t S, float tversky_weight, float alpha, float beta,
                           float tversky_power, float focal_gamma, const float* focal_class_weights,
                           const float* tversky_class_weights, int32_t from_logits, float* dx, void* stream);

/* ------------------------------------------------ top-k cross-entropy + Dice loss
 * HybridTopKDiceLoss (criterions/hybrid_topk_dice_loss.py): the Dice term of m355_hybrid_loss_fwd plus a
 * cross-entropy averaged over the k largest per-voxel values of the whole batch only (online hard-example mining).  x and
 * the target t: dense fp32 [N, C, S], rows at nc * S for any S (no alignment requirement).  eps = 1e-8, M = N * S.
 *   from_logits == 0   x = p (probabilities): lp = log((p + eps) / (1 + eps))
 *   from_logits != 0   x = z (logits), the log-softmax over the C channels of a voxel is taken here as in
 *                      m355_focal_tversky_fwd; p = exp(lp) is formed in registers; no eps
 *   e[n, s] = -sum_c w[c] t[n,c,s] lp[n,c,s]   (w = class_weights or 1, any sign)
 *   tau = the k-th largest of the M values of e (a three-pass 11 / 11 / 10-bit radix select on keys that order like the
 *         floats; every NaN orders above +inf, -0 is +0), n_gt = #{e > tau}, n_eq = #{e == tau}
 *   logistic_loss = (sum_{e > tau} e + (k - n_gt) tau) / (C k): ties at tau share what is left of k, none is drawn
 *   dice_loss: m355_hybrid_loss_fwd's, on p, with its square_dice
 *   out3 = {loss, dice_loss, logistic_loss} = {(1 - dice_weight) logistic_loss + dice_weight dice_loss, ..}
 * With k = M the log term is m355_hybrid_loss_fwd's (from_logits == 0) or m355_focal_tversky_fwd's at gamma 0.
 * k: the count itself, 1 <= k <= M -- or, with k_device != NULL, a device int64 scalar read by the kernels (clamped to
 * [1, M] there; `k` is ignored), so a captured launch follows a schedule of k.
 * Kept for backward: sums [N*C*3] = the Dice sums {sum p t, sum p(^2), sum t(^2)}; e [N*S]; state [4 words] = {tau, r =
 * (k - n_gt) / n_eq as fp32, k as int64}.
 * Deterministic (integer atomics on the histograms only; fp32 per lane, then fp64 block and cross-chunk sums in a fixed
 * order); a misaligned view gives the bits of its aligned copy.  Errors: null pointer, non-positive size, k outside
 * [1, M] M355_EINVALID_ARG; N*C > 65535 or M > 2^32 - 1 M355_EUNSUPPORTED; workspace M355_EWORKSPACE; nothing is
 * launched then.  m355_topk_loss_workspace is 0 for a non-positive size.
 */
size_t m355_topk_loss_workspace(int32_t N, int32_t C, int64_t S);
int m355_topk_loss_fwd(const float* x, const float* t, int32_t N, int32_t C, int64_t S, int64_t k,
                       const int64_t* k_device /* device scalar or NULL */, float dice_weight,
                       const float* class_weights /* [C] or NULL */, int32_t square_dice, int32_t from_logits,
                       float* out3, float* sums /* [N*C*3] */, float* e /* [N*S] */, void* state /* 16 bytes */,
                       void* workspace, size_t workspace_bytes, void* stream);
/* dx = dloss * d(loss)/dx in one pass from x, t, the saved e, sums and state.  A voxel's selection weight sel is 1 where
 * e > tau, r where e == tau, 0 otherwise (sum sel == k); kl = dloss (1 - dice_weight) sel / (C k); h = the Dice gradient
 * with respect to p.
 *   from_logits == 0   dx_c = h_c - kl w_c t_c / (x_c + eps)
 *   from_logits != 0   dz_c = p_c (h_c - sum_j p_j h_j + kl sum_j w_j t_j) - kl w_c t_c
 * Up to 16 channels the per-voxel values stay in registers; above that the planes are read again.  Writes dx[0, N*C*S). */
int m355_topk_loss_bwd(const float* x, const float* t, const float* e, const float* sums, const void* state,
                       const float* dloss /* device scalar */, int32_t N, int32_t C, int64_t S, float dice_weight,
                       const float* class_weights, int32_t square_dice, int32_t from_logits, float* dx, void* stream);

/* ------------------------------------------------ segmented radix sort
 * R segments of M 32-bit keys each, dense [R, M], sorted ascending segment by segment (csrc/segmented_sort.hip, DESIGN
 * §4.30): an LSD radix sort over the bits [0, end_bit) in ceil(end_bit / 8) passes of 8-bit digits; the bits above end_bit
 * travel with their key and do not order it.  Key-only.  `keys` is not written; `out` must not overlap it.
 * Every pass is stable: within a workgroup a key's rank comes from wave-wide digit matching (64-bit ballots) and per-wave
 * digit counts in LDS, added in wave order and, by a scan kernel, in tile order.  Integer atomics count a tile's digits;
 * none decides a position, so a call repeats bit for bit.  No allocation, synchronisation or host read: it can be
 * captured in a graph.
 *   workspace = round_up(4 R M, 256) + 4 * 256 * R * (ceil(M / tile) + 1) + 256 bytes (the second key buffer, the digit
 *   counts of the tiles and of the segments), tile = m355_segmented_sort_tile() keys per workgroup;
 *   m355_segmented_sort_workspace is 0 for a non-positive size.
 * Errors, nothing is launched: null pointer, non-positive size, end_bit outside [1, 32], keys == out M355_EINVALID_ARG;
 * R > 65535 or M > 2^31 - 1 M355_EUNSUPPORTED; workspace M355_EWORKSPACE.
 */
size_t m355_segmented_sort_workspace(int64_t R, int64_t M);
int32_t m355_segmented_sort_tile(void);
int m355_segmented_sort_u32(const uint32_t* keys, uint32_t* out, int64_t R, int64_t M, int32_t end_bit, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ------------------------------------------------ Lovasz-softmax loss
 * LovaszLoss (criterions/lovasz_loss.py; Berman et al., CVPR 2018): the convex surrogate of the Jaccard
 * index.  p (probabilities) and the target t: dense fp32 [N, C, S], rows at nc * S for any S (no alignment requirement).
 *   segments   per_image == 0: one per channel over the M = N S voxels of the batch, R = C; per_image != 0: one per
 *              (n, c), M = S, R = N C
 *   element    fg = (t >= 0.5), e = |fg - p| in one fp32 subtraction, G = the segment's foreground count
 *   sorted by e, descending: F(i) = the foreground elements among the first i, I(i) = G - F(i), U(i) = G + i - F(i),
 *              J(0) = 0, J(i) = 1 - I(i) / U(i);  L_r = sum_i e_(i) (J(i) - J(i - 1))
 *   ties       the elements of one value of e are a group [lo, hi) of the sorted order and each gets
 *              dL_r/de = (J(hi) - J(lo)) / (hi - lo), the mean of the subgradients of every order of the group;
 *              J(hi) - J(lo) = (I(lo) U(hi) - I(hi) U(lo)) / (U(lo) U(hi)) from 64-bit integer products and one fp64
 *              division (J(hi) for lo = 0);  de/dp = -1 for foreground, +1 for background, also at e = 0
 *   reduction  a segment takes part when all_classes != 0 or G > 0, with weight class_weights[c] (NULL: 1, expected
 *              >= 0).  per_image == 0: loss = sum_c w_c L_c / sum_c w_c over them; per_image != 0: that mean per image
 *              first (0 for an image without a segment), then the mean over the N images.  Nothing to average: loss 0,
 *              gradient 0.  The decision is taken on the device.
 *   out2 = {loss, the number of segments of non-zero weight that took part}
 * A NaN or a prediction outside [0, 1] gives a NaN loss and gradient; the key pass clamps such an e to [0, 1] and raises a
 * status word that the finalize kernel reads, so no access leaves the buffers.
 * Kept for backward: sorted_keys [R, M] (key = ~((bits(e) << 1) | fg) & 0x7fffffff, ascending: 31 bits, since e <= 1
 * means bits(e) < 2^30), F [R, M] (F(i) for i = 0 .. M - 1) and state [R x 2 words] = {G, the segment's coefficient
 * dloss/dL_r as fp32}: 8 bytes per (class, voxel).
 *   workspace = round_up(4 R M, 256) + round_up(m355_segmented_sort_workspace(R, M), 256) + round_up(4 R T, 256) + 8 R T
 *   + 8 R + 256 bytes, T = ceil(M / tile), tile = m355_lovasz_loss_tile(): the unsorted keys, the sort's workspace, the
 *   tiles' foreground counts and fp64 partial losses, L_r, the status word.  0 for sizes the entry points refuse.
 * Deterministic: the sort decides no position by an atomic and equal keys are equal elements; the sums are fp64, per
 * lane in index order, then block and tile sums in a fixed order; the one atomic is the OR into the status word.  A
 * misaligned view gives the bits of its aligned copy.  Errors: null pointer, non-positive size M355_EINVALID_ARG;
 * N*C > 65535 or M > 2^31 - 1 M355_EUNSUPPORTED; workspace M355_EWORKSPACE; nothing is launched then.
 */
size_t m355_lovasz_loss_workspace(int32_t N, int32_t C, int64_t S, int32_t per_image);
int32_t m355_lovasz_loss_tile(void);
int m355_lovasz_loss_fwd(const float* p, const float* t, int32_t N, int32_t C, int64_t S, int32_t per_image,
                         int32_t all_classes, const float* class_weights /* [C] or NULL */, float* out2,
                         uint32_t* sorted_keys /* [R*M] */, uint32_t* F /* [R*M] */, void* state /* 8 R bytes */,
                         void* workspace, size_t workspace_bytes, void* stream);
/* dx = dloss * d(loss)/dp in one launch: every element recomputes its key, finds its group [lo, hi) by two binary
 * searches on key >> 1 in its segment's sorted keys, reads F(lo) and F(hi) and writes
 * dx = dloss * coefficient * sign * (J(hi) - J(lo)) / (hi - lo).  Writes dx[0, N*C*S). */
int m355_lovasz_loss_bwd(const float* p, const float* t, const uint32_t* sorted_keys, const uint32_t* F,
                         const void* state, const float* dloss /* device scalar */, int32_t N, int32_t C, int64_t S,
                         int32_t per_image, float* dx, void* stream);

/* ------------------------------------------------ target pyramid (deep supervision)
 * The targets of the auxiliary heads of models.DeepSupervisionUNet (criterions.DeepSupervisionLoss): one
 * launch reads a dense fp32 target y[N, C, D, H, W] once and writes its `levels` coarser levels, level j (1 <= j <= levels)
 * of spatial size (D, H, W) / 2^j.
 *   M355_PYRAMID_AREA     out_j[n, c, z, y, x] = mean of the 2^j cube of y that starts at (z, y, x) 2^j: the soft target of
 *                         the coarse cell (F.avg_pool3d(y, 2^j)).  Level 1 is the pairwise sum of its 8 voxels times 0.125,
 *                         level j the same of its 8 level j-1 cells; for a one-hot target every partial sum is an integer
 *                         <= 4096 and every scale a power of two, so the result is exact.
 *   M355_PYRAMID_NEAREST  out_j[n, c, z, y, x] = y[n, c, z 2^j, y 2^j, x 2^j]: F.interpolate(y, scale_factor=2^-j,
 *                         mode='nearest'), a pure copy.
 * out: the levels back to back, level 1 first, each dense NCDHW; m355_target_pyramid_elems floats in all (0 for arguments
 * m355_target_pyramid refuses).  y and out need 4-byte alignment only: rows go as 16-byte loads where their address allows
 * it, the result does not depend on it.  Element offsets are 64-bit.  No atomics, one summation order, no workspace: a call
 * repeats bit for bit, and it can be captured in a graph.
 * Errors, nothing is launched: null pointer, non-positive size, levels outside 1..4, mode other than the two above
 * M355_EINVALID_ARG; D, H or W not divisible by 2^levels M355_EUNSUPPORTED (the message names the dimension).
 */
enum { M355_PYRAMID_AREA = 0, M355_PYRAMID_NEAREST = 1 };
int64_t m355_target_pyramid_elems(int32_t N, int32_t C, int32_t D, int32_t H, int32_t W, int32_t levels);
int m355_target_pyramid(const float* y, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W, int32_t levels,
                        int32_t mode, float* out, void* stream);

/* ------------------------------------------------------------ elementwise
 * torch.cat([x_up, x_skip], dim=1) (models/modular_unet.py:97) when the
 * producer could not write into the concat buffer directly: strided copy of
 * [N, C, S] (src_batch_stride) into a channel slice (dst_batch_stride).
 * Dropout3d (components.py:58-60,70-71): y = x * scale[n*C + c].
 */
int m355_copy_channels(const float* src, float* dst, int32_t N, int32_t C, int64_t S,
                       int64_t src_batch_stride, int64_t dst_batch_stride, void* stream);
int m355_channel_scale(const float* x, const float* scale, float* y, int32_t N, int32_t C,
                       int64_t S, void* stream);
/* y = a + b (dense, n elements): residual add when not fused. */
int m355_add(const float* a, const float* b, float* y, int64_t n, void* stream);

/* Space-to-depth / depth-to-space by 2 along D, H, W (each other's inverse and adjoint):
 *   s2d: y[n, c*8 + p, z, y, x] = x[n, c, 2z+pz, 2y+py, 2x+px],  p = pz*4 + py*2 + px   (input D,H,W even)
 *   d2s: the inverse; D,H,W below are always those of the FULL-resolution tensor.
 * They turn the reference's strided Blur convolutions (components.py:91-154: effective 4x4x4 kernel,
 * stride 2, padding 1) into stride-1 3x3x3 convolutions that run on the MFMA path:
 *   BlurConv3d:          conv3(s2d(x), W') ;   BlurConvTranspose3d: d2s(conv3(x, W'')).
 * Alignment: the FULL-resolution tensor (x of s2d, y of d2s) 8-byte aligned with an even batch stride (the kernel moves
 * x pairs); M355_EUNSUPPORTED otherwise, nothing is launched.  The packed tensor has no requirement. */
int m355_space_to_depth2(const float* x, float* y, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                         int64_t x_batch_stride, int64_t y_batch_stride, void* stream);
int m355_depth_to_space2(const float* x, float* y, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                         int64_t x_batch_stride, int64_t y_batch_stride, void* stream);

/* Weight transform of BlurConv3d / BlurConvTranspose3d (reference models/components.py:112-119,
 * 145-152) for 3x3x3 filters: optional per-filter standardisation (unbiased std, eps 1e-5), the
 * depthwise 2x2x2 box blur with padding 1 (scale[b] = value of the module's `kernel` buffer for
 * dim-1 channel b) giving a 4x4x4 filter, and its rearrangement into the sparse 3x3x3 filter of the
 * space-to-depth formulation, in one pass.  w: [A][B][27] (the module's weight: A = Cout, B = Cin for
 * the strided conv; A = Cin, B = Cout for the transposed conv).
 *   transposed == 0:  wexp [A][8B][27]   (conv3d weight over the space-to-depth input)
 *   transposed == 1:  wexp [8B][A][27]   (conv3d weight producing the 8 output parities)
 * mean_std: [A][2] saved statistics (written by fwd, read by bwd; may be NULL when standardize == 0).
 * bwd: dw = d(loss)/d(w) from dwexp. */
int m355_blur_weight_fwd(const float* w, const float* scale, float* wexp, float* mean_std, int32_t A, int32_t B,
                         int32_t standardize, int32_t transposed, void* stream);
int m355_blur_weight_bwd(const float* dwexp, const float* w, const float* scale, const float* mean_std, float* dw,
                         int32_t A, int32_t B, int32_t standardize, int32_t transposed, void* stream);

/* WSConv3d weight standardisation (reference models/components.py:81-88; also the optional first step of
 * the Blur convolutions, folded into m355_blur_weight_* above): per dim-0 filter a of n = Cin*k^3 entries,
 *   wn = (w - mean_a) / (std_a + 1e-5)   with torch.std's unbiased estimator.
 * mean_std [A][2] is written by fwd and read by bwd (dw from dwn). */
int m355_weight_standardize_fwd(const float* w, float* wn, float* mean_std, int32_t A, int32_t n, void* stream);
int m355_weight_standardize_bwd(const float* dwn, const float* w, const float* mean_std, float* dw, int32_t A,
                                int32_t n, void* stream);

/* Device-side weighted patch sampling.  Replaces tio.WeightedSampler(patch_size,
 * probability_map='patch_probability') of the reference's patch loader (data_loader_factory.py:36-54,
 * research/msseg2/msseg2.py:148-149; the map comes from ImageFromLabels, transforms/image_from_labels.py:11-57): the
 * patch CENTRE is drawn with probability proportional to the map (negative entries count as 0) restricted to centres
 * whose patch lies inside the volume; the returned location is the patch CORNER.  m355_sampler_build: a two-level
 * cumulative table of the map ((ceil(V / 1024) + 1) doubles, once per map); table[last] is the total weight (the caller
 * checks it is positive).  m355_sampler_draw: locations[p] = corner of the patch whose centre is the first voxel with
 * cumulative weight > u[p] * total, u in [0, 1) -- one wave per patch, one launch per batch; feed the locations to
 * m355_patch_gather.  fp64 sums in a fixed order: a draw is a pure function of (map, u). */
size_t m355_sampler_table_bytes(int32_t V0, int32_t V1, int32_t V2);
int m355_sampler_build(const float* prob, int32_t V0, int32_t V1, int32_t V2, int32_t p0, int32_t p1, int32_t p2,
                       double* table, void* stream);
int m355_sampler_draw(const float* prob, const double* table, int32_t V0, int32_t V1, int32_t V2, int32_t p0, int32_t p1,
                      int32_t p2, const double* u, int32_t P, int32_t* locations, void* stream);

/* The whole aggregation of a sliding window in one pass (torchio GridAggregator('average') as driven by
 * PatchPredict.predict, prediction.py:124-152): tiles [n0*n1*n2, C, ps0, ps1, ps2] in GridSampler order (tile index =
 * (a * n1 + b) * n2 + c over the per-axis start lists starts[0..n0), [n0..n0+n1), [n0+n1..n0+n1+n2), device int32, in
 * coordinates of the padded volume) -> out [C, V0, V1, V2] = per-voxel mean of the covering tiles, where voxel v of the
 * output is voxel v + border of the padded volume (border = 0: no padding).  Same bits as m355_patch_accumulate over
 * all tiles in order followed by m355_patch_finalize(_crop).  Every output voxel must be covered by a tile. */
int m355_patch_aggregate_grid(const float* tiles, const int32_t* starts, int32_t n0, int32_t n1, int32_t n2, float* out,
                              int32_t C, int32_t V0, int32_t V1, int32_t V2, int32_t ps0, int32_t ps1, int32_t ps2,
                              int32_t b0, int32_t b1, int32_t b2, void* stream);

/* The same pass with a separable window (torchio GridAggregator('hann'): PatchPredict(overlap_mode='hann')).  Tiles,
 * starts, border and out as above; window = w0 | w1 | w2, ps0 + ps1 + ps2 device floats given as data (for 'hann' axis
 * x holds torch.hann_window(psx + 2, periodic=False)[1:-1], psx strictly positive values; the kernel evaluates no
 * cosine, so any positive window blends).  With d = v + border - start the offset of a voxel inside a covering tile,
 *   w(d)      = (w0[d0] * w1[d1]) * w2[d2]
 *   sum[c, v] = sum over the covering tiles, in tile order, of tile[c, d] * w(d)
 *   wsum[v]   = sum over the covering tiles, in tile order, of w(d)            (one weight sum for all channels)
 *   out[c, v] = sum[c, v] / wsum[v]
 * each product, sum and the quotient one rounded fp32 operation, never contracted into an fma: the bits of torchio's
 * sequential `out[...] += patch * win; mask[...] += win` over the tiles followed by `out / mask`.  A voxel under one
 * tile gives (t * w) / w, within an ulp or so of t.  An all-ones window gives m355_patch_aggregate_grid's bits. */
int m355_patch_aggregate_grid_weighted(const float* tiles, const int32_t* starts, int32_t n0, int32_t n1, int32_t n2,
                                       const float* window /* device, ps0 + ps1 + ps2 floats: w0 | w1 | w2 */,
                                       float* out, int32_t C, int32_t V0, int32_t V1, int32_t V2,
                                       int32_t ps0, int32_t ps1, int32_t ps2, int32_t b0, int32_t b1, int32_t b2, void* stream);

/* ------------------------------------------------- sliding-window patches
 * PatchPredict (prediction.py:124-152) delegates tiling/aggregation to torchio
 * 0.18.45 GridSampler / GridAggregator(overlap_mode='average').  These entry
 * points are the tensor-level part: gather P patches [P, C, ps0, ps1, ps2] from
 * a volume [C, V0, V1, V2] at integer corner locations loc[P,3] (i0,j0,k0), and
 * the aggregation out[c,v] = (sum over covering patches, in patch order) /
 * (number of covering patches).  m355_patch_accumulate ADDS to accum and count, so that a volume's patches may arrive in
 * several batches: both are zeroed by the CALLER before the first batch.
 */
int m355_patch_gather(const float* volume, const int32_t* loc, float* patches,
                      int32_t P, int32_t C, int32_t V0, int32_t V1, int32_t V2,
                      int32_t ps0, int32_t ps1, int32_t ps2, void* stream);
int m355_patch_accumulate(const float* patches, const int32_t* loc, float* accum /* [C,V] */,
                          float* count /* [V] */, int32_t P, int32_t C,
                          int32_t V0, int32_t V1, int32_t V2,
                          int32_t ps0, int32_t ps1, int32_t ps2, void* stream);
int m355_patch_finalize(const float* accum, const float* count, float* out,
                        int32_t C, int64_t V, void* stream);

/* padding_mode != None (prediction.py:114,132; research/msseg2/competition/ms-inference.py:35 uses "edge"):
 * torchio pads the volume by b = patch_overlap // 2 per side (numpy.pad) before tiling and crops the aggregate.
 * The padded volume is never materialised: loc is in PADDED coordinates, the gather maps indices back
 * (mode: 0 constant `value`, 1 edge, 2 reflect, 3 symmetric, 4 wrap -- numpy.pad's definitions), the accumulators
 * have the padded size [P0,P1,P2] = V + 2b, and the finalize writes the cropped [C, V0,V1,V2] average. */
int m355_patch_gather_padded(const float* volume, const int32_t* loc, float* patches, int32_t P, int32_t C,
                             int32_t V0, int32_t V1, int32_t V2, int32_t ps0, int32_t ps1, int32_t ps2,
                             int32_t b0, int32_t b1, int32_t b2, int32_t mode, float value, void* stream);
int m355_patch_finalize_crop(const float* accum, const float* count, float* out, int32_t C, int32_t P0, int32_t P1,
                             int32_t P2, int32_t b0, int32_t b1, int32_t b2, void* stream);

/* ----------------------------------------------------- evaluation counts
 * CustomArgMax (transforms/custom_label_transforms.py:267) + the TP/FP/FN/TN
 * sums of SegmentationEvaluator (evaluators/segmentation_evaluator.py:69-86):
 * argmax over C of prob [N,C,S] (first max wins, as torch.argmax) against an
 * integer label map [N,S]; counts[n, c, 4] = {TP, FP, FN, TN} as int64.
 * argmax_out (int32 [N,S]) may be NULL.
 */
int m355_argmax_confusion(const float* prob, const int32_t* target, int32_t* argmax_out,
                          int64_t* counts, int32_t N, int32_t C, int64_t S, void* stream);

/* ------------------------------------------------- test-time ensembles
 * EnsembleFlips / EnsembleOrientations / EnsembleModels (models/ensemble.py:38-103): a member predicts on
 * x.permute(0, 1, *perm).flip(f) and the reference maps the prediction back with .flip(f).permute(inverse) before
 * apply_strategy (:16-35) stacks all members and takes the mean, or argmax -> mode -> one_hot.
 * size3 = canonical spatial size; perm3[j] in {0,1,2} = canonical axis of member axis j; flip_mask bit j = member
 * axis j is reversed (identity: perm3 = {0,1,2}, flip_mask = 0).
 *   m355_flip_permute        member input [N,C,size3[perm]] from x [N,C,size3], one gather pass
 *   m355_ensemble_accumulate reads a member prediction THROUGH the inverse transform (it is never mapped back or
 *                            stacked): mode 0: acc[N,C,S] (+)= pred; mode 1: votes[N,C,S] (int32) += 1 at the
 *                            member's argmax class (first maximum, as torch.argmax); first != 0 initialises (the
 *                            accumulator's contents on entry are then irrelevant; with first == 0 they are the sum so far)
 *   m355_ensemble_finalize   mode 0: mean_out = acc / members; mode 1: onehot_out[N,C,S] (int64) of the class with
 *                            the most votes, ties -> the smallest class index (torch.mode on the CPU) */
int m355_flip_permute(const float* x, float* member, int32_t N, int32_t C, const int32_t* size3, const int32_t* perm3,
                      int32_t flip_mask, void* stream);
int m355_ensemble_accumulate(const float* pred, float* acc, int32_t* votes, int32_t N, int32_t C, const int32_t* size3,
                             const int32_t* perm3, int32_t flip_mask, int32_t mode, int32_t first, void* stream);
int m355_ensemble_finalize(const float* acc, const int32_t* votes, float* mean_out, int64_t* onehot_out, int32_t N,
                           int32_t C, int64_t S, int32_t members, int32_t mode, void* stream);

/* ------------------------------------------ uncertainty maps (csrc/uncertainty.hip)
 * Entropies of probability volumes, in float32, natural logarithm.  One expression for all three entry points, so
 * equal probabilities give equal bits:
 *   term(p)  = p > 0 ? p * logf(p) : 0      (0 at p <= 0; a NaN passes through and makes its voxel NaN, no other)
 *   M355_UQ_CATEGORICAL  h(p[0..C)) = -(term(p_0) + term(p_1) + ...), summed in channel order: K = 1 map per volume
 *   M355_UQ_BINARY       h(p) = -(term(p) + term(1 - p)) of every channel on its own, 1 - p in float32, the two
 *                        products and their sum formed exactly and rounded once: K = C maps
 *   m355_predictive_entropy            probs [N, C, S] float32 / bfloat16 / float16 (M355_EV_* codes, 16-bit values
 *                                      widened exactly) -> entropy [N, K, S] float32 and, unless NULL, confidence
 *                                      [N, 1, S]: the maximum channel value (a NaN is the maximum).  One pass.
 *   m355_ensemble_entropy_accumulate   reads a member prediction through the inverse transform of
 *                                      m355_ensemble_accumulate (size3, perm3, flip_mask as there) and adds the member's
 *                                      entropy to eacc [N, K, S] in canonical orientation; first != 0 initialises (the
 *                                      accumulator's contents on entry are then irrelevant).
 *   m355_ensemble_uncertainty_finalize from acc [N, C, S] (the running sum of m355_ensemble_accumulate, mode 0), eacc
 *                                      and the member count: entropy = h(acc * (1 / members)), the product being the one
 *                                      m355_ensemble_finalize writes as the mean, so entropy has the bits of
 *                                      m355_predictive_entropy of that mean; expected_entropy = eacc / members;
 *                                      mutual_information = max(entropy - expected_entropy, 0), a NaN staying NaN;
 *                                      confidence [N, 1, S] = max_c of the mean.  The first three are [N, K, S]. */
enum { M355_UQ_CATEGORICAL = 0, M355_UQ_BINARY = 1 };
int m355_predictive_entropy(const void* probs, int32_t dtype, float* entropy, float* confidence /* or NULL */, int32_t N,
                            int32_t C, int64_t S, int32_t kind, void* stream);
int m355_ensemble_entropy_accumulate(const float* pred, float* eacc, int32_t N, int32_t C, const int32_t* size3,
                                     const int32_t* perm3, int32_t flip_mask, int32_t kind, int32_t first, void* stream);
int m355_ensemble_uncertainty_finalize(const float* acc, const float* eacc, float* entropy, float* expected_entropy,
                                       float* mutual_information, float* confidence, int32_t N, int32_t C, int64_t S,
                                       int32_t members, int32_t kind, void* stream);

/* ------------------------------------------ connected components + post-processing
 * skimage.morphology.label / remove_small_holes / dilation and the np.unique / torch.unique counts under
 * post_processing.py (keep_components, remove_holes, remove_small_components) and
 * evaluators/instance_segmentation_evaluator.py (lesion-wise detection).  Volumes are one int32 [D,H,W] map with
 * fewer than 2^31 voxels (more: M355_EINVALID_ARG).
 *   m355_ccl_label        connected components: mode 0 = non-zero voxels, neighbours connect when they hold the SAME
 *                         value (multi-class, as skimage); mode 1 = voxels <= 0, all connect (the holes of x > 0).
 *                         connectivity 1 / 2 / 3 = 6 / 18 / 26 neighbours.  labels: 0 background, 1..n numbered in
 *                         raster order of each component's first voxel (scipy.ndimage.label's numbering).  *n_out
 *                         (device int32) = n, or -1 when a bounded find / union loop hit its bound (labels then
 *                         undefined).  Workspace: m355_ccl_workspace(D, H, W) bytes.
 *   m355_label_histogram  counts[k - lo] (int64 [nbins], zeroed by the call) = voxels whose key k lies in
 *                         [lo, lo + nbins): k = a[v] (b == NULL) or a[v] * bstride + b[v] (overlap table of two label
 *                         maps).  minmax (int32[2], may be NULL; 1-D keys) receives min and max of a.
 *   m355_masked_dilate6   one Jacobi step of the 6-neighbour grey dilation (ndi.grey_dilation, cross footprint; the
 *                         volume border adds nothing), src -> dst (src != dst), changed only where
 *                         flag[labels[v]] != 0.  class_rank == NULL: such a voxel takes the max of src over itself and
 *                         its neighbours.  Otherwise keys are class_rank[src - lo] (0 for masked voxels) and a masked
 *                         voxel whose neighbours' largest key K is > 0 takes rank_class[K].  *changed (device int64) =
 *                         voxels with dst != src.
 *   m355_label_convert_in / _out  boundary casts: dtype 0 uint8/bool, 1 int8, 2 int16, 3 int32, 4 int64.  in: op 0
 *                         copy (int64 outside int32 sets *status), 1 (x == 0), 2 (x > 0).  out: dst = zero_where ?
 *                         (zero_where[v] ? 0 : orig[v]) : src[v].
 */
size_t m355_ccl_workspace(int32_t D, int32_t H, int32_t W);
int m355_ccl_label(const int32_t* x, int32_t* labels, int32_t* n_out, int32_t D, int32_t H, int32_t W,
                   int32_t connectivity, int32_t mode, void* workspace, size_t ws_bytes, void* stream);
int m355_label_histogram(const int32_t* a, const int32_t* b, int64_t nvox, int64_t bstride, int64_t lo, int64_t nbins,
                         int64_t* counts, int32_t* minmax, void* stream);
int m355_masked_dilate6(const int32_t* src, int32_t* dst, int32_t D, int32_t H, int32_t W, const int32_t* labels,
                        const int32_t* flag, const int32_t* class_rank, const int32_t* rank_class, int32_t lo,
                        int64_t* changed, void* stream);
int m355_label_convert_in(const void* src, int32_t dtype, int32_t op, int32_t* dst, int64_t n, int32_t* status,
                          void* stream);
int m355_label_convert_out(const int32_t* src, const int32_t* zero_where, const void* orig, void* dst, int32_t dtype,
                           int64_t n, void* stream);

/* ------------------------------------------ training augmentation
 * The per-voxel work of the torchio augmentation chains of the reference's production configs
 * (research/dmri_hippo/configs/main_config.py:86-100, research/msseg2/msseg2.py:44-57); parameters are drawn on the
 * host (augmentation.py).  Volumes are float32 [C, D, H, W] (label maps of the resample: 1-, 4- or 8-byte
 * elements) with fewer than 2^31 voxels per channel.
 *   m355_aug_resample     y[c, p] = x[c] at q = M p + t + B d(p) (mat12 = [M | t] row-major, host; disp9 = B, host,
 *                         NULL = identity), p an index of the output size out3, q an index of the input size in3.  d =
 *                         the cubic B-spline displacement of the control grid (device float [K0][K1][K2][3], in input
 *                         voxels before B; NULL = none; grid3 = K, each >= 4) at u = (p + 0.5)(K - 3) / out3.  q inside
 *                         when -0.5 <= q < in3 - 0.5 on every axis, else pad[c] (device double per channel; NULL =
 *                         pad_const; 1- and 8-byte elements pad with 0).  interp 0 nearest clamp(floor(q + 0.5)),
 *                         1 trilinear (neighbours clamped), 2 cubic B-spline on coefficients (m355_aug_prefilter) with
 *                         mirrored neighbours; 1- and 8-byte elements: nearest only.  x != y.
 *   m355_aug_prefilter    cubic B-spline coefficients of x in place (scipy spline_filter order 3, mode 'mirror').
 *   m355_aug_order_stats  out[q] (device double, q < nq <= 2) = lerp(v[ks[q]], v[ks[q] + 1], fracs[q]) (numpy's _lerp;
 *                         ks[q] + 1 capped at n - 1), v = the sorted values of ALL channels of x after the stage list.
 *                         Exact radix select; ranks {0, n - 1} with fracs 0 take one min / max pass.  Workspace:
 *                         m355_aug_workspace() bytes.  ks and fracs are host arrays.
 *   m355_aug_intensity    y = x after the stage list (in place allowed).
 *   m355_aug_blur         one axis of scipy gaussian_filter (mode 'reflect', radius int(4 sigma + 0.5), sigma in voxels),
 *                         then the stage list (no M355_AUG_RESCALE) as an epilogue: the host passes the bias / gamma /
 *                         noise stages that follow a blur to its last axis.  x != y.
 *   m355_aug_otsu_pad     pad[c] (device double) = mean of the face voxels of channel c whose OTSU_BINS = 128-bin
 *                         histogram bin lies at or below the Otsu split (all face voxels when none).
 *   m355_aug_channel_minmax  out[c] (device double) = min (which 0) or max (which 1) of channel c, all channels in one
 *                         pass.  Workspace: >= 8 * C bytes (m355_aug_workspace() covers C <= 4096). */
#define M355_AUG_MAX_STAGES 8
enum {
  M355_AUG_BIAS = 0,     /* v *= exp(sum vec[j] x^a y^b z^c), a + b + c <= order, torchio's term order and coordinates */
  M355_AUG_RESCALE = 1,  /* lo, hi = (float) stats[0..1] (device); lo == hi: unchanged; else clip, (v - lo) / (hi - lo) * (b - a) + a */
  M355_AUG_GAMMA = 2,    /* v = sign(v) |v|^vec[channel] */
  M355_AUG_NOISE = 3     /* v += a + b * N(0, 1), Philox4x32-10 keyed by seed, counter = element index, Box-Muller */
};
typedef struct {
  int32_t op;
  int32_t order;
  float a, b;
  uint64_t seed;
  const double* stats;
  const float* vec;
} m355_aug_stage;
int m355_aug_resample(const void* x, void* y, int32_t C, const int32_t* in3, const int32_t* out3, int32_t elem_bytes,
                      int32_t interp, const double* mat12, const double* disp9, const float* grid, const int32_t* grid3,
                      const double* pad, double pad_const, void* stream);
int m355_aug_prefilter(float* x, int32_t C, const int32_t* size3, void* stream);
size_t m355_aug_workspace(void);
int m355_aug_order_stats(const float* x, int32_t C, const int32_t* size3, const m355_aug_stage* stages, int32_t nstages,
                         int32_t nq, const int64_t* ks, const double* fracs, double* out, void* workspace,
                         size_t ws_bytes, void* stream);
int m355_aug_intensity(const float* x, float* y, int32_t C, const int32_t* size3, const m355_aug_stage* stages,
                       int32_t nstages, void* stream);
int m355_aug_blur(const float* x, float* y, int32_t C, const int32_t* size3, int32_t axis, double sigma,
                  const m355_aug_stage* stages, int32_t nstages, void* stream);
int m355_aug_otsu_pad(const float* x, int32_t C, const int32_t* size3, double* pad, void* stream);
int m355_aug_channel_minmax(const float* x, int32_t C, const int32_t* size3, int32_t which, double* out,
                           void* workspace, size_t ws_bytes, void* stream);

/* ------------------------------------------ preprocessing
 * The deterministic torchio preprocessing transforms of the reference's production configs
 * (research/dmri_hippo/configs/main_config.py:78-120, research/msseg2/msseg2.py:36-80): preprocessing.py, DESIGN §4.11.
 * Volumes are [C, V0, V1, V2] with fewer than 2^31 voxels per channel; element types are the M355_PRE_* codes
 * (bool is one byte, 0 or 1).
 *   m355_pre_bbox         bbox[0..6] (device int32, zeroed here) of the voxels of channel `channel` of `map` where
 *                         pred 0: v != 0, pred 1: v == value.  bbox[a] = V_a - min_a, bbox[3 + a] = max_a + 1 (a < 3),
 *                         bbox[6] = the count; all zero when no voxel matches.  One integer atomic per workgroup and value.
 *   m355_pre_crop_or_pad_offsets  offsets[a] (device int32) = torchio 0.18.45 CropOrPad's begin of a box `bbox`
 *                         (m355_pre_bbox) of an in3 volume cropped / padded to target3: the mask-centred window, or the
 *                         centred one (ceil(n / 2) in front) when the box is empty.  One single-workgroup launch.
 *   m355_pre_min_tables   np.pad(mode='minimum') lookup tables of x (after NaN -> nan_value when replace_nan): per
 *                         channel the minimum over every non-empty subset of the three axes, the other coordinates
 *                         fixed, as order-preserving uint64 keys.  m355_pre_min_tables_bytes(C, size3) bytes; one
 *                         pass over x plus one small pass over the tables.
 *   m355_pre_gather       y[c, p] (out3) = f(v[c, p + off]) with off = off_dev (device, when not NULL) or off3, v the
 *                         in3 box of x (of size src3) at base3 (a crop folded in): in-bounds voxels take v (NaN ->
 *                         nan_value when replace_nan); others the constant pad_value
 *                         (pad_mode 0) or the np.pad 'minimum' value of the axes they leave (pad_mode 1, tables of x; the box is then all of x);
 *                         then the simultaneous remap (every pair tests the value before any remap, the last match
 *                         wins) where the mask holds, then the cast to out_dtype.  y may be a channel slice of a larger
 *                         tensor (concatenation); x != y.
 *   m355_pre_one_hot      y[k, p] = (trunc(x[0, p]) == k), k < K, in x's element type.  Labels outside [0, K) give an
 *                         all-zero column and are counted into *bad (device int32, zeroed here).
 *   m355_pre_image_from_labels  y[0, p] (float32) = 0, then per entry (in order) mode 0: y = weight where the label is
 *                         `id`, mode 1: y += (label == id) * weight; the label is channel 0, or the first argmax over
 *                         the channels of a one-hot map. */
#define M355_PRE_MAX_REMAP 8
#define M355_PRE_MAX_ENTRIES 8
enum { M355_PRE_U8 = 0, M355_PRE_BOOL = 1, M355_PRE_I32 = 2, M355_PRE_I64 = 3, M355_PRE_F32 = 4 };
enum { M355_PRE_MASK_NONE = 0, M355_PRE_MASK_HALF = 1, M355_PRE_MASK_MAP = 2 };
typedef struct {
  const void* x;
  void* y;
  int32_t in_dtype, out_dtype, C;
  int32_t src3[3], base3[3], in3[3], out3[3], off3[3];
  const int32_t* off_dev;      /* NULL: off3 */
  int32_t pad_mode;            /* 0 constant pad_value, 1 per-line minimum (tables) */
  double pad_value;
  const void* tables;
  int32_t replace_nan;
  double nan_value;
  int32_t nremap;
  double remap_old[M355_PRE_MAX_REMAP], remap_new[M355_PRE_MAX_REMAP];
  int32_t mask_kind;           /* M355_PRE_MASK_*: HALF = o[mask_axis] >= out3[mask_axis] / 2 (mask_upper) or < it */
  int32_t mask_axis, mask_upper;
  const void* mask_map;        /* MAP: nonzero voxels of an out3 map of mask_C (1 or C) channels */
  int32_t mask_dtype, mask_C;
} m355_pre_gather_desc;
typedef struct {
  const void* map;
  int32_t dtype, C, one_hot;
  float weight;
  double id;
} m355_pre_label_entry;
int m355_pre_bbox(const void* map, int32_t dtype, int32_t C, const int32_t* size3, int32_t channel, int32_t pred,
                  double value, int32_t* bbox, void* stream);
int m355_pre_crop_or_pad_offsets(const int32_t* bbox, const int32_t* in3, const int32_t* target3, int32_t* offsets,
                                 void* stream);
size_t m355_pre_min_tables_bytes(int32_t C, const int32_t* size3);
int m355_pre_min_tables(const void* x, int32_t dtype, int32_t C, const int32_t* size3, int32_t replace_nan,
                        double nan_value, void* tables, size_t bytes, void* stream);
int m355_pre_gather(const m355_pre_gather_desc* d, void* stream);
int m355_pre_one_hot(const void* x, int32_t dtype, const int32_t* size3, int32_t K, void* y, int32_t* bad, void* stream);
int m355_pre_image_from_labels(const m355_pre_label_entry* entries, int32_t n, const int32_t* size3, int32_t mode,
                               float* y, void* stream);

/* ------------------------------------------ mean diffusion-weighted image
 * The per-voxel work of the reference's ReconstructMeanDWI / ReconstructMeanDWIClassic
 * (segmentation_pipeline/transforms/reconstruct_mean_dwi.py); the channels are drawn on the host (augmentation.py,
 * DESIGN §4.10).
 *   m355_dwi_mean         y[v] (float32, one channel of size3) = (x[idx[0]][v] + x[idx[1]][v] + ... + x[idx[k-1]][v]) / k
 *                         for x float32 [N, V0, V1, V2] (fewer than 2^31 voxels per channel): summed in fp32 in pick
 *                         order, then one correctly rounded fp32 division by (float) k, as np.mean(x[idx], axis=0) and
 *                         torch.mean(x[idx], 0) for float32.  idx: device int32 [k], k >= 1, duplicates allowed; an
 *                         index outside [0, N) makes its voxels NaN (the host checks them before the upload).  One
 *                         launch on `stream`, no synchronisation; x != y. */
int m355_dwi_mean(const float* x, int32_t N, const int32_t* size3, const int32_t* idx, int32_t k, float* y, void* stream);

/* ------------------------------------------ evaluation
 * Confusion counts of the reference's SegmentationEvaluator / LabelMapEvaluator (evaluators.py).
 * counts[subject][l][{TP, FP, FN}] (device uint64, zeroed here) for the L distinct label values labels[0 .. L)
 * (1 <= L <= M355_EV_MAX_LABELS); TN = S - TP - FP - FN.  A voxel equals label v as torch's `data == v` decides: v is
 * cast to the map's element type first (uint8: v mod 256, float32: float(v)); a voxel of no label counts for none.
 * Without a target, FN = 0 and TP + FP is the label's volume.  Element types are the M355_EV_* codes (bool one byte).
 * `nokey`: an int32 that is none of the labels' values in any element type (the host picks it); values no label can
 * equal (non-integral floats, int64 outside int32) take it.  `descs` are host descriptors, copied to `dev_descs`
 * (device, n descriptors) on the stream; all n subjects run in one launch, whatever their sizes.
 *   m355_eval_confusion  label maps [S] of any M355_EV_* type up to float32; the target may be NULL.
 *   m355_eval_scores     from scores [C, S] (float32, bfloat16 or float16; 1 <= C <= M355_EV_MAX_CHANNELS): the first
 *                        maximum over the channels (a NaN is the maximum, the first NaN wins: torch.argmax), then the
 *                        label value table[m * C + c] with m = 1 inside the mask, 0 outside (mask HALF: coordinate
 *                        o[mask_axis] >= size3[mask_axis] / 2 when mask_upper, < it otherwise; MAP: the nonzero voxels
 *                        of each subject's `mask` [S]).  Target: NONE, a one-hot [C, S] map (its argmax goes through
 *                        the same table) or a label map [S].  pred_out / target_out (int64 [S], optional) receive the
 *                        label maps; target_out only from a one-hot target. */
#define M355_EV_MAX_LABELS 64
#define M355_EV_MAX_CHANNELS 64
enum { M355_EV_BOOL = 0, M355_EV_U8 = 1, M355_EV_I8 = 2, M355_EV_I16 = 3, M355_EV_I32 = 4, M355_EV_I64 = 5, M355_EV_F32 = 6,
       M355_EV_BF16 = 7, M355_EV_F16 = 8 };
enum { M355_EV_MASK_NONE = 0, M355_EV_MASK_HALF = 1, M355_EV_MASK_MAP = 2 };
enum { M355_EV_TARGET_NONE = 0, M355_EV_TARGET_ONEHOT = 1, M355_EV_TARGET_MAP = 2 };
typedef struct {
  const void* pred;
  const void* target;          /* NULL: no target */
  int64_t S;
  int32_t pred_dtype, target_dtype;
} m355_eval_map_desc;
typedef struct {
  const void* scores;          /* [C, S] */
  const void* target;          /* NULL, [C, S] one-hot or [S] label map */
  const void* mask;            /* M355_EV_MASK_MAP: [S] */
  int64_t* pred_out;           /* NULL: not written */
  int64_t* target_out;
  int32_t size3[3];
  int32_t target_kind, target_dtype, mask_dtype;
} m355_eval_scores_desc;
int m355_eval_confusion(const m355_eval_map_desc* descs, int32_t n, void* dev_descs, const int32_t* labels, int32_t L,
                        int32_t nokey, uint64_t* counts, void* stream);
int m355_eval_scores(const m355_eval_scores_desc* descs, int32_t n, void* dev_descs, int32_t scores_dtype, int32_t C,
                     const int32_t* table, int32_t mask_kind, int32_t mask_axis, int32_t mask_upper,
                     const int32_t* labels, int32_t L, int32_t nokey, uint64_t* counts, void* stream);
/* Thresholded (multi-label) counts for sigmoid heads: counts[subject][c][{TP, FP, FN}] (device uint64, zeroed here) of
 * predicted = ((float) score > thresholds[c]) against positive = (target != 0), each of the C channels
 * (1 <= C <= M355_EV_MAX_CHANNELS) on its own.  Scores [C, S] float32, bfloat16 or float16 (16-bit values are widened
 * exactly); a NaN score is not predicted (torch's `>`).  Targets [C, S] of any M355_EV_* type, BF16 / F16 included; a
 * NaN target is positive (torch's `!= 0`), -0.0 is not; NULL is an argument error.  thresholds: host floats [C], +-inf
 * allowed.  Host descriptors are copied to `dev_descs` on the stream; one launch for all n subjects whatever their
 * sizes, no synchronisation; integer atomics only, so the counts are exact. */
typedef struct {
  const void* scores;          /* [C, S] */
  const void* target;          /* [C, S] */
  int64_t S;
  int32_t target_dtype;
} m355_eval_multilabel_desc;
int m355_eval_multilabel(const m355_eval_multilabel_desc* descs, int32_t n, void* dev_descs, int32_t scores_dtype,
                         int32_t C, const float* thresholds /* host, [C] */,
                         uint64_t* counts /* device [n][C][3], zeroed here */, void* stream);

/* Calibration of probabilities (csrc/calibration.hip): reliability tables, Brier score and negative
 * log-likelihood per subject, every subject of whatever size in one pass (descriptors as for m355_eval_multilabel: copied
 * to `dev_descs` on the stream, no synchronisation).  Per subject: scores [C, S] float32, bfloat16 or float16 (widened
 * exactly), 1 <= C <= M355_EV_MAX_CHANNELS, holding PROBABILITIES (the output of a softmax or sigmoid head), and a target,
 * of one `target_kind` for all subjects:
 *   M355_EV_TARGET_ONEHOT  a one-hot or soft map [C, S] of any M355_EV_* type: channel c is positive where `!= 0` (a NaN
 *                          is, -0.0 is not); the categorical class is the first maximum over the channels (a NaN is the
 *                          maximum), the rule of m355_eval_scores;
 *   M355_EV_TARGET_MAP     a map [S] of channel indices of an integer M355_EV_* type; an index outside [0, C) makes the
 *                          voxel invalid.  Channel c is positive where the index is c.
 * Definitions:
 *   bin         a confidence q (float32, 0 <= q <= 1) falls into bin min((int)(q * (float)bins), bins - 1): one float32
 *               multiply and a truncation; 1 <= bins <= M355_CAL_MAX_BINS.
 *   entry       {count, hits, conf_sum}, three uint64; conf_sum = sum of rint((double)q * 2^32), a 2^-32 fixed point
 *               (the product is an integer for q >= 2^-8): exact and independent of order.
 *   M355_CAL_CATEGORICAL (softmax).  A voxel is valid when every channel value lies in [0, 1] (so none is NaN, and the
 *               top-label confidence lies there) and the target index is in range.  Invalid voxels are counted in
 *               invalid[subject][0] and enter no table and no sum.  top[subject][bin]: q = the first maximum over the
 *               channels, hit = that channel is the target's class.  classwise[subject][c][bin]: q = p_c, hit = the target
 *               is positive in c.  brier = sum over valid voxels and channels of ((double)p_c - y_c)^2, y_c = 1 where the
 *               target is positive in c, else 0.  nll = sum over valid voxels of -log(((double)p_t + 1e-8) / (1 + 1e-8)),
 *               t the target's class (the reference criterion's prediction_safe shift; fp64 log).
 *   M355_CAL_BINARY (sigmoid).  Every channel a problem of its own: (voxel, c) is valid when p_c lies in [0, 1] and the
 *               target index is in range; invalid pairs are counted in invalid[subject][c].  classwise as above; top stays
 *               zero.  brier as above over the valid pairs; nll = sum over them of -log(ps(p_c)) where the target is
 *               positive and -log(ps(1 - (double)p_c)) where it is not, ps(x) = (x + 1e-8) / (1 + 1e-8).
 *   sums[subject] = {brier, nll} in fp64: per-workgroup partials added in a fixed order, so a repeated call gives the same
 *               bits.  voxels[subject] = S.
 * Invalid values never index a table.  `workspace`: m355_eval_calibration_workspace(n) bytes, contents irrelevant.  The
 * tables, invalid counts, sums and voxel counts are written in full by the call (their contents on entry are irrelevant). */
#define M355_CAL_MAX_BINS 32
enum { M355_CAL_CATEGORICAL = 0, M355_CAL_BINARY = 1 };
typedef struct {
  const void* scores;          /* [C, S] */
  const void* target;          /* [C, S] (ONEHOT) or [S] (MAP) */
  int64_t S;
  int32_t target_dtype;
} m355_eval_calibration_desc;
size_t m355_eval_calibration_workspace(int32_t n);
int m355_eval_calibration(const m355_eval_calibration_desc* descs, int32_t n, void* dev_descs, int32_t scores_dtype,
                          int32_t target_kind /* of every subject */, int32_t C, int32_t bins, int32_t kind, uint64_t* top /* device [n][bins][3] */,
                          uint64_t* classwise /* device [n][C][bins][3] */, uint64_t* invalid /* device [n][C] */,
                          double* sums /* device [n][2] */, int64_t* voxels /* device [n] */, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ------------------------------------------ contour images
 * The device half of the reference's FindInterestingSlice and ContourImageEvaluator (evaluators.py).
 * Volumes are [W, H, D], contiguous with D fastest, fewer than 2^31 voxels, every dimension at most
 * M355_SLICE_MAX_DIM.  Planes are named by the axis they fix: SAGGITAL (the reference's spelling) fixes W, CORONAL H,
 * AXIAL D.  Host descriptors are copied to `dev_descs` (device, room for all of them) on the stream; one launch per
 * call whatever the sizes; nothing synchronises.
 *   m355_slice_counts  counts[counts_offset + {0 .. W, W .. W+H, W+H .. W+H+D}) (device int32, zeroed here) = the
 *                      foreground voxels of every sagittal, coronal and axial slice of subject i.  channels == 0: a
 *                      label map of any M355_EV_* type up to float32, foreground = `data != 0` (a NaN is foreground).
 *                      channels >= 1 (at most M355_EV_MAX_CHANNELS): a one-hot or score map [channels, W, H, D] in
 *                      float32, bfloat16 or float16, foreground = argmax over the channels != 0 with the rule of
 *                      m355_eval_scores (first maximum, a NaN is the maximum).  counts_offset of subject i must be the
 *                      sum of W + H + D over the subjects before it.
 *   m355_slice_rank    for every segment (offset, len) of `counts`: ids[offset ..) = the slices with a non-zero count,
 *                      by count descending, ties by ascending slice id; ranked[offset ..) their counts in that order;
 *                      nums[segment] their number.  Entries past nums[segment] are id -1 and count 0.
 *   m355_slice_mosaic  up to 3 mosaics (torchvision make_grid with padding 1, row 0 of its channels) of 2-D slices:
 *                      AXIAL x[:, :, k] ([W, H]), CORONAL rot90(x[:, k, :]) ([D, W]), SAGGITAL rot90(x[k, :, :])
 *                      ([D, H]), rot90(m)[i, j] = m[j, B - 1 - i].  Mosaic m holds tiles [first_tile, first_tile +
 *                      ntiles), all tile_h x tile_w, xmaps = min(ncol, ntiles) per row; rows x cols is
 *                      (ymaps * (tile_h + 1) + 1) x (xmaps * (tile_w + 1) + 1) filled with `pad`, tile k at row0 =
 *                      (k / xmaps) * (tile_h + 1) + 1, col0 = (k % xmaps) * (tile_w + 1) + 1; a single tile is the
 *                      bare tile_h x tile_w (row0 = col0 = 0).  A tile without a source is zeros.  The mosaic has the
 *                      element type of its tiles (a pure gather); a float32 mosaic also takes bfloat16 / float16
 *                      tiles.  Everything is checked on the host (M355_EINVALID_ARG) before the launch. */
#define M355_SLICE_MAX_DIM 2048
enum { M355_PLANE_SAGGITAL = 0, M355_PLANE_CORONAL = 1, M355_PLANE_AXIAL = 2 };
typedef struct {
  const void* data;            /* [W, H, D] or [channels, W, H, D] */
  int64_t counts_offset;
  int32_t size3[3];
  int32_t dtype, channels;
} m355_slice_counts_desc;
typedef struct {
  int64_t offset;
  int32_t len, reserved;
} m355_slice_seg;
typedef struct {
  const void* src;             /* channel 0 of the volume; NULL: a tile of zeros */
  int32_t dtype;
  int32_t size3[3];
  int32_t plane, slice;
  int32_t row0, col0;
} m355_slice_tile_desc;
typedef struct {
  void* out;                   /* [rows, cols] of element type dtype */
  int32_t dtype, rows, cols, tile_h, tile_w, ncol, ntiles, first_tile;
  float pad;
} m355_slice_mosaic_desc;
int m355_slice_counts(const m355_slice_counts_desc* descs, int32_t n, void* dev_descs, int32_t* counts, void* stream);
int m355_slice_rank(const int32_t* counts, const m355_slice_seg* segs, int32_t nseg, void* dev_descs, int32_t* ids,
                    int32_t* ranked, int32_t* nums, void* stream);
int m355_slice_mosaic(const m355_slice_mosaic_desc* mosaics, int32_t nmosaics, const m355_slice_tile_desc* tiles,
                      int32_t ntiles, void* dev_descs, void* stream);

/* ------------------------------------------ distance transform and surface distances
 * The exact Euclidean distance transform under post_processing.distance_transform_edt, and the device half of
 * evaluators.SurfaceDistanceEvaluator (Hausdorff distance, its percentile, average symmetric surface distance; DESIGN
 * §4.20).  Volumes are [W, H, D], contiguous with D fastest, fewer than 2^31 voxels.  Every entry point enqueues on
 * `stream` and never synchronises; arguments are checked on the host before any launch: a null pointer, a size < 1,
 * 2^31 voxels or more, or a spacing that is not finite and > 0 is M355_EINVALID_ARG; a dimension above
 * M355_EDT_MAX_DIM (m355_edt_sq only: a line of the volume is staged in LDS) is M355_EUNSUPPORTED.
 *   m355_edt_sq          d2[v] = min over the voxels s with sites[s] != 0 of sum_a (spacing3[a] * (v_a - s_a))^2, the
 *                        SQUARED distance to the nearest site; +inf everywhere when there is no site.  spacing3: three
 *                        host floats for the axes W, H, D.  Three launches: a nearest-site sweep along D, then a
 *                        minimum pass along H and one along W.  fp32 throughout, every term formed as
 *                        (spacing3[a] * k) squared, each product and each sum rounded once, in a fixed order: the
 *                        result does not depend on the launch geometry.  With spacing (1, 1, 1) every intermediate is
 *                        an integer and d2 is EXACT while (W-1)^2 + (H-1)^2 + (D-1)^2 < 2^24 (always, within
 *                        M355_EDT_MAX_DIM: 3 * 511^2 < 2^20); otherwise the candidates carry rounding error only --
 *                        the search never drops a site whose rounded value is the smallest.  Workspace:
 *                        m355_edt_workspace(size3) bytes (0 for a null or non-positive size).  sites and d2 must not
 *                        overlap.
 *   m355_edt_sqrt        d[i] = the correctly rounded fp32 square root of d2[i] (+inf stays +inf); d may be d2.
 *   m355_surface_mask    x: an int32 label volume (m355_label_convert_in's output).  border[v] = 1 when x[v] == value
 *                        and v lies on a face of the volume or one of its six face neighbours differs from value (a
 *                        neighbour of another label counts as outside), else 0: mask ^ binary_erosion(mask, 6-connected
 *                        structure, border_value=0).  *count (device int32, zeroed by the CALLER) grows by the number
 *                        of border voxels; integer atomics, so it is exact.
 *   m355_surface_gather  for every voxel with border[v] != 0: out[k] = the correctly rounded sqrt(d2[v]) with k =
 *                        atomicAdd(cursor, 1), when k < capacity.  *cursor (device int32, the caller sets the first
 *                        slot, normally 0) keeps counting past capacity, so a short buffer shows.  The order of the
 *                        entries is unspecified: callers sort.  capacity >= 0.
 */
#define M355_EDT_MAX_DIM 512
size_t m355_edt_workspace(const int32_t* size3);
int m355_edt_sq(const uint8_t* sites, const int32_t* size3, const float* spacing3 /* host */, float* d2, void* workspace,
                void* stream);
int m355_edt_sqrt(const float* d2, float* d, int64_t n, void* stream);
int m355_surface_mask(const int32_t* x, int32_t value, const int32_t* size3, uint8_t* border, int32_t* count,
                      void* stream);
int m355_surface_gather(const uint8_t* border, const float* d2, int64_t nvox, float* out, int32_t* cursor,
                        int32_t capacity, void* stream);

/* ------------------------------------------ boundary loss on a batched signed distance transform
 * The device half of criterions.BoundaryLoss (Kervadec et al., "Boundary loss for highly unbalanced segmentation";
 * DESIGN §4.27).  target, phi, p, dp: fp32 [planes = N * C][size3[0]][size3[1]][size3[2]], contiguous with the last axis
 * fastest -- for a criterion's [N, C, D, H, W] tensors size3 = (D, H, W).  Every entry point enqueues on `stream`, never
 * synchronises, uses no float atomics (a call repeats bit for bit) and checks its arguments on the host before any
 * launch: a null pointer, a size or plane count < 1, 2^31 voxels per plane or more, or a spacing that is not finite
 * and > 0 is M355_EINVALID_ARG; an axis above M355_EDT_MAX_DIM (m355_signed_distance) or N * C > 65535 (the loss) is
 * M355_EUNSUPPORTED; a short workspace is M355_EWORKSPACE.
 *   m355_signed_distance   A voxel is inside when target > 0.5 (a NaN is outside).  Per plane, with d the Euclidean
 *                          distance under spacing3 (three host floats, one per axis of size3):
 *                            outside voxel   phi = +d(v, nearest inside voxel)
 *                            inside voxel    phi = -(d(v, nearest outside voxel) - 1)
 *                            a plane that is all inside or all outside: phi = 0 everywhere
 *                          (the convention of the published implementation; with unit spacing the inside voxels next to
 *                          the border get 0).  plane_on: `planes` host bytes, or null for all planes; a plane whose byte
 *                          is 0 is written as zeros and costs no transform.  One transform per plane -- every voxel
 *                          needs the distance to the other membership only -- in three launches per 1024 planes (the
 *                          last alone when none of them is on).  The arithmetic is m355_edt_sq's, term by term, the
 *                          root correctly rounded and the subtraction from 1 rounded once: with unit spacing phi is the
 *                          fp32 rounding of the exact value.  target is not modified and must not overlap phi.
 *                          Workspace: m355_signed_distance_workspace(planes, size3) bytes (0 for invalid arguments).
 *   m355_boundary_loss_fwd loss[0] = sum_n sum_c w_c sum_v p phi / (N S sum_c w_c), one fp32 device scalar; products and
 *                          sums in fp64 in a fixed order.  class_weights: C device floats >= 0 with a positive sum, or
 *                          null for all ones; rows with w_c == 0 are not read.  Two launches.  Workspace:
 *                          m355_boundary_loss_workspace(N, C, S) bytes (0 for non-positive sizes).
 *   m355_boundary_loss_bwd dp = dloss[0] (w_c / (N S sum_c w_c)) phi, the coefficient rounded to fp32 once and the product
 *                          once; zeros for rows with w_c == 0.  dloss: one device float.  One launch.  The target gets
 *                          no gradient.
 */
size_t m355_signed_distance_workspace(int32_t planes, const int32_t* size3);
int m355_signed_distance(const float* target, int32_t planes, const int32_t* size3, const float* spacing3 /* host */,
                         const uint8_t* plane_on /* host, may be null */, float* phi, void* workspace,
                         size_t workspace_bytes, void* stream);
size_t m355_boundary_loss_workspace(int32_t N, int32_t C, int64_t S);
int m355_boundary_loss_fwd(const float* p, const float* phi, const float* class_weights, int32_t N, int32_t C, int64_t S,
                           float* loss, void* workspace, size_t workspace_bytes, void* stream);
int m355_boundary_loss_bwd(const float* phi, const float* dloss /* device scalar */, const float* class_weights, int32_t N,
                           int32_t C, int64_t S, float* dp, void* stream);

/* ------------------------------------------ lesion-wise (blob) Dice loss on device connected components
 * The device half of criterions.BlobLoss (Kofler et al., "blob loss: instance imbalance aware loss functions for semantic
 * segmentation").  target, p, dp: fp32 [planes = N * C][D][H][W], contiguous.  plane_on: `planes` host
 * bytes, or null for all planes; the P_on planes whose byte is not 0 are "on", in plane order they take the slots
 * 0 .. P_on - 1.  In an on plane a voxel is a member when target > 0.5 (a NaN is none), the members fall into connected
 * components (connectivity 1 | 2 | 3: 6, 18, 26 neighbours), and
 *     S_k = sum_k p,  Q_k = sum_k p^2,  A_k = |k|,  B = sum over the plane's non-members of p (square_dice: of p^2)
 *     d_k = 2 S_k / (A_k + S_k + B + 1e-8)          square_dice: 2 S_k / (A_k + Q_k + B + 1e-8)
 *     loss = sum_{on planes with K > 0 components} w_c (1/K) sum_k (1 - d_k) / sum_{the same planes} w_c
 * which is the Dice of m355_hybrid_loss_fwd per component with the other components masked out of prediction and target.
 * The term is Dice only: there is no per-component log term.
 * Every entry point enqueues on `stream`, never synchronises, uses no float atomics (a call repeats bit for bit) and
 * checks its arguments on the host before any launch: a null pointer, a size or plane count < 1, no plane on, a
 * connectivity outside 1..3, or on planes that stack to 2^31 voxels or more is M355_EINVALID_ARG; more than 1024 planes
 * is M355_EUNSUPPORTED; a short workspace or table buffer is M355_EWORKSPACE.  The queries return 0 for such arguments.
 *   m355_blob_capacity  The number of components the accumulators are sized for, a bound the host can compute:
 *                       P_on ceil(D/2) ceil(H/2) ceil(W/2) with 26 neighbours (two members of one 2 x 2 x 2 cell of a
 *                       plane are connected), P_on ceil(D H W / 2) otherwise (a checkerboard).
 *   m355_blob_label     labels: int32 [P_on][D][H][W], 0 for a non-member, else the number of the voxel's component; the
 *                       components of all planes are numbered 1 .. n in raster order of their first voxel in the stack,
 *                       so those of slot s are the contiguous range ranges[2 s] .. ranges[2 s + 1] (last = first - 1: the
 *                       plane has none).  count[0] = n, or -1 when a bounded find / union loop of the labelling hit its
 *                       bound (ranges are undefined then).  The on planes are thresholded into one int32 volume
 *                       [P_on * D][H][W] whose slot s holds the value s + 1 and m355_ccl_label labels it in mode 0, where
 *                       only equal values connect: planes that touch across the stacking boundary stay apart.  Ten
 *                       launches, nothing is read on the host.  Workspace: m355_blob_label_workspace bytes.
 *   m355_blob_dice_fwd  loss[0]: one fp32 device scalar; total[0] = count[0].  One pass over (p, labels) of the on planes
 *                       accumulates S and Q as 64-bit integers of round(p 2^f), round(p^2 2^f) and A as a count with
 *                       integer atomics, f = min(60, 63 - bits of D H W) >= 32 the largest scale at which no sum can
 *                       overflow (each sum is off by at most 2^-33 per voxel summed, whatever the arrival order);
 *                       zeroing and finalize read count on the device and cost time in the components there are.  p must
 *                       be a probability: a value that is not finite or outside [0, 1] in an on plane makes loss (and the
 *                       gradient) NaN, as count = -1 does; nothing raises.  class_weights: C device floats >= 0, or null
 *                       for all ones.  `tables` (m355_blob_dice_tables bytes) is what the backward needs besides labels:
 *                       two fp64 coefficients per component, one per plane, a status word.  Four launches.  Workspace:
 *                       m355_blob_dice_workspace bytes.
 *   m355_blob_dice_bwd  dp = dloss[0] (a_k + b_k p) for a member of component k (b_k = 0 without square_dice),
 *                       dloss[0] g_nc for a non-member (times 2 p with square_dice), formed in fp64 and rounded to fp32
 *                       once; zeros in planes that are off.  p may be null without square_dice.  One launch.  The target
 *                       gets no gradient.
 */
int64_t m355_blob_capacity(int32_t planes, const uint8_t* plane_on /* host, may be null */, int32_t D, int32_t H, int32_t W,
                           int32_t connectivity);
size_t m355_blob_label_workspace(int32_t planes, const uint8_t* plane_on, int32_t D, int32_t H, int32_t W);
int m355_blob_label(const float* target, int32_t planes, const uint8_t* plane_on /* host, may be null */, int32_t D,
                    int32_t H, int32_t W, int32_t connectivity, int32_t* labels, int32_t* ranges, int32_t* count,
                    void* workspace, size_t workspace_bytes, void* stream);
size_t m355_blob_dice_workspace(int32_t planes, const uint8_t* plane_on, int32_t D, int32_t H, int32_t W,
                                int32_t connectivity);
size_t m355_blob_dice_tables(int32_t planes, const uint8_t* plane_on, int32_t D, int32_t H, int32_t W,
                             int32_t connectivity);
int m355_blob_dice_fwd(const float* p, const int32_t* labels, const int32_t* ranges, const int32_t* count,
                       const float* class_weights, int32_t N, int32_t C, const uint8_t* plane_on /* host, may be null */,
                       int32_t D, int32_t H, int32_t W, int32_t connectivity, int32_t square_dice, float* loss,
                       int32_t* total, void* tables, size_t tables_bytes, void* workspace, size_t workspace_bytes,
                       void* stream);
int m355_blob_dice_bwd(const float* p, const int32_t* labels, const void* tables, const float* dloss /* device scalar */,
                       int32_t N, int32_t C, const uint8_t* plane_on /* host, may be null */, int32_t D, int32_t H,
                       int32_t W, int32_t connectivity, int32_t square_dice, float* dp, void* stream);

/* ------------------------------------------ statistics of image values grouped by the label of the voxel
 * The device half of ops.region_stats, evaluators.ImageRegionEvaluator and data_processing.dataset_fingerprint (DESIGN
 * §4.22).  One label volume [W, H, D] (contiguous, D fastest; any M355_EV_* type up to float32), K >= 0 images
 * [channels, W, H, D] on the same grid (float32, float16, bfloat16, uint8 or int16: each converts to fp32 exactly), L
 * label values (0 <= L <= M355_EV_MAX_LABELS).  Regions, in this order: the L values as given (`data == value` as
 * torch decides it, the value cast to the map's type; of two equal values the first gets the voxels), then 'all'
 * (label != 0) and 'whole' (every voxel): R = L + 2 rows.
 *   count[R]        int64 voxels of the region
 *   bounds[R][6]    int32 (min, max) index along W, H, D; an empty region has (axis size, -1)
 *   stats[R][K][5]  float32 mean, unbiased std, median, min, max of image k inside the region, its channels pooled (the
 *                   mask broadcasts over them), n = count * channels values.  The median is torch.median's: the value of
 *                   rank (n - 1) / 2 of the sorted values.  n == 0: all five NaN; n == 1: std NaN; a NaN among the
 *                   values: all five NaN, for that region and image only; +-inf are ordinary values for min, max and
 *                   median.  min, max and median are exact; mean and std are accumulated in fp64 (sum, then sum of
 *                   (x - mean)^2 in a second pass) and rounded to float32 once.  median == 0 skips the select passes
 *                   and leaves that column NaN.
 * Counts, bounds, min / max and the radix-select histograms use integer atomics; floating-point sums go through
 * per-block partials that one wave per region adds in a fixed order: the same call twice gives the same bits.  A call only
 * enqueues (2 + K * (median ? 9 : 4) launches) and never synchronises; the select resolves prefix and rank on
 * the device.  Workspace: m355_region_stats_workspace(L, K, median) bytes (0 for K <= 0 or an L out of range; K == 0
 * needs none), not preserved between calls.  Arguments are checked on the host before any launch: L < 0, K < 0, a null
 * pointer, a size or channel count < 1 is M355_EINVALID_ARG; L above M355_EV_MAX_LABELS, another element type, a label
 * value float32 cannot hold inside int32, or an image of 2^32 values or more is M355_EUNSUPPORTED; a short workspace is
 * M355_EWORKSPACE.
 *   m355_region_stats_plan  plan4 = {blocks of a pass at most, threads of a block, voxels per thread and loop trip,
 *                           regions per block of a select pass}: a pass takes a second trip through its grid-stride
 *                           loop above plan4[0] * plan4[1] * plan4[2] voxels. */
typedef struct {
  const void* data;            /* [channels, W, H, D] */
  int32_t dtype;               /* M355_EV_F32, _F16, _BF16, _U8 or _I16 */
  int32_t channels;
} m355_region_image;
size_t m355_region_stats_workspace(int32_t L, int32_t K, int32_t median);
int m355_region_stats_plan(int32_t* plan4);
int m355_region_stats(const void* labels, int32_t label_dtype, const int32_t* size3, const m355_region_image* images,
                      int32_t K, const int32_t* values /* host */, int32_t L, int32_t median, int64_t* count,
                      int32_t* bounds, float* stats, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------ multi-tensor optimizer step: clipping, SGD / Adam / AdamW, poly LR, weight EMA
 * The device half of segmentation_pipeline_amd.optim (FusedSGD, FusedAdam); stands in for the
 * torch.optim.Adam / SGD a reference config names as its optimizer component (research/dmri_hippo/configs/main_config.py:128,
 * research/msseg2/msseg2.py:94) and for what a training scheme composes around it: clip_grad_norm_,
 * lr_scheduler.PolynomialLR, an EMA of the weights.  All tensors are float32 and contiguous; a tensor needs no alignment
 * beyond 4 bytes (16-byte accesses are used where every tensor of an entry allows them).
 *
 * A step is   [ m355_optim_norm x ceil(T / CAP) ]  ->  m355_optim_prepare  ->  m355_optim_update x ceil(T / CAP)
 * with the norm launches only when clipping is on.  T tensors are listed once, in any order; m355_optim_plan gives every
 * tensor its run of blocks (blk0, nblk: ceil(n / chunk) blocks of `chunk` elements, numbered through the whole list) and
 * the workspace size (one fp64 partial per block).  A launch takes at most m355_optim_capacity() consecutive tensors of
 * the list; its table travels BY VALUE in the kernel arguments, so a launch captured into a hipGraph replays with the
 * pointers of the capture, and the number of launches never depends on element counts.
 *
 *   m355_optim_norm     partial[blk0 + b] = sum of (double)g * g over block b's chunk, added in a fixed order; a non-finite
 *                       gradient makes the partial NaN.  No floating-point atomics: the same call twice gives the same bits.
 *   m355_optim_prepare  one block.  norm = sqrt(partials added in slot order, fp64) / grad_scale;
 *                       clip_coef = min(1, max_norm / (norm + 1e-6)) (clip_grad_norm_'s expression);
 *                       skip = (found_inf && *found_inf != 0) || norm not finite  -- the one difference from
 *                       clip_grad_norm_, which would write NaN into the weights;  t advances unless skipped;
 *                       lr[g] = group lr * (1 - min(t, total_steps) / total_steps)^power with t = 0 on the first step
 *                       (total_steps == 0: no schedule); Adam: bc1 = 1 - beta1^(t + 1), bc2 likewise, step size lr / bc1;
 *                       all in fp64, each value rounded to fp32 once.  Without clipping (desc.clip == 0) no partial is
 *                       read, norm = NaN and clip_coef = 1.  found_inf / grad_scale: device floats or NULL (the GradScaler
 *                       protocol of torch's fused optimizers).
 *   m355_optim_update   reads the state record and returns at once when skip is set (parameters, state and EMA keep their
 *                       bits).  The gradient is multiplied by clip_coef / grad_scale as it is read and never written back.
 *                       SGD: g += wd * p; buf = momentum * buf + (1 - dampening) * g (`first`: buf = g); g = nesterov ? g +
 *                       momentum * buf : buf; p -= lr * g.  Adam: g += wd * p; AdamW: p *= 1 - lr * wd; then m += (1 - beta1)
 *                       * (g - m); v = beta2 * v + (1 - beta2) * g * g; p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps) --
 *                       torch's own expressions.  ema_decay >= 0: ema += (1 - ema_decay) * (p_new - ema) in the same pass.
 *                       state1 = momentum buffer / exp_avg (SGD without momentum: unused, may be NULL), state2 = exp_avg_sq.
 *
 * State record: M355_OPTIM_STATE_WORDS 4-byte words of device memory, zero before the first step, owned by the caller:
 *   [0] norm f32  [1] clip_coef f32  [2] clip_coef / grad_scale f32  [3] bc1 f32  [4] bc2 f32 (group 0)  [5] skip i32
 *   [6] t i32 (steps applied)  [7] reserved  [8 + g] lr f32  [24 + g] 1 - lr * wd f32  [40 + g] lr / bc1 f32
 *   [56 + g] sqrt(bc2) f32,  g < M355_OPTIM_MAX_GROUPS.
 * Every entry point checks its arguments on the host before any launch and returns M355_EINVALID_ARG with a message that
 * names it: a null pointer, n < 1 or n > capacity, a negative count, a blk0 that does not continue the plan, a group out
 * of range, non-finite or out-of-range hyper-parameters, a workspace too small for the partials.  Calls only enqueue. */
#define M355_OPTIM_CAP 48
#define M355_OPTIM_MAX_GROUPS 16
#define M355_OPTIM_STATE_WORDS 72
enum { M355_OPTIM_SGD = 0, M355_OPTIM_ADAM = 1, M355_OPTIM_ADAMW = 2 };
typedef struct {
  void* param;
  const void* grad;
  void* state1;
  void* state2;
  void* ema;
  int64_t n;                   /* elements */
  int64_t blk0;                /* m355_optim_plan's */
  int32_t group;
  int32_t first;               /* SGD: the momentum buffer holds nothing yet */
} m355_optim_tensor;
typedef struct {
  double lr, weight_decay;
  double momentum, dampening;  /* SGD */
  double beta1, beta2, eps;    /* Adam, AdamW */
  int32_t nesterov, reserved;
} m355_optim_group;
typedef struct {
  int32_t rule;                /* M355_OPTIM_* */
  int32_t groups;              /* 1 .. M355_OPTIM_MAX_GROUPS */
  int32_t clip, reserved;      /* clip != 0: the norm pass ran, max_norm applies */
  double max_norm;
  int64_t total_steps;         /* 0: constant learning rate */
  double power;
  double ema_decay;            /* < 0: no EMA */
  m355_optim_group group[M355_OPTIM_MAX_GROUPS];
} m355_optim_desc;
int32_t m355_optim_capacity(void);
/* pure host: *chunk = elements of a block; blk0[i], nblk[i] = tensor i's blocks (a zero-element tensor owns none);
 * *workspace_bytes = room for one fp64 partial per block */
int m355_optim_plan(const int64_t* counts /* host */, int32_t T, int32_t* chunk, int64_t* blk0, int64_t* nblk,
                    size_t* workspace_bytes);
int m355_optim_norm(const m355_optim_tensor* tensors /* host */, int32_t n, void* workspace, size_t workspace_bytes,
                    void* stream);
int m355_optim_prepare(const m355_optim_desc* desc, int64_t nslots, const void* workspace, size_t workspace_bytes,
                       const float* found_inf, const float* grad_scale, void* state, void* stream);
int m355_optim_update(const m355_optim_desc* desc, const m355_optim_tensor* tensors /* host */, int32_t n, const void* state,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* M355SEG_H */
