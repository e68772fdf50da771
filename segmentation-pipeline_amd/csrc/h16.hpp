// 16-bit operand types of the bf16 / fp16 compute modes (M355_COMPUTE_BF16 / M355_COMPUTE_F16) and the
// "c8" activation layout they read:
//
//   x16[n][cb][s][8]    cb = channel block (channels 8*cb .. 8*cb+7, zero-padded past C), s = voxel (D*H*W)
//
// i.e. the 8 channels of a voxel are one aligned 16-byte item.  That item IS the MFMA operand fragment of
// v_mfma_f32_32x32x16_{bf16,f16} for a lane (voxel, k-half), so the convolution kernels move 16 bytes per
// lane from HBM to LDS to the matrix core without touching them, a tap shift is a whole-item offset, and a
// channel slice of a concat buffer that starts at a multiple of 8 channels is a contiguous run of blocks.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace m355 {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <typename HT>
struct H16;
template <>
struct H16<__bf16> {
  typedef __bf16 x8 __attribute__((ext_vector_type(8)));
  typedef __bf16 x4 __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ f32x16 mfma(x8 a, x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};
template <>
struct H16<_Float16> {
  typedef _Float16 x8 __attribute__((ext_vector_type(8)));
  typedef _Float16 x4 __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ f32x16 mfma(x8 a, x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
};

template <typename HT>
__device__ __forceinline__ HT to_h16_sat(float v);
template <>
__device__ __forceinline__ __bf16 to_h16_sat<__bf16>(float v) { return (__bf16)v; }
template <>
__device__ __forceinline__ _Float16 to_h16_sat<_Float16>(float v) {
  // a scaled gradient past the fp16 range saturates instead of becoming inf (which would turn every downstream sum
  // into NaN); NaN stays NaN -- a select, not fminf / fmaxf, which return the other operand of a NaN (v_max_f32 /
  // v_min_f32: a NaN gradient came out as -65504, finite and unreported)
  return (_Float16)(fabsf(v) > 65504.f ? copysignf(65504.f, v) : v);
}

// the same, remembering in `sat` that a value was clamped (the kernel ORs bit 0 into the overflow word at its end)
template <typename HT>
__device__ __forceinline__ HT to_h16_sat(float v, bool& sat);
template <>
__device__ __forceinline__ __bf16 to_h16_sat<__bf16>(float v, bool&) { return (__bf16)v; }
template <>
__device__ __forceinline__ _Float16 to_h16_sat<_Float16>(float v, bool& sat) {
  const bool big = fabsf(v) > 65504.f;   // (false for NaN: a NaN is not clamped, it stays NaN)
  sat = sat || big;
  return (_Float16)(big ? copysignf(65504.f, v) : v);
}
__device__ __forceinline__ void report_saturation(bool sat, int* __restrict__ oflag) {
  if (sat && oflag) atomicOr(oflag, 1);
}
__device__ __forceinline__ void report_nonfinite(float v, int* __restrict__ oflag) {
  if (oflag && !(fabsf(v) <= 3.4028235e38f)) atomicOr(oflag, 2);   // inf or NaN
}

static inline int64_t c8_blocks(int64_t C) { return (C + 7) / 8; }

// A kernel's template arguments chosen at run time, so that each launch is written once:
//   with_bool(v, [&](auto V) { launch kernel<decltype(V)::value> });   with_h16(compute, [&](auto T) { ...<typename decltype(T)::type> });
template <typename T>
struct TypeTag { typedef T type; };
template <typename F>
static inline void with_bool(bool vec, F&& f) {
  if (vec) f(std::true_type()); else f(std::false_type());
}
template <typename F>
static inline void with_h16(int compute, F&& f) {
  if (compute == M355_COMPUTE_BF16) f(TypeTag<__bf16>()); else f(TypeTag<_Float16>());
}

// fp32 NCDHW -> c8 (round to nearest even) and back; implemented in conv3d_h16.hip
int launch_pack_act16(const float* x, void* x16, int N, int C, int64_t S, int64_t xbs, int64_t x16bs, int compute,
                      hipStream_t st);
int launch_unpack_act16(const void* x16, float* x, int N, int C, int64_t S, int64_t x16bs, int64_t xbs, int compute,
                        hipStream_t st);

// (the launchers the normalisation passes share across files: norm_host.hpp)

// c8-only training flow (train16.hip): bias gradient of a conv from its c8 output gradient
size_t dbias_c8_ws_bytes(int N, int C, int64_t S);
int launch_dbias_c8(const void* dy16, int64_t dybs16, float* dbias, int N, int C, int64_t S, int compute, float unscale,
                    void* ws, hipStream_t st);

}  // namespace m355
