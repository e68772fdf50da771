// Host half of the factor-2 resampling family (elementwise.hip, maxpool.hip, upsample.hip, act16.hip, train16.hip): average
// and max pool, trilinear (both conventions) and nearest upsampling and space-to-depth, fp32 NCDHW and c8.  One row of data
// per entry point, one validator that runs the row's checks in the row's order, and plan_resample(), which resolves a call
// to its batch strides, kernel variant and grid.  The entry points, m355_resample_plan, m355_upsample2x_plan and nothing
// else read these numbers.
#pragma once
#include "h16.hpp"

namespace m355 {

enum ResampleOp {
  RS_AVG_FWD, RS_AVG_BWD, RS_AVG_BWD_ADD, RS_TRI_FWD, RS_TRI_BWD, RS_S2D, RS_D2S, RS_MAX_FWD, RS_MAX_BWD,
  RS_AVG_FWD_H16, RS_AVG_BWD_H16, RS_TRI_FWD_H16, RS_TRI_BWD_H16, RS_S2D_H16, RS_D2S_H16, RS_MAX_FWD_H16, RS_MAX_BWD_H16,
  RS_COUNT,   // the ops m355_resample_plan numbers; the rows behind them are m355_upsample2x_plan's (mode, direction, c8)
  RS_NEAR_FWD = RS_COUNT, RS_NEAR_BWD, RS_HP_FWD, RS_HP_BWD, RS_NEAR_FWD_H16, RS_NEAR_BWD_H16, RS_HP_FWD_H16, RS_HP_BWD_H16,
  RS_ROWS
};

// a tensor's size next to the (D, H, W) the entry point takes: those voxels, an eighth of them (pooled; RS_PACKED: with
// 8 * C channels, the space-to-depth result), eight times as many (upsampled)
enum ResampleRes : uint8_t { RS_NONE, RS_FULL, RS_HALF, RS_PACKED, RS_X8 };
enum ResampleVariant { RS_SCALAR = 0, RS_VECTOR = 1, RS_QUADS = 1, RS_LDS = 2 };

struct ResampleRow {
  const char* name;
  bool c8;
  ResampleRes t[3];   // the tensors, in the order of the entry point's batch strides
  uint8_t need;       // bit i: pointer i must not be null (bit 3: the max-pool route bytes)
  bool routes;        // takes route bytes (c8: 8-byte items, part of the alignment check)
  ResampleRes work;   // the voxels the grid runs over ...
  int per_thread;     // ... this many per thread (twice as many on the vector variant)
  int cap;            // grid.x limit
  const char* order;  // the checks, first to last: n null pointer, d non-positive dimension, o odd size (M355_EUNSUPPORTED),
                      // c compute mode, a alignment (c8: 16 bytes; fp32: 8 bytes of the full tensor, M355_EUNSUPPORTED)
};

// The orders differ from row to row only in where the M355_EUNSUPPORTED checks sit: they are what each entry point has
// always answered for a call that is wrong in two ways, so they stay.
static const ResampleRow RESAMPLE_ROWS[RS_ROWS] = {
    // name                         c8     tensors                           need routes work    /thr  cap    order
    {"avgpool3d_2x_fwd",             false, {RS_FULL, RS_HALF, RS_NONE},     0x3, false, RS_HALF, 1,  8192, "dno"},
    {"avgpool3d_2x_bwd",             false, {RS_HALF, RS_FULL, RS_NONE},     0x3, false, RS_FULL, 2,  8192, "dno"},
    {"avgpool3d_2x_bwd_add",         false, {RS_HALF, RS_FULL, RS_FULL},     0x7, false, RS_FULL, 2,  8192, "dno"},
    {"upsample_trilinear2x_fwd",     false, {RS_FULL, RS_X8, RS_NONE},       0x3, false, RS_X8,   1, 16384, "dn"},
    {"upsample_trilinear2x_bwd",     false, {RS_X8, RS_FULL, RS_NONE},       0x3, false, RS_FULL, 1, 65536, "dn"},
    {"space_to_depth2",              false, {RS_FULL, RS_PACKED, RS_NONE},   0x3, false, RS_FULL, 2, 16384, "ndoa"},
    {"depth_to_space2",              false, {RS_PACKED, RS_FULL, RS_NONE},   0x3, false, RS_FULL, 2, 16384, "ndoa"},
    {"maxpool3d_2x_fwd",             false, {RS_FULL, RS_HALF, RS_NONE},     0x3, true,  RS_HALF, 1,  8192, "ndo"},
    {"maxpool3d_2x_bwd",             false, {RS_HALF, RS_FULL, RS_FULL},     0xd, true,  RS_FULL, 2,  8192, "ndo"},
    {"avgpool3d_2x_fwd_h16",         true,  {RS_FULL, RS_HALF, RS_NONE},     0x3, false, RS_HALF, 1,  8192, "ndoca"},
    {"avgpool3d_2x_bwd_h16",         true,  {RS_HALF, RS_FULL, RS_FULL},     0x5, false, RS_FULL, 1, 16384, "cndoa"},
    {"upsample_trilinear2x_fwd_h16", true,  {RS_FULL, RS_X8, RS_NONE},       0x3, false, RS_X8,   1, 65536, "ndca"},
    {"upsample_trilinear2x_bwd_h16", true,  {RS_X8, RS_FULL, RS_NONE},       0x3, false, RS_FULL, 1, 65536, "ndca"},
    {"space_to_depth2_h16",          true,  {RS_FULL, RS_PACKED, RS_NONE},   0x3, false, RS_HALF, 1, 65536, "ondca"},
    {"depth_to_space2_h16",          true,  {RS_PACKED, RS_FULL, RS_NONE},   0x3, false, RS_HALF, 1, 65536, "ondca"},
    {"maxpool3d_2x_fwd_h16",         true,  {RS_FULL, RS_HALF, RS_NONE},     0x3, true,  RS_HALF, 1,  8192, "ndoca"},
    {"maxpool3d_2x_bwd_h16",         true,  {RS_HALF, RS_FULL, RS_FULL},     0xd, true,  RS_FULL, 1, 16384, "ndoca"},
    // upsample.hip: nearest and half-pixel (hp, align_corners=False) trilinear.  A thread owns an input voxel (vector
    // variant: an x pair) and its 2x2x2 outputs; in the c8 half-pixel forward, a pair of output items along x
    {"upsample_nearest2x_fwd",          false, {RS_FULL, RS_X8, RS_NONE},    0x3, false, RS_FULL, 1, 65536, "dn"},
    {"upsample_nearest2x_bwd",          false, {RS_X8, RS_FULL, RS_NONE},    0x3, false, RS_FULL, 1, 65536, "dn"},
    {"upsample_trilinear2x_hp_fwd",     false, {RS_FULL, RS_X8, RS_NONE},    0x3, false, RS_FULL, 1, 65536, "dn"},
    {"upsample_trilinear2x_hp_bwd",     false, {RS_X8, RS_FULL, RS_NONE},    0x3, false, RS_FULL, 1, 65536, "dn"},
    {"upsample_nearest2x_fwd_h16",      true,  {RS_FULL, RS_X8, RS_NONE},    0x3, false, RS_FULL, 1, 65536, "ndca"},
    {"upsample_nearest2x_bwd_h16",      true,  {RS_X8, RS_FULL, RS_NONE},    0x3, false, RS_FULL, 1, 65536, "ndca"},
    {"upsample_trilinear2x_hp_fwd_h16", true,  {RS_FULL, RS_X8, RS_NONE},    0x3, false, RS_X8,   2, 65536, "ndca"},
    {"upsample_trilinear2x_hp_bwd_h16", true,  {RS_X8, RS_FULL, RS_NONE},    0x3, false, RS_FULL, 1, 65536, "ndca"},
};

// A call as its entry point takes it.  Pointers are integers here: they are compared with zero and masked, never followed.
struct ResampleArgs {
  int32_t N, C, D, H, W, compute;
  int64_t bs[3];       // batch strides in elements, 0 = dense
  uintptr_t ptr[4];    // the tensors in the order of bs[], then the route bytes
};

struct ResamplePlan {
  int64_t bs[3];       // dense-resolved
  int variant;         // ResampleVariant
  dim3 grid;
  size_t lds;          // dynamic LDS bytes
  int64_t total;       // work items of the grid-stride loop (RS_LDS: 0, the grid is the tiling)
};

// output tile (z, y) of a block of trilinear2_fwd_lds_kernel and the input patch it stages: [TRI_PZ][TRI_PY][W] floats
constexpr int TRI_TZ = 4, TRI_TY = 16, TRI_PZ = 4, TRI_PY = 10;

static inline int64_t resample_voxels(ResampleRes r, const ResampleArgs& a) {
  if (r == RS_HALF || r == RS_PACKED) return (int64_t)(a.D / 2) * (a.H / 2) * (a.W / 2);
  return (int64_t)a.D * a.H * a.W * (r == RS_X8 ? 8 : 1);
}

static inline void resample_strides(const ResampleRow& row, const ResampleArgs& a, int64_t bs[3]) {
  for (int i = 0; i < 3; ++i) {
    const int64_t ch = row.t[i] == RS_PACKED ? 8 * (int64_t)a.C : a.C, vox = resample_voxels(row.t[i], a);
    bs[i] = row.t[i] == RS_NONE ? 0 : dense_or(a.bs[i], row.c8 ? c8_blocks(ch) * vox * 8 : ch * vox);
  }
}

static inline int validate_resample(ResampleOp op, const ResampleArgs& a) {
  const ResampleRow& row = RESAMPLE_ROWS[op];
  for (const char* k = row.order; *k; ++k) switch (*k) {
      case 'n':
        for (int i = 0; i < 4; ++i)
          M355_REQUIRE(a.ptr[i] || !(row.need >> i & 1), M355_EINVALID_ARG, "%s: null pointer", row.name);
        break;
      case 'd':
        M355_REQUIRE(a.N > 0 && a.C > 0 && a.D > 0 && a.H > 0 && a.W > 0, M355_EINVALID_ARG, "%s: non-positive dimension",
                     row.name);
        break;
      case 'o':
        M355_REQUIRE(a.D % 2 == 0 && a.H % 2 == 0 && a.W % 2 == 0, M355_EUNSUPPORTED, "%s: odd spatial size (%d,%d,%d)",
                     row.name, a.D, a.H, a.W);
        break;
      case 'c':
        M355_REQUIRE(a.compute == M355_COMPUTE_BF16 || a.compute == M355_COMPUTE_F16, M355_EINVALID_ARG,
                     "%s: compute must be M355_COMPUTE_BF16 or M355_COMPUTE_F16", row.name);
        break;
      case 'a': {
        int64_t bs[3];
        resample_strides(row, a, bs);
        if (row.c8) {
          M355_REQUIRE(((a.ptr[0] | a.ptr[1] | a.ptr[2]) & 15) == 0 && ((bs[0] | bs[1] | bs[2]) & 7) == 0 &&
                           (!row.routes || (a.ptr[3] & 7) == 0),
                       M355_EINVALID_ARG, "%s: c8 tensor not 16B aligned%s", row.name, row.routes ? " (route items: 8B)" : "");
        } else {   // the fp32 space / depth kernels move the full tensor's x pairs as float2
          const int f = row.t[0] == RS_FULL ? 0 : 1;
          M355_REQUIRE((a.ptr[f] & 7) == 0 && bs[f] % 2 == 0, M355_EUNSUPPORTED, "%s: full tensor not 8-byte aligned", row.name);
        }
        break;
      }
    }
  return M355_OK;
}

// For a call that validate_resample accepted.
static inline ResamplePlan plan_resample(ResampleOp op, const ResampleArgs& a) {
  const ResampleRow& row = RESAMPLE_ROWS[op];
  ResamplePlan p = {{0, 0, 0}, RS_SCALAR, dim3(1), 0, 0};
  resample_strides(row, a, p.bs);
  const int64_t* bs = p.bs;
  const uintptr_t* ptr = a.ptr;
  const int64_t NC = (int64_t)a.N * a.C;
  // float4 rows of the full tensors, float2 rows of the pooled one, uchar2 of the route bytes: W % 4 == 0 makes every row
  // offset a multiple of 4 elements (of 2 on the pooled side), the rest is the caller's strides and pointers
  auto vec = [&](int64_t full4, int64_t half2, uintptr_t p16, uintptr_t p8, uintptr_t p2) {
    return a.W % 4 == 0 && full4 % 4 == 0 && half2 % 2 == 0 && (p16 & 15) == 0 && (p8 & 7) == 0 && (p2 & 1) == 0;
  };
  switch (op) {
    // the vector verdicts, term by term       strides % 4       % 2     pointers & 15    & 7      & 1
    case RS_AVG_FWD: p.variant = vec(bs[0],         bs[1],  ptr[0],          ptr[1],  0);       break;   // x | y
    case RS_MAX_FWD: p.variant = vec(bs[0],         bs[1],  ptr[0],          ptr[1],  ptr[3]);  break;   // x | y | idx
    case RS_MAX_BWD: p.variant = vec(bs[1] | bs[2], bs[0],  ptr[1] | ptr[2], ptr[0],  ptr[3]);  break;   // add, dx | dy | idx
    // upsample.hip, fp32: float4 stores of two inputs' four outputs per row (the 1/8 that is read stays scalar); the
    // backward reads dy as float4 and stores its x pair as float2.  W % 2 == 0 makes every row offset a multiple of 4 (2)
    case RS_NEAR_FWD: case RS_HP_FWD:
      p.variant = a.W % 2 == 0 && bs[1] % 4 == 0 && (ptr[1] & 15) == 0;
      break;
    case RS_NEAR_BWD: case RS_HP_BWD:
      p.variant = a.W % 2 == 0 && bs[0] % 4 == 0 && (ptr[0] & 15) == 0 && bs[1] % 2 == 0 && (ptr[1] & 7) == 0;
      break;
    case RS_TRI_FWD: {
      // quads: float4 stores of y rows; lds: a block stages its input patch, grid = (y tiles, z tiles, N * C)
      const bool quads = a.W % 2 == 0 && bs[1] % 4 == 0 && (ptr[1] & 15) == 0;
      const size_t lds = (size_t)TRI_PZ * TRI_PY * a.W * sizeof(float);
      if (quads && a.D >= 2 && a.H >= 2 && lds <= 48 * 1024 && NC <= 65535 && ceil_div(2 * a.D, TRI_TZ) <= 65535) {
        p.variant = RS_LDS;
        p.lds = lds;
        p.grid = dim3((unsigned)ceil_div(2 * a.H, TRI_TY), (unsigned)ceil_div(2 * a.D, TRI_TZ), (unsigned)NC);
        return p;
      }
      if (quads && NC * a.D * a.H * 4 < (1ll << 31)) p.variant = RS_QUADS;
      break;
    }
    default: break;
  }
  p.total = (int64_t)a.N * (row.c8 ? c8_blocks(a.C) : a.C) * resample_voxels(row.work, a) / row.per_thread;
  int64_t cap = row.cap;
  if (op == RS_TRI_FWD && p.variant == RS_QUADS) p.total /= 4, cap = 65536;
  else if (p.variant == RS_VECTOR) p.total /= 2;
  p.grid = dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(p.total, 256), cap)));
  return p;
}

// The plan queries (m355_resample_plan, m355_upsample2x_plan) behind their own argument checks: the row's checks and its
// code, then out8 = variant, grid x y z, LDS bytes, the three strides.
static inline int resample_plan_query(ResampleOp op, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                                      const int64_t* strides3, const uint64_t* pointers4, int32_t compute, int64_t* out8) {
  const ResampleRow& row = RESAMPLE_ROWS[op];
  ResampleArgs a = {N, C, D, H, W, compute, {0, 0, 0}, {0, 0, 0, row.routes ? (uintptr_t)pointers4[3] : 0}};
  for (int i = 0; i < 3; ++i)   // what the entry point does not take, it does not see
    if (row.t[i] != RS_NONE) a.bs[i] = strides3[i], a.ptr[i] = (uintptr_t)pointers4[i];
  if (int rc = validate_resample(op, a)) return rc;
  const ResamplePlan p = plan_resample(op, a);
  const int64_t out[8] = {p.variant, p.grid.x, p.grid.y, p.grid.z, (int64_t)p.lds, p.bs[0], p.bs[1], p.bs[2]};
  std::copy(out, out + 8, out8);
  return M355_OK;
}

}  // namespace m355
