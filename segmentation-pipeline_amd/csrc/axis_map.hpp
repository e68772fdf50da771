// The inverse index transform of a test-time-augmentation member (flip + axis permutation), shared by the kernels that
// read a member's tensor where it lies: ensemble.hip (running mean / votes) and uncertainty.hip (running entropy).
#pragma once
#include "common.hpp"

namespace m355 {

struct AxisMap {
  int size[3];      // canonical spatial size (i0, i1, i2)
  int64_t mstride[3];  // stride, in the MEMBER tensor, of canonical axis k (negative when that axis is flipped)
  int64_t moff;     // member offset of canonical voxel (0, 0, 0)
};

// perm[j] in {0,1,2}: member axis j is canonical axis perm[j]; flip bit j: member axis j is reversed
static AxisMap make_axis_map(const int32_t* size, const int32_t* perm, int flip_mask) {
  AxisMap m{};
  int msize[3];
  for (int j = 0; j < 3; ++j) msize[j] = size[perm[j]];
  int64_t mst[3] = {(int64_t)msize[1] * msize[2], msize[2], 1};
  m.moff = 0;
  for (int k = 0; k < 3; ++k) m.size[k] = size[k];
  for (int j = 0; j < 3; ++j) {
    const int k = perm[j];
    if ((flip_mask >> j) & 1) {
      m.mstride[k] = -mst[j];
      m.moff += (int64_t)(msize[j] - 1) * mst[j];
    } else {
      m.mstride[k] = mst[j];
    }
  }
  return m;
}

// member offset (inside one channel) of canonical voxel v
__device__ __forceinline__ int64_t member_offset(const AxisMap& m, int64_t v) {
  const int64_t s12 = (int64_t)m.size[1] * m.size[2];
  const int i0 = (int)(v / s12), r = (int)(v - i0 * s12);
  const int i1 = r / m.size[2], i2 = r - i1 * m.size[2];
  return m.moff + i0 * m.mstride[0] + i1 * m.mstride[1] + i2 * m.mstride[2];
}

static int check_map_args(const char* who, const int32_t* size3, const int32_t* perm3, int flip_mask) {
  M355_REQUIRE(size3 && perm3, M355_EINVALID_ARG, "%s: null shape / permutation", who);
  M355_REQUIRE(size3[0] > 0 && size3[1] > 0 && size3[2] > 0, M355_EINVALID_ARG, "%s: non-positive size", who);
  int seen = 0;
  for (int j = 0; j < 3; ++j) {
    M355_REQUIRE(perm3[j] >= 0 && perm3[j] <= 2, M355_EINVALID_ARG, "%s: permutation entry %d out of range", who, perm3[j]);
    seen |= 1 << perm3[j];
  }
  M355_REQUIRE(seen == 7, M355_EINVALID_ARG, "%s: not a permutation of (0, 1, 2)", who);
  M355_REQUIRE(flip_mask >= 0 && flip_mask <= 7, M355_EINVALID_ARG, "%s: flip mask out of range", who);
  return M355_OK;
}

static unsigned grid_of(int64_t total) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(total, 256), 16384)); }

}  // namespace m355
