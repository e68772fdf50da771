// Lesion-wise (blob) Dice loss on device connected components (criterions/blob_loss.py): the Dice of
// HybridLogisticDiceLoss once per connected component k of the target, the other components masked out of prediction and
// target, averaged over the components of a plane and then over the planes by their channel weights (Kofler et al.,
// "blob loss: instance imbalance aware loss functions for semantic segmentation").
//
//   members of an on plane: target > 0.5 (a NaN is none);  S_k = sum_k p, Q_k = sum_k p^2, A_k = |k|,
//   B = sum of p (square_dice: of p^2) over the plane's non-members
//   d_k = 2 S_k / (A_k + S_k + B + eps)        square_dice: 2 S_k / (A_k + Q_k + B + eps),  eps = 1e-8
//   blob = sum_{on planes, K > 0} w_c (1/K) sum_k (1 - d_k) / sum_{the same planes} w_c        (0 when there is none)
//
// m355_blob_label: the on planes are thresholded into ONE stacked int32 volume [P_on * D, H, W] in which slot s holds the
// value s + 1, and m355_ccl_label (components.hip, mode 0: only equal values connect) labels it in its six launches --
// planes that touch across the stacking boundary hold different values and cannot merge.  Numbers go in raster order of
// the first voxel, so a plane's components are one contiguous range: an integer atomicMax of the label per slot and a
// running maximum over the slots give [first, last] of every plane.  n stays on the device.
// m355_blob_dice_fwd: one pass over (p, labels) of the on planes accumulates S, Q as 64-bit integers of round(p 2^f),
// round(p^2 2^f) and A as a count, with integer atomics only: integer addition is associative, so the sums repeat bit
// for bit whatever the arrival order.  f = 63 - (bits of the voxels of a plane), 60 at the most, is the largest scale at
// which no sum can overflow; planes have fewer than 2^31 voxels, so f >= 32 and each sum is off by at most (number of
// voxels summed) 2^-33 -- by far less in a small plane, where an fp32 p down to 2^(23 - f) is held exactly.  A thread owns 16
// contiguous voxels and hands a run of one label on as one add; a per-workgroup LDS hash leaves one global atomic per
// distinct component and workgroup (a probe overflow goes straight to global memory).  Zeroing and finalize read n on the
// device: their cost follows the components there are, not the capacity the accumulators are sized for.  The finalize
// kernel (one block per plane, fixed order, fp64) writes per component the two backward coefficients and per plane g_nc.
// m355_blob_dice_bwd: one launch, dp = dloss * (a_k + b_k p) for a member of k, dloss * g_nc (* 2p) for a non-member,
// formed in fp64 and rounded to fp32 once; zeros in planes that are off.
// p must be a probability: a value that is not finite or outside [0, 1] sets a status bit and loss and gradient are NaN,
// as they are when the labelling reports n = -1.
#include "loss_common.hpp"

namespace m355 {

constexpr int BLOB_NT = 256;
constexpr int BLOB_CHUNK = 4096;           // voxels per block and round of the reduction: 16 contiguous ones per thread
constexpr int BLOB_VPT = BLOB_CHUNK / BLOB_NT;
constexpr int BLOB_SLOTS = 1024;           // LDS bins of the per-workgroup hash
constexpr int BLOB_PROBES = 8;
constexpr int BLOB_MASK_PLANES = 1024;     // N * C at the most: the plane mask is 128 bytes of kernel arguments
constexpr double BLOB_EPS = 1e-8;
enum { BLOB_BAD_P = 1, BLOB_OVER_CAPACITY = 2, BLOB_LABEL_BOUND = 4 };
typedef unsigned long long u64;

struct BlobPlanes {
  uint32_t on[BLOB_MASK_PLANES / 32];
};
__device__ __forceinline__ bool blob_on(const BlobPlanes& m, int plane) { return (m.on[plane >> 5] >> (plane & 31)) & 1; }
// the slot of an on plane in the stacked volume: the on planes before it
__device__ __forceinline__ int blob_slot(const BlobPlanes& m, int plane) {
  int s = 0;
  for (int w = 0; w < (plane >> 5); ++w) s += __popc(m.on[w]);
  return s + __popc(m.on[plane >> 5] & ((1u << (plane & 31)) - 1u));
}
__device__ __forceinline__ int blob_plane_of_slot(const BlobPlanes& m, int slot) {
  for (int w = 0; w < BLOB_MASK_PLANES / 32; ++w) {
    const int c = __popc(m.on[w]);
    if (slot < c) {
      uint32_t word = m.on[w];
      for (; slot > 0; --slot) word &= word - 1;
      return w * 32 + __ffs(word) - 1;
    }
    slot -= c;
  }
  return -1;
}

__device__ __forceinline__ void row_load_i4(const int* __restrict__ p, int nv, int (&v)[4]) {
  if (nv >= 4 && ((uintptr_t)p & 15) == 0) {
    const int4 r = *reinterpret_cast<const int4*>(p);
    v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < nv ? p[j] : 0;
  }
}
__device__ __forceinline__ void row_store_i4(int* __restrict__ p, int nv, const int (&v)[4]) {
  if (nv >= 4 && ((uintptr_t)p & 15) == 0) {
    *reinterpret_cast<int4*>(p) = make_int4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nv) p[j] = v[j];
  }
}

// ---------------------------------------------------------------------------------------------------------- labelling
// x[slot][v] = slot + 1 where target > 0.5, else 0; blockIdx.y = plane.  Also zeroes the slot's label maximum.
__global__ __launch_bounds__(BLOB_NT) void blob_threshold_kernel(const float* __restrict__ t, BlobPlanes planes, int64_t S,
                                                                 int* __restrict__ x, int* __restrict__ mx) {
  const int plane = blockIdx.y;
  if (!blob_on(planes, plane)) return;
  const int slot = blob_slot(planes, plane);
  if (blockIdx.x == 0 && threadIdx.x == 0) mx[slot] = 0;
  const float* tp = t + (int64_t)plane * S;
  int* xp = x + (int64_t)slot * S;
  for (int64_t v0 = (blockIdx.x * (int64_t)BLOB_NT + threadIdx.x) * 4; v0 < S; v0 += gridDim.x * (int64_t)BLOB_NT * 4) {
    const int nv = row_valid(v0, S, 4);
    float a[4];
    int o[4];
    row_load<4>(tp + v0, nv, a);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = a[j] > 0.5f ? slot + 1 : 0;   // (a NaN compares false)
    row_store_i4(xp + v0, nv, o);
  }
}

// mx[slot] = the largest label of the slot (0: no member); blockIdx.y = slot
__global__ __launch_bounds__(BLOB_NT) void blob_range_max_kernel(const int* __restrict__ labels, int64_t S, int* mx) {
  const int* lp = labels + (int64_t)blockIdx.y * S;
  int m = 0;
  for (int64_t v0 = (blockIdx.x * (int64_t)BLOB_NT + threadIdx.x) * 4; v0 < S; v0 += gridDim.x * (int64_t)BLOB_NT * 4) {
    int l[4];
    row_load_i4(lp + v0, row_valid(v0, S, 4), l);
    m = max(max(m, l[0]), max(l[1], max(l[2], l[3])));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(&mx[blockIdx.y], m);
}

// one wave: ranges[s] = {first, last} = {1 + the largest label before slot s, max(that, mx[s])}; last < first: no component
__global__ __launch_bounds__(64) void blob_range_scan_kernel(const int* __restrict__ mx, int P_on, int* __restrict__ ranges) {
  const int lane = threadIdx.x;
  int carry = 0;
  for (int s0 = 0; s0 < P_on; s0 += 64) {
    const int s = s0 + lane;
    int v = s < P_on ? mx[s] : 0;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int t = __shfl_up(v, off, 64);
      if (lane >= off) v = max(v, t);
    }
    v = max(v, carry);
    int prev = __shfl_up(v, 1, 64);
    if (lane == 0) prev = carry;
    if (s < P_on) {
      ranges[2 * s] = prev + 1;
      ranges[2 * s + 1] = v;
    }
    carry = __shfl(v, 63, 64);
  }
}

// ---------------------------------------------------------------------------------------------------------- reduction
// the accumulators of the n components there are (3 words each: S, Q, A), of the slots, and the status word
__global__ __launch_bounds__(BLOB_NT) void blob_zero_kernel(const int* __restrict__ count, int64_t cap, int P_on,
                                                            u64* __restrict__ acc, u64* __restrict__ bacc, int* status) {
  const int64_t n = min((int64_t)max(*count, 0), cap) * 3;
  for (int64_t i = blockIdx.x * (int64_t)BLOB_NT + threadIdx.x; i < n; i += gridDim.x * (int64_t)BLOB_NT) acc[i] = 0;
  if (blockIdx.x == 0) {
    for (int s = threadIdx.x; s < P_on; s += BLOB_NT) bacc[s] = 0;
    if (threadIdx.x == 0) *status = 0;
  }
}

template <bool SQ>
__device__ __forceinline__ void blob_hash_add(int* hkey, u64* hs, u64* hq, unsigned* ha, u64* __restrict__ acc, int label,
                                              u64 s, u64 q, unsigned a) {
  int h = (int)(((unsigned)label * 2654435761u) >> 22) & (BLOB_SLOTS - 1);
  for (int p = 0; p < BLOB_PROBES; ++p) {
    const int k = atomicCAS(&hkey[h], -1, label);
    if (k == -1 || k == label) {
      atomicAdd(&hs[h], s);
      if (SQ) atomicAdd(&hq[h], q);
      atomicAdd(&ha[h], a);
      return;
    }
    h = (h + 1) & (BLOB_SLOTS - 1);
  }
  u64* o = acc + (int64_t)(label - 1) * 3;   // every probe taken by another component
  atomicAdd(&o[0], s);
  if (SQ) atomicAdd(&o[1], q);
  atomicAdd(&o[2], (u64)a);
}

// blockIdx.y = plane; the blocks of a plane walk its 4096-voxel chunks grid-stride with one hash
template <bool SQ>
__global__ __launch_bounds__(BLOB_NT) void blob_reduce_kernel(const float* __restrict__ p, const int* __restrict__ labels,
                                                              BlobPlanes planes, int64_t S, int cap, double fix,
                                                              u64* __restrict__ acc, u64* __restrict__ bacc, int* status) {
  __shared__ int hkey[BLOB_SLOTS];
  __shared__ u64 hs[BLOB_SLOTS], hq[BLOB_SLOTS];
  __shared__ unsigned ha[BLOB_SLOTS];
  __shared__ u64 scratch[BLOB_NT / 64];
  const int plane = blockIdx.y;
  if (!blob_on(planes, plane)) return;
  const int slot = blob_slot(planes, plane);
  for (int i = threadIdx.x; i < BLOB_SLOTS; i += BLOB_NT) { hkey[i] = -1; hs[i] = 0; hq[i] = 0; ha[i] = 0; }
  __syncthreads();
  const float* pp = p + (int64_t)plane * S;
  const int* lp = labels + (int64_t)slot * S;
  u64 bsum = 0;
  int flags = 0;
  const int64_t nchunks = (S + BLOB_CHUNK - 1) / BLOB_CHUNK;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t base = c * BLOB_CHUNK + (int64_t)threadIdx.x * BLOB_VPT;
    int run_l = 0;
    u64 rs = 0, rq = 0;
    unsigned ra = 0;
#pragma unroll
    for (int j = 0; j < BLOB_VPT / 4; ++j) {
      const int64_t v0 = base + 4 * j;
      const int nv = row_valid(v0, S, 4);
      if (nv == 0) break;
      float a[4];
      int l[4];
      row_load<4>(pp + v0, nv, a);
      row_load_i4(lp + v0, nv, l);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i >= nv) break;
        const float x = a[i];
        const bool ok = x >= 0.f && x <= 1.f;   // (false for a NaN)
        if (!ok) flags |= BLOB_BAD_P;
        const double xd = ok ? (double)x : 0.0;
        const u64 q1 = __double2ull_rn(xd * fix);
        const u64 q2 = SQ ? __double2ull_rn(xd * xd * fix) : 0;   // (x * x is exact in fp64)
        int lab = l[i];
        if (lab < 0 || lab > cap) { flags |= BLOB_OVER_CAPACITY; lab = 0; }
        if (lab != run_l) {
          if (run_l) blob_hash_add<SQ>(hkey, hs, hq, ha, acc, run_l, rs, rq, ra);
          run_l = lab;
          rs = 0; rq = 0; ra = 0;
        }
        if (lab == 0) bsum += SQ ? q2 : q1;
        else { rs += q1; rq += q2; ++ra; }
      }
    }
    if (run_l) blob_hash_add<SQ>(hkey, hs, hq, ha, acc, run_l, rs, rq, ra);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < BLOB_SLOTS; i += BLOB_NT) {
    const int k = hkey[i];
    if (k < 0) continue;
    u64* o = acc + (int64_t)(k - 1) * 3;
    atomicAdd(&o[0], hs[i]);
    if (SQ) atomicAdd(&o[1], hq[i]);
    atomicAdd(&o[2], (u64)ha[i]);
  }
  const u64 btotal = block_sum<u64, BLOB_NT>(bsum, scratch);
  if (threadIdx.x == 0 && btotal) atomicAdd(&bacc[slot], btotal);
  if (flags) atomicOr(status, flags);
}

// one block per slot: the plane's components in index order, thread t the components first + t, first + t + 256, ..;
// coef[k] = {a_k, b_k} with the plane's factor w_c / (K sum of the weights of the planes with a component) inside
__global__ __launch_bounds__(BLOB_NT) void blob_finalize_kernel(const u64* __restrict__ acc, const u64* __restrict__ bacc,
                                                                const int* __restrict__ ranges, const int* __restrict__ count,
                                                                const float* __restrict__ cw, BlobPlanes planes, int C,
                                                                int P_on, int cap, int sq, double fix,
                                                                double* __restrict__ coef,
                                                                double* __restrict__ gnc, double* __restrict__ plane_loss) {
  __shared__ double scratch[BLOB_NT / 64];
  const int slot = blockIdx.x;
  if (*count < 0) return;                                  // (the whole grid: the loss kernel writes NaN)
  double wpart = 0.0;
  for (int s = threadIdx.x; s < P_on; s += BLOB_NT)
    if (ranges[2 * s + 1] >= ranges[2 * s]) wpart += cw ? (double)cw[blob_plane_of_slot(planes, s) % C] : 1.0;
  const double wsum = block_sum<double, BLOB_NT, true>(wpart, scratch);
  const int first = ranges[2 * slot], last = min(ranges[2 * slot + 1], cap);
  const int K = last - first + 1;
  if (K <= 0 || !(wsum > 0.0)) {
    if (threadIdx.x == 0) { plane_loss[slot] = 0.0; gnc[slot] = 0.0; }
    return;
  }
  const double wc = cw ? (double)cw[blob_plane_of_slot(planes, slot) % C] : 1.0;
  const double f = wc / ((double)K * wsum);
  const double Bd = (double)bacc[slot] / fix;
  double lsum = 0.0, gsum = 0.0;
  for (int k = first + (int)threadIdx.x; k <= last; k += BLOB_NT) {
    const u64* a = acc + (int64_t)(k - 1) * 3;
    const double Sd = (double)a[0] / fix, Ad = (double)a[2];
    const double den = Ad + (sq ? (double)a[1] / fix : Sd) + Bd + BLOB_EPS;
    const double dB = 2.0 * Sd / (den * den);              // d(1 - d_k) / dB
    lsum += 1.0 - 2.0 * Sd / den;
    gsum += dB;
    // member of k: square form -2/den + (4 S / den^2) p; else -2/den + 2 S/den^2 = -2 (A + B + eps) / den^2, no cancellation
    coef[2 * (int64_t)(k - 1)] = f * (sq ? -2.0 / den : -2.0 * (Ad + Bd + BLOB_EPS) / (den * den));
    coef[2 * (int64_t)(k - 1) + 1] = sq ? f * 2.0 * dB : 0.0;
  }
  const double L = block_sum<double, BLOB_NT>(lsum, scratch);
  const double G = block_sum<double, BLOB_NT>(gsum, scratch);
  if (threadIdx.x == 0) { plane_loss[slot] = f * L; gnc[slot] = f * G; }
}

// one thread: the planes in index order; NaN when a status bit is set or the labelling hit a bound
__global__ void blob_loss_kernel(const double* __restrict__ plane_loss, const int* __restrict__ count, int P_on, int* status,
                                 float* __restrict__ loss, int* __restrict__ total) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int n = *count;
  int st = *status;
  if (n < 0) st |= BLOB_LABEL_BOUND;
  *status = st;                                            // (the backward reads it)
  *total = n;
  if (st) { loss[0] = __builtin_nanf(""); return; }
  double sum = 0.0;
  for (int s = 0; s < P_on; ++s) sum += plane_loss[s];
  loss[0] = (float)sum;
}

// ----------------------------------------------------------------------------------------------------------- backward
template <bool SQ>
__global__ __launch_bounds__(BLOB_NT) void blob_bwd_kernel(const float* __restrict__ p, const int* __restrict__ labels,
                                                           const double* __restrict__ coef, const double* __restrict__ gnc,
                                                           const int* __restrict__ status, const float* __restrict__ dloss,
                                                           BlobPlanes planes, int64_t S, int cap, float* __restrict__ dp) {
  const int plane = blockIdx.y;
  float* op = dp + (int64_t)plane * S;
  const bool on = blob_on(planes, plane);
  const int slot = on ? blob_slot(planes, plane) : 0;
  const bool bad = on && *status != 0;
  const double g = (double)dloss[0];
  const double gn = on && !bad ? g * gnc[slot] : 0.0;
  const float nan = __builtin_nanf("");
  const float* pp = p + (int64_t)plane * S;
  const int* lp = labels + (int64_t)slot * S;
  for (int64_t v0 = (blockIdx.x * (int64_t)BLOB_NT + threadIdx.x) * 4; v0 < S; v0 += gridDim.x * (int64_t)BLOB_NT * 4) {
    const int nv = row_valid(v0, S, 4);
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (bad) {
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = nan;
    } else if (on) {
      float a[4] = {0.f, 0.f, 0.f, 0.f};
      int l[4];
      if (SQ) row_load<4>(pp + v0, nv, a);
      row_load_i4(lp + v0, nv, l);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int lab = l[j];
        if (lab == 0) {
          o[j] = SQ ? (float)(gn * 2.0 * (double)a[j]) : (float)gn;
        } else if (lab > 0 && lab <= cap) {
          const double ca = coef[2 * (int64_t)(lab - 1)];
          o[j] = SQ ? (float)(g * fma(coef[2 * (int64_t)(lab - 1) + 1], (double)a[j], ca)) : (float)(g * ca);
        } else {
          o[j] = nan;
        }
      }
    }
    row_store<4>(op + v0, nv, o);
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
struct BlobGeom {
  int32_t P_on;
  int64_t S, cap;
  double fix;   // the scale of the fixed-point sums
  BlobPlanes mask;
};

// the shared argument checks; fills the geometry
static int blob_geom(const char* who, int32_t planes, const uint8_t* plane_on, int32_t D, int32_t H, int32_t W,
                     int32_t connectivity, BlobGeom* g) {
  M355_REQUIRE(planes >= 1, M355_EINVALID_ARG, "%s: %d planes", who, planes);
  M355_REQUIRE(D >= 1 && H >= 1 && W >= 1, M355_EINVALID_ARG, "%s: non-positive size %d x %d x %d", who, D, H, W);
  M355_REQUIRE(connectivity >= 1 && connectivity <= 3, M355_EINVALID_ARG,
               "%s: connectivity %d not in {1, 2, 3} (6, 18, 26 neighbours)", who, connectivity);
  M355_REQUIRE(planes <= BLOB_MASK_PLANES, M355_EUNSUPPORTED, "%s: %d planes (at most %d)", who, planes, BLOB_MASK_PLANES);
  *g = BlobGeom{};
  for (int32_t i = 0; i < planes; ++i)
    if (!plane_on || plane_on[i]) {
      g->mask.on[i >> 5] |= 1u << (i & 31);
      ++g->P_on;
    }
  M355_REQUIRE(g->P_on >= 1, M355_EINVALID_ARG, "%s: no plane is on", who);
  g->S = (int64_t)D * H * W;
  M355_REQUIRE(g->S < ((int64_t)1 << 31) && g->P_on * g->S < ((int64_t)1 << 31), M355_EINVALID_ARG,
               "%s: %d planes of %d x %d x %d stack to 2^31 voxels or more (labels are int32)", who, g->P_on, D, H, W);
  // components a plane can hold: 26 neighbours -- one per 2 x 2 x 2 cell; 6 or 18 -- every other voxel (a checkerboard)
  const int64_t per_plane = connectivity == 3 ? ceil_div(D, 2) * ceil_div(H, 2) * ceil_div(W, 2) : ceil_div(g->S, 2);
  g->cap = g->P_on * per_plane;
  // no sum exceeds S 2^f < 2^63: f = 63 - (bits of S) >= 32 fraction bits, 60 at the most
  int bits = 0;
  while ((g->S >> bits) != 0) ++bits;
  g->fix = ldexp(1.0, std::min(60, 63 - bits));
  return M355_OK;
}

struct BlobLabelWs {
  int* x;
  int* mx;
  void* ccl;
  size_t ccl_bytes, bytes;
};
static BlobLabelWs blob_label_layout(void* base, const BlobGeom& g, int32_t D, int32_t H, int32_t W) {
  BlobLabelWs w{};
  char* p = (char*)base;
  const size_t x_b = (size_t)round_up(g.P_on * g.S * 4, 256), mx_b = (size_t)round_up((int64_t)g.P_on * 4, 256);
  w.x = (int*)p;
  w.mx = (int*)(p + x_b);
  w.ccl = p + x_b + mx_b;
  w.ccl_bytes = m355_ccl_workspace(g.P_on * D, H, W);
  w.bytes = x_b + mx_b + w.ccl_bytes;
  return w;
}

struct BlobTables {   // saved between forward and backward
  int* status;
  double* gnc;
  double* coef;
  size_t bytes;
};
static BlobTables blob_tables_layout(void* base, const BlobGeom& g) {
  BlobTables t{};
  char* p = (char*)base;
  const size_t g_b = (size_t)round_up((int64_t)g.P_on * 8, 256);
  t.status = (int*)p;
  t.gnc = (double*)(p + 256);
  t.coef = (double*)(p + 256 + g_b);
  t.bytes = 256 + g_b + (size_t)g.cap * 16;
  return t;
}

struct BlobDiceWs {
  u64* acc;
  u64* bacc;
  double* plane_loss;
  size_t bytes;
};
static BlobDiceWs blob_dice_layout(void* base, const BlobGeom& g) {
  BlobDiceWs w{};
  char* p = (char*)base;
  const size_t s_b = (size_t)round_up((int64_t)g.P_on * 8, 256);
  w.bacc = (u64*)p;
  w.plane_loss = (double*)(p + s_b);
  w.acc = (u64*)(p + 2 * s_b);
  w.bytes = 2 * s_b + (size_t)g.cap * 24;
  return w;
}

static unsigned blob_row_blocks(int64_t S, int64_t per_block, int64_t cap) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(S, per_block), cap));
}

}  // namespace m355

using namespace m355;

extern "C" int64_t m355_blob_capacity(int32_t planes, const uint8_t* plane_on, int32_t D, int32_t H, int32_t W,
                                      int32_t connectivity) {
  BlobGeom g;
  if (blob_geom("blob_capacity", planes, plane_on, D, H, W, connectivity, &g)) return 0;
  return g.cap;
}

extern "C" size_t m355_blob_label_workspace(int32_t planes, const uint8_t* plane_on, int32_t D, int32_t H, int32_t W) {
  BlobGeom g;
  if (blob_geom("blob_label_workspace", planes, plane_on, D, H, W, 3, &g)) return 0;
  return blob_label_layout(nullptr, g, D, H, W).bytes;
}

extern "C" int m355_blob_label(const float* target, int32_t planes, const uint8_t* plane_on, int32_t D, int32_t H, int32_t W,
                               int32_t connectivity, int32_t* labels, int32_t* ranges, int32_t* count, void* workspace,
                               size_t workspace_bytes, void* stream) {
  M355_REQUIRE(target && labels && ranges && count && workspace, M355_EINVALID_ARG, "blob_label: null pointer");
  BlobGeom g;
  if (int rc = blob_geom("blob_label", planes, plane_on, D, H, W, connectivity, &g)) return rc;
  const BlobLabelWs w = blob_label_layout(workspace, g, D, H, W);
  M355_REQUIRE(workspace_bytes >= w.bytes, M355_EWORKSPACE, "blob_label: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(blob_threshold_kernel, dim3(blob_row_blocks(g.S, BLOB_NT * 4, 1024), (unsigned)planes), dim3(BLOB_NT), 0,
                     st, target, g.mask, g.S, w.x, w.mx);
  if (int rc = check_launch("blob_label: threshold")) return rc;
  if (int rc = m355_ccl_label(w.x, labels, count, g.P_on * D, H, W, connectivity, 0, w.ccl, w.ccl_bytes, stream)) return rc;
  hipLaunchKernelGGL(blob_range_max_kernel, dim3(blob_row_blocks(g.S, BLOB_CHUNK, 256), (unsigned)g.P_on), dim3(BLOB_NT), 0,
                     st, labels, g.S, w.mx);
  hipLaunchKernelGGL(blob_range_scan_kernel, dim3(1), dim3(64), 0, st, w.mx, (int)g.P_on, ranges);
  return check_launch("blob_label");
}

extern "C" size_t m355_blob_dice_workspace(int32_t planes, const uint8_t* plane_on, int32_t D, int32_t H, int32_t W,
                                           int32_t connectivity) {
  BlobGeom g;
  if (blob_geom("blob_dice_workspace", planes, plane_on, D, H, W, connectivity, &g)) return 0;
  return blob_dice_layout(nullptr, g).bytes;
}

extern "C" size_t m355_blob_dice_tables(int32_t planes, const uint8_t* plane_on, int32_t D, int32_t H, int32_t W,
                                        int32_t connectivity) {
  BlobGeom g;
  if (blob_geom("blob_dice_tables", planes, plane_on, D, H, W, connectivity, &g)) return 0;
  return blob_tables_layout(nullptr, g).bytes;
}

extern "C" int m355_blob_dice_fwd(const float* p, const int32_t* labels, const int32_t* ranges, const int32_t* count,
                                  const float* class_weights, int32_t N, int32_t C, const uint8_t* plane_on, int32_t D,
                                  int32_t H, int32_t W, int32_t connectivity, int32_t square_dice, float* loss,
                                  int32_t* total, void* tables, size_t tables_bytes, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  M355_REQUIRE(p && labels && ranges && count && loss && total && tables && workspace, M355_EINVALID_ARG,
               "blob_dice_fwd: null pointer");
  M355_REQUIRE(N >= 1 && C >= 1, M355_EINVALID_ARG, "blob_dice_fwd: non-positive size N = %d, C = %d", N, C);
  M355_REQUIRE((int64_t)N * C <= BLOB_MASK_PLANES, M355_EUNSUPPORTED, "blob_dice_fwd: N * C = %lld planes (at most %d)",
               (long long)N * C, BLOB_MASK_PLANES);
  BlobGeom g;
  if (int rc = blob_geom("blob_dice_fwd", N * C, plane_on, D, H, W, connectivity, &g)) return rc;
  const BlobTables t = blob_tables_layout(tables, g);
  const BlobDiceWs w = blob_dice_layout(workspace, g);
  M355_REQUIRE(tables_bytes >= t.bytes, M355_EWORKSPACE, "blob_dice_fwd: tables %zu < %zu bytes", tables_bytes, t.bytes);
  M355_REQUIRE(workspace_bytes >= w.bytes, M355_EWORKSPACE, "blob_dice_fwd: workspace %zu < %zu bytes", workspace_bytes,
               w.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int cap = (int)g.cap, sq = square_dice ? 1 : 0;
  hipLaunchKernelGGL(blob_zero_kernel, dim3(256), dim3(BLOB_NT), 0, st, count, g.cap, (int)g.P_on, w.acc, w.bacc, t.status);
  const dim3 grid(blob_row_blocks(g.S, BLOB_CHUNK, 512), (unsigned)(N * C));
  if (sq) hipLaunchKernelGGL(blob_reduce_kernel<true>, grid, dim3(BLOB_NT), 0, st, p, labels, g.mask, g.S, cap, g.fix, w.acc, w.bacc, t.status);
  else hipLaunchKernelGGL(blob_reduce_kernel<false>, grid, dim3(BLOB_NT), 0, st, p, labels, g.mask, g.S, cap, g.fix, w.acc, w.bacc, t.status);
  if (int rc = check_launch("blob_dice_fwd: reduction")) return rc;
  hipLaunchKernelGGL(blob_finalize_kernel, dim3((unsigned)g.P_on), dim3(BLOB_NT), 0, st, w.acc, w.bacc, ranges, count,
                     class_weights, g.mask, (int)C, (int)g.P_on, cap, sq, g.fix, t.coef, t.gnc, w.plane_loss);
  hipLaunchKernelGGL(blob_loss_kernel, dim3(1), dim3(64), 0, st, w.plane_loss, count, (int)g.P_on, t.status, loss, total);
  return check_launch("blob_dice_fwd");
}

extern "C" int m355_blob_dice_bwd(const float* p, const int32_t* labels, const void* tables, const float* dloss, int32_t N,
                                  int32_t C, const uint8_t* plane_on, int32_t D, int32_t H, int32_t W, int32_t connectivity,
                                  int32_t square_dice, float* dp, void* stream) {
  M355_REQUIRE(labels && tables && dloss && dp && (p || !square_dice), M355_EINVALID_ARG, "blob_dice_bwd: null pointer");
  M355_REQUIRE(N >= 1 && C >= 1, M355_EINVALID_ARG, "blob_dice_bwd: non-positive size N = %d, C = %d", N, C);
  M355_REQUIRE((int64_t)N * C <= BLOB_MASK_PLANES, M355_EUNSUPPORTED, "blob_dice_bwd: N * C = %lld planes (at most %d)",
               (long long)N * C, BLOB_MASK_PLANES);
  BlobGeom g;
  if (int rc = blob_geom("blob_dice_bwd", N * C, plane_on, D, H, W, connectivity, &g)) return rc;
  const BlobTables t = blob_tables_layout(const_cast<void*>(tables), g);
  const dim3 grid(blob_row_blocks(g.S, BLOB_NT * 4, 2048), (unsigned)(N * C));
  hipStream_t st = (hipStream_t)stream;
  if (square_dice) hipLaunchKernelGGL(blob_bwd_kernel<true>, grid, dim3(BLOB_NT), 0, st, p, labels, t.coef, t.gnc, t.status, dloss, g.mask, g.S, (int)g.cap, dp);
  else hipLaunchKernelGGL(blob_bwd_kernel<false>, grid, dim3(BLOB_NT), 0, st, p, labels, t.coef, t.gnc, t.status, dloss, g.mask, g.S, (int)g.cap, dp);
  return check_launch("blob_dice_bwd");
}
