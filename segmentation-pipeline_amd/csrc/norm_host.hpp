// Host half of the normalisation family (norm.hip, act16.hip, train16.hip): a descriptor resolves ONCE to a NormPlan --
// statistics geometry, the chunk geometry and workspace offsets of the backward partials, dense-resolved batch strides --
// and norm_pass() turns (plan, pass, pointers) into the vector-path verdict and the grid of that pass.  The workspace
// query, the workspace check, m355_norm_plan and every launcher read these numbers and no others.
#pragma once
#include "h16.hpp"

namespace m355 {

// which tensors a call moves: fp32 NCDHW | fp32 in, a c8 twin of the output (forward: grid.y = channel blocks) | c8
enum NormLayout { NORM_F32, NORM_F32_C8, NORM_C8 };

// The backward's first pass writes partial[((n*C + c)*nblk + b)*2 + {0,1}] (double) at the start of the workspace, one
// entry per chunk b of channel (n, c); stat_m[nstats][2] (float) follows at stat_m_off, the partials' size rounded to 256.
struct NormBwdGeom {
  int nblk;
  size_t stat_m_off;
};

struct NormPlan {
  NormLayout layout;
  // statistics.  BN: s = channel, N runs of S floats; GN: s = n*groups + g, one run of (C/groups)*S floats
  int64_t nstats, runs, len, count;   // count = runs * len
  int nblk;                           // NORM_CHUNK blocks per statistic: partial[(s*nblk + b)*2 + {0,1}] at the workspace's start
  int64_t xbs, ybs, abs_;             // batch strides of the descriptor's fp32 tensors, dense-resolved (elements)
  int64_t dense16;                    // dense batch stride of a c8 tensor of C channels (elements)
  NormBwdGeom bwd_f32, bwd_c8;        // NORM_CHUNK (fp32 first pass) and NORM_CHUNK_C8 (c8 first pass)
  size_t stat_m_bytes, workspace_bytes;

  const NormBwdGeom& bwd() const { return layout >= NORM_C8 ? bwd_c8 : bwd_f32; }
  double* partial(void* ws) const { return (double*)ws; }
  float* stat_m(void* ws) const { return (float*)((char*)ws + bwd().stat_m_off); }
  int64_t bs16(int64_t stride) const { return dense_or(stride, dense16); }
};

static inline NormPlan plan_norm(const m355_norm_desc* d, NormLayout layout) {
  NormPlan p;
  p.layout = layout;
  if (d->groups == 0) {
    p.nstats = d->C;
    p.runs = d->N;
    p.len = d->S;
  } else {
    p.nstats = (int64_t)d->N * d->groups;
    p.runs = 1;
    p.len = (int64_t)(d->C / d->groups) * d->S;
  }
  p.count = p.runs * p.len;
  p.nblk = (int)ceil_div(p.count, NORM_CHUNK);
  const int64_t CS = (int64_t)d->C * d->S, NC = (int64_t)d->N * d->C;
  p.xbs = dense_or(d->x_batch_stride, CS);
  p.ybs = dense_or(d->y_batch_stride, CS);
  p.abs_ = dense_or(d->add_batch_stride, CS);
  p.dense16 = c8_blocks(d->C) * d->S * 8;
  auto bwd = [&](int chunk) {
    NormBwdGeom g;
    g.nblk = (int)ceil_div(d->S, chunk);
    g.stat_m_off = (size_t)round_up(NC * g.nblk * 2 * (int64_t)sizeof(double), 256);
    return g;
  };
  p.bwd_f32 = bwd(NORM_CHUNK);
  p.bwd_c8 = bwd(NORM_CHUNK_C8);
  p.stat_m_bytes = (size_t)p.nstats * 2 * sizeof(float);
  // One buffer serves every layout: the largest end over the statistics partials and the two backward layouts.  With
  // today's chunk sizes that is always the c8 end (N*C*ceil(S/4096) >= nstats*ceil(count/16384) for BN and GN alike);
  // the maximum is written out so that a change of either chunk size cannot undersize the buffer.  Behind it stays the
  // room the former two-stage finalize had for per-channel sums (N*C pairs of doubles) and 512 bytes of slack: nothing
  // lives there now, the query's answers are kept as they were.
  const size_t stats_bytes = (size_t)p.nstats * p.nblk * 2 * sizeof(double);
  const size_t reserve = (size_t)round_up(NC * 2 * (int64_t)sizeof(double), 256) + 512;
  p.workspace_bytes = std::max({stats_bytes, p.bwd_f32.stat_m_off + p.stat_m_bytes, p.bwd_c8.stat_m_off + p.stat_m_bytes}) +
                      reserve;
  return p;
}

// One validator for the family.  fp32 layout: grid.y = C, so N, C <= 65535 (M355_EUNSUPPORTED past them, checked last);
// every layout with a c8 side: grid.y = channel blocks, the limit is part of the shape check (M355_EINVALID_ARG, as
// before).  The activation code (0..6, activation.hpp) is checked for the fp32 layout only: the c8 forward passes treat an
// unknown code as "none", the c8 backward checks it itself (norm_bwd_c8_check).
static inline int validate_norm(const m355_norm_desc* d, const char* who, NormLayout layout) {
  M355_REQUIRE(d != nullptr, M355_EINVALID_ARG, "%s: null descriptor", who);
  if (layout == NORM_F32)
    M355_REQUIRE(d->N > 0 && d->C > 0 && d->S > 0, M355_EINVALID_ARG, "%s: non-positive size", who);
  else
    M355_REQUIRE(d->N > 0 && d->C > 0 && d->S > 0 && d->N <= 65535 && c8_blocks(d->C) <= 65535, M355_EINVALID_ARG,
                 "%s: bad shape", who);
  M355_REQUIRE(d->groups >= 0 && (d->groups == 0 || d->C % d->groups == 0), M355_EINVALID_ARG,
               "%s: C=%d not divisible by groups=%d", who, d->C, d->groups);
  if (layout != NORM_F32) return M355_OK;
  M355_REQUIRE(d->act >= M355_ACT_NONE && d->act <= M355_ACT_SILU, M355_EINVALID_ARG, "%s: bad activation %d", who,
               d->act);
  M355_REQUIRE(d->N <= 65535 && d->C <= 65535, M355_EUNSUPPORTED, "%s: N or C > 65535", who);
  return M355_OK;
}

static inline int check_h16(const char* who, int32_t compute) {
  M355_REQUIRE(compute == M355_COMPUTE_BF16 || compute == M355_COMPUTE_F16, M355_EINVALID_ARG,
               "%s: compute must be M355_COMPUTE_BF16 or M355_COMPUTE_F16", who);
  return M355_OK;
}

// the passes, in the numbering of m355_norm_plan's `which`
enum NormPass {
  NORM_STATS,      // norm_partial_kernel
  NORM_FWD,        // norm_act_fwd_kernel
  NORM_FWD_H16,    // norm_act_fwd_c8_kernel (fp32 in, c8 + optional fp32 out)
  NORM_FWD_C8,     // norm_act_c8c8_kernel
  NORM_POOL_FWD,   // norm_act_pool_fwd_kernel
  NORM_BWD1,       // norm_bwd_partial_kernel
  NORM_BWD2,       // norm_bwd_apply_kernel
  NORM_BWD2_H16,   // norm_bwd_apply_c8_kernel (dx as fp32 and c8)
  NORM_BWD1_C8,    // norm_bwd_partial_c8_kernel
  NORM_BWD2_C8,    // norm_bwd_apply_c8c8_kernel
  NORM_PASS_COUNT
};

struct NormLaunch {
  bool vec;            // the kernel's VEC variant (false where the kernel has none)
  int nblk;            // chunks per statistic (NORM_STATS) / per channel (first backward passes), else 0
  dim3 grid;
};

// `ptrs`: the OR of the addresses the pass's verdict looks at (0 = all aligned, what m355_norm_plan assumes).
static inline NormLaunch norm_pass(const m355_norm_desc* d, const NormPlan& p, NormPass pass, uintptr_t ptrs = 0) {
  const int64_t S = d->S;
  const unsigned N = (unsigned)d->N, Cc = (unsigned)d->C, CB = (unsigned)c8_blocks(d->C);
  // a float4 never straddles a run or a sample: every listed size a multiple of 4 elements, every pointer 16-byte aligned
  auto vec4 = [&](int64_t a, int64_t b, int64_t c, int64_t e) { return ((a | b | c | e) & 3) == 0 && (ptrs & 15) == 0; };
  auto bx = [](int64_t work, int per_thread, int cap) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(work, 256 * per_thread), cap));
  };
  NormLaunch L = {false, 0, dim3(1)};
  switch (pass) {
    // the vector verdicts, term by term     sizes % 4                          pointers
    case NORM_STATS: L.vec = vec4(p.len, S, p.xbs, 0);       break;   // x              (len: a run's end is a float4's end)
    case NORM_FWD:   L.vec = vec4(S, p.xbs, p.ybs, p.abs_);  break;   // x, y, add      (abs_ counts with a null add too)
    case NORM_BWD1:  L.vec = vec4(S, p.xbs, p.ybs, 0);       break;   // x, dy
    case NORM_BWD2:  L.vec = vec4(S, p.xbs, p.ybs, 0);       break;   // x, dy, dx
    case NORM_FWD_H16: L.vec = S >= 4096; break;   // not an alignment verdict: four voxels per thread in flight on large tensors
    default: break;
  }
  switch (pass) {
    case NORM_STATS: L.nblk = p.nblk; L.grid = dim3((unsigned)p.nblk, (unsigned)p.nstats); break;
    case NORM_FWD: case NORM_BWD2: L.grid = dim3(bx(L.vec ? S / 4 : S, 4, 1024), Cc, N); break;
    case NORM_FWD_H16: L.grid = dim3(bx(S, L.vec ? 4 : 1, 2048), CB, N); break;
    case NORM_FWD_C8: L.grid = dim3(bx(S, 4, 2048), CB, N); break;
    case NORM_POOL_FWD: L.grid = dim3(bx(S / 8, 2, 1024), Cc, N); break;
    case NORM_BWD1: L.nblk = p.bwd_f32.nblk; L.grid = dim3((unsigned)L.nblk, Cc, N); break;
    case NORM_BWD1_C8: L.nblk = p.bwd_c8.nblk; L.grid = dim3((unsigned)L.nblk, CB, N); break;
    case NORM_BWD2_H16: case NORM_BWD2_C8: L.grid = dim3(bx(S, 2, 1024), CB, N); break;
    default: break;
  }
  return L;
}

// launchers that cross the three files.  Second backward pass with dx as fp32 and c8 (act16.hip):
int launch_norm_bwd_apply_c8(const m355_norm_desc* d, const NormPlan& p, const float* x, const float* dy, const float* mean,
                             const float* rstd, const float* gamma, const float* beta, const float* stat_m, float* dx,
                             void* dx16, int64_t dx16bs, int compute, hipStream_t st);
// finalize stage of the backward (norm.hip), shared by the fp32 and c8 first passes: nblk = p.bwd().nblk
int launch_norm_bwd_reduce(const m355_norm_desc* d, const NormPlan& p, const double* partial, const float* gamma, float* dgamma,
                           float* dbeta, float* stat_m, int training, const double* count_ptr, float grad_unscale, int* oflag,
                           hipStream_t st);

}  // namespace m355
