// Multi-tensor optimizer step (segmentation_pipeline_amd/optim.py: FusedSGD, FusedAdam): gradient clipping by
// global norm, torch.optim.SGD / Adam / AdamW, a polynomial learning-rate schedule and an exponential moving average of the
// weights in one norm pass and one update pass over fp32 tensors.
//
//   optim_norm_kernel     (clipping only) one fp64 partial of sum g^2 per block, written to the block's own slot
//   optim_prepare_kernel  one block: partials added in slot order -> norm, clip coefficient, skip decision, step counter,
//                         learning rate / decay factor / Adam step size per group -> the state record
//   optim_update_kernel   <rule>: p, state and EMA of every tensor in one read and one write each
//
// Tensors are addressed like the entries of m355_conv3d_pack_batch (PackBatch, conv3d_common.hpp): a table of at most
// OPT_CAP entries BY VALUE in the kernel arguments, entry k owning the blocks [blk0, blk0 + ceil(n / OPT_CHUNK)) of the
// launch, a block finding its entry by scanning blk0.  A captured launch replays with the pointers of the capture, and the
// number of launches depends on the number of tensors only.
//
// Everything a step decides lives in the state record in device memory: the step counter t, the current learning rates,
// the clip coefficient and whether the step is skipped.  The update pass reads it and returns at once when `skip` is set,
// so a replayed hipGraph advances the schedule by itself and a skipped step leaves every bit where it was.
//
// No floating-point atomics: a block adds its chunk in a fixed order (thread-strided, then block_sum), the prepare block
// adds the slots in a fixed order.  Two calls on the same gradients give the same bits (region_stats.hip does the same).
// Element arithmetic is written with __f*_rn / __fmaf_rn, one expression for the vector and the scalar path, so results
// do not depend on contraction choices or on which path an element takes.
#include "common.hpp"
#include <math.h>

namespace {

using namespace m355;

constexpr int OPT_NT = 256;
constexpr int OPT_CHUNK = 8192;   // elements of one block: 8 float4 per thread and tensor class
constexpr int OPT_CAP = M355_OPTIM_CAP;
constexpr int OPT_G = M355_OPTIM_MAX_GROUPS;

// words of the state record (include/m355seg.h)
enum { ST_NORM = 0, ST_CLIP = 1, ST_GMUL = 2, ST_BC1 = 3, ST_BC2 = 4, ST_SKIP = 5, ST_T = 6, ST_LR = 8, ST_DECAY = 8 + OPT_G,
       ST_STEP = 8 + 2 * OPT_G, ST_BC2S = 8 + 3 * OPT_G };
static_assert(8 + 4 * OPT_G == M355_OPTIM_STATE_WORDS, "state record layout");

struct OptEntry {
  float* p;
  const float* g;
  float* s1;
  float* s2;
  float* ema;
  int64_t n;
  int blk0;            // first block of this entry in the launch
  short group, first;  // first: SGD sets the momentum buffer to the gradient
};
struct OptTable {
  OptEntry e[OPT_CAP];
  int n;
};
static_assert(sizeof(OptEntry) == 56, "48 entries = 2688 B of kernel arguments");

// per-group constants of the update pass, rounded once from the caller's doubles
//   SGD : a = momentum, b = 1 - dampening;              flags bit 0 momentum != 0, bit 1 nesterov
//   Adam: a = 1 - beta1, b = beta2, c = 1 - beta2, d = eps;   flags bit 0 decoupled decay (AdamW)
struct GroupH {
  float a, b, c, d, wd;
  int flags;
};
struct UpdArgs {
  GroupH g[OPT_G];
  float ema_w;   // 1 - ema_decay
  int has_ema;
};

struct PrepArgs {
  double lr[OPT_G], wd[OPT_G], beta1[OPT_G], beta2[OPT_G];
  double max_norm, power;
  int64_t nslots, total_steps;
  int groups, rule, clip;
};

__device__ __forceinline__ const OptEntry& find_entry(const OptTable& tb, int& chunk) {
  int k = 0;
  while (k + 1 < tb.n && (int)blockIdx.x >= tb.e[k + 1].blk0) ++k;
  chunk = (int)blockIdx.x - tb.e[k].blk0;
  return tb.e[k];
}

// ------------------------------------------------------------------------------------------------ norm pass
__global__ __launch_bounds__(OPT_NT) void optim_norm_kernel(const OptTable tb, int64_t slot0, double* __restrict__ part) {
  __shared__ double scratch[OPT_NT / 64];
  int chunk;
  const OptEntry& e = find_entry(tb, chunk);
  const int64_t start = (int64_t)chunk * OPT_CHUNK;
  const int cnt = (int)min((int64_t)OPT_CHUNK, e.n - start);
  const float* g = e.g + start;
  const int head = min(cnt, (int)(((16u - ((uintptr_t)g & 15u)) & 15u) >> 2));
  const int nv = (cnt - head) >> 2;
  double s = 0.0;
  bool bad = false;
  auto take = [&](float v) {
    bad |= !isfinite(v);
    s += (double)v * (double)v;   // exact in fp64
  };
  if ((int)threadIdx.x < head) take(g[threadIdx.x]);
  const float4* gv = (const float4*)(g + head);
#pragma unroll 4
  for (int i = threadIdx.x; i < nv; i += OPT_NT) {
    const float4 v = gv[i];
    take(v.x); take(v.y); take(v.z); take(v.w);
  }
  const int tail0 = head + (nv << 2);
  if (tail0 + (int)threadIdx.x < cnt) take(g[tail0 + threadIdx.x]);
  const double total = block_sum<double, OPT_NT>(s, scratch);
  const int nbad = __syncthreads_or(bad);
  // a non-finite load makes the square and so the sum non-finite by itself (squares of finite floats cannot overflow
  // fp64); the explicit flag keeps that independent of how inf and NaN meet in the sum
  if (threadIdx.x == 0) part[slot0 + blockIdx.x] = nbad ? nan("") : total;
}

// ------------------------------------------------------------------------------------------------ prepare
__global__ __launch_bounds__(OPT_NT) void optim_prepare_kernel(const PrepArgs a, const double* __restrict__ part,
                                                               const float* __restrict__ found_inf,
                                                               const float* __restrict__ grad_scale,
                                                               int32_t* __restrict__ state) {
  __shared__ double scratch[OPT_NT / 64];
  double s = 0.0;
  if (a.clip)
    for (int64_t i = threadIdx.x; i < a.nslots; i += OPT_NT) s += part[i];
  const double total = block_sum<double, OPT_NT>(s, scratch);
  if (threadIdx.x != 0) return;
  float* fs = (float*)state;
  const double inv_scale = grad_scale ? 1.0 / (double)*grad_scale : 1.0;
  const double norm = a.clip ? sqrt(total) * inv_scale : nan("");
  // clip_grad_norm_'s expression; a non-finite norm skips the step instead (the one deliberate difference)
  const float clip_coef = a.clip ? (float)fmin(1.0, a.max_norm / (norm + 1e-6)) : 1.f;
  const bool skip = (found_inf && *found_inf != 0.f) || (a.clip && !isfinite(norm));
  const int t = state[ST_T];
  fs[ST_NORM] = (float)norm;
  fs[ST_CLIP] = clip_coef;
  fs[ST_GMUL] = (float)((double)clip_coef * inv_scale);
  state[ST_SKIP] = skip ? 1 : 0;
  state[ST_T] = skip ? t : t + 1;
  double frac = 1.0;   // PolynomialLR's closed form, t = 0 on the first step
  if (a.total_steps > 0) {
    const double tt = (double)min((int64_t)t, a.total_steps);
    frac = pow(1.0 - tt / (double)a.total_steps, a.power);
  }
  for (int g = 0; g < a.groups; ++g) {
    const double lr = a.lr[g] * frac;
    fs[ST_LR + g] = (float)lr;
    fs[ST_DECAY + g] = (float)(1.0 - lr * a.wd[g]);   // AdamW: p *= 1 - lr * wd
    if (a.rule != M355_OPTIM_SGD) {
      const double bc1 = 1.0 - pow(a.beta1[g], (double)(t + 1)), bc2 = 1.0 - pow(a.beta2[g], (double)(t + 1));
      fs[ST_STEP + g] = (float)(lr / bc1);
      fs[ST_BC2S + g] = (float)sqrt(bc2);
      if (g == 0) { fs[ST_BC1] = (float)bc1; fs[ST_BC2] = (float)bc2; }
    }
  }
}

// ------------------------------------------------------------------------------------------------ update pass
struct GroupState {
  float gmul, lr, decay, step, bc2s;
};

// torch.optim.SGD (_single_tensor_sgd): g += wd * p; buf = momentum * buf + (1 - dampening) * g (the first step: buf = g);
// g = nesterov ? g + momentum * buf : buf; p -= lr * g
__device__ __forceinline__ void rule_sgd(float& p, float g, float& s1, const GroupH& h, const GroupState& st, bool first) {
  g = __fmul_rn(g, st.gmul);
  if (h.wd != 0.f) g = __fmaf_rn(h.wd, p, g);
  if (h.flags & 1) {
    const float b = first ? g : __fmaf_rn(h.b, g, __fmul_rn(h.a, s1));
    s1 = b;
    g = (h.flags & 2) ? __fmaf_rn(h.a, b, g) : b;
  }
  p = __fmaf_rn(-st.lr, g, p);
}

// torch.optim.Adam / AdamW (_single_tensor_adam): L2 decay g += wd * p, or decoupled p *= 1 - lr * wd;
// m.lerp_(g, 1 - beta1); v = beta2 * v + (1 - beta2) * g * g; denom = sqrt(v) / sqrt(bc2) + eps; p -= (lr / bc1) * m / denom
template <bool DECOUPLED>
__device__ __forceinline__ void rule_adam(float& p, float g, float& m, float& v, const GroupH& h, const GroupState& st) {
  g = __fmul_rn(g, st.gmul);
  if (DECOUPLED) p = __fmul_rn(p, st.decay);
  else if (h.wd != 0.f) g = __fmaf_rn(h.wd, p, g);
  m = __fmaf_rn(h.a, __fsub_rn(g, m), m);
  v = __fmaf_rn(__fmul_rn(h.c, g), g, __fmul_rn(h.b, v));
  const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), st.bc2s), h.d);
  p = __fmaf_rn(-st.step, __fdiv_rn(m, denom), p);
}

template <int RULE>
__device__ __forceinline__ void update_one(float& p, float g, float& s1, float& s2, float& ema, const GroupH& h,
                                           const GroupState& st, bool first, float ema_w, bool has_ema) {
  if (RULE == M355_OPTIM_SGD) rule_sgd(p, g, s1, h, st, first);
  else if (RULE == M355_OPTIM_ADAM) rule_adam<false>(p, g, s1, s2, h, st);
  else rule_adam<true>(p, g, s1, s2, h, st);
  // ema = d * ema + (1 - d) * p_new, evaluated as torch's lerp: ema + (1 - d) * (p_new - ema)
  if (has_ema) ema = __fmaf_rn(ema_w, __fsub_rn(p, ema), ema);
}

template <int RULE>
__global__ __launch_bounds__(OPT_NT) void optim_update_kernel(const OptTable tb, const UpdArgs a,
                                                              const int32_t* __restrict__ state) {
  if (state[ST_SKIP]) return;
  int chunk;
  const OptEntry& e = find_entry(tb, chunk);
  const GroupH h = a.g[e.group];
  const float* fs = (const float*)state;
  GroupState st;
  st.gmul = fs[ST_GMUL];
  st.lr = fs[ST_LR + e.group];
  st.decay = fs[ST_DECAY + e.group];
  st.step = fs[ST_STEP + e.group];
  st.bc2s = fs[ST_BC2S + e.group];
  const bool first = e.first != 0, has_ema = a.has_ema != 0;
  const bool has1 = RULE != M355_OPTIM_SGD || (h.flags & 1), has2 = RULE != M355_OPTIM_SGD;
  const int64_t start = (int64_t)chunk * OPT_CHUNK;
  const int cnt = (int)min((int64_t)OPT_CHUNK, e.n - start);
  float* p = e.p + start;
  const float* g = e.g + start;
  float* s1 = has1 ? e.s1 + start : nullptr;
  float* s2 = has2 ? e.s2 + start : nullptr;
  float* ema = has_ema ? e.ema + start : nullptr;
  // 16-byte accesses need every tensor of the entry aligned at the same element: a common scalar head brings them there
  // when they share their offset inside 16 bytes; tensors that do not (a view 4 bytes into its storage next to an aligned
  // gradient) take the scalar path for the whole chunk
  const unsigned mis = (unsigned)((uintptr_t)p & 15u);
  bool same = ((uintptr_t)g & 15u) == mis;
  if (has1) same = same && ((uintptr_t)s1 & 15u) == mis;
  if (has2) same = same && ((uintptr_t)s2 & 15u) == mis;
  if (has_ema) same = same && ((uintptr_t)ema & 15u) == mis;
  const int head = same ? min(cnt, (int)(((16u - mis) & 15u) >> 2)) : cnt;
  const int nv = (cnt - head) >> 2;
  const int tail0 = head + (nv << 2);

  auto scalar = [&](int i) {
    float pv = p[i], m1 = has1 ? s1[i] : 0.f, m2 = has2 ? s2[i] : 0.f, ev = has_ema ? ema[i] : 0.f;
    update_one<RULE>(pv, g[i], m1, m2, ev, h, st, first, a.ema_w, has_ema);
    p[i] = pv;
    if (has1) s1[i] = m1;
    if (has2) s2[i] = m2;
    if (has_ema) ema[i] = ev;
  };
  for (int i = threadIdx.x; i < head; i += OPT_NT) scalar(i);
  for (int i = tail0 + threadIdx.x; i < cnt; i += OPT_NT) scalar(i);

  float4* pv4 = (float4*)(p + head);
  const float4* gv4 = (const float4*)(g + head);
  float4* s1v4 = has1 ? (float4*)(s1 + head) : nullptr;
  float4* s2v4 = has2 ? (float4*)(s2 + head) : nullptr;
  float4* ev4 = has_ema ? (float4*)(ema + head) : nullptr;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 2
  for (int i = threadIdx.x; i < nv; i += OPT_NT) {
    float4 pv = pv4[i];
    const float4 gv = gv4[i];
    float4 m1 = has1 ? s1v4[i] : zero, m2 = has2 ? s2v4[i] : zero, ev = has_ema ? ev4[i] : zero;
    update_one<RULE>(pv.x, gv.x, m1.x, m2.x, ev.x, h, st, first, a.ema_w, has_ema);
    update_one<RULE>(pv.y, gv.y, m1.y, m2.y, ev.y, h, st, first, a.ema_w, has_ema);
    update_one<RULE>(pv.z, gv.z, m1.z, m2.z, ev.z, h, st, first, a.ema_w, has_ema);
    update_one<RULE>(pv.w, gv.w, m1.w, m2.w, ev.w, h, st, first, a.ema_w, has_ema);
    pv4[i] = pv;
    if (has1) s1v4[i] = m1;
    if (has2) s2v4[i] = m2;
    if (has_ema) ev4[i] = ev;
  }
}

// ------------------------------------------------------------------------------------------------ host
inline bool fin(double v) { return std::isfinite(v); }

// the checks every entry point that takes a descriptor shares; `fn` names it in the message
int check_desc(const m355_optim_desc* d, const char* fn) {
  M355_REQUIRE(d, M355_EINVALID_ARG, "%s: null descriptor", fn);
  M355_REQUIRE(d->rule >= M355_OPTIM_SGD && d->rule <= M355_OPTIM_ADAMW, M355_EINVALID_ARG, "%s: rule %d", fn, d->rule);
  M355_REQUIRE(d->groups >= 1 && d->groups <= OPT_G, M355_EINVALID_ARG, "%s: %d parameter groups (1 .. %d)", fn, d->groups,
               OPT_G);
  M355_REQUIRE(d->clip == 0 || (fin(d->max_norm) && d->max_norm > 0.0), M355_EINVALID_ARG,
               "%s: max_norm must be finite and positive", fn);
  M355_REQUIRE(d->total_steps >= 0 && fin(d->power) && d->power >= 0.0, M355_EINVALID_ARG,
               "%s: schedule needs total_steps >= 0 and a finite power >= 0", fn);
  M355_REQUIRE(d->ema_decay < 0.0 || (fin(d->ema_decay) && d->ema_decay < 1.0), M355_EINVALID_ARG,
               "%s: ema_decay must lie in [0, 1) (negative: no EMA)", fn);
  for (int g = 0; g < d->groups; ++g) {
    const m355_optim_group& q = d->group[g];
    M355_REQUIRE(fin(q.lr) && q.lr >= 0.0, M355_EINVALID_ARG, "%s: group %d: lr must be finite and >= 0", fn, g);
    M355_REQUIRE(fin(q.weight_decay) && q.weight_decay >= 0.0, M355_EINVALID_ARG,
                 "%s: group %d: weight_decay must be finite and >= 0", fn, g);
    if (d->rule == M355_OPTIM_SGD) {
      M355_REQUIRE(fin(q.momentum) && q.momentum >= 0.0 && fin(q.dampening), M355_EINVALID_ARG,
                   "%s: group %d: momentum must be finite and >= 0, dampening finite", fn, g);
      M355_REQUIRE(!q.nesterov || (q.momentum > 0.0 && q.dampening == 0.0), M355_EINVALID_ARG,
                   "%s: group %d: nesterov needs a momentum and zero dampening", fn, g);
    } else {
      M355_REQUIRE(fin(q.beta1) && q.beta1 >= 0.0 && q.beta1 < 1.0 && fin(q.beta2) && q.beta2 >= 0.0 && q.beta2 < 1.0,
                   M355_EINVALID_ARG, "%s: group %d: betas must lie in [0, 1)", fn, g);
      M355_REQUIRE(fin(q.eps) && q.eps >= 0.0, M355_EINVALID_ARG, "%s: group %d: eps must be finite and >= 0", fn, g);
    }
  }
  return M355_OK;
}

// entries -> the kernel's table; `blocks` = the grid.  need_state: the update pass (param, state and EMA pointers)
int build_table(const m355_optim_tensor* t, int32_t n, const m355_optim_desc* d, OptTable& tb, int64_t& blocks,
                const char* fn) {
  M355_REQUIRE(t, M355_EINVALID_ARG, "%s: null tensor table", fn);
  M355_REQUIRE(n >= 1, M355_EINVALID_ARG, "%s: %d tensors", fn, n);
  M355_REQUIRE(n <= OPT_CAP, M355_EINVALID_ARG, "%s: %d tensors (at most %d a launch)", fn, n, OPT_CAP);
  blocks = 0;
  for (int i = 0; i < n; ++i) {
    const m355_optim_tensor& s = t[i];
    M355_REQUIRE(s.n >= 0, M355_EINVALID_ARG, "%s: tensor %d: negative element count", fn, i);
    M355_REQUIRE(s.grad && ((uintptr_t)s.grad & 3u) == 0, M355_EINVALID_ARG, "%s: tensor %d: null or misaligned gradient", fn,
                 i);
    M355_REQUIRE(s.blk0 >= 0 && s.blk0 == t[0].blk0 + blocks, M355_EINVALID_ARG,
                 "%s: tensor %d: blk0 does not continue the plan (m355_optim_plan)", fn, i);
    OptEntry& e = tb.e[i];
    e.g = (const float*)s.grad;
    e.n = s.n;
    e.blk0 = (int)blocks;
    e.p = e.s1 = e.s2 = e.ema = nullptr;
    e.group = 0;
    e.first = 0;
    if (d) {
      M355_REQUIRE(s.group >= 0 && s.group < d->groups, M355_EINVALID_ARG, "%s: tensor %d: group %d of %d", fn, i, s.group,
                   d->groups);
      const bool need1 = d->rule != M355_OPTIM_SGD || d->group[s.group].momentum != 0.0, need2 = d->rule != M355_OPTIM_SGD;
      M355_REQUIRE(s.param && (!need1 || s.state1) && (!need2 || s.state2) && (d->ema_decay < 0.0 || s.ema),
                   M355_EINVALID_ARG, "%s: tensor %d: null parameter, state or EMA pointer", fn, i);
      M355_REQUIRE((((uintptr_t)s.param | (uintptr_t)s.state1 | (uintptr_t)s.state2 | (uintptr_t)s.ema) & 3u) == 0,
                   M355_EINVALID_ARG, "%s: tensor %d: pointer not aligned to 4 bytes", fn, i);
      e.p = (float*)s.param;
      e.s1 = (float*)s.state1;
      e.s2 = (float*)s.state2;
      e.ema = (float*)s.ema;
      e.group = (short)s.group;
      e.first = (short)(s.first != 0);
    }
    blocks += ceil_div(s.n, OPT_CHUNK);
    M355_REQUIRE(blocks <= INT32_MAX, M355_EINVALID_ARG, "%s: more than 2^31 - 1 blocks in one launch", fn);
  }
  tb.n = n;
  return M355_OK;
}

}  // namespace

extern "C" int32_t m355_optim_capacity(void) { return OPT_CAP; }

extern "C" int m355_optim_plan(const int64_t* counts, int32_t T, int32_t* chunk, int64_t* blk0, int64_t* nblk,
                               size_t* workspace_bytes) {
  M355_REQUIRE(T >= 0, M355_EINVALID_ARG, "optim_plan: negative number of tensors");
  M355_REQUIRE((counts && blk0 && nblk) || T == 0, M355_EINVALID_ARG, "optim_plan: null pointer");
  M355_REQUIRE(chunk && workspace_bytes, M355_EINVALID_ARG, "optim_plan: null pointer");
  int64_t blocks = 0;
  for (int i = 0; i < T; ++i) {
    M355_REQUIRE(counts[i] >= 0, M355_EINVALID_ARG, "optim_plan: tensor %d: negative element count", i);
    blk0[i] = blocks;
    nblk[i] = ceil_div(counts[i], OPT_CHUNK);
    blocks += nblk[i];
  }
  *chunk = OPT_CHUNK;
  *workspace_bytes = (size_t)round_up(std::max<int64_t>(blocks, 1) * (int64_t)sizeof(double), 256);   // one partial per block
  return M355_OK;
}

extern "C" int m355_optim_norm(const m355_optim_tensor* tensors, int32_t n, void* workspace, size_t workspace_bytes,
                               void* stream) {
  OptTable tb;
  int64_t blocks;
  const int rc = build_table(tensors, n, nullptr, tb, blocks, "optim_norm");
  if (rc != M355_OK) return rc;
  M355_REQUIRE(workspace, M355_EINVALID_ARG, "optim_norm: null workspace");
  M355_REQUIRE((uint64_t)(tensors[0].blk0 + blocks) * sizeof(double) <= workspace_bytes, M355_EINVALID_ARG,
               "optim_norm: workspace too small for the partials of these blocks");
  if (blocks == 0) return M355_OK;
  hipLaunchKernelGGL(optim_norm_kernel, dim3((unsigned)blocks), dim3(OPT_NT), 0, (hipStream_t)stream, tb, tensors[0].blk0,
                     (double*)workspace);
  return check_launch("optim_norm");
}

extern "C" int m355_optim_prepare(const m355_optim_desc* desc, int64_t nslots, const void* workspace, size_t workspace_bytes,
                                  const float* found_inf, const float* grad_scale, void* state, void* stream) {
  const int rc = check_desc(desc, "optim_prepare");
  if (rc != M355_OK) return rc;
  M355_REQUIRE(state && ((uintptr_t)state & 3u) == 0, M355_EINVALID_ARG, "optim_prepare: null or misaligned state record");
  M355_REQUIRE(nslots >= 0, M355_EINVALID_ARG, "optim_prepare: negative number of partials");
  M355_REQUIRE(!desc->clip || (workspace && (uint64_t)nslots * sizeof(double) <= workspace_bytes), M355_EINVALID_ARG,
               "optim_prepare: null workspace, or too small for %lld partials", (long long)nslots);
  PrepArgs a;
  for (int g = 0; g < OPT_G; ++g) {
    const bool on = g < desc->groups;
    a.lr[g] = on ? desc->group[g].lr : 0.0;
    a.wd[g] = on ? desc->group[g].weight_decay : 0.0;
    a.beta1[g] = on ? desc->group[g].beta1 : 0.0;
    a.beta2[g] = on ? desc->group[g].beta2 : 0.0;
  }
  a.max_norm = desc->max_norm;
  a.power = desc->power;
  a.nslots = nslots;
  a.total_steps = desc->total_steps;
  a.groups = desc->groups;
  a.rule = desc->rule;
  a.clip = desc->clip != 0;
  hipLaunchKernelGGL(optim_prepare_kernel, dim3(1), dim3(OPT_NT), 0, (hipStream_t)stream, a, (const double*)workspace,
                     found_inf, grad_scale, (int32_t*)state);
  return check_launch("optim_prepare");
}

extern "C" int m355_optim_update(const m355_optim_desc* desc, const m355_optim_tensor* tensors, int32_t n, const void* state,
                                 void* stream) {
  int rc = check_desc(desc, "optim_update");
  if (rc != M355_OK) return rc;
  OptTable tb;
  int64_t blocks;
  rc = build_table(tensors, n, desc, tb, blocks, "optim_update");
  if (rc != M355_OK) return rc;
  M355_REQUIRE(state && ((uintptr_t)state & 3u) == 0, M355_EINVALID_ARG, "optim_update: null or misaligned state record");
  if (blocks == 0) return M355_OK;
  UpdArgs a;
  for (int g = 0; g < OPT_G; ++g) {
    GroupH& h = a.g[g];
    h = GroupH{0.f, 0.f, 0.f, 0.f, 0.f, 0};
    if (g >= desc->groups) continue;
    const m355_optim_group& q = desc->group[g];
    h.wd = (float)q.weight_decay;
    if (desc->rule == M355_OPTIM_SGD) {
      h.a = (float)q.momentum;
      h.b = (float)(1.0 - q.dampening);
      h.flags = (q.momentum != 0.0 ? 1 : 0) | (q.nesterov ? 2 : 0);
    } else {
      h.a = (float)(1.0 - q.beta1);
      h.b = (float)q.beta2;
      h.c = (float)(1.0 - q.beta2);
      h.d = (float)q.eps;
      h.flags = desc->rule == M355_OPTIM_ADAMW ? 1 : 0;
    }
  }
  a.has_ema = desc->ema_decay >= 0.0;
  a.ema_w = a.has_ema ? (float)(1.0 - desc->ema_decay) : 0.f;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), block(OPT_NT);
  const int32_t* rec = (const int32_t*)state;
  if (desc->rule == M355_OPTIM_SGD)
    hipLaunchKernelGGL((optim_update_kernel<M355_OPTIM_SGD>), grid, block, 0, st, tb, a, rec);
  else if (desc->rule == M355_OPTIM_ADAM)
    hipLaunchKernelGGL((optim_update_kernel<M355_OPTIM_ADAM>), grid, block, 0, st, tb, a, rec);
  else
    hipLaunchKernelGGL((optim_update_kernel<M355_OPTIM_ADAMW>), grid, block, 0, st, tb, a, rec);
  return check_launch("optim_update");
}
