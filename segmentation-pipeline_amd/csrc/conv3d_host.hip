// Host layer of the 3x3x3 convolutions: every extern "C" conv, pack and act16 entry point.  A query returns a number of the
// route (conv3d_route.hpp) under the facts "aligned, everything optional absent"; a launching entry point writes its
// arguments into a ConvArgs, runs the ONE check of its group -- which resolves the route -- and hands route and pointers
// to the launcher; m355_conv3d_launch_plan stops after the check and reports the route.  Kernels: conv3d*.hip, none here.
#include "conv3d_common.hpp"

using namespace m355;

// ---------------------------------------------------------------------- ABI
static ConvRoute query_conv(const m355_conv3d_desc* d, int which) { return route_conv(d, conv_query_args(which)); }
static BwwRoute query_bww(const m355_conv3d_desc* d) { return route_bww(d, conv_query_args(2)); }
static BwwRoute query_bww_c8(const m355_conv3d_desc* d) {
  ConvArgs a{};
  a.entry = CE_BWD_WEIGHT_H16;
  return route_bww_c8(d, a);
}

// ---- queries: a number of the route ----
extern "C" size_t m355_conv3d_fwd_workspace(const m355_conv3d_desc* d) { return d ? query_conv(d, 0).workspace_bytes : 0; }
extern "C" size_t m355_conv3d_bwd_data_workspace(const m355_conv3d_desc* d) { return d ? query_conv(d, 1).workspace_bytes : 0; }
extern "C" size_t m355_conv3d_h16_workspace(const m355_conv3d_desc* d, int32_t which) {
  return d ? query_conv(d, which).h16_workspace_bytes : 0;
}
extern "C" size_t m355_conv3d_bwd_weight_workspace(const m355_conv3d_desc* d) { return d ? query_bww(d).workspace_bytes : 0; }
extern "C" size_t m355_conv3d_bwd_weight_h16_workspace(const m355_conv3d_desc* d) {
  return d ? query_bww_c8(d).h16_workspace_bytes : 0;
}
extern "C" size_t m355_conv3d_bwd_weight_c8_workspace(const m355_conv3d_desc* d) {
  return d ? query_bww_c8(d).c8_workspace_bytes : 0;
}
extern "C" size_t m355_conv3d_packed_bytes(const m355_conv3d_desc* d, int32_t which) {
  if (!d || d->N <= 0 || d->Cin <= 0 || d->Cout <= 0) return 0;
  return query_conv(d, which).packed_bytes;
}
extern "C" int64_t m355_conv3d_stats_slots(const m355_conv3d_desc* d) { return d ? query_conv(d, 0).stats_slots : 0; }
extern "C" int64_t m355_conv3d_stats_slots_c8(const m355_conv3d_desc* d) { return d ? query_conv(d, 0).stats_slots_c8 : 0; }
extern "C" int32_t m355_conv3d_fuses_softmax(const m355_conv3d_desc* d) { return d && query_conv(d, 0).fuses_softmax ? 1 : 0; }
extern "C" int32_t m355_conv3d_fuses_sigmoid(const m355_conv3d_desc* d) { return m355_conv3d_fuses_softmax(d); }   // the same epilogue slot
// (the codes: include/m355seg.h; 2 = the small-Cout forward, conv3_valu_smallcout_kernel unless M355_SMALLCOUT_VALU=0)
extern "C" int m355_conv3d_plan(const m355_conv3d_desc* d, int32_t which, int32_t* out4) {
  M355_REQUIRE(d && out4, M355_EINVALID_ARG, "conv3d_plan: null pointer");
  std::copy_n(which == 2 ? query_bww(d).plan_code : query_conv(d, which).plan_code, 4, out4);
  return M355_OK;
}

// ---- forward and data gradient: one check (it resolves the route), then the launcher of the route's kind ----
static inline uintptr_t P(const void* p) { return (uintptr_t)p; }

static int run_conv(const ConvArgs& a, const m355_conv3d_desc* d, void* stream) {
  ConvRoute r;
  if (int rc = check_conv(a, d, &r)) return rc;
  const bool in16 = conv_entry_c8_in(a.entry);
  const ConvCall c = {d, in16 ? nullptr : (const float*)a.in, in16 ? (const void*)a.in : nullptr, (const float*)a.w,
                      (const float*)a.bias, (const float*)a.add, (float*)a.out, (float*)a.stat,
                      r.out16 && r.transpose && d->compute == M355_COMPUTE_F16 ? overflow_flag() : nullptr, (void*)a.ws,
                      (hipStream_t)stream};
  return is_h16(r.kind) ? launch_h16_conv(r, c) : launch_f32_conv(r, c);
}

extern "C" int m355_conv3d_fwd(const m355_conv3d_desc* d, const float* x, const float* w,
                               const float* bias, const float* add, float* y, void* workspace,
                               size_t workspace_bytes, void* stream) {
  return run_conv({CE_FWD, P(x), P(w), P(bias), P(add), P(y), 0, P(workspace), workspace_bytes, {0, 0}}, d, stream);
}

extern "C" int m355_conv3d_fwd_stats(const m355_conv3d_desc* d, const float* x, const float* w,
                                     const float* bias, const float* add, float* y, float* stat_partials,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  return run_conv({CE_FWD_STATS, P(x), P(w), P(bias), P(add), P(y), P(stat_partials), P(workspace), workspace_bytes, {0, 0}}, d,
                  stream);
}

extern "C" int m355_conv3d_bwd_data(const m355_conv3d_desc* d, const float* dy, const float* w, float* dx, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  return run_conv({CE_BWD_DATA, P(dy), P(w), 0, 0, P(dx), 0, P(workspace), workspace_bytes, {0, 0}}, d, stream);
}

// ---- packed weights (M355_CONV_W_PACKED) ----
extern "C" int m355_conv3d_pack(const m355_conv3d_desc* d, int32_t which, const float* w, void* packed, void* stream) {
  if (int rc = validate_conv(d, "conv3d_pack")) return rc;
  M355_REQUIRE(w && packed && ((uintptr_t)packed & 15) == 0, M355_EINVALID_ARG, "conv3d_pack: null / unaligned pointer");
  const ConvRoute r = query_conv(d, which);   // (the packed layout depends on the descriptor alone)
  M355_REQUIRE(r.kind != ConvKind::Direct && (which == 0 || which == 1), M355_EUNSUPPORTED,
               "conv3d_pack: only the 3x3x3 / stride 1 / pad 1 kernels have packed weights");
  launch_pack_weights(r, d, which == 1, w, packed, (hipStream_t)stream);
  return check_launch("conv3d_pack");
}

extern "C" int m355_conv3d_pack_batch(const m355_pack_item* items, int32_t n, void* stream) {
  M355_REQUIRE(items || n == 0, M355_EINVALID_ARG, "conv3d_pack_batch: null items");
  hipStream_t st = (hipStream_t)stream;
  PackBatch b;
  X3PackBatch b3;
  int nb = 0, nb3 = 0;
  for (int i = 0; i < n; ++i) {
    const m355_pack_item& it = items[i];
    const m355_conv3d_desc* d = &it.desc;
    if (int rc = validate_conv(d, "conv3d_pack_batch")) return rc;
    M355_REQUIRE(it.w && it.packed && ((uintptr_t)it.packed & 15) == 0, M355_EINVALID_ARG,
                 "conv3d_pack_batch: item %d: null / unaligned pointer", i);
    const ConvRoute r = query_conv(d, it.which);
    const FwdPlan& p = r.plan;
    M355_REQUIRE(r.kind != ConvKind::Direct && (it.which == 0 || it.which == 1), M355_EUNSUPPORTED,
                 "conv3d_pack_batch: item %d: only the 3x3x3 / stride 1 / pad 1 kernels have packed weights", i);
    if (is_smallcout(r.kind)) {
      launch_pack_weights(r, d, false, it.w, it.packed, st);   // (the Cout <= 4 forward layouts: one per model, launched on its own)
      continue;
    }
    if (r.kind == ConvKind::X3) {   // split + fragment-ordered weights: a batch of their own
      X3PackEntry& e = b3.e[nb3++];
      e.w = it.w; e.wq = it.packed;
      e.Cout = d->Cout; e.Cin = d->Cin;
      e.nchunks = p.nchunks; e.otiles = p.otiles; e.tile16 = p.tile16;
      e.transpose = it.which == 1;
      if (nb3 == PACK_BATCH) {
        launch_pack_x3_batch(b3, nb3, st);
        nb3 = 0;
      }
      continue;
    }
    const int kind = !is_h16(r.kind) ? 0 : (d->compute == M355_COMPUTE_BF16 ? 1 : 2);
    if (nb && (kind == 0) != (b.e[0].kind == 0)) {   // a launch holds fp32 entries or 16-bit entries, not both
      launch_pack_batch(b, nb, st);
      nb = 0;
    }
    PackEntry& e = b.e[nb++];
    e.w = it.w; e.wp = it.packed;
    e.counter = (int*)((char*)it.packed + p.wp_bytes - 256);
    e.Cout = d->Cout; e.Cin = d->Cin;
    e.kdim = kind == 0 ? p.kin_pad : p.nchunks;
    e.mout_pad = p.mout_pad;
    e.transpose = it.which == 1; e.kind = kind;
    if (nb == PACK_BATCH) {
      launch_pack_batch(b, nb, st);
      nb = 0;
    }
  }
  if (nb) launch_pack_batch(b, nb, st);
  if (nb3) launch_pack_x3_batch(b3, nb3, st);
  return check_launch("conv3d_pack_batch");
}

// ---- 16-bit operand modes with c8 tensors handed over by the caller (h16.hpp) ----
extern "C" size_t m355_act16_bytes(int32_t N, int32_t C, int64_t S) {
  if (N <= 0 || C <= 0 || S <= 0) return 0;
  return (size_t)N * (size_t)c8_blocks(C) * (size_t)S * 16;
}

static int validate_act16(const char* who, const void* a, const void* b, int N, int C, int64_t S, int compute) {
  M355_REQUIRE(a && b, M355_EINVALID_ARG, "%s: null pointer", who);
  M355_REQUIRE(N > 0 && C > 0 && S > 0 && N <= 65535 && c8_blocks(C) <= 65535, M355_EINVALID_ARG, "%s: bad shape", who);
  M355_REQUIRE(compute == M355_COMPUTE_BF16 || compute == M355_COMPUTE_F16, M355_EINVALID_ARG,
               "%s: compute must be M355_COMPUTE_BF16 or M355_COMPUTE_F16", who);
  return M355_OK;
}

extern "C" int m355_act16_pack(const float* x, void* x16, int32_t N, int32_t C, int64_t S, int64_t x_batch_stride,
                               int64_t x16_batch_stride, int32_t compute, void* stream) {
  if (int rc = validate_act16("act16_pack", x, x16, N, C, S, compute)) return rc;
  M355_REQUIRE(((uintptr_t)x16 & 15) == 0 && x16_batch_stride % 8 == 0, M355_EINVALID_ARG, "act16_pack: c8 tensor not 16B aligned");
  return launch_pack_act16(x, x16, N, C, S, dense_or(x_batch_stride, (int64_t)C * S),
                           dense_or(x16_batch_stride, c8_blocks(C) * S * 8), compute, (hipStream_t)stream);
}

extern "C" int m355_act16_unpack(const void* x16, float* x, int32_t N, int32_t C, int64_t S, int64_t x16_batch_stride,
                                 int64_t x_batch_stride, int32_t compute, void* stream) {
  if (int rc = validate_act16("act16_unpack", x16, x, N, C, S, compute)) return rc;
  M355_REQUIRE(((uintptr_t)x16 & 15) == 0 && x16_batch_stride % 8 == 0, M355_EINVALID_ARG, "act16_unpack: c8 tensor not 16B aligned");
  return launch_unpack_act16(x16, x, N, C, S, dense_or(x16_batch_stride, c8_blocks(C) * S * 8),
                             dense_or(x_batch_stride, (int64_t)C * S), compute, (hipStream_t)stream);
}

// forward from a c8 x: fp32 y with optional residual / softmax, or (_c8) a c8 y
extern "C" int m355_conv3d_fwd_h16(const m355_conv3d_desc* d, const void* x16, int64_t x16_batch_stride, const float* w,
                                   const float* bias, const float* add, float* y, float* stat_partials, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  return run_conv({CE_FWD_H16, P(x16), P(w), P(bias), P(add), P(y), P(stat_partials), P(workspace), workspace_bytes,
                   {x16_batch_stride, 0}}, d, stream);
}

extern "C" int m355_conv3d_fwd_h16_c8(const m355_conv3d_desc* d, const void* x16, int64_t x16_batch_stride,
                                      const float* w, const float* bias, void* y16, int64_t y16_batch_stride,
                                      float* stat_partials, void* workspace, size_t workspace_bytes, void* stream) {
  return run_conv({CE_FWD_H16_C8, P(x16), P(w), P(bias), 0, P(y16), P(stat_partials), P(workspace), workspace_bytes,
                   {x16_batch_stride, y16_batch_stride}}, d, stream);
}

// data gradient from a c8 dy: fp32 dx, or (_c8, the c8-only training flow) a c8 dx whose fp16 stores report overflow
extern "C" int m355_conv3d_bwd_data_h16(const m355_conv3d_desc* d, const void* dy16, int64_t dy16_batch_stride,
                                        const float* w, float* dx, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  return run_conv({CE_BWD_DATA_H16, P(dy16), P(w), 0, 0, P(dx), 0, P(workspace), workspace_bytes, {dy16_batch_stride, 0}}, d,
                  stream);
}

extern "C" int m355_conv3d_bwd_data_h16_c8(const m355_conv3d_desc* d, const void* dy16, int64_t dy16_batch_stride,
                                           const float* w, void* dx16, int64_t dx16_batch_stride, void* workspace,
                                           size_t workspace_bytes, void* stream) {
  return run_conv({CE_BWD_DATA_H16_C8, P(dy16), P(w), 0, 0, P(dx16), 0, P(workspace), workspace_bytes,
                   {dy16_batch_stride, dx16_batch_stride}}, d, stream);
}

// ---- weight gradients: from fp32 NCDHW operands, and with both operands in c8 (the 16-bit training flow keeps the packed
// conv input of the forward pass and packs dy once for the data and the weight gradient): m355_conv3d_bwd_weight_h16 (bias
// gradient from the fp32 dy) and m355_conv3d_bwd_weight_c8 (the c8-only training flow: edge-layer kernel, bias gradient
// reduced from the c8 dy, the loss scale of the fp16 mode removed in the fp32 epilogue by grad_unscale) ----
static int run_bww(const ConvArgs& a, const m355_conv3d_desc* d, float grad_unscale, void* stream) {
  BwwRoute r;
  if (int rc = check_bww(a, d, &r)) return rc;
  const BwwCall c = {d, (const void*)a.in, (const void*)a.w, (const float*)(a.entry == CE_BWD_WEIGHT ? a.w : a.bias),
                     (float*)a.out, (float*)a.stat, grad_unscale, (void*)a.ws, (hipStream_t)stream};
  return launch_bww(r, c);
}

extern "C" int m355_conv3d_bwd_weight(const m355_conv3d_desc* d, const float* x, const float* dy, float* dw, float* dbias,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  return run_bww({CE_BWD_WEIGHT, P(x), P(dy), 0, 0, P(dw), P(dbias), P(workspace), workspace_bytes, {0, 0}}, d, 1.f, stream);
}

extern "C" int m355_conv3d_bwd_weight_h16(const m355_conv3d_desc* d, const void* x16, int64_t x16_batch_stride,
                                          const void* dy16, int64_t dy16_batch_stride, const float* dy, float* dw,
                                          float* dbias, void* workspace, size_t workspace_bytes, void* stream) {
  return run_bww({CE_BWD_WEIGHT_H16, P(x16), P(dy16), P(dy), 0, P(dw), P(dbias), P(workspace), workspace_bytes,
                  {x16_batch_stride, dy16_batch_stride}}, d, 1.f, stream);
}

extern "C" int m355_conv3d_bwd_weight_c8(const m355_conv3d_desc* d, const void* x16, int64_t x16_batch_stride,
                                         const void* dy16, int64_t dy16_batch_stride, float* dw, float* dbias,
                                         float grad_unscale, void* workspace, size_t workspace_bytes, void* stream) {
  return run_bww({CE_BWD_WEIGHT_C8, P(x16), P(dy16), 0, 0, P(dw), P(dbias), P(workspace), workspace_bytes,
                  {x16_batch_stride, dy16_batch_stride}}, d, grad_unscale, stream);
}

// ---- what a call would launch: the entry point's checks and its route, nothing started, no pointer followed ----
extern "C" int m355_conv3d_launch_plan(int32_t entry, const m355_conv3d_desc* d, const int64_t* batch_strides,
                                       const uint64_t* pointers, size_t workspace_bytes, int64_t* out12) {
  M355_REQUIRE(entry >= 0 && entry < CE_COUNT && batch_strides && pointers && out12, M355_EINVALID_ARG,
               "conv3d_launch_plan: bad entry point index / null pointer");
  const ConvArgs a = {entry, (uintptr_t)pointers[0], (uintptr_t)pointers[1], (uintptr_t)pointers[2], (uintptr_t)pointers[3],
                      (uintptr_t)pointers[4], (uintptr_t)pointers[5], (uintptr_t)pointers[6], workspace_bytes,
                      {batch_strides[0], batch_strides[1]}};
  if (entry == CE_BWD_WEIGHT || entry == CE_BWD_WEIGHT_H16 || entry == CE_BWD_WEIGHT_C8) {
    BwwRoute r;
    if (int rc = check_bww(a, d, &r)) return rc;
    const int64_t o[12] = {(int64_t)r.kind, r.grid.x, r.grid.y, r.grid.z, r.block, 0, 0, r.aux, (int64_t)r.need, r.reduce_grid.x,
                           (int64_t)r.dbias_off, (int64_t)r.x16_off};
    std::copy_n(o, 12, out12);
  } else {
    ConvRoute r;
    if (int rc = check_conv(a, d, &r)) return rc;
    const int64_t o[12] = {(int64_t)r.kind, r.grid.x, r.grid.y, r.grid.z, r.block, r.grid16.x, r.grid16.z, r.aux, (int64_t)r.need,
                           r.reduce_grid.x, (int64_t)r.slab_off, (int64_t)r.stage_off};
    std::copy_n(o, 12, out12);
  }
  return M355_OK;
}
