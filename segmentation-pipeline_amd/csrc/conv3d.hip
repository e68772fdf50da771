// conv3d kernels for gfx950 and their launcher (the host layer that resolves a descriptor to one of them, plans it and
// carries the C ABI is conv3d_host.hip): fp32 implicit-GEMM on v_mfma_f32_32x32x2_f32 (exact fp32,
// k-ordered fma chain) for the 3x3x3 / stride 1 / pad 1 convolutions that carry
// ~97 % of the U-Net FLOPs, plus generic direct kernels for any other
// kernel-size / stride / padding (the reference's BlurConv3d, k=4 s=2, reaches the
// 3x3x3 kernels through a space-to-depth rearrangement, models/components.py).
//
// Reference ops replaced: nn.Conv3d in Block3d (models/components.py:36,42,51),
// out conv (models/modular_unet.py:83,99), F.conv3d in BlurConv3d
// (components.py:119); autograd of those for bwd-data / bwd-weight.
//
// GEMM view of the 3x3x3 forward:  Y[o, v] = sum_k Wp[k, o] * X[k, v]
//   M = Cout (A operand = packed weights), N = voxels (B operand = input read
//   from an LDS halo tile with compile-time tap offsets), K = 27 * Cin.
// The MFMA's k-pair (lanes 0-31 / 32-63) is (channel c, channel c+1) at the same
// tap, so both halves use one immediate offset.
#include "conv3d_common.hpp"

namespace m355 {

// ---------------------------------------------------------------- weight pack
// fwd:      wp[(c*27 + tap)*cout_pad + o]          = w[(o*Cin + c)*27 + tap]
// bwd-data: wp[(o*27 + (26-tap))*cin_pad32 + c]    = w[(o*Cin + c)*27 + tap]
//           (the data-gradient is a conv of dy with the flipped, transposed filter)
// Padded rows/cols are zero-filled.
__global__ void pack_w3_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cout,
                               int Cin, int kin_pad, int mout_pad, int transpose, int* __restrict__ counter) {
  // logical conv being run: K-channels = kin (padded to kin_pad), M-channels = mout_pad
  if (counter && blockIdx.x == 0 && threadIdx.x < 16) counter[threadIdx.x] = 0;  // work queues of the persistent conv kernel
  pack_w3_body(w, wp, Cout, Cin, kin_pad, mout_pad, transpose, blockIdx.x, gridDim.x);
}

// ------------------------------------------------------------ MFMA fwd kernel
// One output tile per workgroup (used when a launch has no more tiles than resident workgroups;
// otherwise conv3_mfma_fwd_p_kernel below).  Two workgroups per CU up to NTW = 4, one for NTW = 8,
// i.e. one or two waves per SIMD: the next chunk's input halo tile and weights travel
// global -> registers -> the other LDS buffer while the current chunk is multiplied, with the
// prefetch instructions interleaved into the MFMA stream; one barrier per chunk (~14k MFMA cycles).
template <int NTW, int GX>
__global__ __launch_bounds__(256, 1) void conv3_mfma_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ bias,
    const float* __restrict__ add, float* __restrict__ y, float* __restrict__ slab, int Cin,
    int Cout, int D, int H, int W, int cout_pad, int ty_tiles, int tx_tiles, int nchunks,
    int ksplit, int64_t xbs, int64_t ybs, int64_t slab_stride, float* __restrict__ stat, int otiles, int order) {
  using T = FwdTile<NTW, GX>;
  constexpr int GY = T::GY, TZ = T::TZ, TY = T::TY, TX = T::TX, RS = T::RS, PS = T::PS,
                CS = T::CS, CC = T::CC;
  constexpr int XE = CC * CS;                 // floats of one staged input chunk
  constexpr int XPER = (XE + 255) / 256;      // per-thread elements
  constexpr int WE4 = CC * 27 * 8;            // float4s of one staged weight chunk
  constexpr int WPER = (WE4 + 255) / 256;
  __shared__ float xs[2][XE];
  __shared__ __attribute__((aligned(16))) float ws[2][CC * 27 * 32];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int l32 = lane & 31;
  const int ly = l32 / GX, lx = l32 % GX;

  // XCD-aware placement (speed only, a bijection of the grid's x range): workgroups are dealt to the 8 XCDs round-robin
  // in launch order (x fastest); when the workgroup count along x is a multiple of 8 every XCD gets a contiguous run
  // of tiles, whose shared halos then hit in its L2.  The channel tile is the FASTEST index of x: the workgroups that
  // need the same input tile for different output channels run side by side on one XCD (the channel tile as the
  // outer index made every pass over the channel tiles re-read the whole input from HBM).
  int bt = blockIdx.x;
  if ((gridDim.x & 7) == 0) bt = (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);
  const int sp_count = (int)gridDim.x / otiles;
  const int otile = (order & 2) ? bt % otiles : bt / sp_count;
  bt = (order & 2) ? bt / otiles : bt % sp_count;
  const int sp_index = bt;   // spatial tile (statistics slot)
  const int txt = bt % tx_tiles;
  bt /= tx_tiles;
  const int tyt = bt % ty_tiles;
  const int tzt = bt / ty_tiles;
  const int z0 = tzt * TZ, y0 = tyt * TY, x0 = txt * TX;
  const int o0 = otile * 32;
  const int n = blockIdx.z / ksplit;
  const int ks = blockIdx.z % ksplit;

  const int cps = (nchunks + ksplit - 1) / ksplit;
  const int ch_begin = ks * cps;
  const int ch_end = min(nchunks, ch_begin + cps);

  const float* xn = x + (int64_t)n * xbs;
  const int64_t HW = (int64_t)H * W;
  const int DHW = (int)(HW * D);

  // chunk-invariant gather offsets of this thread's elements, in bytes; zero padding and elements
  // past the tile get an offset no buffer descriptor covers, so the hardware returns 0 for them
  constexpr unsigned OOB = 0x80000000u;
  unsigned goff[XPER];
#pragma unroll
  for (int i = 0; i < XPER; ++i) {
    const int e = tid + 256 * i;
    unsigned off = OOB;
    if (e < XE) {
      const int c = e / CS, r = e - c * CS;
      const int zz = r / PS, r2 = r - zz * PS;
      const int yy = r2 / RS, xx = r2 - yy * RS;
      const int gz = z0 + zz - 1, gy = y0 + yy - 1, gx = x0 + xx - 1;
      if (gz >= 0 && gz < D && gy >= 0 && gy < H && gx >= 0 && gx < W)
        off = (unsigned)(c * DHW + gz * (int)HW + gy * W + gx) * 4u;
    }
    goff[i] = off;
  }

  f32x16 acc[NTW];
#pragma unroll
  for (int g = 0; g < NTW; ++g)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[g][r] = 0.f;

  // Prefetch of the next chunk into registers.  x comes through a raw buffer descriptor that
  // covers exactly the channels of the chunk that exist (base at channel c0, num_records =
  // min(CC, Cin - c0) channels): padding, tile overhang and channels past Cin are out of range and
  // read as 0, so there are no validity masks, no branches, and the commit is plain LDS writes.
  // The prefetch is cut into per-step items issued inside the MFMA loop (see below).
  float xr[XPER];
  f32x4 wr[WPER];
  __amdgpu_buffer_rsrc_t rx;
  const float* wsrc = wp;
  auto chunk_setup = [&](int ch, bool live) {  // !live: zero-sized descriptor, every load returns 0
    const int c0 = ch * CC;
    rx = __builtin_amdgcn_make_buffer_rsrc((void*)(xn + (int64_t)c0 * DHW), 0,
                                           live ? min(CC, Cin - c0) * DHW * 4 : 0, 0x00020000);
    wsrc = wp + (int64_t)c0 * 27 * cout_pad + o0;
  };
  auto fetch_item = [&](int s) {  // s is a compile-time constant wherever this is called
    if (s < XPER) xr[s] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, goff[s], 0, 0));
    if (s < WPER) {
      const int idx = tid + 256 * s;
      const int idc = idx < WE4 ? idx : WE4 - 1;  // clamp: keeps the array fully scalarised
      wr[s] = *reinterpret_cast<const f32x4*>(wsrc + (int64_t)(idc >> 3) * cout_pad + (idc & 7) * 4);
    }
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int i = 0; i < XPER; ++i)
      if (tid + 256 * i < XE) xs[buf][tid + 256 * i] = xr[i];
#pragma unroll
    for (int j = 0; j < WPER; ++j)
      if (tid + 256 * j < WE4) *reinterpret_cast<f32x4*>(&ws[buf][(tid + 256 * j) * 4]) = wr[j];
  };
  constexpr int NSTEP = (CC / 2) * 27;
  static_assert(XPER <= NSTEP && WPER <= NSTEP, "one prefetch item per MFMA step");

  if (ch_begin < ch_end) {
    chunk_setup(ch_begin, true);
#pragma unroll
    for (int s = 0; s < NSTEP; ++s) fetch_item(s);
    commit(0);
  }
  __syncthreads();

  for (int ch = ch_begin; ch < ch_end; ++ch) {
    const int cur = (ch - ch_begin) & 1;
    const bool more = ch + 1 < ch_end;
    chunk_setup(more ? ch + 1 : ch, more);  // unconditional, so the loop body has no branch
    const float* xb = xs[cur] + half * CS + wave * PS + ly * RS + lx;
    const float* wb = ws[cur] + half * (27 * 32) + l32;
    // ---- MFMA over K = CC * 27, software-pipelined over the (channel pair, tap) steps: the LDS
    // reads of step s+1 and one item of the next chunk's prefetch are issued before the MFMAs of
    // step s.  The sched_barriers pin that order; left alone, hipcc sinks LDS reads to just before
    // their MFMA (waiting lgkmcnt(0) on them) and hoists the whole prefetch in front of the loop,
    // which with one wave per SIMD leaves the matrix core idle meanwhile.
    float av[2], bv[2][NTW];
    auto lds_step = [&](int s, int slot) {  // s is a compile-time constant after unrolling
      const int cp = s / 27, tap = s % 27;
      const int dz = tap / 9, dy = (tap / 3) % 3, dx = tap % 3;
      av[slot] = wb[(2 * cp * 27 + tap) * 32];
#pragma unroll
      for (int g = 0; g < NTW; ++g) bv[slot][g] = xb[2 * cp * CS + dz * PS + (g * GY + dy) * RS + dx];
    };
    lds_step(0, 0);
#pragma unroll
    for (int s = 0; s < NSTEP; ++s) {
      if (s + 1 < NSTEP) lds_step(s + 1, (s + 1) & 1);
      fetch_item(s);
#pragma unroll
      for (int g = 0; g < NTW; ++g)
        acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s & 1], bv[s & 1][g], acc[g], 0, 0, 0);
      // issue order inside the step: each MFMA is followed by up to two of the LDS reads of step
      // s+1, then the prefetch loads -- they go out while the matrix core is busy
#pragma unroll
      for (int g = 0; g < NTW; ++g) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // DS read
      }
      __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);    // VMEM read
      __builtin_amdgcn_sched_barrier(0);
    }
    if (more) commit(cur ^ 1);
    __syncthreads();
  }

  // ---- epilogue ----
  const int z = z0 + wave;
  const int xg = x0 + lx;
  const bool lane_ok = z < D && xg < W;
  if (ksplit == 1) {
    // statistics slot of this wave: stat[n][spatial tile * 4 + wave][Cout][2]
    float* st = stat ? stat + (((int64_t)n * sp_count + sp_index) * 4 + wave) * Cout * 2 : nullptr;
    store_conv_tile<NTW, GY>(acc, y + (int64_t)n * ybs, add ? add + (int64_t)n * ybs : nullptr, bias, o0, Cout, z,
                             y0, xg, ly, half, D, H, W, lane_ok, st);
  } else {
    store_conv_tile<NTW, GY>(acc, slab + (int64_t)ks * slab_stride + (int64_t)n * Cout * D * HW, nullptr, nullptr,
                             o0, Cout, z, y0, xg, ly, half, D, H, W, lane_ok, nullptr);
  }
}

// ---- persistent variant of conv3_mfma_fwd_kernel ----
// A workgroup of the kernel above lives for nchunks/ksplit chunks and pays ~2.5 chunks of fixed
// cost around them (measured: 8-chunk layers reach 112 TFLOP/s, 48-chunk layers 140): the first
// chunk's load latency + commit, the output stores, the launch of the next workgroup.  Here the grid
// is one residency (2 workgroups per CU) and every workgroup takes items from a queue (item = output
// tile x 32-channel tile x sample x split, same order as the grid above; XCD-aware, see "work queue"
// below), so a workgroup that starts late -- another kernel, e.g. an RCCL collective, still holding
// its CU -- simply takes fewer items; every item's result is independent of who computes it, so
// this stays bit-reproducible.  The
// (item, chunk) sequence is flattened: during the last chunk of an item the FIRST chunk of the next
// item is prefetched, so the MFMA stream only stops for the output stores.
// M16: the 16-row remainder tile (see store_conv_tile16): the items are the spatial tiles x ONE 16-channel tile at
// o_base; one MFMA 16x16x4 per (tap, 16-voxel half group) covers the chunk's 4 channels, 27 steps per chunk.
// The LDS channel stride is padded to == 16 (mod 32) so the four channels of a B fragment (lane >> 4) and the two
// voxel halves fall on distinct banks; the weights of odd channels are read from the upper 16 columns of their
// LDS row (both halves of a row are staged with the same 16 output channels).
template <int NTW, int GX, bool M16 = false>
__global__ __launch_bounds__(256, (NTW <= 4 ? 2 : 1)) void conv3_mfma_fwd_p_kernel(
    const float* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ bias,
    const float* __restrict__ add, float* __restrict__ y, float* __restrict__ slab, int Cin,
    int Cout, int D, int H, int W, int cout_pad, int tz_tiles, int ty_tiles, int tx_tiles, int otiles,
    int nchunks, int ksplit, int nbatch, int64_t xbs, int64_t ybs, int64_t slab_stride,
    float* __restrict__ stat, int* __restrict__ work_counter, int o_base, int order) {
  using T = FwdTile<NTW, GX>;
  constexpr int GY = T::GY, TZ = T::TZ, TY = T::TY, TX = T::TX, RS = T::RS, PS = T::PS,
                CS0 = T::CS, CC = T::CC;
  constexpr int CS = M16 ? ((CS0 + 31) / 32) * 32 + 16 : CS0;   // LDS channel stride (elements past CS0: padding)
  constexpr int XE = CC * CS;
  constexpr int XPER = (XE + 255) / 256;
  constexpr int WE4 = CC * 27 * 8;
  constexpr int WPER = (WE4 + 255) / 256;
  constexpr int NSTEP = M16 ? 27 : (CC / 2) * 27;
  static_assert(XPER <= NSTEP && WPER <= NSTEP, "one prefetch item per MFMA step");
  __shared__ float xs[2][XE];
  __shared__ __attribute__((aligned(16))) float ws[2][CC * 27 * 32];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int l32 = lane & 31;
  const int ly = l32 / GX, lx = l32 % GX;
  const int64_t HW = (int64_t)H * W;
  const int DHW = (int)(HW * D);
  const int iHW = (int)HW;

  const int sp_tiles = tz_tiles * ty_tiles * tx_tiles;
  const int total = sp_tiles * otiles * nbatch * ksplit;
  const int cps = (nchunks + ksplit - 1) / ksplit;

  struct Item {
    int z0, y0, x0, o0, n, ks, ch_begin, ch_end, sp;
  };
  // Tile order inside a region: the ~64 items in flight on one XCD should form a CUBE of tiles (all x, 4 y, 4 z), not
  // a slab one tile thick: with the linear (x, y, z) order every tile's two z-halo planes (a third of its input) are
  // re-read from HBM when the next slab comes around (PMC: 1.6x the algorithmic bytes); in the blocked order they
  // are shared with a z neighbour that is in flight at the same time.  A bijection of the item range: results unchanged.
  const bool cube = (ty_tiles & 3) == 0 && (tz_tiles & 3) == 0 && (order & 1);
  auto decode = [&](int it) {
    Item q;
    // channel tile fastest (the items that share an input tile are adjacent: same XCD, same time), then the spatial tile
    const int ot = (order & 2) ? it % otiles : (it / sp_tiles) % otiles;
    int sp = (order & 2) ? (it / otiles) % sp_tiles : it % sp_tiles, r = it / (otiles * sp_tiles);
    const int txt = sp % tx_tiles;
    sp /= tx_tiles;
    int tyt, tzt;
    if (cube) {   // sp = ((tz_hi * (ty_tiles / 4) + ty_hi) * 4 + tz_lo) * 4 + ty_lo
      const int ty_lo = sp & 3, tz_lo = (sp >> 2) & 3, hi = sp >> 4;
      const int tyh = ty_tiles >> 2;
      tyt = (hi % tyh) * 4 + ty_lo;
      tzt = (hi / tyh) * 4 + tz_lo;
    } else {
      tyt = sp % ty_tiles;
      tzt = sp / ty_tiles;
    }
    q.sp = (tzt * ty_tiles + tyt) * tx_tiles + txt;   // canonical tile index (statistics slot)
    q.x0 = txt * TX;
    q.y0 = tyt * TY;
    q.z0 = tzt * TZ;
    q.o0 = o_base + ot * 32;
    q.ks = r % ksplit;
    q.n = r / ksplit;
    q.ch_begin = q.ks * cps;
    q.ch_end = min(nchunks, q.ch_begin + cps);
    return q;
  };

  // gather offsets of this thread's halo elements for item q, in bytes from the chunk's first channel;
  // zero padding and elements past the tile get an offset no descriptor covers (hardware returns 0).
  // Recomputed per item from the element index (divisions by compile-time constants) rather than
  // kept as per-thread tables: 40 registers this kernel does not have.
  constexpr unsigned OOB = 0x80000000u;
  unsigned goff[XPER];
  auto compute_goff = [&](const Item& q) {
#pragma unroll
    for (int i = 0; i < XPER; ++i) {
      const int e = tid + 256 * i;
      const int c = e / CS, r = e - c * CS;
      const int zz = r / PS, r2 = r - zz * PS;
      const int yy = r2 / RS, xx = r2 - yy * RS;
      const int gz = q.z0 + zz - 1, gy = q.y0 + yy - 1, gx = q.x0 + xx - 1;
      const bool ok = e < XE && r < CS0 && (unsigned)gz < (unsigned)D && (unsigned)gy < (unsigned)H &&
                      (unsigned)gx < (unsigned)W;
      goff[i] = ok ? (unsigned)(c * DHW + gz * iHW + gy * W + gx) * 4u : OOB;
    }
  };

  float xr[XPER];
  f32x4 wr[WPER];
  __amdgpu_buffer_rsrc_t rx;
  const float* wsrc = wp;
  auto chunk_setup = [&](const Item& q, int ch, bool live) {  // !live: zero-sized descriptor
    const int c0 = ch * CC;
    rx = __builtin_amdgcn_make_buffer_rsrc((void*)(x + (int64_t)q.n * xbs + (int64_t)c0 * DHW), 0,
                                           live ? min(CC, Cin - c0) * DHW * 4 : 0, 0x00020000);
    wsrc = wp + (int64_t)c0 * 27 * cout_pad + q.o0;
  };
  auto fetch_item = [&](int s) {
    if (s < XPER) xr[s] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, goff[s], 0, 0));
    if (s < WPER) {
      const int idx = tid + 256 * s;
      const int idc = idx < WE4 ? idx : WE4 - 1;
      wr[s] = *reinterpret_cast<const f32x4*>(wsrc + (int64_t)(idc >> 3) * cout_pad + (idc & (M16 ? 3 : 7)) * 4);
    }
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int i = 0; i < XPER; ++i)
      if (tid + 256 * i < XE) xs[buf][tid + 256 * i] = xr[i];
#pragma unroll
    for (int j = 0; j < WPER; ++j)
      if (tid + 256 * j < WE4) *reinterpret_cast<f32x4*>(&ws[buf][(tid + 256 * j) * 4]) = wr[j];
  };

  // ---- work queue.  The items are dealt in eight contiguous regions, one per XCD label
  // (blockIdx % 8: blocks b and b + 8 are observed to share an XCD and therefore an L2), so the
  // tiles in flight on one L2 are neighbours and their shared input halos hit in it.  A workgroup
  // takes its region's items in order from an atomic counter (its first item is static) and steals
  // from the other regions once its own is empty.  Only thread 0 talks to the counters.
  __shared__ int next_item_s;
  const int G = (int)gridDim.x;
  const int xl = blockIdx.x & 7;
  const int cpx = (total + 7) >> 3;  // items per region
  auto region_size = [&](int r) { return max(0, min(cpx, total - r * cpx)); };
  auto region_static = [&](int r) { return min(region_size(r), (G - r + 7) >> 3); };  // workgroups starting there
  auto steal = [&]() {  // thread 0; `total` = nothing left anywhere
    // One 32-byte read of all eight ticket counters first: when every region is drained (what every
    // workgroup finds once, at the end of its life) that is one memory round trip instead of seven
    // dependent atomics (~15-40k cycles, a quarter of the lifetime of a short 16-bit launch).
    int seen[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) seen[r] = __hip_atomic_load(work_counter + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int a = 1; a < 8; ++a) {
      const int r = (xl + a) & 7;
      if (region_static(r) + seen[r] >= region_size(r)) continue;  // nothing dynamic left there (counters only grow)
      const int k = region_static(r) + atomicAdd(work_counter + r, 1);
      if (k < region_size(r)) return r * cpx + k;
    }
    return total;
  };
  auto resolve = [&](int taken) {  // thread 0: `taken` = this workgroup's ticket in its own region
    const int k = region_static(xl) + taken;
    return k < region_size(xl) ? xl * cpx + k : steal();
  };
  int it = xl * cpx + (int)(blockIdx.x >> 3);
  if ((int)(blockIdx.x >> 3) >= region_size(xl)) {  // more workgroups than items in this region (uniform)
    if (tid == 0) next_item_s = steal();
    __syncthreads();
    it = next_item_s;
    __syncthreads();
    if (it >= total) {
      queue_leave(work_counter);
      return;
    }
  }
  Item cur = decode(it);
  compute_goff(cur);
  chunk_setup(cur, cur.ch_begin, true);
#pragma unroll
  for (int s = 0; s < NSTEP; ++s) fetch_item(s);
  commit(0);
  __syncthreads();
  int buf = 0;

  f32x16 acc[M16 ? 1 : NTW];
  f32x4v acc16[M16 ? NTW : 1][2];
  while (true) {
    // thread 0 takes a ticket for this workgroup's next item now; the item is published through
    // LDS after the first chunk (a barrier later) and consumed at the start of the last chunk
    int pending = 0;
    if (tid == 0) pending = atomicAdd(work_counter + xl, 1);
    if (cur.ch_end - cur.ch_begin == 1) {  // single-chunk items: no chunk to hide the round trip behind
      if (tid == 0) next_item_s = resolve(pending);
      __syncthreads();
    }
    if constexpr (M16) {
#pragma unroll
      for (int g = 0; g < NTW; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc16[g][0][r] = acc16[g][1][r] = 0.f;
    } else {
#pragma unroll
      for (int g = 0; g < NTW; ++g)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[g][r] = 0.f;
    }
    Item nxt = cur;
    int nit = total;
    for (int ch = cur.ch_begin; ch < cur.ch_end; ++ch) {
      if (ch + 1 < cur.ch_end) {
        chunk_setup(cur, ch + 1, true);
      } else {  // last chunk of this item: prefetch the first chunk of the next one
        nit = next_item_s;
        const bool live = nit < total;
        nxt = decode(live ? nit : it);
        compute_goff(nxt);
        chunk_setup(nxt, nxt.ch_begin, live);
      }
      if constexpr (M16) {
        const int kq = lane >> 4, l16 = lane & 15;                       // channel of the chunk, voxel / output row
        const float* wb = ws[buf] + kq * (27 * 32) + l16 + 16 * (kq & 1);
        const float* xb0 = xs[buf] + kq * CS + wave * PS + (l16 / GX) * RS + l16 % GX;                  // x-half 0
        const float* xb1 = xs[buf] + kq * CS + wave * PS + ((16 + l16) / GX) * RS + (16 + l16) % GX;    // x-half 1
        float av[2], bv[2][NTW][2];
        auto lds_step = [&](int s, int slot) {  // s = tap
          const int dz = s / 9, dy = (s / 3) % 3, dx = s % 3;
          av[slot] = wb[s * 32];
#pragma unroll
          for (int g = 0; g < NTW; ++g) {
            bv[slot][g][0] = xb0[dz * PS + (g * GY + dy) * RS + dx];
            bv[slot][g][1] = xb1[dz * PS + (g * GY + dy) * RS + dx];
          }
        };
        lds_step(0, 0);
#pragma unroll
        for (int s = 0; s < NSTEP; ++s) {
          if (s + 1 < NSTEP) lds_step(s + 1, (s + 1) & 1);
          fetch_item(s);
#pragma unroll
          for (int g = 0; g < NTW; ++g)
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2)
              acc16[g][h2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s & 1], bv[s & 1][g][h2], acc16[g][h2], 0, 0, 0);
#pragma unroll
          for (int g = 0; g < 2 * NTW; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // DS read
          }
          __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);    // VMEM read
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
      const float* xb = xs[buf] + half * CS + wave * PS + ly * RS + lx;
      const float* wb = ws[buf] + half * (27 * 32) + l32;
      float av[2], bv[2][NTW];
      auto lds_step = [&](int s, int slot) {
        const int cp = s / 27, tap = s % 27;
        const int dz = tap / 9, dy = (tap / 3) % 3, dx = tap % 3;
        av[slot] = wb[(2 * cp * 27 + tap) * 32];
#pragma unroll
        for (int g = 0; g < NTW; ++g) bv[slot][g] = xb[2 * cp * CS + dz * PS + (g * GY + dy) * RS + dx];
      };
      lds_step(0, 0);
#pragma unroll
      for (int s = 0; s < NSTEP; ++s) {
        if (s + 1 < NSTEP) lds_step(s + 1, (s + 1) & 1);
        fetch_item(s);
#pragma unroll
        for (int g = 0; g < NTW; ++g)
          acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s & 1], bv[s & 1][g], acc[g], 0, 0, 0);
#pragma unroll
        for (int g = 0; g < NTW; ++g) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // DS read
        }
        __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);    // VMEM read
        __builtin_amdgcn_sched_barrier(0);
      }
      }
      if (ch == cur.ch_begin && cur.ch_end - cur.ch_begin > 1 && tid == 0) next_item_s = resolve(pending);
      commit(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }

    // ---- output tile of `cur` ----
    if constexpr (M16) {
      const int z = cur.z0 + wave;
      if (ksplit == 1) {
        float* st = stat ? stat + (((int64_t)cur.n * sp_tiles + cur.sp) * 4 + wave) * Cout * 2 : nullptr;
        store_conv_tile16<NTW, GX>(acc16, y + (int64_t)cur.n * ybs, add ? add + (int64_t)cur.n * ybs : nullptr, bias,
                                   cur.o0, Cout, z, cur.y0, cur.x0, lane, D, H, W, st);
      } else {
        store_conv_tile16<NTW, GX>(acc16, slab + (int64_t)cur.ks * slab_stride + (int64_t)cur.n * Cout * D * HW, nullptr,
                                   nullptr, cur.o0, Cout, z, cur.y0, cur.x0, lane, D, H, W, nullptr);
      }
    } else {
      const int z = cur.z0 + wave;
      const int xg = cur.x0 + lx;
      const bool lane_ok = z < D && xg < W;
      if (ksplit == 1) {
        float* st = stat ? stat + (((int64_t)cur.n * sp_tiles + cur.sp) * 4 + wave) * Cout * 2 : nullptr;
        store_conv_tile<NTW, GY>(acc, y + (int64_t)cur.n * ybs, add ? add + (int64_t)cur.n * ybs : nullptr, bias,
                                 cur.o0, Cout, z, cur.y0, xg, ly, half, D, H, W, lane_ok, st);
      } else {
        store_conv_tile<NTW, GY>(acc, slab + (int64_t)cur.ks * slab_stride + (int64_t)cur.n * Cout * D * HW, nullptr,
                                 nullptr, cur.o0, Cout, z, cur.y0, xg, ly, half, D, H, W, lane_ok, nullptr);
      }
    }
    if (nit >= total) break;
    it = nit;
    cur = nxt;
  }
  queue_leave(work_counter);
}

// A 32-row MFMA tile would carry only Cout useful rows.  z-Toeplitz packing fills the rows
// with (o, s), s = 0..7 being eight consecutive output planes of one (y, x) column:
//   y[o, z0+s, y, x] = sum_{c,dy,dx} sum_{u=0..9} Wz[(c,dy,dx,u), (o,s)] * x[c, z0-1+u, y+dy-1, x+dx-1]
//   Wz[(c,dy,dx,u), (o,s)] = w[o,c,u-s,dy,dx] if 0 <= u-s <= 2 else 0
// K grows by 10/3 but each MFMA column now yields 8 outputs: 2.4x fewer MFMAs than the padded tile.
// Tile = 8 z x 8 y x 32 x; wave w owns rows y = 2w, 2w+1; 2 input channels (one MFMA k-pair) per chunk.
constexpr int TZ_K = 90;  // (dy, dx, u) combinations
__global__ void pack_w3_toeplitz_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cout,
                                        int Cin, int kin_pad) {
  const int64_t total = (int64_t)kin_pad * TZ_K * 32;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int m = (int)(i & 31);
    int64_t r = i >> 5;
    const int t = (int)(r % TZ_K);
    const int c = (int)(r / TZ_K);
    const int u = t % 10, dyx = t / 10;  // dyx = dy*3 + dx
    const int o = m >> 3, sft = m & 7;
    const int dz = u - sft;
    float v = 0.f;
    if (c < Cin && o < Cout && dz >= 0 && dz <= 2) v = w[((int64_t)o * Cin + c) * 27 + dz * 9 + dyx];
    wp[i] = v;
  }
}

__global__ __launch_bounds__(256, 2) void conv3_mfma_fwd_smallcout_kernel(
    const float* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ bias,
    const float* __restrict__ add, float* __restrict__ y, int Cin, int Cout, int D, int H, int W,
    int ty_tiles, int tx_tiles, int nchunks, int64_t xbs, int64_t ybs) {
  constexpr int TZ = 8, TY = 8, TX = 32, RS = TX + 2, PS = (TY + 2) * RS, CS = (TZ + 2) * PS;
  constexpr int XE = 2 * CS, XPER = (XE + 255) / 256;   // 6800 floats
  constexpr int WE4 = 2 * TZ_K * 8, WPER = (WE4 + 255) / 256;
  __shared__ float xs[XE];
  __shared__ __attribute__((aligned(16))) float ws[2 * TZ_K * 32];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l32 = lane & 31;
  int bt = blockIdx.x;
  const int txt = bt % tx_tiles;
  bt /= tx_tiles;
  const int tyt = bt % ty_tiles;
  const int tzt = bt / ty_tiles;
  const int z0 = tzt * TZ, y0 = tyt * TY, x0 = txt * TX;
  const int n = blockIdx.y;
  const float* xn = x + (int64_t)n * xbs;
  const int iHW = H * W, iDHW = D * H * W;

  int goff[XPER];
#pragma unroll
  for (int i = 0; i < XPER; ++i) {
    const int e = tid + 256 * i;
    int off = -1;
    if (e < XE) {
      const int c = e / CS, r = e - c * CS;
      const int zz = r / PS, r2 = r - zz * PS;
      const int yy = r2 / RS, xx = r2 - yy * RS;
      const int gz = z0 + zz - 1, gy = y0 + yy - 1, gx = x0 + xx - 1;
      if (gz >= 0 && gz < D && gy >= 0 && gy < H && gx >= 0 && gx < W) off = c * iDHW + gz * iHW + gy * W + gx;
    }
    goff[i] = off;
  }
  f32x16 acc[2];
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[g][r] = 0.f;

  const float* xb = xs + half * CS + (wave * 2) * RS + l32;
  const float* wb = ws + half * (TZ_K * 32) + l32;
  for (int ch = 0; ch < nchunks; ++ch) {
    const int c0 = ch * 2;
    __syncthreads();
    {
      float xr[XPER];
      const float* xc = xn + (int64_t)c0 * iDHW;
      const bool full = c0 + 2 <= Cin;
#pragma unroll
      for (int i = 0; i < XPER; ++i) {
        bool ok = goff[i] >= 0;
        if (!full) ok = ok && (c0 + (tid + 256 * i) / CS < Cin);
        xr[i] = xc[ok ? goff[i] : 0];
      }
      f32x4 wr[WPER];
      const f32x4* wsrc = reinterpret_cast<const f32x4*>(wp + (int64_t)c0 * TZ_K * 32);
#pragma unroll
      for (int j = 0; j < WPER; ++j) wr[j] = wsrc[min(tid + 256 * j, WE4 - 1)];
#pragma unroll
      for (int i = 0; i < XPER; ++i) {
        bool ok = goff[i] >= 0;
        if (!full) ok = ok && (c0 + (tid + 256 * i) / CS < Cin);
        if (tid + 256 * i < XE) xs[tid + 256 * i] = ok ? xr[i] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < WPER; ++j)
        if (tid + 256 * j < WE4) reinterpret_cast<f32x4*>(ws)[tid + 256 * j] = wr[j];
    }
    __syncthreads();
#pragma unroll
    for (int dyx = 0; dyx < 9; ++dyx) {
      const int dy = dyx / 3, dx = dyx % 3;
#pragma unroll
      for (int u = 0; u < 10; ++u) {
        const float a = wb[(dyx * 10 + u) * 32];
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          const float b = xb[u * PS + (g + dy) * RS + dx];
          acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[g], 0, 0, 0);
        }
      }
    }
  }
  const int xg = x0 + l32;
  if (xg >= W) return;
  float* yn = y + (int64_t)n * ybs;
  const float* an = add ? add + (int64_t)n * ybs : nullptr;
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const int yg = y0 + wave * 2 + g;
    if (yg >= H) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = (r & 3) + 8 * (r >> 2) + 4 * half;  // row = o*8 + s
      const int o = m >> 3, zg = z0 + (m & 7);
      if (o < Cout && zg < D) {
        const int64_t idx = (int64_t)o * iDHW + (int64_t)zg * iHW + (int64_t)yg * W + xg;
        float v = acc[g][r];
        if (bias) v += bias[o];
        if (an) v += an[idx];
        yn[idx] = v;
      }
    }
  }
}

// ---- Cout <= 4 forward on the vector ALU ----
// With three output channels the MFMA formulations above still spend 4.4x the useful flops (row
// padding x z-Toeplitz inflation).  The packed fp32 FMA (v_pk_fma_f32: two FMAs per lane per issue)
// runs at the same peak rate as the fp32 MFMA and wastes only the 4th channel: each thread owns a run
// of 8 x-adjacent voxels and all (padded to 4) output channels -- 16 float2 accumulators; an input
// row segment of 10 floats is read from LDS once per (channel, dz, dy) and used for 3 taps x 8 voxels
// x 4 channels; the weights of a tap are one uniform 16-byte scalar load (SGPR operands of the FMA,
// the voxel value is broadcast with op_sel).  Tile = 4 z x 8 y x 64 x, 4 input channels per LDS chunk,
// the next chunk prefetched into registers through a buffer descriptor; two workgroups per CU.
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int VS_TZ = 4, VS_TY = 8, VS_TX = 64, VS_CC = 4;
constexpr int VS_RS = VS_TX + 4;                 // row: [left halo][64][right halo][2 pad] -> 16-byte aligned segments
constexpr int VS_PS = (VS_TY + 2) * VS_RS, VS_CS = (VS_TZ + 2) * VS_PS;
// wq[(c*27 + tap)*4 + o] = w[o][c][tap] (o >= Cout: 0)
__global__ void pack_w3_valu_kernel(const float* __restrict__ w, float* __restrict__ wq, int Cout, int Cin) {
  const int total = Cin * 27 * 4;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int o = i & 3, r = i >> 2;
    wq[i] = o < Cout ? w[((int64_t)o * Cin + r / 27) * 27 + r % 27] : 0.f;
  }
}

__global__ __launch_bounds__(256, 2) void conv3_valu_smallcout_kernel(
    const float* __restrict__ x, const float* __restrict__ wq, const float* __restrict__ bias,
    const float* __restrict__ add, float* __restrict__ y, int Cin, int Cout, int D, int H, int W,
    int ty_tiles, int tx_tiles, int64_t xbs, int64_t ybs, int head) {
  // head (wave-uniform): 0 none, 1 nn.Softmax(dim=1), 2 nn.Sigmoid (sigmoid_f32 per element, the bits of m355_sigmoid_fwd).
  // softmax: nn.Softmax(dim=1) of the hypothesis (models/modular_unet.py:100) applied in the epilogue -- all
  // (<= 4) channels of a voxel are in this thread's registers, so the logits never travel through HBM.  Same
  // formula and order as softmax_fwd_kernel (max, sum of expf in channel order, one reciprocal): identical bits.
  constexpr int XE = VS_CC * VS_CS, XPER = (XE + 255) / 256;
  constexpr unsigned OOB = 0x80000000u;
  __shared__ __attribute__((aligned(16))) float xs[XE];
  const int tid = threadIdx.x;
  const int tx = tid & 7, ty = (tid >> 3) & 7, tz = tid >> 6;
  // XCD-aware placement (speed only, a bijection of the grid): blocks b and b + 8 share an XCD and its L2; give each
  // XCD a contiguous run of tiles, so that the 1.9x halo overlap of neighbouring tiles hits in that L2 instead of
  // being fetched from HBM again (PMC: 543 MB per launch for 293 MB of algorithmic bytes before)
  int bt;
  {
    const int nwg = (int)gridDim.x, bid = (int)blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    bt = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int txt = bt % tx_tiles;
  bt /= tx_tiles;
  const int tyt = bt % ty_tiles;
  const int tzt = bt / ty_tiles;
  const int z0 = tzt * VS_TZ, y0 = tyt * VS_TY, x0 = txt * VS_TX;
  const int n = blockIdx.y;
  const float* xn = x + (int64_t)n * xbs;
  const int iHW = H * W, iDHW = D * H * W;

  // chunk-invariant byte offsets of this thread's halo elements (padding / past the tile: out of range)
  unsigned goff[XPER];
#pragma unroll
  for (int i = 0; i < XPER; ++i) {
    const int e = tid + 256 * i;
    const int c = e / VS_CS, r = e - c * VS_CS;
    const int zz = r / VS_PS, r2 = r - zz * VS_PS;
    const int yy = r2 / VS_RS, xx = r2 - yy * VS_RS;
    const int gz = z0 + zz - 1, gy = y0 + yy - 1, gx = x0 + xx - 1;
    const bool ok = e < XE && xx < VS_TX + 2 && (unsigned)gz < (unsigned)D && (unsigned)gy < (unsigned)H &&
                    (unsigned)gx < (unsigned)W;
    goff[i] = ok ? (unsigned)(c * iDHW + gz * iHW + gy * W + gx) * 4u : OOB;
  }

  f32x2 acc[8][2];
#pragma unroll
  for (int v = 0; v < 8; ++v) acc[v][0] = acc[v][1] = (f32x2){0.f, 0.f};

  float xr[XPER];
  auto fetch = [&](int c0, bool live) {  // !live: zero-sized descriptor, no memory traffic
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(xn + (int64_t)c0 * iDHW), 0, live ? min(VS_CC, Cin - c0) * iDHW * 4 : 0, 0x00020000);
#pragma unroll
    for (int i = 0; i < XPER; ++i) xr[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, goff[i], 0, 0));
  };
  fetch(0, true);
  for (int c0 = 0; c0 < Cin; c0 += VS_CC) {
    __syncthreads();  // the previous chunk has been consumed
#pragma unroll
    for (int i = 0; i < XPER; ++i)
      if (tid + 256 * i < XE) xs[tid + 256 * i] = xr[i];
    __syncthreads();
    fetch(c0 + VS_CC < Cin ? c0 + VS_CC : c0, c0 + VS_CC < Cin);  // next chunk in flight during the FMAs
    const int cn = min(VS_CC, Cin - c0);
    for (int c = 0; c < cn; ++c) {
      const float* wc = wq + (int64_t)(c0 + c) * 27 * 4;
      const float* xc = xs + c * VS_CS + tz * VS_PS + ty * VS_RS + tx * 8;
      // software-pipelined over the 9 (dz, dy) rows: the LDS segment and the 12 scalar weights of row
      // r + 1 are requested before the 48 packed FMAs of row r (sched_barrier: hipcc otherwise issues
      // each scalar load right before its first use and waits on it)
      float seg[2][10];
      f32x4 wrow[2][3];
      auto request = [&](int r, int slot) {  // r is a compile-time constant after unrolling
        const float* row = xc + (r / 3) * VS_PS + (r % 3) * VS_RS;
        const f32x4 s0 = *reinterpret_cast<const f32x4*>(row), s1 = *reinterpret_cast<const f32x4*>(row + 4);
        const f32x2 s2 = *reinterpret_cast<const f32x2*>(row + 8);
        seg[slot][0] = s0[0]; seg[slot][1] = s0[1]; seg[slot][2] = s0[2]; seg[slot][3] = s0[3];
        seg[slot][4] = s1[0]; seg[slot][5] = s1[1]; seg[slot][6] = s1[2]; seg[slot][7] = s1[3];
        seg[slot][8] = s2[0]; seg[slot][9] = s2[1];
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) wrow[slot][dx] = *reinterpret_cast<const f32x4*>(wc + (r * 3 + dx) * 4);  // uniform
      };
      request(0, 0);
#pragma unroll
      for (int r = 0; r < 9; ++r) {
        if (r + 1 < 9) request(r + 1, (r + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const f32x2 w01 = (f32x2){wrow[r & 1][dx][0], wrow[r & 1][dx][1]};
          const f32x2 w23 = (f32x2){wrow[r & 1][dx][2], wrow[r & 1][dx][3]};
#pragma unroll
          for (int v = 0; v < 8; ++v) {
            const f32x2 xv = (f32x2){seg[r & 1][v + dx], seg[r & 1][v + dx]};
            acc[v][0] = __builtin_elementwise_fma(xv, w01, acc[v][0]);
            acc[v][1] = __builtin_elementwise_fma(xv, w23, acc[v][1]);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  const int gz = z0 + tz, gy = y0 + ty, gx0 = x0 + tx * 8;
  if (gz >= D || gy >= H || gx0 >= W) return;
  float* yn = y + (int64_t)n * ybs;
  const float* an = add ? add + (int64_t)n * ybs : nullptr;
  const bool vec = gx0 + 8 <= W && ((((uintptr_t)yn) | ((uintptr_t)an)) & 15) == 0 && (W & 3) == 0;
  float val[4][8];
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const float bv = (bias && o < Cout) ? bias[o] : 0.f;
    const int64_t idx = (int64_t)o * iDHW + (int64_t)gz * iHW + (int64_t)gy * W + gx0;
#pragma unroll
    for (int k = 0; k < 8; ++k) val[o][k] = acc[k][o >> 1][o & 1] + bv;
    if (an && o < Cout) {
      if (vec) {
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(an + idx), a1 = *reinterpret_cast<const f32x4*>(an + idx + 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) { val[o][k] += a0[k]; val[o][4 + k] += a1[k]; }
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (gx0 + k < W) val[o][k] += an[idx + k];
      }
    }
  }
  if (head == 1) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float mx = -INFINITY;
#pragma unroll
      for (int o = 0; o < 4; ++o)
        if (o < Cout) mx = fmaxf(mx, val[o][k]);
      float sum = 0.f;
#pragma unroll
      for (int o = 0; o < 4; ++o)
        if (o < Cout) sum += expf(val[o][k] - mx);
      const float inv = 1.f / sum;
#pragma unroll
      for (int o = 0; o < 4; ++o)
        if (o < Cout) val[o][k] = expf(val[o][k] - mx) * inv;
    }
  } else if (head == 2) {
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (o < Cout) val[o][k] = sigmoid_f32(val[o][k]);
  }
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    if (o >= Cout) break;
    const int64_t idx = (int64_t)o * iDHW + (int64_t)gz * iHW + (int64_t)gy * W + gx0;
    if (vec) {
      *reinterpret_cast<f32x4*>(yn + idx) = (f32x4){val[o][0], val[o][1], val[o][2], val[o][3]};
      *reinterpret_cast<f32x4*>(yn + idx + 4) = (f32x4){val[o][4], val[o][5], val[o][6], val[o][7]};
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (gx0 + k < W) yn[idx + k] = val[o][k];
    }
  }
}

// y[n,o,s] = bias[o] + add[n,o,s] + sum_ks slab[ks][n,o,s]   (fixed order)
__global__ void splitk_reduce_kernel(const float* __restrict__ slab, const float* __restrict__ bias,
                                     const float* __restrict__ add, float* __restrict__ y, int N,
                                     int Cout, int64_t S, int ksplit, int64_t slab_stride,
                                     int64_t ybs) {
  const int64_t total = (int64_t)N * Cout * S;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = i % S;
    const int64_t no = i / S;
    const int o = (int)(no % Cout);
    const int n = (int)(no / Cout);
    float v = slab[i];
    for (int k = 1; k < ksplit; ++k) v += slab[(int64_t)k * slab_stride + i];
    if (bias) v += bias[o];
    const int64_t yi = (int64_t)n * ybs + (int64_t)o * S + s;
    if (add) v += add[yi];
    y[yi] = v;
  }
}

// The same with the statistics partials of the following normalisation (what the unsplit kernels emit from their
// epilogue): grid (voxel chunks, Cout, N), one (sum, sum of squares) slot per block:
// stat[((n * gridDim.x + blockIdx.x) * Cout + o) * 2 + {0,1}] -- the norm then never re-reads y for its statistics.
__global__ __launch_bounds__(256) void splitk_reduce_stats_kernel(const float* __restrict__ slab,
                                                                  const float* __restrict__ bias,
                                                                  const float* __restrict__ add, float* __restrict__ y,
                                                                  int Cout, int64_t S, int ksplit, int64_t slab_stride,
                                                                  int64_t ybs, float* __restrict__ stat) {
  __shared__ float scratch[4];
  const int o = blockIdx.y, n = blockIdx.z;
  const float* sp = slab + ((int64_t)n * Cout + o) * S;
  const float b = bias ? bias[o] : 0.f;
  float* yp = y + (int64_t)n * ybs + (int64_t)o * S;
  const float* ap = add ? add + (int64_t)n * ybs + (int64_t)o * S : nullptr;
  float s1 = 0.f, s2 = 0.f;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < S; i += gridDim.x * 256ll) {
    float v = sp[i];
    int k = 1;
    for (; k + 8 <= ksplit; k += 8) {   // eight splits' loads in flight together; summed in split order all the same
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = sp[(int64_t)(k + u) * slab_stride + i];
#pragma unroll
      for (int u = 0; u < 8; ++u) v += t[u];
    }
    for (; k < ksplit; ++k) v += sp[(int64_t)k * slab_stride + i];
    v += b;
    if (ap) v += ap[i];
    yp[i] = v;
    s1 += v;
    s2 = fmaf(v, v, s2);
  }
  s1 = block_sum<float, 256>(s1, scratch);
  s2 = block_sum<float, 256>(s2, scratch);
  if (threadIdx.x == 0) {
    float* q = stat + (((int64_t)n * gridDim.x + blockIdx.x) * Cout + o) * 2;
    q[0] = s1;
    q[1] = s2;
  }
}

// ------------------------------------------------------- MFMA bwd-weight kernel
// dW[o, c, tap] = sum_v dy[o, v] * x[c, v + off(tap)]
// MFMA view: i = o (A = dy tile [32 o][256 voxels]), j = c (B = x halo tile
// [32 c][halo]), k = a pair of x-adjacent voxels.  Each wave owns 7 of the 27 taps
// (112 accumulator registers); the A fragment is reused across its 7 MFMAs.
// Channel strides are == 1 (mod 32) so the 32 lanes of a half hit 32 banks.
template <int GX>
struct BwTile {
  static constexpr int TX = GX;
  static constexpr int TY = (GX == 32) ? 4 : 8;
  static constexpr int TZ = (GX == 8) ? 4 : 2;
  static constexpr int NV = TZ * TY * TX;  // 256
  static constexpr int RS = TX + 2;
  static constexpr int PS = (TY + 2) * RS;
  static constexpr int HV = (TZ + 2) * PS;
  static constexpr int CSW = ((HV + 30) / 32) * 32 + 1;  // >= HV, == 1 mod 32
  static constexpr int DSW = NV + 1;
  static constexpr int XROWS = 32 * (TZ + 2) * (TY + 2);
};

template <int GX, bool VEC>
__global__ __launch_bounds__(256, 1) void conv3_mfma_bww_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ slab, int N,
    int Cin, int Cout, int D, int H, int W, int tz_tiles, int ty_tiles, int tx_tiles, int nsplit,
    int64_t xbs, int64_t ybs) {
  using T = BwTile<GX>;
  constexpr int TX = T::TX, TY = T::TY, TZ = T::TZ, RS = T::RS, PS = T::PS,
                CSW = T::CSW, DSW = T::DSW, NV = T::NV;
  static_assert(NV == 256, "one dy voxel per thread");
  __shared__ float xs[32 * CSW];
  __shared__ float ds[32 * DSW];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l32 = lane & 31;
  const int ctile = blockIdx.x, otile = blockIdx.y, split = blockIdx.z;
  const int c0 = ctile * 32, o0 = otile * 32;
  const int64_t HW = (int64_t)H * W;
  const int64_t DHW = HW * D;

  int toff[7];
#pragma unroll
  for (int t = 0; t < 7; ++t) {
    const int tap = min(wave * 7 + t, 26);
    toff[t] = (tap / 9) * PS + ((tap / 3) % 3) * RS + (tap % 3);
  }

  f32x16 acc[7];
#pragma unroll
  for (int t = 0; t < 7; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  const float* xb = xs + l32 * CSW + half;
  const float* db = ds + l32 * DSW + half;

  const int tiles_per_n = tz_tiles * ty_tiles * tx_tiles;
  const int ntiles = N * tiles_per_n;
  // this thread's dy voxel inside a tile
  const int vz = tid / (TY * TX), vy = (tid / TX) % TY, vx = tid % TX;

  // The next tile is fetched into registers while the MFMAs of the current one run
  // (1 workgroup per CU: nothing else would hide the global-memory latency).  The halo
  // tile is fetched as aligned float4 interior rows + two scalar halo columns, with 32-bit
  // offsets from a uniform base, to keep the address arithmetic per tile small.
  constexpr int RPC = (TZ + 2) * (TY + 2);   // rows per channel
  constexpr int ROWS = 32 * RPC;
  constexpr int Q = TX / 4;                  // float4 per interior row
  constexpr int NI = ROWS * Q;
  constexpr int IPER = (NI + 255) / 256;
  constexpr int NH = ROWS * 2;
  constexpr int HPER = (NH + 255) / 256;
  f32x4 xi[IPER];
  float xh[HPER];
  float dr[32];
  // validity bits of the prefetched registers (zero padding is applied at commit time; the
  // loads themselves are unconditional from clamped addresses -- see the forward kernel)
  unsigned mi[4], mh, md;
  const int iDHW = (int)DHW, iHW = (int)HW;

  // Tile-invariant part of every prefetch item, computed once: global offset relative to the
  // tile origin, LDS address, and a one-hot code (bit zz | bit 8+yy | bit 20+q) that a
  // per-tile uniform mask of valid rows / columns turns into a 2-instruction bounds check.
  int relI[IPER], ldsI[IPER], relH[HPER], ldsH[HPER];
  unsigned codeI[IPER], codeH[HPER];
#pragma unroll
  for (int k = 0; k < IPER; ++k) {
    const int m = tid + 256 * k;
    const int q = m % Q, row = m / Q;
    const int c = row / RPC, rem = row - c * RPC;
    const int zz = rem / (TY + 2), yy = rem - zz * (TY + 2);
    relI[k] = c * iDHW + zz * iHW + yy * W + 4 * q;
    ldsI[k] = m < NI ? c * CSW + zz * PS + yy * RS + 1 + 4 * q : -1;
    codeI[k] = (m < NI && c0 + c < Cin) ? ((1u << zz) | (1u << (8 + yy)) | (1u << (20 + q))) : 0xFFFFFFFFu;
  }
#pragma unroll
  for (int j = 0; j < HPER; ++j) {
    const int h = tid + 256 * j;
    const int side = h & 1, row = h >> 1;
    const int c = row / RPC, rem = row - c * RPC;
    const int zz = rem / (TY + 2), yy = rem - zz * (TY + 2);
    relH[j] = c * iDHW + zz * iHW + yy * W + (side ? TX : -1);
    ldsH[j] = h < NH ? c * CSW + zz * PS + yy * RS + (side ? TX + 1 : 0) : -1;
    codeH[j] = (h < NH && c0 + c < Cin) ? ((1u << zz) | (1u << (8 + yy)) | (1u << (20 + side))) : 0xFFFFFFFFu;
  }

  auto fetch = [&](int tile) {
    int t = tile;
    const int n = t / tiles_per_n;
    t -= n * tiles_per_n;
    const int txt = t % tx_tiles;
    t /= tx_tiles;
    const int tyt = t % ty_tiles;
    const int tzt = t / ty_tiles;
    const int z0 = tzt * TZ, y0 = tyt * TY, x0 = txt * TX;
    const float* xn = x + (int64_t)n * xbs;
    const float* dn = dy + (int64_t)n * ybs;
    // uniform masks of the halo rows / interior float4s / halo sides that fall inside the volume
    unsigned zy = 0u;
    for (int zz = 0; zz < TZ + 2; ++zz)
      if (z0 + zz - 1 >= 0 && z0 + zz - 1 < D) zy |= 1u << zz;
    for (int yy = 0; yy < TY + 2; ++yy)
      if (y0 + yy - 1 >= 0 && y0 + yy - 1 < H) zy |= 1u << (8 + yy);
    unsigned qm[4] = {0u, 0u, 0u, 0u};
    for (int q = 0; q < Q; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (x0 + 4 * q + e < W) qm[e] |= 1u << (20 + q);
    const unsigned sm = (x0 - 1 >= 0 ? (1u << 20) : 0u) | (x0 + TX < W ? (1u << 21) : 0u);
    const int base = c0 * iDHW + (z0 - 1) * iHW + (y0 - 1) * W + x0;
    mi[0] = mi[1] = mi[2] = mi[3] = 0u;
    mh = 0u;
#pragma unroll
    for (int k = 0; k < IPER; ++k) {
      if constexpr (VEC) {
        const bool ok = (codeI[k] & ~(zy | qm[0])) == 0u;  // W % 4 == 0: a float4 is in or out as a whole
        xi[k] = *reinterpret_cast<const f32x4*>(xn + (ok ? base + relI[k] : 0));
        const unsigned bit = ok ? (1u << k) : 0u;
        mi[0] |= bit; mi[1] |= bit; mi[2] |= bit; mi[3] |= bit;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool ok = (codeI[k] & ~(zy | qm[e])) == 0u;
          xi[k][e] = xn[ok ? base + relI[k] + e : 0];
          mi[e] |= ok ? (1u << k) : 0u;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < HPER; ++j) {
      const bool ok = (codeH[j] & ~(zy | sm)) == 0u;
      xh[j] = xn[ok ? base + relH[j] : 0];
      mh |= ok ? (1u << j) : 0u;
    }
    const int gz = z0 + vz, gy = y0 + vy, gx = x0 + vx;
    const bool vok = gz < D && gy < H && gx < W;
    const int sp = vok ? gz * iHW + gy * W + gx : 0;
    md = 0u;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const bool ok = vok && o0 + j < Cout;
      dr[j] = dn[ok ? (o0 + j) * iDHW + sp : 0];
      md |= ok ? (1u << j) : 0u;
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int k = 0; k < IPER; ++k) {
      if (ldsI[k] >= 0) {
        float* p = xs + ldsI[k];
#pragma unroll
        for (int e = 0; e < 4; ++e) p[e] = ((mi[e] >> k) & 1u) ? xi[k][e] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < HPER; ++j)
      if (ldsH[j] >= 0) xs[ldsH[j]] = ((mh >> j) & 1u) ? xh[j] : 0.f;
#pragma unroll
    for (int j = 0; j < 32; ++j) ds[j * DSW + tid] = ((md >> j) & 1u) ? dr[j] : 0.f;
  };

  if (split < ntiles) {
    fetch(split);
    commit();
  }
  __syncthreads();

  for (int tile = split; tile < ntiles; tile += nsplit) {
    const bool more = tile + nsplit < ntiles;
    if (more) fetch(tile + nsplit);
    for (int z = 0; z < TZ; ++z) {
      for (int yy = 0; yy < TY; ++yy) {
        const float* xr_ = xb + z * PS + yy * RS;
        const float* dr_ = db + (z * TY + yy) * TX;
#pragma unroll
        for (int xp = 0; xp < TX / 2; ++xp) {
          const float a = dr_[2 * xp];
#pragma unroll
          for (int t = 0; t < 7; ++t) {
            const float b = xr_[2 * xp + toff[t]];
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[t], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();  // every wave is done reading this tile
    if (more) commit();
    __syncthreads();
  }

  // partial dW -> slab[split][Cout][Cin][27]
  float* sl = slab + (int64_t)split * Cout * Cin * 27;
  const int c = c0 + l32;
#pragma unroll
  for (int t = 0; t < 7; ++t) {
    const int tap = wave * 7 + t;
    if (tap < 27 && c < Cin) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = o0 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (o < Cout) sl[((int64_t)o * Cin + c) * 27 + tap] = acc[t][r];
      }
    }
  }
}

// ---- bwd-weight, second generation (used whenever W % 4 == 0 and a sample fits 2 GiB) ----
// Same tiling and MFMA mapping as conv3_mfma_bww_kernel.  What changed is everything AROUND the
// MFMAs: with one wave per SIMD nothing else covers the matrix core while a wave issues the
// prefetch of the next tile (~1000 VALU/VMEM instructions) and commits it to LDS (~1000 more),
// which cost ~20 % of the kernel.  Here
//  * the prefetch uses raw buffer loads: out-of-volume halo elements and channels past Cin/Cout
//    get an out-of-range offset and the hardware returns 0, so there are no validity masks and the
//    commit is a plain sequence of LDS writes;
//  * the row loop is fully unrolled and the prefetch is cut into one slice per row, so its
//    instructions are issued in the shadow of that row's MFMAs (the sched_barrier at the end of
//    each row keeps the slices from being hoisted back into one block).  The prefetch is
//    unconditional (the last iteration re-fetches its own tile): a branch would split the row into
//    basic blocks and undo the interleaving.
// Channel counts that are no multiple of 32 (the reference's real widths are 40 / 80 / 120): a remainder of 1..16
// channels on the o and / or the c side runs on v_mfma_f32_16x16x4_f32 over 16-channel sub-tiles (MT x NT of them;
// the full 32 x 32 pair keeps the 32x32x2 form): a (32 o, 16 c) pair costs half a full pair, (16, 16) a quarter --
// 40 x 40 channels are 2.25 pair-units of MFMA time instead of 4.  K is a quad of x-adjacent voxels; the fragments
// are (channel = lane & 15, voxel = lane >> 4), so the LDS channel strides are == 2 (mod 32) there.
// C/D layout 16x16x4: col (c) = lane & 15, row (o) = 4 * (lane >> 4) + reg.

template <int GX, int MT, int NT>
__device__ __forceinline__ void bww2_body(const float* __restrict__ x, const float* __restrict__ dy,
                                          float* __restrict__ sl, int N, int Cin, int Cout, int D, int H, int W,
                                          int tz_tiles, int ty_tiles, int tx_tiles, int nsplit, int split, int c0,
                                          int o0, int64_t xbs, int64_t ybs, float* __restrict__ xs,
                                          float* __restrict__ ds) {
  using T = BwTile<GX>;
  constexpr bool F = MT == 2 && NT == 2;     // full pair: one 32x32x2 MFMA per (tap, voxel pair)
  constexpr int NCX = 16 * NT, NCO = 16 * MT;
  constexpr int TX = T::TX, TY = T::TY, TZ = T::TZ, RS = T::RS, PS = T::PS, NV = T::NV;
  constexpr int CSW = F ? T::CSW : T::CSW + 1, DSW = F ? T::DSW : T::DSW + 1;
  static_assert(NV == 256, "one dy voxel per thread");

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l32 = lane & 31;
  const int kq = lane >> 4, l16 = lane & 15;
  const int iHW = H * W, iDHW = D * H * W;

  f32x16 acc[F ? 7 : 1];
  f32x4v acc16[F ? 1 : 7][MT][NT];
  if constexpr (F) {
#pragma unroll
    for (int t = 0; t < 7; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  } else {
#pragma unroll
    for (int t = 0; t < 7; ++t)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc16[t][mt][nt][r] = 0.f;
  }

  // per-wave tap bases into the x halo tile; everything else in an LDS read address is an immediate
  const float* xt[7];
#pragma unroll
  for (int t = 0; t < 7; ++t) {
    const int tap = min(wave * 7 + t, 26);
    xt[t] = xs + (F ? l32 * CSW + half : l16 * CSW + kq) + (tap / 9) * PS + ((tap / 3) % 3) * RS + (tap % 3);
  }
  const float* db = ds + (F ? l32 * DSW + half : l16 * DSW + kq);

  const int tiles_per_n = tz_tiles * ty_tiles * tx_tiles;
  const int ntiles = N * tiles_per_n;
  const int vz = tid / (TY * TX), vy = (tid / TX) % TY, vx = tid % TX;

  constexpr int RPC = (TZ + 2) * (TY + 2);   // rows per channel
  constexpr int ROWS = NCX * RPC;
  constexpr int Q = TX / 4;                  // float4 per interior row
  constexpr int NI = ROWS * Q, IPER = (NI + 255) / 256;
  constexpr int NH = ROWS * 2, HPER = (NH + 255) / 256;
  constexpr bool IFULL = NI % 256 == 0, HFULL = NH % 256 == 0;   // every thread owns whole prefetch items
  constexpr int NR = TZ * TY;                // MFMA rows per tile == prefetch slices
  constexpr unsigned OOB = 0x80000000u;      // >= num_records of any sample we accept: load returns 0
  f32x4 xi[IPER];
  float xh[HPER];
  float dr[NCO];

  // tile-invariant descriptors (see conv3_mfma_bww_kernel)
  int relI[IPER], ldsI[IPER], relH[HPER], ldsH[HPER];
  unsigned codeI[IPER], codeH[HPER];
#pragma unroll
  for (int k = 0; k < IPER; ++k) {
    const int m = tid + 256 * k;
    const int q = m % Q, row = m / Q;
    const int c = row / RPC, rem = row - c * RPC;
    const int zz = rem / (TY + 2), yy = rem - zz * (TY + 2);
    relI[k] = c * iDHW + zz * iHW + yy * W + 4 * q;
    ldsI[k] = c * CSW + zz * PS + yy * RS + 1 + 4 * q;
    codeI[k] = (IFULL || m < NI) ? (1u << zz) | (1u << (8 + yy)) | (1u << (20 + q)) : 0xffffffffu;  // past the end: never valid
  }
#pragma unroll
  for (int j = 0; j < HPER; ++j) {
    const int h = tid + 256 * j;
    const int side = h & 1, row = h >> 1;
    const int c = row / RPC, rem = row - c * RPC;
    const int zz = rem / (TY + 2), yy = rem - zz * (TY + 2);
    relH[j] = c * iDHW + zz * iHW + yy * W + (side ? TX : -1);
    ldsH[j] = c * CSW + zz * PS + yy * RS + (side ? TX + 1 : 0);
    codeH[j] = (HFULL || h < NH) ? (1u << zz) | (1u << (8 + yy)) | (1u << (20 + side)) : 0xffffffffu;
  }

  // per-tile uniform state of the prefetch
  __amdgpu_buffer_rsrc_t rx, rd;
  unsigned inI = 0u, inH = 0u;  // valid halo rows | interior float4s (resp. halo sides)
  int base = 0, dsp = 0;
  bool vok = false;
  auto tile_setup = [&](int tile, bool live) {  // !live: zero-sized descriptors, no memory traffic
    int t = tile;
    const int n = t / tiles_per_n;
    t -= n * tiles_per_n;
    const int txt = t % tx_tiles;
    t /= tx_tiles;
    const int tyt = t % ty_tiles;
    const int tzt = t / ty_tiles;
    const int z0 = tzt * TZ, y0 = tyt * TY, x0 = txt * TX;
    // channels past Cin / Cout are past num_records: zero-filled by the hardware as well
    rx = __builtin_amdgcn_make_buffer_rsrc((void*)(x + (int64_t)n * xbs), 0, live ? Cin * iDHW * 4 : 0, 0x00020000);
    rd = __builtin_amdgcn_make_buffer_rsrc((void*)(dy + (int64_t)n * ybs), 0, live ? Cout * iDHW * 4 : 0, 0x00020000);
    unsigned zy = 0u;
    for (int zz = 0; zz < TZ + 2; ++zz)
      if (z0 + zz - 1 >= 0 && z0 + zz - 1 < D) zy |= 1u << zz;
    for (int yy = 0; yy < TY + 2; ++yy)
      if (y0 + yy - 1 >= 0 && y0 + yy - 1 < H) zy |= 1u << (8 + yy);
    unsigned qm = 0u;
    for (int q = 0; q < Q; ++q)
      if (x0 + 4 * q < W) qm |= 1u << (20 + q);  // W % 4 == 0: a float4 is in or out as a whole
    inI = zy | qm;
    inH = zy | (x0 - 1 >= 0 ? (1u << 20) : 0u) | (x0 + TX < W ? (1u << 21) : 0u);
    base = c0 * iDHW + (z0 - 1) * iHW + (y0 - 1) * W + x0;
    const int gz = z0 + vz, gy = y0 + vy, gx = x0 + vx;
    vok = gz < D && gy < H && gx < W;
    dsp = o0 * iDHW + gz * iHW + gy * W + gx;
  };
  // slice r of the prefetch (r is a compile-time constant wherever this is called)
  auto fetch_slice = [&](int r) {
#pragma unroll
    for (int k = 0; k < IPER; ++k)
      if (k % NR == r) {
        const bool ok = (codeI[k] & ~inI) == 0u;
        xi[k] = __builtin_bit_cast(
            f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, ok ? (unsigned)(base + relI[k]) * 4u : OOB, 0, 0));
      }
#pragma unroll
    for (int j = 0; j < HPER; ++j)
      if (j % NR == r) {
        const bool ok = (codeH[j] & ~inH) == 0u;
        xh[j] = __builtin_bit_cast(
            float, __builtin_amdgcn_raw_buffer_load_b32(rx, ok ? (unsigned)(base + relH[j]) * 4u : OOB, 0, 0));
      }
#pragma unroll
    for (int j = 0; j < NCO; ++j)
      if (j % NR == r)
        dr[j] = __builtin_bit_cast(
            float, __builtin_amdgcn_raw_buffer_load_b32(rd, vok ? (unsigned)(dsp + j * iDHW) * 4u : OOB, 0, 0));
  };
  auto commit = [&]() {
#pragma unroll
    for (int k = 0; k < IPER; ++k)
      if (IFULL || tid + 256 * k < NI) {
        float* p = xs + ldsI[k];
#pragma unroll
        for (int e = 0; e < 4; ++e) p[e] = xi[k][e];
      }
#pragma unroll
    for (int j = 0; j < HPER; ++j)
      if (HFULL || tid + 256 * j < NH) xs[ldsH[j]] = xh[j];
#pragma unroll
    for (int j = 0; j < NCO; ++j) ds[j * DSW + tid] = dr[j];
  };

  if (split < ntiles) {
    tile_setup(split, true);
#pragma unroll
    for (int r = 0; r < NR; ++r) fetch_slice(r);
    commit();
  }
  __syncthreads();

  for (int tile = split; tile < ntiles; tile += nsplit) {
    const bool more = tile + nsplit < ntiles;
    tile_setup(more ? tile + nsplit : tile, more);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      fetch_slice(r);
      const int ro = (r / TY) * PS + (r % TY) * RS;  // immediate
      if constexpr (F) {
#pragma unroll
        for (int xp = 0; xp < TX / 2; ++xp) {
          const float a = db[r * TX + 2 * xp];
#pragma unroll
          for (int t = 0; t < 7; ++t)
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xt[t][ro + 2 * xp], acc[t], 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int xq = 0; xq < TX / 4; ++xq) {
          float a[MT];
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) a[mt] = db[mt * 16 * DSW + r * TX + 4 * xq];
#pragma unroll
          for (int t = 0; t < 7; ++t)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
              const float b = xt[t][nt * 16 * CSW + ro + 4 * xq];
#pragma unroll
              for (int mt = 0; mt < MT; ++mt)
                acc16[t][mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], b, acc16[t][mt][nt], 0, 0, 0);
            }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();  // every wave is done reading this tile
    if (more) commit();
    __syncthreads();
  }

  // partial dW -> slab[split][27][Cout][Cin]: the lane index is the input channel, so every store
  // writes 32 (16) consecutive floats (the [o][c][27] order of dW would scatter each lane to its own
  // cache line: 28k line requests per workgroup instead of ~900)
  if constexpr (F) {
    const int c = c0 + l32;
#pragma unroll
    for (int t = 0; t < 7; ++t) {
      const int tap = wave * 7 + t;
      if (tap < 27 && c < Cin) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int o = o0 + (r & 3) + 8 * (r >> 2) + 4 * half;
          if (o < Cout) sl[((int64_t)tap * Cout + o) * Cin + c] = acc[t][r];
        }
      }
    }
  } else {
#pragma unroll
    for (int t = 0; t < 7; ++t) {
      const int tap = wave * 7 + t;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const int c = c0 + 16 * nt + l16;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int o = o0 + 16 * mt + 4 * kq + r;
            if (tap < 27 && c < Cin && o < Cout) sl[((int64_t)tap * Cout + o) * Cin + c] = acc16[t][mt][nt][r];
          }
        }
    }
  }
}

template <int GX>
__global__ __launch_bounds__(256, 1) void conv3_mfma_bww2_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ slab, int N,
    int Cin, int Cout, int D, int H, int W, int tz_tiles, int ty_tiles, int tx_tiles, int nsplit,
    int ctiles, int otiles, int64_t xbs, int64_t ybs) {
  using T = BwTile<GX>;
  __shared__ float xs[32 * T::CSW];
  __shared__ float ds[32 * T::DSW];
  // XCD-aware placement (speed only): blocks b and b + 8 are observed to share an XCD and its L2, so
  // the block id is swizzled to give each XCD a contiguous run of virtual ids, and the virtual id is
  // decoded with the (c-tile, o-tile) pair fastest: the workgroups on one L2 work on the same and on
  // neighbouring voxel tiles, sharing the dy tile, the x tile and the halos.  A bijection of the
  // grid -- which partial sums land in which slab does not change, so results stay bit-identical.
  int vid;
  {
    const int nwg = (int)gridDim.x, bid = (int)blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    vid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int pairs = ctiles * otiles;
  const int pair = vid % pairs, split = vid / pairs;
  const int ctile = pair % ctiles, otile = pair / ctiles;
  bww2_body<GX, 2, 2>(x, dy, slab + (int64_t)split * 27 * Cout * Cin, N, Cin, Cout, D, H, W, tz_tiles, ty_tiles, tx_tiles,
                      nsplit, split, ctile * 32, otile * 32, xbs, ybs, xs, ds);
}

// The same, with the pairs of a channel remainder on their 16-row sub-tiles: ONE launch holds all four pair
// classes, each class cut into a number of voxel-range splits proportional to its MFMA cost, so that every
// workgroup of the launch lasts about equally long (the grid still fills the chip in whole residencies).
template <int GX>
__global__ __launch_bounds__(256, 1) void conv3_mfma_bww2c_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ slab, int N,
    int Cin, int Cout, int D, int H, int W, int tz_tiles, int ty_tiles, int tx_tiles, BwwClasses k,
    int64_t xbs, int64_t ybs) {
  using T = BwTile<GX>;
  __shared__ float xs[32 * (T::CSW + 1)];
  __shared__ float ds[32 * (T::DSW + 1)];
  int vid;
  {
    const int nwg = (int)gridDim.x, bid = (int)blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    vid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int cls = vid >= k.start[3] ? 3 : (vid >= k.start[2] ? 2 : (vid >= k.start[1] ? 1 : 0));
  const int idx = vid - k.start[cls];
  const int npairs = cls == 0 ? k.of * k.cf : (cls == 1 ? k.of : (cls == 2 ? k.cf : 1));
  const int pair = idx % npairs, split = idx / npairs;
  float* sl = slab + (int64_t)split * 27 * Cout * Cin;
  const int ns = k.ns[cls];
  if (cls == 0) {
    bww2_body<GX, 2, 2>(x, dy, sl, N, Cin, Cout, D, H, W, tz_tiles, ty_tiles, tx_tiles, ns, split, (pair % k.cf) * 32,
                        (pair / k.cf) * 32, xbs, ybs, xs, ds);
  } else if (cls == 1) {
    bww2_body<GX, 2, 1>(x, dy, sl, N, Cin, Cout, D, H, W, tz_tiles, ty_tiles, tx_tiles, ns, split, k.cf * 32, pair * 32,
                        xbs, ybs, xs, ds);
  } else if (cls == 2) {
    bww2_body<GX, 1, 2>(x, dy, sl, N, Cin, Cout, D, H, W, tz_tiles, ty_tiles, tx_tiles, ns, split, pair * 32, k.of * 32,
                        xbs, ybs, xs, ds);
  } else {
    bww2_body<GX, 1, 1>(x, dy, sl, N, Cin, Cout, D, H, W, tz_tiles, ty_tiles, tx_tiles, ns, split, k.cf * 32, k.of * 32,
                        xbs, ybs, xs, ds);
  }
}

// dW[o][c][27] = sum over splits of slab[split][27][o][c] (fixed order): one block per (o, 32 input
// channels); coalesced reads along c, transposed through LDS, one contiguous 864-float write.
__global__ __launch_bounds__(256) void slab_reduce_t_kernel(const float* __restrict__ slab, float* __restrict__ out,
                                                            int Cin, int Cout, BwwClasses k, float scale, int* __restrict__ oflag) {
  __shared__ float tr[32 * 27 + 32];
  const int o = blockIdx.x, c0 = blockIdx.y * 32;
  const int nsplit = k.ns[(o >= k.of * 32 ? 2 : 0) + ((int)blockIdx.y >= k.cf ? 1 : 0)];  // splits of this pair's class
  const int64_t plane = (int64_t)Cout * Cin, split_stride = 27 * plane;
  const int cw = min(32, Cin - c0);
  for (int e = threadIdx.x; e < 27 * 32; e += 256) {
    const int tap = e >> 5, cl = e & 31;
    float v = 0.f;
    if (cl < cw) {
      const float* p = slab + (int64_t)tap * plane + (int64_t)o * Cin + c0 + cl;
      int s = 0;
      for (; s + 16 <= nsplit; s += 16) {  // 16 independent loads in flight, summed in split order
        float t[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) t[u] = p[(int64_t)(s + u) * split_stride];
#pragma unroll
        for (int u = 0; u < 16; ++u) v += t[u];
      }
      for (; s + 4 <= nsplit; s += 4) {
        const float t0 = p[(int64_t)s * split_stride], t1 = p[(int64_t)(s + 1) * split_stride],
                    t2 = p[(int64_t)(s + 2) * split_stride], t3 = p[(int64_t)(s + 3) * split_stride];
        v += t0; v += t1; v += t2; v += t3;
      }
      for (; s < nsplit; ++s) v += p[(int64_t)s * split_stride];
    }
    tr[cl * 27 + tap] = v * scale;   // (scale != 1 only in the fp16 training flow: the loss scale leaves here)
    report_nonfinite(v * scale, oflag);
  }
  __syncthreads();
  float* dst = out + ((int64_t)o * Cin + c0) * 27;
  for (int e = threadIdx.x; e < cw * 27; e += 256) dst[e] = tr[e];
}

// The same reduction for FEW (o, c-tile) pairs with MANY splits (32 -> 32 at 128^3: 32 blocks each walking 256 slabs,
// 22 us on 32 of 256 CUs): one block per (o, c-tile, tap); its 256 threads are 32 channels x 8 split lanes, lane j sums
// the splits s = j, j + 8, ... and the eight partial sums are added in lane order -- fixed order, bit-reproducible.
__global__ __launch_bounds__(256) void slab_reduce_tap_kernel(const float* __restrict__ slab, float* __restrict__ out,
                                                              int Cin, int Cout, BwwClasses k, float scale, int* __restrict__ oflag) {
  __shared__ float part[8][32];
  const int o = blockIdx.x, ct = blockIdx.y, tap = blockIdx.z;
  const int nsplit = k.ns[(o >= k.of * 32 ? 2 : 0) + (ct >= k.cf ? 1 : 0)];
  const int64_t plane = (int64_t)Cout * Cin, split_stride = 27 * plane;
  const int cl = threadIdx.x & 31, j = threadIdx.x >> 5;
  const int c = ct * 32 + cl;
  float v = 0.f;
  if (c < Cin) {
    const float* p = slab + (int64_t)tap * plane + (int64_t)o * Cin + c;
    int s = j;
    for (; s + 24 < nsplit; s += 32) {   // four loads in flight
      const float t0 = p[(int64_t)s * split_stride], t1 = p[(int64_t)(s + 8) * split_stride],
                  t2 = p[(int64_t)(s + 16) * split_stride], t3 = p[(int64_t)(s + 24) * split_stride];
      v += t0; v += t1; v += t2; v += t3;
    }
    for (; s < nsplit; s += 8) v += p[(int64_t)s * split_stride];
  }
  part[j][cl] = v;
  __syncthreads();
  if (j == 0 && c < Cin) {
    float t = part[0][cl];
#pragma unroll
    for (int q = 1; q < 8; ++q) t += part[q][cl];
    out[((int64_t)o * Cin + c) * 27 + tap] = t * scale;
    report_nonfinite(t * scale, oflag);
  }
}

// the transposed reduction the route chose: per-tap blocks where the (o, c-tile) grid alone cannot fill the chip
static void launch_slab_reduce_t(const BwwRoute& r, const float* slab, float* dw, int Cin, int Cout, float scale,
                                 hipStream_t st) {
  if (r.aux & AUX_SLAB_TAP)
    hipLaunchKernelGGL(slab_reduce_tap_kernel, r.reduce_grid, dim3(256), 0, st, slab, dw, Cin, Cout, r.kred, scale,
                       overflow_flag());
  else
    hipLaunchKernelGGL(slab_reduce_t_kernel, r.reduce_grid, dim3(256), 0, st, slab, dw, Cin, Cout, r.kred, scale,
                       overflow_flag());
}

// ------------------------------------------- bwd-weight, tiny channel count on one side
// dW[o,c,tap] when Cin <= 4 (first conv) or Cout <= 4 (out conv).  The generic kernel would
// pad the narrow side to 32 MFMA rows/cols (8-10x waste).  Here the narrow channel AND the
// tap share the lane index: j = (s = l32>>3, t8 = l32&7), tap = wave*8 + t8 (27 of 32 used),
// so ONE MFMA per k-step per wave covers all taps:
//    G[i, (s,tap)] = sum_v P[i, v] * Q[s, v + off(tap)]
//  swap=0 (Cin small):  P = dy (wide = Cout), Q = x,  dW[o=i][c=s][tap]
//  swap=1 (Cout small): P = x (wide = Cin),  Q = dy read at v - off(tap) = v + off(26-tap),
//                       dW[o=s][c=i][tap]
// 16 accumulators and 46 KB of LDS -> three workgroups per CU; the next tile is prefetched into
// registers through buffer descriptors (out-of-volume halo and channels past CP / CQ read as 0)
// while the current one is multiplied.
template <int GX>
__global__ __launch_bounds__(256) void conv3_mfma_bww_small_kernel(
    const float* __restrict__ P, const float* __restrict__ Q, float* __restrict__ slab, int N,
    int CP, int CQ, int D, int H, int W, int tz_tiles, int ty_tiles, int tx_tiles, int nsplit,
    int64_t pbs, int64_t qbs, int swap, int Cin, int Cout) {
  using T = BwTile<GX>;
  constexpr int TX = T::TX, TY = T::TY, TZ = T::TZ, RS = T::RS, PS = T::PS, HV = T::HV,
                DSW = T::DSW;
  static_assert(T::NV == 256, "one wide-tile voxel per thread");
  constexpr int QS = HV + 1;
  constexpr int QE = 4 * HV, QPER = (QE + 255) / 256;
  constexpr unsigned OOB = 0x80000000u;
  __shared__ float ps[32 * DSW];
  __shared__ float qs[4 * QS];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l32 = lane & 31;
  const int p0 = blockIdx.x * 32, split = blockIdx.y;
  const int iHW = H * W, iDHW = D * H * W;

  const int s_l = l32 >> 3, t8 = l32 & 7;
  const int tap_raw = wave * 8 + t8;
  const int tap_eff = min(swap ? 26 - tap_raw : tap_raw, 26);
  const int toff = (max(tap_eff, 0) / 9) * PS + ((max(tap_eff, 0) / 3) % 3) * RS + (max(tap_eff, 0) % 3);
  const float* qb = qs + s_l * QS + toff + half;
  const float* pb = ps + l32 * DSW + half;

  f32x16 acc, acc2;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = acc2[r] = 0.f;

  const int vz = tid / (TY * TX), vy = (tid / TX) % TY, vx = tid % TX;
  const int tiles_per_n = tz_tiles * ty_tiles * tx_tiles;
  const int ntiles = N * tiles_per_n;

  // tile-invariant description of this thread's narrow-halo elements: offset from the halo origin,
  // LDS slot, halo coordinates (zz | yy << 8 | xx << 16; 0xFFFFFF past the tile: never valid)
  int qrel[QPER], qlds[QPER];
  unsigned qcode[QPER];
#pragma unroll
  for (int k = 0; k < QPER; ++k) {
    const int e = tid + 256 * k;
    const int c = e / HV, r = e - c * HV;
    const int zz = r / PS, r2 = r - zz * PS;
    const int yy = r2 / RS, xx = r2 - yy * RS;
    qrel[k] = c * iDHW + zz * iHW + yy * W + xx;
    qlds[k] = e < QE ? c * QS + r : -1;
    qcode[k] = e < QE ? ((unsigned)zz | ((unsigned)yy << 8) | ((unsigned)xx << 16)) : 0x00FFFFFFu;
  }

  float pr[32], qr[QPER];
  auto fetch = [&](int tile, bool live) {  // !live: zero-sized descriptors, no memory traffic
    int t = tile;
    const int n = t / tiles_per_n;
    t -= n * tiles_per_n;
    const int txt = t % tx_tiles;
    t /= tx_tiles;
    const int tyt = t % ty_tiles;
    const int tzt = t / ty_tiles;
    const int z0 = tzt * TZ, y0 = tyt * TY, x0 = txt * TX;
    const __amdgpu_buffer_rsrc_t rp =
        __builtin_amdgcn_make_buffer_rsrc((void*)(P + (int64_t)n * pbs), 0, live ? CP * iDHW * 4 : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rq =
        __builtin_amdgcn_make_buffer_rsrc((void*)(Q + (int64_t)n * qbs), 0, live ? CQ * iDHW * 4 : 0, 0x00020000);
    const int gz = z0 + vz, gy = y0 + vy, gx = x0 + vx;
    const bool vok = gz < D && gy < H && gx < W;
    const int sp = p0 * iDHW + gz * iHW + gy * W + gx;
#pragma unroll
    for (int j = 0; j < 32; ++j)
      pr[j] = __builtin_bit_cast(
          float, __builtin_amdgcn_raw_buffer_load_b32(rp, vok ? (unsigned)(sp + j * iDHW) * 4u : OOB, 0, 0));
    const int qbase = (z0 - 1) * iHW + (y0 - 1) * W + (x0 - 1);
#pragma unroll
    for (int k = 0; k < QPER; ++k) {
      const unsigned cd = qcode[k];
      const bool ok = (unsigned)(z0 - 1 + (int)(cd & 0xFFu)) < (unsigned)D &&
                      (unsigned)(y0 - 1 + (int)((cd >> 8) & 0xFFu)) < (unsigned)H &&
                      (unsigned)(x0 - 1 + (int)(cd >> 16)) < (unsigned)W;
      qr[k] = __builtin_bit_cast(
          float, __builtin_amdgcn_raw_buffer_load_b32(rq, ok ? (unsigned)(qbase + qrel[k]) * 4u : OOB, 0, 0));
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int j = 0; j < 32; ++j) ps[j * DSW + tid] = pr[j];
#pragma unroll
    for (int k = 0; k < QPER; ++k)
      if (qlds[k] >= 0) qs[qlds[k]] = qr[k];
  };

  if (split < ntiles) fetch(split, true);
  for (int tile = split; tile < ntiles; tile += nsplit) {
    __syncthreads();  // every wave is done reading the previous tile
    commit();
    __syncthreads();
    const bool more = tile + nsplit < ntiles;
    fetch(more ? tile + nsplit : tile, more);  // in flight during the MFMAs below
    for (int z = 0; z < TZ; ++z)
      for (int yy = 0; yy < TY; ++yy) {
        const float* prow = pb + (z * TY + yy) * TX;
        const float* qrow = qb + z * PS + yy * RS;
        // two independent accumulation chains (even / odd voxel pairs): a single chain makes every MFMA
        // wait for the previous one's result
#pragma unroll
        for (int xp = 0; xp < TX / 2; xp += 2) {
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(prow[2 * xp], qrow[2 * xp], acc, 0, 0, 0);
          acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(prow[2 * xp + 2], qrow[2 * xp + 2], acc2, 0, 0, 0);
        }
      }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] += acc2[r];
  float* sl = slab + (int64_t)split * Cout * Cin * 27;
  if (tap_raw < 27 && s_l < CQ) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = p0 + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (i < CP) {
        const int o = swap ? s_l : i, c = swap ? i : s_l;
        sl[((int64_t)o * Cin + c) * 27 + tap_raw] = acc[r];
      }
    }
  }
}

__global__ void slab_reduce_kernel(const float* __restrict__ slab, float* __restrict__ out,
                                   int64_t total, int nsplit) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    // fixed summation order; the loads of 8 splits are independent and stay in flight together
    float v = 0.f;
    int s = 0;
    for (; s + 8 <= nsplit; s += 8) {
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = slab[(int64_t)(s + u) * total + i];
#pragma unroll
      for (int u = 0; u < 8; ++u) v += t[u];
    }
    for (; s < nsplit; ++s) v += slab[(int64_t)s * total + i];
    out[i] = v;
  }
}

// dbias[o] = sum_{n,s} dy[n,o,s]: grid (chunks, Cout) of partial sums, then a fixed-order
// finalize (deterministic).  Short fp32 runs per thread, double across threads / blocks.  Chunks of 8192 voxels
// (float4 loads, 8 per thread and sample): the 32768-voxel chunks this started with gave the small volumes of the
// reference's dmri_hippo net (40 channels x 48x88x24) 160 workgroups of scalar loads -- 303 us for a 130 MB tensor.
template <bool VEC>
__global__ __launch_bounds__(256) void dbias_partial_kernel(const float* __restrict__ dy,
                                                            double* __restrict__ partial, int N,
                                                            int64_t S, int64_t ybs, int nblk) {
  __shared__ double scratch[4];
  const int b = blockIdx.x, o = blockIdx.y;
  const int64_t begin = (int64_t)b * DBIAS_CHUNK, end = min(S, begin + DBIAS_CHUNK);
  double acc = 0.0;
  for (int n = 0; n < N; ++n) {
    const float* p = dy + (int64_t)n * ybs + (int64_t)o * S;
    float part = 0.f;
    if (VEC) {   // S, ybs multiples of 4 and dy 16-byte aligned: every chunk starts on a float4
      for (int64_t s = begin + threadIdx.x * 4; s < end; s += 1024) {
        const float4 v = *reinterpret_cast<const float4*>(p + s);
        part += (v.x + v.y) + (v.z + v.w);
      }
    } else {
      for (int64_t s = begin + threadIdx.x; s < end; s += 256) part += p[s];
    }
    acc += part;
  }
  const double tot = block_sum<double, 256>(acc, scratch);
  if (threadIdx.x == 0) partial[(int64_t)o * nblk + b] = tot;
}
__global__ void dbias_finalize_kernel(const double* __restrict__ partial, float* __restrict__ dbias,
                                      int Cout, int nblk) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= Cout) return;
  double acc = 0.0;
  for (int b = 0; b < nblk; ++b) acc += partial[(int64_t)o * nblk + b];
  dbias[o] = (float)acc;
}

// ------------------------------------------------------ generic direct kernels
// Any cubic k / stride / pad; one thread per output element.  Fallback path.
__global__ void conv3d_direct_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                         const float* __restrict__ bias,
                                         const float* __restrict__ add, float* __restrict__ y,
                                         int N, int Cin, int Cout, int D, int H, int W, int OD,
                                         int OH, int OW, int k, int stride, int pad, int64_t xbs,
                                         int64_t ybs) {
  const int64_t OS = (int64_t)OD * OH * OW;
  const int64_t total = (int64_t)N * Cout * OS;
  const int k3 = k * k * k;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int ox = (int)(i % OW);
    int64_t r = i / OW;
    const int oy = (int)(r % OH);
    r /= OH;
    const int oz = (int)(r % OD);
    r /= OD;
    const int o = (int)(r % Cout);
    const int n = (int)(r / Cout);
    const float* xn = x + (int64_t)n * xbs;
    float acc = 0.f;
    for (int c = 0; c < Cin; ++c) {
      const float* wc = w + ((int64_t)o * Cin + c) * k3;
      const float* xc = xn + (int64_t)c * D * H * W;
      for (int dz = 0; dz < k; ++dz) {
        const int iz = oz * stride + dz - pad;
        if (iz < 0 || iz >= D) continue;
        for (int dy = 0; dy < k; ++dy) {
          const int iy = oy * stride + dy - pad;
          if (iy < 0 || iy >= H) continue;
          for (int dx = 0; dx < k; ++dx) {
            const int ix = ox * stride + dx - pad;
            if (ix < 0 || ix >= W) continue;
            acc = fmaf(wc[(dz * k + dy) * k + dx], xc[((int64_t)iz * H + iy) * W + ix], acc);
          }
        }
      }
    }
    if (bias) acc += bias[o];
    const int64_t yi = (int64_t)n * ybs + (int64_t)o * OS + ((int64_t)oz * OH + oy) * OW + ox;
    if (add) acc += add[yi];
    y[yi] = acc;
  }
}

// dx[n,c,iz,iy,ix] = sum_{o,taps: (i + pad - d) % stride == 0} w[o,c,d] * dy[n,o,(i+pad-d)/stride]
__global__ void conv3d_direct_bwd_data_kernel(const float* __restrict__ dy,
                                              const float* __restrict__ w, float* __restrict__ dx,
                                              int N, int Cin, int Cout, int D, int H, int W,
                                              int OD, int OH, int OW, int k, int stride, int pad,
                                              int64_t xbs, int64_t ybs) {
  const int64_t S = (int64_t)D * H * W;
  const int64_t OS = (int64_t)OD * OH * OW;
  const int64_t total = (int64_t)N * Cin * S;
  const int k3 = k * k * k;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int ix = (int)(i % W);
    int64_t r = i / W;
    const int iy = (int)(r % H);
    r /= H;
    const int iz = (int)(r % D);
    r /= D;
    const int c = (int)(r % Cin);
    const int n = (int)(r / Cin);
    const float* dyn = dy + (int64_t)n * ybs;
    float acc = 0.f;
    for (int o = 0; o < Cout; ++o) {
      const float* wc = w + ((int64_t)o * Cin + c) * k3;
      const float* dyo = dyn + (int64_t)o * OS;
      for (int dz = 0; dz < k; ++dz) {
        const int tz = iz + pad - dz;
        if (tz < 0 || tz % stride) continue;
        const int oz = tz / stride;
        if (oz >= OD) continue;
        for (int dyy = 0; dyy < k; ++dyy) {
          const int ty = iy + pad - dyy;
          if (ty < 0 || ty % stride) continue;
          const int oy = ty / stride;
          if (oy >= OH) continue;
          for (int dxx = 0; dxx < k; ++dxx) {
            const int tx = ix + pad - dxx;
            if (tx < 0 || tx % stride) continue;
            const int ox = tx / stride;
            if (ox >= OW) continue;
            acc = fmaf(wc[(dz * k + dyy) * k + dxx], dyo[((int64_t)oz * OH + oy) * OW + ox], acc);
          }
        }
      }
    }
    dx[(int64_t)n * xbs + (int64_t)c * S + ((int64_t)iz * H + iy) * W + ix] = acc;
  }
}

// dw[o,c,d] = sum_{n,ov} dy[n,o,ov] * x[n,c,ov*stride + d - pad]; one block per (o,c,tap).
__global__ __launch_bounds__(256) void conv3d_direct_bwd_weight_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dw, int N,
    int Cin, int Cout, int D, int H, int W, int OD, int OH, int OW, int k, int stride, int pad,
    int64_t xbs, int64_t ybs) {
  __shared__ double scratch[4];
  const int k3 = k * k * k;
  int b = blockIdx.x;
  const int tap = b % k3;
  b /= k3;
  const int c = b % Cin;
  const int o = b / Cin;
  const int dz = tap / (k * k), dyy = (tap / k) % k, dxx = tap % k;
  const int64_t OS = (int64_t)OD * OH * OW;
  double acc = 0.0;
  for (int n = 0; n < N; ++n) {
    const float* xc = x + (int64_t)n * xbs + (int64_t)c * D * H * W;
    const float* dyo = dy + (int64_t)n * ybs + (int64_t)o * OS;
    float part = 0.f;
    int cnt = 0;
    for (int64_t s = threadIdx.x; s < OS; s += 256) {
      const int ox = (int)(s % OW);
      const int oy = (int)((s / OW) % OH);
      const int oz = (int)(s / ((int64_t)OW * OH));
      const int iz = oz * stride + dz - pad, iy = oy * stride + dyy - pad,
                ix = ox * stride + dxx - pad;
      if (iz >= 0 && iz < D && iy >= 0 && iy < H && ix >= 0 && ix < W)
        part = fmaf(dyo[s], xc[((int64_t)iz * H + iy) * W + ix], part);
      if (++cnt == 64) { acc += part; part = 0.f; cnt = 0; }
    }
    acc += part;
  }
  const double tot = block_sum<double, 256>(acc, scratch);
  if (threadIdx.x == 0) dw[((int64_t)o * Cin + c) * k3 + tap] = (float)tot;
}

// ------------------------------------------------------------------ launchers
// Everything the host layer (conv3d_host.hip) starts from this file's kernels: it hands over a resolved route
// (conv3d_route.hpp) and the call's pointers; nothing here decides a kernel, a grid or an offset.
static_assert(TZ_K == SMALLCOUT_TZ_K && VS_TZ == SMALLCOUT_VS_TZ && VS_TY == SMALLCOUT_VS_TY && VS_TX == SMALLCOUT_VS_TX,
              "conv3d_route.hpp sizes the Cout <= 4 forward kernels' buffer and grids");

template <int NTW, int GX>
static void launch_fwd(const ConvRoute& r, const ConvCall& c, const float* wp, const float* bias, const float* add, float* slab,
                       float* stat, int* work_counter) {
  const FwdPlan& p = r.plan;
  const m355_conv3d_desc* d = c.d;
  const int N = d->N, D = d->D, H = d->H, W = d->W;
  const int64_t slab_stride = (int64_t)N * r.mout * D * H * W;
  if (r.grid.x) {
    if (r.kind == ConvKind::MfmaF32Queue) {
      hipLaunchKernelGGL((conv3_mfma_fwd_p_kernel<NTW, GX, false>), r.grid, dim3(256), 0, c.st, c.in, wp, bias, add, c.out,
                         slab, r.kin, r.mout, D, H, W, p.mout_pad, p.tz_tiles, p.ty_tiles, p.tx_tiles, p.otiles, p.nchunks,
                         p.ksplit, N, r.in_bs, r.out_bs, slab_stride, stat, work_counter, 0, r.sched);
    } else {
      hipLaunchKernelGGL((conv3_mfma_fwd_kernel<NTW, GX>), r.grid, dim3(256), 0, c.st, c.in, wp, bias, add, c.out, slab,
                         r.kin, r.mout, D, H, W, p.mout_pad, p.ty_tiles, p.tx_tiles, p.nchunks, p.ksplit, r.in_bs, r.out_bs,
                         slab_stride, stat, p.otiles, r.sched);
    }
  }
  if constexpr (NTW <= 4) {
    if (r.aux & AUX_TILE16)   // the 16-row remainder tile: queue-driven kernel over (spatial tile x sample x split) items
      hipLaunchKernelGGL((conv3_mfma_fwd_p_kernel<NTW, GX, true>), r.grid16, dim3(256), 0, c.st, c.in, wp, bias, add, c.out,
                         slab, r.kin, r.mout, D, H, W, p.mout_pad, p.tz_tiles, p.ty_tiles, p.tx_tiles, 1, p.nchunks, p.ksplit,
                         N, r.in_bs, r.out_bs, slab_stride, stat, work_counter, 32 * p.otiles, r.sched);
  }
}

void launch_pack_weights(const ConvRoute& r, const m355_conv3d_desc* d, bool transpose, const float* w, void* packed,
                         hipStream_t st) {
  const FwdPlan& p = r.plan;
  if (is_h16(r.kind)) return launch_pack_w3_h16(p, d->compute, w, packed, d->Cout, d->Cin, transpose, st);
  switch (r.kind) {
    case ConvKind::SmallCoutValu:
      hipLaunchKernelGGL(pack_w3_valu_kernel, dim3((unsigned)ceil_div(d->Cin * 27 * 4, 256)), dim3(256), 0, st, w,
                         (float*)packed, d->Cout, d->Cin);
      break;
    case ConvKind::SmallCoutToeplitz: {
      const int kin_pad = (int)round_up(d->Cin, 2);
      const int64_t total = (int64_t)kin_pad * TZ_K * 32;
      hipLaunchKernelGGL(pack_w3_toeplitz_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(total, 256), 2048)), dim3(256),
                         0, st, w, (float*)packed, d->Cout, d->Cin, kin_pad);
      break;
    }
    case ConvKind::X3:
      launch_pack_w3_x3(p, w, packed, d->Cout, d->Cin, transpose, st);
      break;
    default: {
      const int64_t total = (int64_t)p.kin_pad * 27 * p.mout_pad;
      const int blocks = (int)std::min<int64_t>(ceil_div(total, 256), 2048);
      hipLaunchKernelGGL(pack_w3_kernel, dim3(blocks), dim3(256), 0, st, w, (float*)packed, d->Cout, d->Cin, p.kin_pad,
                         p.mout_pad, transpose ? 1 : 0, (int*)((char*)packed + p.wp_bytes - 256));
    }
  }
}

int launch_f32_conv(const ConvRoute& r, const ConvCall& c) {
  const m355_conv3d_desc* d = c.d;
  const FwdPlan& p = r.plan;
  hipStream_t st = c.st;
  const int D = d->D, H = d->H, W = d->W, N = d->N;
  if (r.kind == ConvKind::Direct) {
    const int OD = out_dim(D, d->k, d->stride, d->pad), OH = out_dim(H, d->k, d->stride, d->pad),
              OW = out_dim(W, d->k, d->stride, d->pad);
    if (r.transpose)   // in = dy, out = dx
      hipLaunchKernelGGL(conv3d_direct_bwd_data_kernel, r.grid, dim3(256), 0, st, c.in, c.w, c.out, N, d->Cin, d->Cout,
                         D, H, W, OD, OH, OW, d->k, d->stride, d->pad, r.out_bs, r.in_bs);
    else
      hipLaunchKernelGGL(conv3d_direct_fwd_kernel, r.grid, dim3(256), 0, st, c.in, c.w, c.bias, c.add, c.out, N,
                         d->Cin, d->Cout, D, H, W, OD, OH, OW, d->k, d->stride, d->pad, r.in_bs, r.out_bs);
    return check_launch(r.transpose ? "conv3d_direct_bwd_data" : "conv3d_direct_fwd");
  }
  int* work_counter = nullptr;
  if (!is_smallcout(r.kind)) {
    work_counter = queue_state(st);   // per (device, stream): concurrent launches over one model never share it
    M355_REQUIRE(work_counter, M355_ELAUNCH, "conv3d: could not allocate the work-queue state");
  }
  float* wp = r.prepacked ? (float*)c.w : (float*)c.ws;
  if (r.aux & AUX_PACK_W) launch_pack_weights(r, d, r.transpose, c.w, wp, st);
  if (r.kind == ConvKind::SmallCoutValu) {   // packed-FMA kernel (see conv3_valu_smallcout_kernel)
    hipLaunchKernelGGL(conv3_valu_smallcout_kernel, r.grid, dim3(256), 0, st, c.in, wp, c.bias, c.add, c.out, d->Cin, d->Cout,
                       D, H, W, (int)ceil_div(H, VS_TY), (int)ceil_div(W, VS_TX), r.in_bs, r.out_bs, r.head);
    return check_launch("conv3_valu_smallcout");
  }
  if (r.kind == ConvKind::SmallCoutToeplitz) {
    hipLaunchKernelGGL(conv3_mfma_fwd_smallcout_kernel, r.grid, dim3(256), 0, st, c.in, wp, c.bias, c.add, c.out, d->Cin,
                       d->Cout, D, H, W, (int)ceil_div(H, 8), (int)ceil_div(W, 32), (int)round_up(d->Cin, 2) / 2, r.in_bs,
                       r.out_bs);
    return check_launch("conv3_mfma_fwd_smallcout");
  }
  float* slab = (float*)((char*)c.ws + r.slab_off);
  const bool split = (r.aux & AUX_SPLITK) != 0;   // bias, residual and statistics then come from the reduction pass
  const float* kb = split ? nullptr : c.bias;
  const float* ka = split ? nullptr : c.add;
  float* kstat = split ? nullptr : c.stat;
  if (r.kind == ConvKind::X3) {
    if (int rc = launch_x3_conv(r, c.in, wp, kb, ka, c.out, slab, d, st, kstat)) return rc;
  } else {
#define M355_FWD_CASE(NTW, GX)                                          \
  if (p.ntw == NTW && p.gx == GX) {                                     \
    launch_fwd<NTW, GX>(r, c, wp, kb, ka, slab, kstat, work_counter);   \
  } else
  M355_FWD_CASE(8, 32) M355_FWD_CASE(4, 32) M355_FWD_CASE(2, 32) M355_FWD_CASE(1, 32)
  M355_FWD_CASE(8, 16) M355_FWD_CASE(4, 16) M355_FWD_CASE(2, 16) M355_FWD_CASE(1, 16)
  M355_FWD_CASE(8, 8) M355_FWD_CASE(4, 8) M355_FWD_CASE(2, 8) M355_FWD_CASE(1, 8) {
    set_error("conv3d: no kernel for ntw=%d gx=%d", p.ntw, p.gx);
    return M355_EUNSUPPORTED;
  }
#undef M355_FWD_CASE
  }
  const int64_t S = (int64_t)D * H * W, total = (int64_t)N * r.mout * S;
  if (r.aux & AUX_SPLITK_STATS)   // split plan + fused statistics: the reduction pass emits the partials
    hipLaunchKernelGGL(splitk_reduce_stats_kernel, r.reduce_grid, dim3(256), 0, st, slab, c.bias, c.add, c.out, r.mout, S,
                       p.ksplit, total, r.out_bs, c.stat);
  else if (split)
    hipLaunchKernelGGL(splitk_reduce_kernel, r.reduce_grid, dim3(256), 0, st, slab, c.bias, c.add, c.out, N, r.mout, S,
                       p.ksplit, total, r.out_bs);
  return check_launch("conv3d_mfma");
}

template <int GX>
static void launch_bww_mfma(const BwwRoute& r, const float* x, const float* dy, float* slab, const m355_conv3d_desc* d,
                            hipStream_t st) {
  const BwwPlan& p = r.plan;
  switch (r.kind) {
    case BwwKind::Small: {   // narrow side (<= 4 channels) shares the lane index with the taps
      const int swap = d->Cin <= 4 ? 0 : 1;
      hipLaunchKernelGGL((conv3_mfma_bww_small_kernel<GX>), r.grid, dim3(256), 0, st, swap ? x : dy, swap ? dy : x, slab, d->N,
                         swap ? d->Cin : d->Cout, swap ? d->Cout : d->Cin, d->D, d->H, d->W, p.tz_tiles, p.ty_tiles,
                         p.tx_tiles, p.nsplit, swap ? r.xbs : r.ybs, swap ? r.ybs : r.xbs, swap, d->Cin, d->Cout);
      break;
    }
    case BwwKind::Mfma2c:
      hipLaunchKernelGGL((conv3_mfma_bww2c_kernel<GX>), r.grid, dim3(256), 0, st, x, dy, slab, d->N, d->Cin, d->Cout, d->D,
                         d->H, d->W, p.tz_tiles, p.ty_tiles, p.tx_tiles, p.k, r.xbs, r.ybs);
      break;
    case BwwKind::Mfma2:
      hipLaunchKernelGGL((conv3_mfma_bww2_kernel<GX>), r.grid, dim3(256), 0, st, x, dy, slab, d->N, d->Cin, d->Cout, d->D,
                         d->H, d->W, p.tz_tiles, p.ty_tiles, p.tx_tiles, p.nsplit, p.ctiles, p.otiles, r.xbs, r.ybs);
      break;
    default:
      with_bool(r.kind == BwwKind::MfmaVec, [&](auto V) {
        hipLaunchKernelGGL((conv3_mfma_bww_kernel<GX, decltype(V)::value>), r.grid, dim3(256), 0, st, x, dy, slab, d->N,
                           d->Cin, d->Cout, d->D, d->H, d->W, p.tz_tiles, p.ty_tiles, p.tx_tiles, p.nsplit, r.xbs, r.ybs);
      });
  }
}

int launch_bww(const BwwRoute& r, const BwwCall& c) {
  const m355_conv3d_desc* d = c.d;
  hipStream_t st = c.st;
  const int64_t S = (int64_t)d->D * d->H * d->W;
  float* slab = (float*)c.ws;
  const void *x = c.x, *dy = c.dy;
  if (r.via_pack) {
    // fp32 NCDHW operands in a 16-bit compute mode (the model path hands over c8 tensors through
    // m355_conv3d_bwd_weight_h16 / _c8): both operands are rounded into c8 copies and the c8 kernel runs
    void* x16 = (char*)c.ws + r.x16_off;
    void* dy16 = (char*)c.ws + r.dy16_off;
    if (int rc = launch_pack_act16((const float*)x, x16, d->N, d->Cin, S, r.x32_bs, r.xbs, d->compute, st)) return rc;
    if (int rc = launch_pack_act16((const float*)dy, dy16, d->N, d->Cout, S, r.dy_bs, r.ybs, d->compute, st)) return rc;
    x = x16;
    dy = dy16;
  }
  switch (r.kind) {
    case BwwKind::Direct:
      hipLaunchKernelGGL(conv3d_direct_bwd_weight_kernel, r.grid, dim3(256), 0, st, (const float*)x, (const float*)dy, c.dw,
                         d->N, d->Cin, d->Cout, d->D, d->H, d->W, out_dim(d->D, d->k, d->stride, d->pad),
                         out_dim(d->H, d->k, d->stride, d->pad), out_dim(d->W, d->k, d->stride, d->pad), d->k, d->stride,
                         d->pad, r.xbs, r.ybs);
      break;
    case BwwKind::X3:
    case BwwKind::X3c:
      launch_bww_x3(r, (const float*)x, (const float*)dy, slab, d, st);
      break;
    case BwwKind::C8:
    case BwwKind::C8Small:
      launch_bww_c8(r, x, dy, slab, d, st);
      if (int rc = check_launch(r.kind == BwwKind::C8 ? "conv3_bww_c8" : "conv3_bww_c8_small")) return rc;
      break;
    default:
      if (r.plan.gx == 32) launch_bww_mfma<32>(r, (const float*)x, (const float*)dy, slab, d, st);
      else if (r.plan.gx == 16) launch_bww_mfma<16>(r, (const float*)x, (const float*)dy, slab, d, st);
      else launch_bww_mfma<8>(r, (const float*)x, (const float*)dy, slab, d, st);
  }
  if (r.aux & (AUX_SLAB_T | AUX_SLAB_TAP))
    launch_slab_reduce_t(r, slab, c.dw, d->Cin, d->Cout, c.grad_unscale, st);
  else if (r.aux & AUX_SLAB_PLAIN)
    hipLaunchKernelGGL(slab_reduce_kernel, r.reduce_grid, dim3(r.reduce_block), 0, st, slab, c.dw, (int64_t)d->Cout * d->Cin * 27,
                       r.plan.nsplit);
  void* dbias_ws = (char*)c.ws + r.dbias_off;   // its scratch follows the slabs
  if (r.aux & AUX_DBIAS_C8) {
    if (int rc = launch_dbias_c8(dy, r.ybs, c.dbias, d->N, d->Cout, S, d->compute, c.grad_unscale, dbias_ws, st)) return rc;
  } else if (r.aux & AUX_DBIAS_F32) {
    launch_dbias(c.dy32, c.dbias, d->N, d->Cout, out_voxels(d), r.dy_bs, dbias_ws, st);
  }
  return check_launch(r.who);
}

}  // namespace m355

// (global namespace: convt.hip shares it)  dbias through the shared two-stage reduction; `ws` holds Cout * ceil(S / DBIAS_CHUNK) doubles
int launch_dbias(const float* dy, float* dbias, int N, int Cout, int64_t S, int64_t ybs, void* ws, hipStream_t st) {
  const int nblk = (int)m355::ceil_div(S, m355::DBIAS_CHUNK);
  if (S % 4 == 0 && ybs % 4 == 0 && ((uintptr_t)dy & 15) == 0)
    hipLaunchKernelGGL(m355::dbias_partial_kernel<true>, dim3((unsigned)nblk, (unsigned)Cout), dim3(256), 0, st, dy,
                       (double*)ws, N, S, ybs, nblk);
  else
    hipLaunchKernelGGL(m355::dbias_partial_kernel<false>, dim3((unsigned)nblk, (unsigned)Cout), dim3(256), 0, st, dy,
                       (double*)ws, N, S, ybs, nblk);
  hipLaunchKernelGGL(m355::dbias_finalize_kernel, dim3((unsigned)m355::ceil_div(Cout, 64)), dim3(64), 0, st,
                     (const double*)ws, dbias, Cout, nblk);
  return M355_OK;
}
