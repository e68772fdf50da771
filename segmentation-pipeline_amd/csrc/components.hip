// Connected components, masked grey dilation and label histograms (post-processing and lesion detection).
//
// Reference ops replaced (segmentation_pipeline/post_processing.py and evaluators/instance_segmentation_evaluator.py,
// both on top of skimage.morphology): `label` (scipy.ndimage.label with a 6 / 18 / 26 neighbourhood),
// `dilation` (ndi.grey_dilation with the cross footprint), and the np.unique / torch.unique counts.
//
// Labelling of an int32 volume [D,H,W] (< 2^31 voxels) in six launches:
//   A  ccl_local_kernel   union-find inside 8x8x64 tiles, in LDS (a 1-D grid walks the tiles, so any shape fits):
//                         every voxel is hung under the smallest local index of its in-tile component;
//                         par[v] = global index of that voxel (-1: background)
//   B  ccl_merge_kernel   voxels on a tile face unite with their backward neighbours in OTHER tiles, in global memory:
//                         roots always move to the smaller linear index (atomicMin), so every component's final root
//                         is its first voxel in raster order
//   C  ccl_flatten_kernel par[v] = root of v, and the number of roots of every 4096-voxel chunk
//   D  ccl_scan_kernel    one workgroup: exclusive scan of the chunk counts, n (or -1 when a bound was hit)
//   E  ccl_number_kernel  roots take 1 + the number of roots before them in raster order
//   F  ccl_relabel_kernel every other voxel takes its root's number (background 0)
// Visibility (MI355X: per-XCD L2s are not coherent, a CU's L1 never sees another CU's stores): in pass B the parent
// entries other workgroups rewrite are read with agent-scope atomic loads and every link is an agent-scope atomicMin
// whose returned value decides the next step, so a stale read only costs a retry.  Every other hand-off crosses a
// kernel boundary.  No grid-wide barrier.  Parent indices only ever decrease (par[v] <= v), so every find / union loop
// ends; each is bounded all the same: at the bound the error word is set and the entry point's n reads -1.
#include "common.hpp"

namespace m355 {

constexpr int CCL_TX = 64, CCL_TY = 8, CCL_TZ = 8, CCL_TILE = CCL_TX * CCL_TY * CCL_TZ;  // 4096 voxels
constexpr int CCL_NT = 256;
constexpr int CHUNK = 4096;            // voxels per block of the flatten / number / histogram passes (16 per thread)
constexpr int CHUNK_VPT = CHUNK / CCL_NT;
constexpr int FIND_BOUND = 1 << 20;    // steps of one find, retries of one union (global passes)
constexpr int HASH_SLOTS = 1024;       // LDS bins of the per-workgroup histogram reduction
constexpr int HASH_PROBES = 8;

struct Vol {
  int D, H, W;
};

// backward neighbours (smaller linear index): 3 faces, then 6 edges, then 4 corners
__constant__ int8_t k_nb[13][3] = {{-1, 0, 0},  {0, -1, 0},  {0, 0, -1},                                        // faces
                                   {-1, -1, 0}, {-1, 1, 0},  {-1, 0, -1}, {-1, 0, 1}, {0, -1, -1}, {0, -1, 1},  // edges
                                   {-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}};                        // corners

// mode 0: non-zero voxels, equal values connect (multi-class, as skimage label); mode 1: voxels <= 0, all connect
__device__ __forceinline__ bool ccl_fg(int v, int mode) { return mode == 0 ? v != 0 : v <= 0; }
__device__ __forceinline__ bool ccl_same(int a, int b, int mode) { return mode == 0 ? a == b : true; }

__device__ __forceinline__ int lds_load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int agent_load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ int find_lds(int* lp, int a) {
  for (int s = 0; s < CCL_TILE; ++s) {
    const int p = lds_load(&lp[a]);
    if (p == a) return a;
    a = p;
  }
  return -1;
}

// hang the larger root under the smaller; false when a bound was hit
__device__ bool unite_lds(int* lp, int a, int b) {
  for (int it = 0; it < CCL_TILE; ++it) {
    a = find_lds(lp, a);
    b = find_lds(lp, b);
    if (a < 0 || b < 0) return false;
    if (a == b) return true;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&lp[a], b);
    if (old == a) return true;
    a = old;   // a had been linked meanwhile: unite what it was linked to with b
  }
  return false;
}

__device__ int find_global(int* par, int a) {
  const int start = a;
  int steps = 0;
  for (; steps < FIND_BOUND; ++steps) {
    const int p = agent_load(&par[a]);
    if (p == a) break;
    a = p;
  }
  if (steps == FIND_BOUND) return -1;
  if (steps > 1) {   // path compression: a root found is <= every entry on the path, so atomicMin keeps it a forest
    int b = start;
    for (int s = 0; s < steps && b != a; ++s) {
      const int old = atomicMin(&par[b], a);
      b = old;
    }
  }
  return a;
}

__device__ bool unite_global(int* par, int a, int b) {
  for (int it = 0; it < FIND_BOUND; ++it) {
    a = find_global(par, a);
    b = find_global(par, b);
    if (a < 0 || b < 0) return false;
    if (a == b) return true;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&par[a], b);
    if (old == a) return true;
    a = old;
  }
  return false;
}

__global__ __launch_bounds__(CCL_NT) void ccl_local_kernel(const int* __restrict__ x, int* __restrict__ par, Vol v,
                                                           int mode, int nnb, int* err) {
  __shared__ int key[CCL_TILE];
  __shared__ int lp[CCL_TILE];
  // tiles in one flat index (x fastest), walked grid-stride: any volume below 2^31 voxels fits a 1-D grid
  const int64_t ntx = (v.W + CCL_TX - 1) / CCL_TX, nty = (v.H + CCL_TY - 1) / CCL_TY;
  const int64_t ntiles = ntx * nty * ((v.D + CCL_TZ - 1) / CCL_TZ);
  bool ok = true;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int x0 = (int)(tile % ntx) * CCL_TX, y0 = (int)((tile / ntx) % nty) * CCL_TY;
    const int z0 = (int)(tile / (ntx * nty)) * CCL_TZ;
    for (int i = threadIdx.x; i < CCL_TILE; i += CCL_NT) {
      const int gz = z0 + (i >> 9), gy = y0 + ((i >> 6) & 7), gx = x0 + (i & 63);
      const bool in = gz < v.D && gy < v.H && gx < v.W;
      const int val = in ? x[((int64_t)gz * v.H + gy) * v.W + gx] : 0;
      key[i] = val;
      lp[i] = in && ccl_fg(val, mode) ? i : -1;   // the sign never changes: lp[j] >= 0 <=> j is foreground
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CCL_TILE; i += CCL_NT) {
      if (lds_load(&lp[i]) < 0) continue;
      const int lz = i >> 9, ly = (i >> 6) & 7, lx = i & 63;
      for (int k = 0; k < nnb; ++k) {
        const int nz = lz + k_nb[k][0], ny = ly + k_nb[k][1], nx = lx + k_nb[k][2];
        if (nz < 0 || ny < 0 || ny >= CCL_TY || nx < 0 || nx >= CCL_TX) continue;   // another tile: pass B
        const int j = (nz << 9) | (ny << 6) | nx;
        if (lds_load(&lp[j]) >= 0 && ccl_same(key[i], key[j], mode)) ok &= unite_lds(lp, i, j);
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CCL_TILE; i += CCL_NT) {
      const int gz = z0 + (i >> 9), gy = y0 + ((i >> 6) & 7), gx = x0 + (i & 63);
      if (gz >= v.D || gy >= v.H || gx >= v.W) continue;
      int r = lp[i];
      if (r >= 0) {
        r = find_lds(lp, i);
        if (r < 0) { ok = false; r = i; }
        r = (int)(((int64_t)(z0 + (r >> 9)) * v.H + y0 + ((r >> 6) & 7)) * v.W + x0 + (r & 63));
      }
      par[((int64_t)gz * v.H + gy) * v.W + gx] = r;
    }
    __syncthreads();   // the next tile reuses key / lp
  }
  if (!ok) atomicOr(err, 1);
}

__global__ __launch_bounds__(CCL_NT) void ccl_merge_kernel(const int* __restrict__ x, int* par, Vol v, int mode, int nnb,
                                                           int* err) {
  const int64_t nvox = (int64_t)v.D * v.H * v.W;
  bool ok = true;
  for (int64_t g = blockIdx.x * (int64_t)CCL_NT + threadIdx.x; g < nvox; g += (int64_t)gridDim.x * CCL_NT) {
    const int gx = (int)(g % v.W), gy = (int)((g / v.W) % v.H), gz = (int)(g / ((int64_t)v.W * v.H));
    const int lz = gz & (CCL_TZ - 1), ly = gy & (CCL_TY - 1), lx = gx & (CCL_TX - 1);
    if (lz != 0 && ly != 0 && ly != CCL_TY - 1 && lx != 0 && lx != CCL_TX - 1) continue;   // no neighbour in another tile
    const int val = x[g];
    if (!ccl_fg(val, mode)) continue;
    for (int k = 0; k < nnb; ++k) {
      const int nz = gz + k_nb[k][0], ny = gy + k_nb[k][1], nx = gx + k_nb[k][2];
      if (nz < 0 || ny < 0 || ny >= v.H || nx < 0 || nx >= v.W) continue;
      if ((nz >> 3) == (gz >> 3) && (ny >> 3) == (gy >> 3) && (nx >> 6) == (gx >> 6)) continue;   // same tile: pass A
      const int64_t n = ((int64_t)nz * v.H + ny) * v.W + nx;
      const int nv = x[n];
      if (ccl_fg(nv, mode) && ccl_same(val, nv, mode)) ok &= unite_global(par, (int)g, (int)n);
    }
  }
  if (!ok) atomicOr(err, 2);
}

// block-wide exclusive scan of one int per thread (NT a multiple of 64); `sh` holds NT/64 + 1 ints; total -> *total
template <int NT>
__device__ int block_exclusive_scan(int val, int* sh, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = val;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(inc, off, 64);
    if (lane >= off) inc += t;
  }
  __syncthreads();
  if (lane == 63) sh[w] = inc;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int i = 0; i < NT / 64; ++i) { const int t = sh[i]; sh[i] = run; run += t; }
    sh[NT / 64] = run;
  }
  __syncthreads();
  *total = sh[NT / 64];
  return sh[w] + inc - val;
}

// par[g] = root of g; cnt[chunk] = roots in the chunk
__global__ __launch_bounds__(CCL_NT) void ccl_flatten_kernel(int* par, int64_t nvox, int* __restrict__ cnt, int* err) {
  __shared__ int sh[CCL_NT / 64 + 1];
  const int64_t base = (int64_t)blockIdx.x * CHUNK;
  int roots = 0;
  bool ok = true;
  for (int k = 0; k < CHUNK_VPT; ++k) {
    const int64_t g = base + k * CCL_NT + threadIdx.x;
    if (g >= nvox) break;
    int a = par[g];
    if (a < 0) continue;
    int s = 0;
    for (; s < FIND_BOUND; ++s) {
      const int p = par[a];   // any value read, stale or not, is an ancestor: plain loads suffice after pass B
      if (p == a) break;
      a = p;
    }
    if (s == FIND_BOUND) { ok = false; continue; }
    if (a == g) ++roots;
    else par[g] = a;
  }
  int total;
  block_exclusive_scan<CCL_NT>(roots, sh, &total);
  if (threadIdx.x == 0) cnt[blockIdx.x] = total;
  if (!ok) atomicOr(err, 4);
}

// one workgroup: cnt[0..nb) -> exclusive offsets; *n_out = number of components, or -1 when a bound was hit
__global__ __launch_bounds__(1024) void ccl_scan_kernel(int* cnt, int nb, const int* err, int* n_out) {
  __shared__ int sh[1024 / 64 + 1];
  int carry = 0;
  for (int b0 = 0; b0 < nb; b0 += 1024) {
    const int i = b0 + threadIdx.x;
    const int c = i < nb ? cnt[i] : 0;
    int total;
    const int ex = block_exclusive_scan<1024>(c, sh, &total);
    if (i < nb) cnt[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) *n_out = *err ? -1 : carry;
}

// roots (par[g] == g) take numbers in raster order: thread t owns the 16 contiguous voxels [base + 16 t, +16)
__global__ __launch_bounds__(CCL_NT) void ccl_number_kernel(const int* __restrict__ par, int64_t nvox,
                                                            const int* __restrict__ off, int* __restrict__ labels) {
  __shared__ int sh[CCL_NT / 64 + 1];
  const int64_t base = (int64_t)blockIdx.x * CHUNK + (int64_t)threadIdx.x * CHUNK_VPT;
  int mask = 0;
  for (int k = 0; k < CHUNK_VPT; ++k) {
    const int64_t g = base + k;
    if (g < nvox && par[g] == g) mask |= 1 << k;
  }
  int total;
  int num = off[blockIdx.x] + block_exclusive_scan<CCL_NT>(__popc(mask), sh, &total) + 1;
  for (int k = 0; k < CHUNK_VPT; ++k)
    if (mask >> k & 1) labels[base + k] = num++;
}

__global__ __launch_bounds__(CCL_NT) void ccl_relabel_kernel(const int* __restrict__ par, int64_t nvox, int* labels) {
  for (int64_t g = blockIdx.x * (int64_t)CCL_NT + threadIdx.x; g < nvox; g += (int64_t)gridDim.x * CCL_NT) {
    const int p = par[g];
    if (p < 0) labels[g] = 0;
    else if (p != g) labels[g] = labels[p];   // roots were numbered by the previous launch
  }
}

// ---- histograms: LDS hash per workgroup, one global atomic per distinct bin and workgroup (plus probe overflow) ----
__device__ __forceinline__ void hash_add(int* hkey, unsigned* hcnt, unsigned long long* counts, int bin, unsigned n) {
  int h = (int)(((unsigned)bin * 2654435761u) >> 22) & (HASH_SLOTS - 1);
  for (int p = 0; p < HASH_PROBES; ++p) {
    const int k = atomicCAS(&hkey[h], -1, bin);
    if (k == -1 || k == bin) {
      atomicAdd(&hcnt[h], n);
      return;
    }
    h = (h + 1) & (HASH_SLOTS - 1);
  }
  atomicAdd(&counts[bin], (unsigned long long)n);
}

// counts[key - lo] += 1 for every voxel whose key is in [lo, lo + nbins): key = a (b == null) or a * bstride + b.
// minmax (1-D only, may be null): atomicMin / atomicMax of every a.  Thread t of a chunk owns 16 contiguous voxels
// and hands runs of one key to the hash as one add.
__global__ __launch_bounds__(CCL_NT) void hist_kernel(const int* __restrict__ a, const int* __restrict__ b, int64_t nvox,
                                                      int64_t bstride, int64_t lo, int64_t nbins,
                                                      unsigned long long* counts, int* minmax) {
  __shared__ int hkey[HASH_SLOTS];
  __shared__ unsigned hcnt[HASH_SLOTS];
  __shared__ int shmin[CCL_NT / 64], shmax[CCL_NT / 64];
  for (int i = threadIdx.x; i < HASH_SLOTS; i += CCL_NT) { hkey[i] = -1; hcnt[i] = 0; }
  __syncthreads();
  int vmin = 0x7fffffff, vmax = (int)0x80000000;
  const int64_t nchunks = (nvox + CHUNK - 1) / CHUNK;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t base = c * CHUNK + (int64_t)threadIdx.x * CHUNK_VPT;
    int64_t run_bin = -1;
    unsigned run = 0;
    for (int k = 0; k < CHUNK_VPT; ++k) {
      const int64_t g = base + k;
      if (g >= nvox) break;
      const int av = a[g];
      vmin = min(vmin, av);
      vmax = max(vmax, av);
      const int64_t key = (b ? (int64_t)av * bstride + b[g] : (int64_t)av) - lo;
      const int64_t bin = key >= 0 && key < nbins ? key : -1;
      if (bin != run_bin) {
        if (run_bin >= 0) hash_add(hkey, hcnt, counts, (int)run_bin, run);
        run_bin = bin;
        run = 0;
      }
      ++run;
    }
    if (run_bin >= 0) hash_add(hkey, hcnt, counts, (int)run_bin, run);
  }
  if (minmax) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      vmin = min(vmin, __shfl_xor(vmin, off, 64));
      vmax = max(vmax, __shfl_xor(vmax, off, 64));
    }
    if ((threadIdx.x & 63) == 0) { shmin[threadIdx.x >> 6] = vmin; shmax[threadIdx.x >> 6] = vmax; }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < HASH_SLOTS; i += CCL_NT)
    if (hkey[i] >= 0) atomicAdd(&counts[hkey[i]], (unsigned long long)hcnt[i]);
  if (minmax && threadIdx.x == 0) {
    for (int w = 1; w < CCL_NT / 64; ++w) { vmin = min(vmin, shmin[w]); vmax = max(vmax, shmax[w]); }
    atomicMin(&minmax[0], vmin);
    atomicMax(&minmax[1], vmax);
  }
}

__global__ void hist_init_kernel(unsigned long long* counts, int64_t nbins, int* minmax) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nbins; i += (int64_t)gridDim.x * blockDim.x) counts[i] = 0;
  if (minmax && blockIdx.x == 0 && threadIdx.x == 0) { minmax[0] = 0x7fffffff; minmax[1] = (int)0x80000000; }
}

// ---- masked 6-neighbour grey dilation (Jacobi: reads src, writes dst) ----
// voxel v is masked when flag[labels[v]] != 0.  Raw mode (class_rank == null): masked voxels take the maximum of src
// over v and its 6 neighbours.  Rank mode: the key of a voxel is 0 when it is masked, else class_rank[src - lo]; a
// masked voxel whose neighbourhood maximum key K is > 0 takes rank_class[K].  Unmasked voxels are copied.
__global__ __launch_bounds__(CCL_NT) void dilate6_kernel(const int* __restrict__ src, int* __restrict__ dst, Vol v,
                                                         const int* __restrict__ labels, const int* __restrict__ flag,
                                                         const int* __restrict__ class_rank, const int* __restrict__ rank_class,
                                                         int lo, unsigned long long* changed) {
  __shared__ int sh[CCL_NT / 64];
  const int64_t nvox = (int64_t)v.D * v.H * v.W, HW = (int64_t)v.H * v.W;
  int nchg = 0;
  for (int64_t g = blockIdx.x * (int64_t)CCL_NT + threadIdx.x; g < nvox; g += (int64_t)gridDim.x * CCL_NT) {
    const int s = src[g];
    int out = s;
    if (flag[labels[g]]) {
      const int gx = (int)(g % v.W), gy = (int)((g / v.W) % v.H), gz = (int)(g / HW);
      int64_t nb[6];
      int cnt = 0;
      if (gz > 0) nb[cnt++] = g - HW;
      if (gz < v.D - 1) nb[cnt++] = g + HW;
      if (gy > 0) nb[cnt++] = g - v.W;
      if (gy < v.H - 1) nb[cnt++] = g + v.W;
      if (gx > 0) nb[cnt++] = g - 1;
      if (gx < v.W - 1) nb[cnt++] = g + 1;
      if (class_rank) {
        int kmax = 0;
        for (int i = 0; i < cnt; ++i)
          if (!flag[labels[nb[i]]]) kmax = max(kmax, class_rank[src[nb[i]] - lo]);
        if (kmax > 0) out = rank_class[kmax];
      } else {
        for (int i = 0; i < cnt; ++i) out = max(out, src[nb[i]]);
      }
    }
    dst[g] = out;
    nchg += out != s;
  }
  const int total = block_sum<int, CCL_NT>(nchg, sh);
  if (threadIdx.x == 0 && total) atomicAdd(changed, (unsigned long long)total);
}

// ---- dtype conversion at the boundary (codes: 0 uint8 / bool, 1 int8, 2 int16, 3 int32, 4 int64) ----
__device__ __forceinline__ int64_t load_any(const void* p, int dt, int64_t i) {
  switch (dt) {
    case 0: return ((const uint8_t*)p)[i];
    case 1: return ((const int8_t*)p)[i];
    case 2: return ((const int16_t*)p)[i];
    case 3: return ((const int32_t*)p)[i];
    default: return ((const int64_t*)p)[i];
  }
}
__device__ __forceinline__ void store_any(void* p, int dt, int64_t i, int64_t v) {
  switch (dt) {
    case 0: ((uint8_t*)p)[i] = (uint8_t)v; break;
    case 1: ((int8_t*)p)[i] = (int8_t)v; break;
    case 2: ((int16_t*)p)[i] = (int16_t)v; break;
    case 3: ((int32_t*)p)[i] = (int32_t)v; break;
    default: ((int64_t*)p)[i] = v; break;
  }
}

// op 0: dst = src (int64 values outside int32 set *status); 1: dst = (src == 0); 2: dst = (src > 0)
__global__ __launch_bounds__(CCL_NT) void convert_in_kernel(const void* src, int dt, int op, int* __restrict__ dst,
                                                            int64_t n, int* status) {
  bool bad = false;
  for (int64_t i = blockIdx.x * (int64_t)CCL_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * CCL_NT) {
    const int64_t v = load_any(src, dt, i);
    bad |= v != (int64_t)(int32_t)v;
    dst[i] = op == 0 ? (int)v : op == 1 ? (v == 0) : (v > 0);
  }
  if (bad && op == 0) atomicOr(status, 1);
}

// dst = zero_where ? (zero_where[i] ? 0 : orig[i]) : src[i], stored as dtype dt
__global__ __launch_bounds__(CCL_NT) void convert_out_kernel(const int* __restrict__ src, const int* __restrict__ zero_where,
                                                             const void* orig, void* dst, int dt, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)CCL_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * CCL_NT)
    store_any(dst, dt, i, zero_where ? (zero_where[i] ? 0 : load_any(orig, dt, i)) : (int64_t)src[i]);
}

static unsigned grid_for(int64_t n, int64_t cap = 8192) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, CCL_NT), cap));
}

static int check_vol(const char* who, int32_t D, int32_t H, int32_t W) {
  M355_REQUIRE(D > 0 && H > 0 && W > 0, M355_EINVALID_ARG, "%s: non-positive size %d x %d x %d", who, D, H, W);
  M355_REQUIRE((int64_t)D * H * W < ((int64_t)1 << 31), M355_EINVALID_ARG,
               "%s: %d x %d x %d has 2^31 voxels or more (labels are int32)", who, D, H, W);
  return M355_OK;
}

struct CclWs {
  int* par;
  int* cnt;
  int* err;
  int64_t nchunks;
  size_t bytes;
};
static CclWs ccl_ws_layout(void* base, int64_t nvox) {
  CclWs w{};
  w.nchunks = ceil_div(nvox, CHUNK);
  char* p = (char*)base;
  const size_t par_b = (size_t)round_up(nvox * 4, 256), cnt_b = (size_t)round_up(w.nchunks * 4, 256);
  w.par = (int*)p;
  w.cnt = (int*)(p + par_b);
  w.err = (int*)(p + par_b + cnt_b);
  w.bytes = par_b + cnt_b + 256;
  return w;
}

}  // namespace m355

using namespace m355;

extern "C" size_t m355_ccl_workspace(int32_t D, int32_t H, int32_t W) {
  if (check_vol("ccl_workspace", D, H, W)) return 0;
  return ccl_ws_layout(nullptr, (int64_t)D * H * W).bytes;
}

extern "C" int m355_ccl_label(const int32_t* x, int32_t* labels, int32_t* n_out, int32_t D, int32_t H, int32_t W,
                              int32_t connectivity, int32_t mode, void* workspace, size_t ws_bytes, void* stream) {
  if (int rc = check_vol("ccl_label", D, H, W)) return rc;
  M355_REQUIRE(connectivity >= 1 && connectivity <= 3, M355_EINVALID_ARG,
               "ccl_label: connectivity %d not in {1, 2, 3} (6, 18, 26 neighbours)", connectivity);
  M355_REQUIRE(mode == 0 || mode == 1, M355_EINVALID_ARG, "ccl_label: mode %d not in {0, 1}", mode);
  M355_REQUIRE(x && labels && n_out && workspace, M355_EINVALID_ARG, "ccl_label: null pointer");
  const int64_t nvox = (int64_t)D * H * W;
  const CclWs w = ccl_ws_layout(workspace, nvox);
  M355_REQUIRE(ws_bytes >= w.bytes, M355_EWORKSPACE, "ccl_label: workspace %zu < %zu bytes", ws_bytes, w.bytes);
  hipStream_t st = (hipStream_t)stream;
  const Vol v{D, H, W};
  const int nnb = connectivity == 1 ? 3 : connectivity == 2 ? 9 : 13;
  if (hipMemsetAsync(w.err, 0, sizeof(int), st) != hipSuccess) return check_launch("ccl_label: memset");
  const int64_t ntiles = ceil_div(W, CCL_TX) * ceil_div(H, CCL_TY) * ceil_div(D, CCL_TZ);
  hipLaunchKernelGGL(ccl_local_kernel, dim3((unsigned)std::min<int64_t>(ntiles, 1 << 20)), dim3(CCL_NT), 0, st, x, w.par, v,
                     mode, nnb, w.err);
  hipLaunchKernelGGL(ccl_merge_kernel, dim3(grid_for(nvox)), dim3(CCL_NT), 0, st, x, w.par, v, mode, nnb, w.err);
  hipLaunchKernelGGL(ccl_flatten_kernel, dim3(w.nchunks), dim3(CCL_NT), 0, st, w.par, nvox, w.cnt, w.err);
  hipLaunchKernelGGL(ccl_scan_kernel, dim3(1), dim3(1024), 0, st, w.cnt, (int)w.nchunks, w.err, n_out);
  hipLaunchKernelGGL(ccl_number_kernel, dim3(w.nchunks), dim3(CCL_NT), 0, st, w.par, nvox, w.cnt, labels);
  hipLaunchKernelGGL(ccl_relabel_kernel, dim3(grid_for(nvox)), dim3(CCL_NT), 0, st, w.par, nvox, labels);
  return check_launch("ccl_label");
}

extern "C" int m355_label_histogram(const int32_t* a, const int32_t* b, int64_t nvox, int64_t bstride, int64_t lo,
                                    int64_t nbins, int64_t* counts, int32_t* minmax, void* stream) {
  M355_REQUIRE(a && counts && nvox > 0 && nvox < ((int64_t)1 << 31), M355_EINVALID_ARG,
               "label_histogram: null pointer or voxel count %lld outside [1, 2^31)", (long long)nvox);
  M355_REQUIRE(nbins > 0 && nbins <= ((int64_t)1 << 31) - 1, M355_EINVALID_ARG, "label_histogram: %lld bins",
               (long long)nbins);
  M355_REQUIRE(!b || bstride > 0, M355_EINVALID_ARG, "label_histogram: two-map keys need bstride > 0");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(hist_init_kernel, dim3(grid_for(nbins, 4096)), dim3(CCL_NT), 0, st, (unsigned long long*)counts, nbins,
                     (int*)minmax);
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(nvox, CHUNK), 2048));
  hipLaunchKernelGGL(hist_kernel, dim3(grid), dim3(CCL_NT), 0, st, a, b, nvox, bstride, lo, nbins,
                     (unsigned long long*)counts, (int*)minmax);
  return check_launch("label_histogram");
}

extern "C" int m355_masked_dilate6(const int32_t* src, int32_t* dst, int32_t D, int32_t H, int32_t W,
                                   const int32_t* labels, const int32_t* flag, const int32_t* class_rank,
                                   const int32_t* rank_class, int32_t lo, int64_t* changed, void* stream) {
  if (int rc = check_vol("masked_dilate6", D, H, W)) return rc;
  M355_REQUIRE(src && dst && labels && flag && changed && src != dst, M355_EINVALID_ARG,
               "masked_dilate6: null pointer, or src == dst (the pass reads one snapshot and writes another buffer)");
  M355_REQUIRE(!class_rank == !rank_class, M355_EINVALID_ARG, "masked_dilate6: class_rank and rank_class go together");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(changed, 0, sizeof(int64_t), st) != hipSuccess) return check_launch("masked_dilate6: memset");
  const int64_t nvox = (int64_t)D * H * W;
  hipLaunchKernelGGL(dilate6_kernel, dim3(grid_for(nvox)), dim3(CCL_NT), 0, st, src, dst, Vol{D, H, W}, labels, flag,
                     class_rank, rank_class, lo, (unsigned long long*)changed);
  return check_launch("masked_dilate6");
}

extern "C" int m355_label_convert_in(const void* src, int32_t dtype, int32_t op, int32_t* dst, int64_t n,
                                     int32_t* status, void* stream) {
  M355_REQUIRE(src && dst && status && n > 0, M355_EINVALID_ARG, "label_convert_in: null pointer or empty volume");
  M355_REQUIRE(dtype >= 0 && dtype <= 4 && op >= 0 && op <= 2, M355_EINVALID_ARG, "label_convert_in: dtype %d / op %d",
               dtype, op);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(status, 0, sizeof(int32_t), st) != hipSuccess) return check_launch("label_convert_in: memset");
  hipLaunchKernelGGL(convert_in_kernel, dim3(grid_for(n)), dim3(CCL_NT), 0, st, src, dtype, op, dst, n, status);
  return check_launch("label_convert_in");
}

extern "C" int m355_label_convert_out(const int32_t* src, const int32_t* zero_where, const void* orig, void* dst,
                                      int32_t dtype, int64_t n, void* stream) {
  M355_REQUIRE(dst && n > 0 && dtype >= 0 && dtype <= 4, M355_EINVALID_ARG, "label_convert_out: bad arguments");
  M355_REQUIRE(zero_where ? orig != nullptr : src != nullptr, M355_EINVALID_ARG, "label_convert_out: null source");
  hipLaunchKernelGGL(convert_out_kernel, dim3(grid_for(n)), dim3(CCL_NT), 0, (hipStream_t)stream, src, zero_where, orig,
                     dst, dtype, n);
  return check_launch("label_convert_out");
}
