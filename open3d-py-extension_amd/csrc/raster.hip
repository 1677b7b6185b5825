// raster.hip — the floor-map segmentation's device side (reference
// open3dpypro/PointCloud.py:785-823 to_2D_Img, :888-916
// simple_seg_connected_components[_by_img]):
//   1. rasterisation of a cloud's (x, y) onto a pixel grid (k_raster2d);
//   2. 8-connected component labelling of a uint8 image (k_ccl_*);
//   3. the points grouped by the label of their pixel (k_label_points + a
//      stable radix sort).
// include/o3dx.h states the rules.  The labelling is tile-local first: one
// workgroup labels a 64 x 64 tile in LDS and writes, per pixel, the global
// index of its tile-local root; only the pixels on the tiles' left columns and
// top rows then touch the global union-find (unionfind.hpp), and the areas are
// summed from the tiles' local counts, one add per (tile, component).  A floor map is a few
// huge blobs: a global union-find over every pixel would send every pixel of a
// blob down one tree (profiles/dbscan_time.txt: 19-32 ms at 2M elements).
//
// The tile: 64 columns = one wave64 per row, so a row's occupancy is one
// ballot (a 64-bit mask) and a pixel's horizontal run is two bit scans of it,
// with no LDS traffic; 64 rows = 16 per wave of the 256-thread workgroup.  The
// LDS union-find has one node per run (its first pixel); a run links to the
// runs of the row above it overlaps (W is inside the run; N, NW, NE).  LDS:
// 16 KiB of nodes + 16 KiB of counts + 512 B of row masks, 4 workgroups per CU.
//
// Integer atomics only; nothing depends on launch order: every root is the
// smallest row-major index of its component (links go from the larger index to
// the smaller), the labels are the ranks of the roots.
#include <hipcub/hipcub.hpp>

#include "unionfind.hpp"

namespace o3dx {

// ------------------------------------------------------------ rasterisation
struct RasterParams {
  double ir, tx, ty;  // ix = rint(x * ir + tx), the product and the sum rounded separately
  int w, h;
};

// The reference's size: max over the points of rint(x * ir + tx); both maps are
// monotone, so it is the image of the bounds' maximum.
static int raster_params(const char* who, double resolution, const double* b, RasterParams* P, int64_t* w, int64_t* h) {
  if (!(resolution > 0.0) || !std::isfinite(resolution))
    return fail(O3DX_EINVAL, "%s: resolution must be finite and > 0", who);
  if (!b) return fail(O3DX_EINVAL, "%s: null bounds_host", who);
  for (int a = 0; a < 4; ++a)
    if (!std::isfinite(b[a])) return fail(O3DX_EINVAL, "%s: bounds must be finite", who);
  if (b[2] < b[0] || b[3] < b[1]) return fail(O3DX_EINVAL, "%s: bounds max below min", who);
  P->ir = 1.0 / resolution;
  P->tx = P->ir * (-b[0]);
  P->ty = P->ir * (-b[1]);
  const double px = b[2] * P->ir;
  const double py = b[3] * P->ir;
  const double sx = std::rint(px + P->tx), sy = std::rint(py + P->ty);
  if (!(sx < 2147483648.0) || !(sy < 2147483648.0) || !(sx * sy < 2147483648.0))
    return fail(O3DX_ENOTSUP, "%s: image %.0f x %.0f has 2^31 pixels or more", who, sx, sy);
  *w = (int64_t)sx;
  *h = (int64_t)sy;
  P->w = (int)*w;
  P->h = (int)*h;
  return 0;
}

// rint(v * ir + t) clamped to [0, size - 1]; a NaN lands on 0 (never outside)
__device__ __forceinline__ int raster_coord(double v, double ir, double t, int size) {
  const double p = v * ir;
  double r = rint(p + t);
  if (!(r >= 0.0)) r = 0.0;
  if (r > (double)(size - 1)) r = (double)(size - 1);
  return (int)r;
}

__global__ void __launch_bounds__(kBlock) k_raster_clear(uint8_t* __restrict__ img, int32_t* __restrict__ winner,
                                                         int64_t npx) {
  grid_zero(img, (size_t)npx);
  if (winner)
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npx; p += (int64_t)gridDim.x * blockDim.x)
      winner[p] = -1;
}

template <bool F64>
__global__ void __launch_bounds__(kBlock) k_raster2d(const typename std::conditional<F64, double, float>::type* __restrict__ xyz,
                                                     int64_t n, RasterParams P, int32_t* __restrict__ pix,
                                                     uint8_t* __restrict__ img, int32_t* winner) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const double x = (double)xyz[3 * i], y = (double)xyz[3 * i + 1];
  const int ix = raster_coord(x, P.ir, P.tx, P.w), iy = raster_coord(y, P.ir, P.ty, P.h);
  pix[2 * i] = ix;
  pix[2 * i + 1] = iy;
  const int64_t p = (int64_t)iy * P.w + ix;
  img[p] = 255;  // racing stores carry the same value
  if (winner) atomicMax(winner + p, (int)i);
}

template <bool F64, class T>
static int raster_run(const char* who, const T* xyz, int64_t n, double resolution, const double* bounds,
                      int32_t* pix, uint8_t* img, int32_t* winner, int64_t img_cap, void* stream) {
  if (n <= 0 || n >= ((int64_t)1 << 31)) return fail(O3DX_EINVAL, "%s: n = %lld outside [1, 2^31)", who, (long long)n);
  if (!xyz || !pix || !img) return fail(O3DX_EINVAL, "%s: null points, pix or img", who);
  RasterParams P;
  int64_t w, h;
  O3DX_TRY(raster_params(who, resolution, bounds, &P, &w, &h));
  if (w < 1 || h < 1) return fail(O3DX_EINVAL, "%s: empty image (%lld x %lld)", who, (long long)w, (long long)h);
  if (img_cap < w * h)
    return fail(O3DX_ENOMEM, "%s: image buffer too small: need %lld pixels, have %lld", who, (long long)(w * h),
                (long long)img_cap);
  hipStream_t s = as_stream(stream);
  KTimer kt("raster2d", s);
  hipLaunchKernelGGL(k_raster_clear, dim3(grid_for(w * h / 16 + 1, kBlock, 4096)), dim3(kBlock), 0, s, img, winner,
                     w * h);
  hipLaunchKernelGGL(k_raster2d<F64>, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, xyz, n, P, pix,
                     img, winner);
  O3DX_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------- connected components
constexpr int kTW = 64, kTH = 64, kTilePx = kTW * kTH;
constexpr int kTileRowsPerWave = kTH / (kBlock / 64);

// bit x of m is set: the first position of its run of set bits
__device__ __forceinline__ int run_start(uint64_t m, int x) {
  const uint64_t below = x == 0 ? 0ull : (~m & (~0ull >> (64 - x)));
  return below ? 64 - __clzll((long long)below) : 0;
}
// ... and one past its last position
__device__ __forceinline__ int run_end(uint64_t m, int x) {
  const uint64_t z = ~m >> x;
  return z ? x + __ffsll((unsigned long long)z) - 1 : 64;
}

// The tile's union-find in LDS: the same rules as unionfind.hpp (links from
// the larger index to the smaller, bounded loops), workgroup scope.
__device__ __forceinline__ int luf_load(const int* lab, int x) {
  return __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ int luf_find(const int* lab, int x, int* err) {
  for (int it = 0; it <= kTilePx; ++it) {
    const int p = luf_load(lab, x);
    if (p >= x) {
      if (p > x) atomicOr(err, 1);
      return x;
    }
    x = p;
  }
  atomicOr(err, 1);
  return x;
}
__device__ __forceinline__ void luf_unite(int* lab, int a, int b, int* err) {
  for (int it = 0; it <= 2 * kTilePx; ++it) {
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicCAS(lab + a, a, b);
    if (old == a) return;
    if (old > a) {
      atomicOr(err, 1);
      return;
    }
    a = old;
  }
  atomicOr(err, 1);
}

// One workgroup per tile, a wave per row, a lane per pixel.  parent[p]: the
// global index of p's tile-local root (p itself for a background pixel);
// cnt[p]: the local component's pixel count at its local root, 0 elsewhere.
__global__ void __launch_bounds__(kBlock) k_ccl_tile(const uint8_t* __restrict__ img, int w, int h, int ntx,
                                                     int32_t* __restrict__ parent, int32_t* __restrict__ cnt,
                                                     int* err) {
  __shared__ int lab[kTilePx];
  __shared__ int cn[kTilePx];
  __shared__ uint64_t rmask[kTH];
  const int tx0 = (int)(blockIdx.x % (unsigned)ntx) * kTW, ty0 = (int)(blockIdx.x / (unsigned)ntx) * kTH;
  const int lane = threadIdx.x & 63, row0 = (threadIdx.x >> 6) * kTileRowsPerWave;
  const int gx = tx0 + lane;

  // the rows' masks; a pixel starts at the first pixel of its run
  for (int k = 0; k < kTileRowsPerWave; ++k) {
    const int row = row0 + k, gy = ty0 + row;
    const bool fg = gx < w && gy < h && img[(int64_t)gy * w + gx] != 0;
    const uint64_t m = __ballot(fg);
    if (lane == 0) rmask[row] = m;
    const int p = row * kTW + lane;
    lab[p] = fg ? row * kTW + run_start(m, lane) : p;
    cn[p] = 0;
  }
  __syncthreads();

  // runs against the runs of the row above: every 8-adjacent pair (x, q) of
  // the two rows ends up connected — (x, x) links unless (x-1, x-1) is a pair
  // of the same two runs; a diagonal links only when neither the pixel above
  // nor the pixel beside x makes it a consequence of a straight pair
  for (int k = 0; k < kTileRowsPerWave; ++k) {
    const int row = row0 + k;
    if (row == 0) continue;
    const uint64_t m = rmask[row], up = rmask[row - 1];
    if (!((m >> lane) & 1)) continue;
    const bool c_w = lane > 0 && ((m >> (lane - 1)) & 1), c_e = lane < 63 && ((m >> (lane + 1)) & 1);
    const bool u_c = (up >> lane) & 1, u_w = lane > 0 && ((up >> (lane - 1)) & 1),
               u_e = lane < 63 && ((up >> (lane + 1)) & 1);
    const int me = row * kTW + run_start(m, lane);
    auto link = [&](int q) {
      const int a = luf_find(lab, me, err);
      const int b = luf_find(lab, (row - 1) * kTW + run_start(up, q), err);
      if (a != b) luf_unite(lab, a, b, err);
    };
    if (u_c) {
      if (!c_w || !u_w) link(lane);
    } else {
      if (u_w && !c_w) link(lane - 1);
      if (u_e && !c_e) link(lane + 1);
    }
  }
  __syncthreads();

  // a run's first lane: the run's root (stored over its link: still an
  // ancestor for every concurrent find) and the run's length into the root's count
  for (int k = 0; k < kTileRowsPerWave; ++k) {
    const int row = row0 + k;
    const uint64_t m = rmask[row];
    if (!((m >> lane) & 1) || (lane > 0 && ((m >> (lane - 1)) & 1))) continue;
    const int p = row * kTW + lane;
    const int r = luf_find(lab, p, err);
    __hip_atomic_store(lab + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    atomicAdd(cn + r, run_end(m, lane) - lane);
  }
  __syncthreads();

  for (int k = 0; k < kTileRowsPerWave; ++k) {
    const int row = row0 + k, gy = ty0 + row;
    if (gx >= w || gy >= h) continue;
    const uint64_t m = rmask[row];
    const int p = row * kTW + lane;
    const int g = gy * w + gx;
    if ((m >> lane) & 1) {
      const int r = lab[row * kTW + run_start(m, lane)];
      parent[g] = (ty0 + r / kTW) * w + tx0 + r % kTW;
      cnt[g] = r == p ? cn[p] : 0;
    } else {
      parent[g] = g;
      cnt[g] = 0;
    }
  }
}

// The seams: a pixel on a tile's top row unites with N, or with NW and NE when
// N is empty (N set: NW and NE hang on N through the row above); a pixel on a
// tile's left column with W, or with NW and SW when W is empty (SW from here
// is NE from there).  Every 8-adjacent pair in two different tiles is one of
// these, or connected through one.
__global__ void __launch_bounds__(kBlock) k_ccl_seam(const uint8_t* __restrict__ img, int w, int h, int nsx, int nsy,
                                                     int32_t* parent, int* err) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t ncol = (int64_t)nsx * h, total = ncol + (int64_t)nsy * w;
  if (t >= total) return;
  const int64_t bound = 2 * (int64_t)w * h + 2;
  int x, y;
  bool col;
  if (t < ncol) {
    col = true;
    x = (int)(t % nsx + 1) * kTW;
    y = (int)(t / nsx);
  } else {
    col = false;
    x = (int)((t - ncol) % w);
    y = (int)((t - ncol) / w + 1) * kTH;
  }
  const int p = y * w + x;
  if (!img[p]) return;
  int ra = p;  // a member of p's component, its root when last seen
  auto link = [&](int q) {
    if (!img[q]) return false;
    const int rb = uf_find<true>(parent, q, bound, err);
    ra = uf_find<true>(parent, ra, bound, err);
    if (ra != rb) ra = uf_unite(parent, ra, rb, bound, err);
    return true;
  };
  if (col) {  // x >= kTW
    if (!link(p - 1)) {
      if (y > 0) link(p - w - 1);
      if (y + 1 < h) link(p + w - 1);
    }
  } else {  // y >= kTH
    if (!link(p - w)) {
      if (x > 0) link(p - w - 1);
      if (x + 1 < w) link(p - w + 1);
    }
  }
}

// Between the seams and the roots: every tile-local root (cnt > 0) finds its
// root, halving on the way, and points straight at it.  The pixels' finds of
// k_ccl_roots are then two or three hops instead of one walk per pixel down a
// blob's chain of tiles.  parent[i] only decreases to a member of i's tree and
// a root is never written: the union-find's invariants hold.
__global__ void __launch_bounds__(kBlock) k_ccl_compress(int64_t n, const int32_t* __restrict__ cnt, int32_t* parent,
                                                         int* err) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n || cnt[i] <= 0) return;
  const int r = uf_find<true>(parent, (int)i, 2 * n + 2, err);
  if (r < (int)i) atomicMin(parent + i, r);
}

// root[p] = find(p) in a launch of its own (parent[] is final and only read),
// -1 for the background; flag[p] = p is a root
__global__ void __launch_bounds__(kBlock) k_ccl_roots(const uint8_t* __restrict__ img, int64_t n, const int32_t* parent,
                                                      int32_t* __restrict__ root, int32_t* __restrict__ flag,
                                                      int* err) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const bool fg = img[i] != 0;
  const int r = fg ? uf_find(parent, (int)i, n + 1, err) : -1;
  root[i] = r;
  flag[i] = r == (int)i ? 1 : 0;
}

// rank[n] = the number of components; areas[0] = n (the label pass subtracts
// the foreground), areas[1..] cleared lazily by k_ccl_areas_clear
__global__ void k_ccl_count(int64_t n, const int32_t* __restrict__ flag, int32_t* __restrict__ rank) {
  rank[n] = rank[n - 1] + flag[n - 1];
}

__global__ void __launch_bounds__(kBlock) k_ccl_areas_clear(int64_t* __restrict__ areas, int64_t k, int64_t n) {
  for (int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; l <= k; l += (int64_t)gridDim.x * blockDim.x)
    areas[l] = l == 0 ? n : 0;
}

// labels[p] (holding root[p]) -> rank[root] + 1, 0 for the background; the
// block's foreground total leaves areas[0] in one add
__global__ void __launch_bounds__(kBlock) k_ccl_label(int64_t n, const int32_t* __restrict__ rank,
                                                      int32_t* __restrict__ labels, int64_t* areas) {
  __shared__ int64_t sh[kBlock / 64];
  int64_t fgsum = 0;
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kBlock) {
    const int r = labels[p];
    const int l = r >= 0 ? rank[r] + 1 : 0;
    labels[p] = l;
    fgsum += r >= 0 ? 1 : 0;
  }
  fgsum = wave_sum(fgsum);  // after the loop: every lane of the wave is here
  if (lane_id() == 0) sh[threadIdx.x >> 6] = fgsum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t tot = 0;
    for (int v = 0; v < kBlock / 64; ++v) tot += sh[v];
    if (tot) atomicAdd(reinterpret_cast<unsigned long long*>(areas), (unsigned long long)(-tot));
  }
}

// The areas: a workgroup per tile sums its local components' counts by label
// in a small LDS table (open addressing; a label that finds no slot within
// kAreaProbes adds straight to memory) and adds each slot once: one integer
// add per (tile, component) — a blob through every tile otherwise receives one
// add per local component on one address (a 1-pixel serpentine through 8192^2:
// 524k adds, 7 ms).
constexpr int kAreaSlots = 1024, kAreaProbes = 32;
__global__ void __launch_bounds__(kBlock) k_ccl_areas(int w, int h, int ntx, const int32_t* __restrict__ cnt,
                                                      const int32_t* __restrict__ labels, int64_t* areas) {
  __shared__ int key[kAreaSlots];
  __shared__ int val[kAreaSlots];
  for (int s = threadIdx.x; s < kAreaSlots; s += kBlock) {
    key[s] = 0;  // labels start at 1
    val[s] = 0;
  }
  __syncthreads();
  const int tx0 = (int)(blockIdx.x % (unsigned)ntx) * kTW, ty0 = (int)(blockIdx.x / (unsigned)ntx) * kTH;
  const int lane = threadIdx.x & 63, row0 = (threadIdx.x >> 6) * kTileRowsPerWave;
  const int gx = tx0 + lane;
  for (int k = 0; k < kTileRowsPerWave; ++k) {
    const int gy = ty0 + row0 + k;
    if (gx >= w || gy >= h) continue;
    const int g = gy * w + gx;
    const int c = cnt[g];
    if (c <= 0) continue;
    const int l = labels[g];
    const unsigned h0 = ((unsigned)l * 2654435761u) >> 22;
    bool done = false;
    for (int t = 0; t < kAreaProbes && !done; ++t) {
      const int s = (int)((h0 + t) & (kAreaSlots - 1));
      const int old = atomicCAS(key + s, 0, l);
      if (old == 0 || old == l) {
        atomicAdd(val + s, c);
        done = true;
      }
    }
    if (!done) atomicAdd(reinterpret_cast<unsigned long long*>(areas + l), (unsigned long long)c);
  }
  __syncthreads();
  for (int s = threadIdx.x; s < kAreaSlots; s += kBlock)
    if (key[s]) atomicAdd(reinterpret_cast<unsigned long long*>(areas + key[s]), (unsigned long long)val[s]);
}

static size_t ccl_scan_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const int32_t*)nullptr, (int32_t*)nullptr, (int)n);
  return b;
}

struct CclWs {
  int32_t *parent, *cnt, *flag, *rank;  // rank: n scan entries, the component count, the error word
  char* scan_tmp;
  size_t scan_bytes;
};

static size_t ccl_carve(Arena& ar, int64_t n, CclWs* w) {
  w->parent = ar.take<int32_t>(n);
  w->cnt = ar.take<int32_t>(n);
  w->flag = ar.take<int32_t>(n);
  w->rank = ar.take<int32_t>(n + 2);
  w->scan_bytes = ccl_scan_bytes(n);
  w->scan_tmp = ar.take<char>(w->scan_bytes);
  return ar.used;
}

static bool ccl_size_ok(int64_t w, int64_t h) {
  return w >= 1 && h >= 1 && w < ((int64_t)1 << 31) && h < ((int64_t)1 << 31) && w * h < ((int64_t)1 << 31);
}

static size_t ccl_ws_bytes(int64_t w, int64_t h) {
  if (!ccl_size_ok(w, h)) return 0;
  Arena ar(nullptr, 0);
  CclWs ws;
  return ccl_carve(ar, w * h, &ws) + 1024;
}

static int ccl_run(const uint8_t* img, int64_t w64, int64_t h64, int32_t* labels, int64_t* areas, int64_t* n_labels_host,
                   void* ws, size_t ws_bytes, void* stream) {
  const char* who = "o3dx_ccl2d";
  if (w64 < 1 || h64 < 1) return fail(O3DX_EINVAL, "%s: image %lld x %lld is empty", who, (long long)w64, (long long)h64);
  if (!ccl_size_ok(w64, h64))
    return fail(O3DX_ENOTSUP, "%s: image %lld x %lld has 2^31 pixels or more", who, (long long)w64, (long long)h64);
  if (!img || !labels || !areas || !n_labels_host)
    return fail(O3DX_EINVAL, "%s: null img, labels, areas or n_labels_host", who);
  if (!ws || ws_bytes < ccl_ws_bytes(w64, h64)) return fail(O3DX_ENOMEM, "%s: workspace too small", who);
  hipStream_t s = as_stream(stream);
  const int w = (int)w64, h = (int)h64;
  const int64_t n = w64 * h64;
  Arena ar(ws, ws_bytes);
  CclWs W;
  ccl_carve(ar, n, &W);
  O3DX_ARENA_CHECK(ar);
  int* err = W.rank + n + 1;
  const int ntx = (w + kTW - 1) / kTW, nty = (h + kTH - 1) / kTH;
  const dim3 gn((unsigned)((n + kBlock - 1) / kBlock)), bk(kBlock);
  O3DX_HIP(hipMemsetAsync(err, 0, sizeof(int), s));
  {
    KTimer kt("ccl_tile", s);
    hipLaunchKernelGGL(k_ccl_tile, dim3((unsigned)((int64_t)ntx * nty)), bk, 0, s, img, w, h, ntx, W.parent, W.cnt, err);
  }
  {
    KTimer kt("ccl_seam", s);
    const int64_t seam = (int64_t)(ntx - 1) * h + (int64_t)(nty - 1) * w;
    if (seam > 0)
      hipLaunchKernelGGL(k_ccl_seam, dim3((unsigned)((seam + kBlock - 1) / kBlock)), bk, 0, s, img, w, h, ntx - 1,
                         nty - 1, W.parent, err);
  }
  int32_t res[2] = {0, 0};  // {component count, error word}
  {
    KTimer kt("ccl_label", s);
    hipLaunchKernelGGL(k_ccl_compress, gn, bk, 0, s, n, W.cnt, W.parent, err);
    hipLaunchKernelGGL(k_ccl_roots, gn, bk, 0, s, img, n, W.parent, labels, W.flag, err);
    size_t sb = W.scan_bytes;
    O3DX_HIP(hipcub::DeviceScan::ExclusiveSum(W.scan_tmp, sb, W.flag, W.rank, (int)n, s));
    hipLaunchKernelGGL(k_ccl_count, dim3(1), dim3(1), 0, s, n, W.flag, W.rank);
    O3DX_HIP(hipGetLastError());
    O3DX_TRY(read_back(res, W.rank + n, sizeof(res), s));
    if (res[1] != 0) return fail(O3DX_EIO, "%s: union-find exceeded its iteration bound", who);
    const int64_t k = res[0];
    hipLaunchKernelGGL(k_ccl_areas_clear, dim3(grid_for(k + 1, kBlock, 1024)), bk, 0, s, areas, k, n);
    hipLaunchKernelGGL(k_ccl_label, dim3(grid_for(n, kBlock, 4096)), bk, 0, s, n, W.rank, labels, areas);
    hipLaunchKernelGGL(k_ccl_areas, dim3((unsigned)((int64_t)ntx * nty)), bk, 0, s, w, h, ntx, W.cnt, labels, areas);
  }
  O3DX_HIP(hipGetLastError());
  O3DX_TRY(host_wait(s));
  *n_labels_host = res[0];
  return 0;
}

// --------------------------------------------------- points by label
__global__ void __launch_bounds__(kBlock) k_label_points(const int32_t* __restrict__ pix, int64_t n,
                                                         const int32_t* __restrict__ labels, int w, int h,
                                                         int64_t n_labels, uint32_t* __restrict__ point_label,
                                                         int32_t* __restrict__ iota, int64_t* __restrict__ counts,
                                                         int* err) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i <= n_labels) counts[i] = 0;
  if (i >= n) return;
  const int ix = pix[2 * i], iy = pix[2 * i + 1];
  int l = 0;
  if (ix < 0 || iy < 0 || ix >= w || iy >= h) {
    atomicOr(err, 1);
  } else {
    l = labels[(int64_t)iy * w + ix];
    if (l < 0 || l > n_labels) {  // a label the caller did not announce
      atomicOr(err, 2);
      l = 0;
    }
  }
  point_label[i] = (uint32_t)l;
  iota[i] = (int32_t)i;
}

// counts[l] = (one past l's last sorted position) - (its first): two integer
// adds per label that has points
__global__ void __launch_bounds__(kBlock) k_label_counts(const uint32_t* __restrict__ skey, int64_t n,
                                                         int64_t* counts) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= n) return;
  const uint32_t l = skey[j];
  if (j == 0 || skey[j - 1] != l)
    atomicAdd(reinterpret_cast<unsigned long long*>(counts + l), (unsigned long long)(-j));
  if (j == n - 1 || skey[j + 1] != l)
    atomicAdd(reinterpret_cast<unsigned long long*>(counts + l), (unsigned long long)(j + 1));
}

static int label_bits(int64_t n_labels) {
  int bits = 1;
  while (bits < 32 && ((int64_t)1 << bits) < n_labels + 1) ++bits;
  return bits;
}

struct LgWs {
  uint32_t* skey;
  int32_t *iota, *err;
  char* sort_tmp;
  size_t sort_bytes;
};

static size_t lg_carve(Arena& ar, int64_t n, int64_t n_labels, LgWs* w) {
  w->skey = ar.take<uint32_t>(n);
  w->iota = ar.take<int32_t>(n);
  w->err = ar.take<int32_t>(1);
  size_t b = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                           (const int32_t*)nullptr, (int32_t*)nullptr, (int)n, 0,
                                           label_bits(n_labels));
  w->sort_bytes = b;
  w->sort_tmp = ar.take<char>(b);
  return ar.used;
}

static bool lg_size_ok(int64_t n, int64_t n_labels) {
  return n >= 1 && n < ((int64_t)1 << 31) && n_labels >= 0 && n_labels < ((int64_t)1 << 31);
}

static size_t lg_ws_bytes(int64_t n, int64_t n_labels) {
  if (!lg_size_ok(n, n_labels)) return 0;
  Arena ar(nullptr, 0);
  LgWs w;
  return lg_carve(ar, n, n_labels, &w) + 1024;
}

static int label_group_run(const int32_t* pix, int64_t n, const int32_t* labels, int64_t w, int64_t h,
                           int64_t n_labels, int32_t* point_label, int32_t* order, int64_t* counts, void* ws,
                           size_t ws_bytes, void* stream) {
  const char* who = "o3dx_label_group";
  if (!lg_size_ok(n, n_labels))
    return fail(O3DX_EINVAL, "%s: n = %lld or n_labels = %lld outside [1, 2^31) / [0, 2^31)", who, (long long)n,
                (long long)n_labels);
  if (!ccl_size_ok(w, h)) return fail(O3DX_EINVAL, "%s: image %lld x %lld outside [1, 2^31) pixels", who, (long long)w, (long long)h);
  if (!pix || !labels || !point_label || !order || !counts)
    return fail(O3DX_EINVAL, "%s: null pix, labels, point_label, order or counts", who);
  if (!ws || ws_bytes < lg_ws_bytes(n, n_labels)) return fail(O3DX_ENOMEM, "%s: workspace too small", who);
  hipStream_t s = as_stream(stream);
  Arena ar(ws, ws_bytes);
  LgWs W;
  lg_carve(ar, n, n_labels, &W);
  O3DX_ARENA_CHECK(ar);
  int32_t res = 0;
  {
    KTimer kt("label_group", s);
    O3DX_HIP(hipMemsetAsync(W.err, 0, sizeof(int), s));
    const int64_t span = std::max(n, n_labels + 1);
    hipLaunchKernelGGL(k_label_points, dim3((unsigned)((span + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, pix, n,
                       labels, (int)w, (int)h, n_labels, reinterpret_cast<uint32_t*>(point_label), W.iota, counts,
                       W.err);
    size_t sb = W.sort_bytes;
    O3DX_HIP(hipcub::DeviceRadixSort::SortPairs(W.sort_tmp, sb, reinterpret_cast<const uint32_t*>(point_label), W.skey,
                                                W.iota, order, (int)n, 0, label_bits(n_labels), s));
    hipLaunchKernelGGL(k_label_counts, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, W.skey, n,
                       counts);
    O3DX_HIP(hipGetLastError());
  }
  O3DX_TRY(read_back(&res, W.err, sizeof(res), s));
  if (res & 1) return fail(O3DX_EINVAL, "%s: a pixel lies outside the %lld x %lld image", who, (long long)w, (long long)h);
  if (res & 2) return fail(O3DX_EINVAL, "%s: a label lies outside [0, n_labels = %lld]", who, (long long)n_labels);
  return 0;
}

}  // namespace o3dx

using namespace o3dx;

extern "C" int o3dx_raster2d_size(double resolution, const double* bounds_host, int64_t* wh_host) {
  if (!wh_host) return fail(O3DX_EINVAL, "o3dx_raster2d_size: null wh_host");
  RasterParams P;
  return raster_params("o3dx_raster2d_size", resolution, bounds_host, &P, wh_host, wh_host + 1);
}

extern "C" int o3dx_raster2d(const float* xyz, int64_t n, double resolution, const double* bounds_host, int32_t* pix,
                             uint8_t* img, int32_t* winner, int64_t img_cap, void* stream) {
  return raster_run<false>("o3dx_raster2d", xyz, n, resolution, bounds_host, pix, img, winner, img_cap, stream);
}

extern "C" int o3dx_raster2d_f64(const double* xyz, int64_t n, double resolution, const double* bounds_host,
                                 int32_t* pix, uint8_t* img, int32_t* winner, int64_t img_cap, void* stream) {
  return raster_run<true>("o3dx_raster2d_f64", xyz, n, resolution, bounds_host, pix, img, winner, img_cap, stream);
}

extern "C" size_t o3dx_ccl2d_workspace_bytes(int64_t w, int64_t h) { return ccl_ws_bytes(w, h); }

extern "C" int64_t o3dx_ccl2d_max_labels(int64_t w, int64_t h) {
  if (w < 1 || h < 1) return 0;
  return ((w + 1) / 2) * ((h + 1) / 2);
}

extern "C" int o3dx_ccl2d(const uint8_t* img, int64_t w, int64_t h, int32_t* labels, int64_t* areas,
                          int64_t* n_labels_host, void* ws, size_t ws_bytes, void* stream) {
  return ccl_run(img, w, h, labels, areas, n_labels_host, ws, ws_bytes, stream);
}

extern "C" size_t o3dx_label_group_workspace_bytes(int64_t n, int64_t n_labels) { return lg_ws_bytes(n, n_labels); }

extern "C" int o3dx_label_group(const int32_t* pix, int64_t n, const int32_t* labels, int64_t w, int64_t h,
                                int64_t n_labels, int32_t* point_label, int32_t* order, int64_t* counts, void* ws,
                                size_t ws_bytes, void* stream) {
  return label_group_run(pix, n, labels, w, h, n_labels, point_label, order, counts, ws, ws_bytes, stream);
}
