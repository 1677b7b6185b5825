// cluster.hip — DBSCAN on the device (reference open3dpypro/PointCloud.py:921-927:
// sklearn.cluster.DBSCAN(eps, min_samples).fit(get_points()).labels_).
//
// sklearn's labels are a deterministic function of the input, restated here:
//   1. neighbourhood: j is a neighbour of i when d^2(i,j) <= eps*eps
//      (inclusive; i is its own neighbour), d^2 in float64 as ((dx dx) + dy dy)
//      + dz dz on the float64 coordinates (the KD-tree's rdist; dist2_f64);
//   2. core: |N(i)| >= min_samples;
//   3. clusters: the connected components of the core points under the
//      neighbour relation, numbered 0, 1, ... by ascending smallest core index;
//   4. border: a non-core point with a core neighbour takes the smallest label
//      among its core neighbours;
//   5. noise: everything else is -1.
//
// The search structure is the uniform grid of grid.hpp with cell size h >= eps
// (+ the float32 cell-assignment slack), so a point's neighbourhood lies in the
// 3^3 cube of cells around its own; the cube is 9 contiguous row ranges of the
// cell-sorted array (for_cube_rows).  A float32 d^2 settles the pairs clearly
// inside or outside; the pairs in its rounding band are decided by the exact
// float64 d^2.  Four passes, a lane per cell-sorted point:
//   k_dbscan_core    counts neighbours up to min_samples, writes the core bytes;
//   k_dbscan_union   lock-free union-find over parent[] (original indices):
//                    each core point unites with its core neighbours of lower
//                    sorted position; links go from the larger index to the
//                    smaller, so a component's final root is its smallest index
//                    for any thread order;
//   k_dbscan_roots / ExclusiveSum / k_dbscan_label
//                    root[i] = find(i) into its own array, the roots flagged
//                    and scanned: rank[root] is the cluster id in ascending
//                    order of smallest core index;
//   k_dbscan_border  non-core points: the minimum label over core neighbours.
// No float atomics; the labels do not depend on launch or in-cell order.
#include <hipcub/hipcub.hpp>
#include <type_traits>

#include "grid.hpp"
#include "unionfind.hpp"

namespace o3dx {

struct DbParams {
  float lo;     // float32 frame d^2 <= lo: a neighbour for certain (-1: none is)
  float hi;     // float32 frame d^2 >  hi: not a neighbour for certain
  double eps2;  // the deciding bound: exact d^2 <= eps2
  int min_samples;
};

template <bool F64>
__device__ __forceinline__ bool db_within(const GridView& g, const DbParams& P, const float4& qf, double qx, double qy,
                                          double qz, int p, const float4& v) {
  const float d = dist2_f32(qf, v.x, v.y, v.z);
  if (d <= P.lo) return true;
  if (!(d <= P.hi)) return false;  // NaN coordinates: never a neighbour
  return exact_d2<F64>(g, qx, qy, qz, p, v) <= P.eps2;
}

// sorted point s: its frame coordinates (cells, filter), the coordinates that
// decide, and its original index
template <bool F64>
__device__ __forceinline__ void db_query(const GridView& g, int s, float4& qf, double& qx, double& qy, double& qz,
                                         int& oi) {
  qf = g.pts[s];
  oi = __float_as_int(qf.w);
  if constexpr (F64) {
    const double4 q = g.pts64[s];
    qx = q.x;
    qy = q.y;
    qz = q.z;
  } else {
    qx = (double)qf.x;
    qy = (double)qf.y;
    qz = (double)qf.z;
  }
}

template <bool F64>
__global__ void __launch_bounds__(kBlock) k_dbscan_core(GridView g, DbParams P, uint8_t* __restrict__ core_s,
                                                        uint8_t* __restrict__ core_o) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= g.n) return;
  const int s = (int)t;
  float4 qf;
  double qx, qy, qz;
  int oi;
  db_query<F64>(g, s, qf, qx, qy, qz, oi);
  int cx, cy, cz;
  grid_cell(g, qf.x, qf.y, qf.z, cx, cy, cz);
  int cnt = 0;
  for_cube_rows(g, cx, cy, cz, 1, [&](int p0, int p1) {
    if (cnt >= P.min_samples) return;
    for_points4(g, p0, p1, [&](int p, const float4 v) {
      if (cnt < P.min_samples && db_within<F64>(g, P, qf, qx, qy, qz, p, v)) ++cnt;
    });
  });
  const uint8_t c = cnt >= P.min_samples ? 1 : 0;
  core_s[s] = c;
  core_o[oi] = c;
}

// the union-find (uf_load / uf_find / uf_unite): unionfind.hpp

template <bool F64>
__global__ void __launch_bounds__(kBlock) k_dbscan_union(GridView g, DbParams P, const uint8_t* __restrict__ core_s,
                                                         int32_t* parent, int* err) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= g.n) return;
  const int s = (int)t;
  if (!core_s[s]) return;
  float4 qf;
  double qx, qy, qz;
  int oi;
  db_query<F64>(g, s, qf, qx, qy, qz, oi);
  int cx, cy, cz;
  grid_cell(g, qf.x, qf.y, qf.z, cx, cy, cz);
  const int64_t bound = 2 * g.n + 2;
  int ra = oi;  // a member of this point's component, its root when last seen
  for_cube_rows(g, cx, cy, cz, 1, [&](int p0, int p1) {
    // neighbours of lower sorted position only: every edge is handled once
    for_points4(g, p0, min(p1, s), [&](int p, const float4 v) {
      if (!core_s[p] || !db_within<F64>(g, P, qf, qx, qy, qz, p, v)) return;
      const int rb = uf_find<true>(parent, __float_as_int(v.w), bound, err);
      if (rb != ra) ra = uf_unite(parent, ra, rb, bound, err);
    });
  });
}

__global__ void __launch_bounds__(kBlock) k_dbscan_init(int64_t n, int32_t* __restrict__ parent, int* err) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) parent[i] = (int32_t)i;
  if (i == 0) *err = 0;
}

// root[i] = find(i) in a launch of its own (parent[] is final and only read);
// flag[i] = i is a core root
__global__ void __launch_bounds__(kBlock) k_dbscan_roots(int64_t n, const int32_t* parent,
                                                         const uint8_t* __restrict__ core_o,
                                                         int32_t* __restrict__ root, int32_t* __restrict__ flag,
                                                         int* err) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const bool c = core_o[i] != 0;
  const int r = c ? uf_find(parent, (int)i, n + 1, err) : (int)i;
  root[i] = r;
  flag[i] = (c && r == (int)i) ? 1 : 0;
}

__global__ void __launch_bounds__(kBlock) k_dbscan_label(int64_t n, const uint8_t* __restrict__ core_o,
                                                         const int32_t* __restrict__ root,
                                                         const int32_t* __restrict__ flag, int32_t* rank,
                                                         int32_t* __restrict__ labels) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  labels[i] = core_o[i] ? rank[root[i]] : -1;
  if (i == n - 1) rank[n] = rank[i] + flag[i];  // the cluster count, read back with the error word
}

// labels: the core points' are final (k_dbscan_label) and only read here; a
// non-core point writes only its own
template <bool F64>
__global__ void __launch_bounds__(kBlock) k_dbscan_border(GridView g, DbParams P, const uint8_t* __restrict__ core_s,
                                                          int32_t* labels) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= g.n) return;
  const int s = (int)t;
  if (core_s[s]) return;
  float4 qf;
  double qx, qy, qz;
  int oi;
  db_query<F64>(g, s, qf, qx, qy, qz, oi);
  int cx, cy, cz;
  grid_cell(g, qf.x, qf.y, qf.z, cx, cy, cz);
  int best = 0x7fffffff;
  for_cube_rows(g, cx, cy, cz, 1, [&](int p0, int p1) {
    for_points4(g, p0, p1, [&](int p, const float4 v) {
      if (!core_s[p] || !db_within<F64>(g, P, qf, qx, qy, qz, p, v)) return;
      best = min(best, labels[__float_as_int(v.w)]);
    });
  });
  if (best != 0x7fffffff) labels[oi] = best;
}

// ------------------------------------------------------------------- host
constexpr double kDbOcc = 1.0;  // mean points per occupied cell where eps leaves the choice
constexpr int kDbCapMult = 4;

static size_t db_scan_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const int32_t*)nullptr, (int32_t*)nullptr, (int)n);
  return b;
}

struct DbWs {
  uint8_t *core_s, *core_o;
  int32_t *parent, *root, *flag, *rank;  // rank: n scan entries, the cluster count, the error word
  char* scan_tmp;
  size_t scan_bytes;
  char* grid;
  size_t grid_bytes;
};

template <bool F64>
static size_t db_carve(Arena& ar, int64_t n, DbWs* w) {
  n = std::max<int64_t>(n, 1);
  w->core_s = ar.take<uint8_t>(n);
  w->core_o = ar.take<uint8_t>(n);
  w->parent = ar.take<int32_t>(n);
  w->root = ar.take<int32_t>(n);
  w->flag = ar.take<int32_t>(n);
  w->rank = ar.take<int32_t>(n + 2);
  w->scan_bytes = db_scan_bytes(n);
  w->scan_tmp = ar.take<char>(w->scan_bytes);
  w->grid_bytes = F64 ? grid64_ws_bytes(n, kDbCapMult) : grid_ws_bytes(n, kDbCapMult);
  w->grid = ar.take<char>(w->grid_bytes);
  return ar.used;
}

template <bool F64>
static size_t db_ws_bytes(int64_t n) {
  if (n <= 0 || n >= ((int64_t)1 << 31)) return 0;
  Arena ar(nullptr, 0);
  DbWs w;
  return db_carve<F64>(ar, n, &w) + 1024;
}

template <bool F64, class T>
static int db_grid(const T* xyz, int64_t n, double min_h, const DbWs& w, hipStream_t s, GridBuild* G) {
  if constexpr (F64)
    return grid64_build(xyz, n, kDbOcc, min_h, w.grid, w.grid_bytes, s, G, nullptr, kDbCapMult);
  else  // nothing here depends on the order inside a cell
    return grid_build(xyz, n, kDbOcc, min_h, w.grid, w.grid_bytes, s, G, nullptr, nullptr, false, kDbCapMult, false);
}

template <bool F64, class T>
static int dbscan_run(const char* who, const T* xyz, int64_t n, double eps, int min_samples, int32_t* labels,
                      uint8_t* core, int64_t* n_clusters_host, void* ws, size_t ws_bytes, void* stream) {
  if (n <= 0 || n >= ((int64_t)1 << 31)) return fail(O3DX_EINVAL, "%s: n = %lld outside [1, 2^31)", who, (long long)n);
  if (!(eps > 0.0) || !std::isfinite(eps)) return fail(O3DX_EINVAL, "%s: eps must be finite and > 0", who);
  if (min_samples < 1) return fail(O3DX_EINVAL, "%s: min_samples must be >= 1", who);
  if (!xyz || !labels || !n_clusters_host) return fail(O3DX_EINVAL, "%s: null points, labels or n_clusters_host", who);
  if (!ws || ws_bytes < db_ws_bytes<F64>(n)) return fail(O3DX_ENOMEM, "%s: workspace too small", who);
  hipStream_t s = as_stream(stream);
  Arena ar(ws, ws_bytes);
  DbWs w;
  db_carve<F64>(ar, n, &w);
  O3DX_ARENA_CHECK(ar);
  uint8_t* core_o = core ? core : w.core_o;
  int* err = w.rank + n + 1;

  // The grid: h >= eps + the float32 cell-assignment slack (+ the float64
  // frame's rounding), so two points within eps lie in adjacent cells.  The
  // slack is known only once the bounds are: rebuilt once when the first h
  // falls short (coordinates large against eps).
  GridBuild G;
  auto need_h = [&]() { return eps + (double)G.view.slack + (double)G.view.d64; };
  {
    KTimer kt("dbscan_grid", s);
    O3DX_TRY((db_grid<F64, T>(xyz, n, eps * (1.0 + 1e-3), w, s, &G)));
    if (!((double)G.view.h >= need_h())) {
      O3DX_TRY((db_grid<F64, T>(xyz, n, need_h() * (1.0 + 1e-3), w, s, &G)));
      if (!((double)G.view.h >= need_h()))
        return fail(O3DX_EIO, "%s: no grid with cells >= eps (h = %g, eps = %g, slack = %g)", who, (double)G.view.h,
                    eps, (double)G.view.slack + (double)G.view.d64);
    }
  }
  const GridView g = G.view;

  // float32 prefilter bounds: the float32 d^2 of the frame coordinates is
  // within a relative 5 * 2^-24 of their exact d^2 (1e-6 taken), whose root is
  // within d64 of the exact distance (float64 clouds; 0 otherwise)
  DbParams P;
  P.eps2 = eps * eps;
  P.min_samples = min_samples;
  {
    const double d64 = (double)g.d64, ein = eps - d64, eout = eps + d64;
    const double lo = ein > 0.0 ? ein * ein * (1.0 - 1e-6) : -1.0, hi = eout * eout * (1.0 + 1e-6);
    // below 1e-30 float32 products may be subnormal: everything there is decided exactly
    P.lo = lo > 1e-30 ? std::nextafterf((float)std::min(lo, 3e38), -INFINITY) : -1.0f;
    P.hi = hi > 1e-30 ? std::nextafterf((float)std::min(hi, 3e38), INFINITY) : 1e-30f;
    if (!(hi < 3e38)) P.hi = INFINITY;
  }

  const dim3 gn((unsigned)((n + kBlock - 1) / kBlock)), bk(kBlock);
  {
    KTimer kt("dbscan_core", s);
    hipLaunchKernelGGL(k_dbscan_init, gn, bk, 0, s, n, w.parent, err);
    hipLaunchKernelGGL(k_dbscan_core<F64>, gn, bk, 0, s, g, P, w.core_s, core_o);
  }
  {
    KTimer kt("dbscan_union", s);
    hipLaunchKernelGGL(k_dbscan_union<F64>, gn, bk, 0, s, g, P, w.core_s, w.parent, err);
  }
  {
    KTimer kt("dbscan_label", s);
    hipLaunchKernelGGL(k_dbscan_roots, gn, bk, 0, s, n, w.parent, core_o, w.root, w.flag, err);
    size_t sb = w.scan_bytes;
    O3DX_HIP(hipcub::DeviceScan::ExclusiveSum(w.scan_tmp, sb, w.flag, w.rank, (int)n, s));
    hipLaunchKernelGGL(k_dbscan_label, gn, bk, 0, s, n, core_o, w.root, w.flag, w.rank, labels);
  }
  {
    KTimer kt("dbscan_border", s);
    hipLaunchKernelGGL(k_dbscan_border<F64>, gn, bk, 0, s, g, P, w.core_s, labels);
  }
  O3DX_HIP(hipGetLastError());
  int32_t res[2] = {0, 0};  // {cluster count, error word}
  O3DX_TRY(read_back(res, w.rank + n, sizeof(res), s));
  if (res[1] != 0) return fail(O3DX_EIO, "%s: union-find exceeded its iteration bound", who);
  *n_clusters_host = res[0];
  return 0;
}

}  // namespace o3dx

using namespace o3dx;

extern "C" size_t o3dx_dbscan_workspace_bytes(int64_t n) { return db_ws_bytes<false>(n); }
extern "C" size_t o3dx_dbscan_f64_workspace_bytes(int64_t n) { return db_ws_bytes<true>(n); }

extern "C" int o3dx_dbscan(const float* xyz, int64_t n, double eps, int min_samples, int32_t* labels, uint8_t* core,
                           int64_t* n_clusters_host, void* ws, size_t ws_bytes, void* stream) {
  return dbscan_run<false>("o3dx_dbscan", xyz, n, eps, min_samples, labels, core, n_clusters_host, ws, ws_bytes,
                           stream);
}

extern "C" int o3dx_dbscan_f64(const double* xyz, int64_t n, double eps, int min_samples, int32_t* labels,
                               uint8_t* core, int64_t* n_clusters_host, void* ws, size_t ws_bytes, void* stream) {
  return dbscan_run<true>("o3dx_dbscan_f64", xyz, n, eps, min_samples, labels, core, n_clusters_host, ws, ws_bytes,
                          stream);
}
