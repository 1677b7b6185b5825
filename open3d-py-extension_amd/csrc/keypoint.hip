// keypoint.hip — uncapped fixed-radius sweeps on the device: the neighbour
// count (Open3D RemoveRadiusOutliers), the ISS saliency and the ISS
// non-maximum suppression (o3d.geometry.keypoint.compute_iss_keypoints).
//
// Neighbourhood rule, everywhere: j is in N_r(i) when d^2(i,j) < r*r (strict;
// i itself is in), d^2 in float64 as ((dx dx) + dy dy) + dz dz (dist2_f64, the
// rule of the radius normals).  On float64 clouds every deciding d^2 and every
// moment comes from pts64; the float32 frame only filters, with db_within's
// guard band.
//
// Saliency rule: s[i] is a function of the neighbour SET alone.  The nine raw
// moments are taken about the set's first member in cell-sorted order and
// accumulated per query in ascending cell-sorted position, in float64, in the
// query's own registers: two queries with the same set add the same terms in
// the same order and get the same bits.  No cross-lane reduction takes part.
// (An origin common to the whole cloud gives the same property, but its raw
// moments lose (extent / spread)^2 ulps in the covariance's subtraction: 4e-10
// of |C| on tight clusters a unit apart.  About a member every term is within
// 2 r of the origin.)
//
// Search structure: the grid of grid.hpp with h >= r (+ slack), so N_r(i) lies
// in the 3^3 cube of cells around i's cell: 9 contiguous row ranges of the
// cell-sorted array, ascending (for_cube_rows).  In-cell order is ascending
// index (an ordered build), so the sorted array is the same run to run.
//
// Two forms of one sweep, bit-identical in every output:
//   lane  a lane per cell-sorted point walking its 9 ranges from global memory;
//   tile  a wave takes 64 consecutive cell-sorted points; for each cell with at
//         least kTileMin of them it stages the cell's 9 ranges through LDS in
//         chunks of 64 (a lane loads one candidate), and every query lane of
//         that cell reads the chunk at the same address (LDS broadcast, no
//         bank conflicts).  Lanes of cells with fewer queries walk as `lane`.
// A lane visits its candidates in ascending sorted position in both forms.
// O3DX_ISS_FORM=lane|tile (read at call time) picks the form.  Default: lane.
// Measured (profiles/iss_keypoints_time.txt), the tile form loses every pass
// on every input, 2 to 3.5 times: neighbouring lanes of the lane form read the
// same rows, which the caches already serve, while a wave of the tile form
// holds queries of several cells and idles the lanes of the others per cell.
// No float atomics, no host synchronisation beyond the grid build's bounds and
// the keypoint count.
#include "eigen3.hpp"
#include "grid.hpp"

namespace o3dx {

constexpr int kTile = 64;     // queries per wave = candidates per LDS chunk
constexpr int kTileMin = 8;   // queries of one cell in a wave that make staging worth it

struct RadParams {
  float lo;   // float32 frame d^2 <= lo: a neighbour for certain (-1: none is)
  float hi;   // float32 frame d^2 >  hi: not a neighbour for certain
  double r2;  // the deciding bound: exact d^2 < r2
};

enum SweepMode { kCount = 0, kSaliency = 1, kNms = 2 };

struct SweepArgs {
  int32_t* count;      // per point, original order (kCount, kSaliency)
  double* s_out;       // kSaliency
  const double* s_in;  // kNms: saliency, original order
  uint8_t* flag;       // kNms: keep flags, original order
  int cap;             // kCount: stop counting at cap (INT_MAX: none)
  int min_nb;
  double g21, g32;
};

struct SweepQuery {
  float4 qf;
  double qx, qy, qz;
  int oi;
};

template <int MODE>
struct SweepState {
  int cnt = 0;
  double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  double rx = 0.0, ry = 0.0, rz = 0.0;  // the moments' origin: the first member taken
  double si = 0.0;
  bool beaten = false;
};

template <bool F64>
__device__ __forceinline__ void sweep_query(const GridView& g, int s, SweepQuery& q) {
  q.qf = g.pts[s];
  q.oi = __float_as_int(q.qf.w);
  if constexpr (F64) {
    const double4 e = g.pts64[s];
    q.qx = e.x;
    q.qy = e.y;
    q.qz = e.z;
  } else {
    q.qx = (double)q.qf.x;
    q.qy = (double)q.qf.y;
    q.qz = (double)q.qf.z;
  }
}

template <int MODE>
__device__ __forceinline__ bool sweep_done(const SweepState<MODE>& st, const SweepArgs& a) {
  if constexpr (MODE == kCount) return st.cnt >= a.cap;
  return false;
}

// one member of the neighbourhood: (x, y, z) its deciding coordinates, sv its saliency
template <int MODE>
__device__ __forceinline__ void sweep_take(SweepState<MODE>& st, const SweepArgs& a, double x, double y, double z,
                                           double sv) {
  if constexpr (MODE == kCount) {
    if (st.cnt < a.cap) ++st.cnt;
  } else if constexpr (MODE == kSaliency) {
    if (st.cnt == 0) {
      st.rx = x;
      st.ry = y;
      st.rz = z;
    }
    ++st.cnt;
    const double px = x - st.rx, py = y - st.ry, pz = z - st.rz;
    st.m[0] += px;
    st.m[1] += py;
    st.m[2] += pz;
    st.m[3] += px * px;
    st.m[4] += px * py;
    st.m[5] += px * pz;
    st.m[6] += py * py;
    st.m[7] += py * pz;
    st.m[8] += pz * pz;
  } else {
    ++st.cnt;
    if (st.si < sv) st.beaten = true;
  }
}

// Candidates from global memory (the lane form)
template <bool F64, int MODE>
struct GlobalSrc {
  const GridView& g;
  const SweepArgs& a;
  __device__ __forceinline__ void visit(const RadParams& P, const SweepQuery& q, SweepState<MODE>& st, int p,
                                        const float4& v) const {
    const float d = dist2_f32(q.qf, v.x, v.y, v.z);
    if (!(d <= P.hi)) return;  // NaN coordinates: never a neighbour
    double ex = (double)v.x, ey = (double)v.y, ez = (double)v.z;
    if constexpr (F64) {
      if (MODE == kSaliency || !(d <= P.lo)) {
        const double4 e = g.pts64[p];
        ex = e.x;
        ey = e.y;
        ez = e.z;
      }
    }
    if (!(d <= P.lo)) {
      const double dx = q.qx - ex, dy = q.qy - ey, dz = q.qz - ez;
      double r = dx * dx;
      r = r + dy * dy;
      r = r + dz * dz;
      if (!(r < P.r2)) return;
    }
    double sv = 0.0;
    if constexpr (MODE == kNms) sv = a.s_in[__float_as_int(v.w)];
    sweep_take<MODE>(st, a, ex, ey, ez, sv);
  }
};

template <bool F64, int MODE>
__device__ __forceinline__ void sweep_lane(const GridView& g, const RadParams& P, const SweepArgs& a,
                                           const SweepQuery& q, int cx, int cy, int cz, SweepState<MODE>& st) {
  const GlobalSrc<F64, MODE> src{g, a};
  for_cube_rows(g, cx, cy, cz, 1, [&](int p0, int p1) {
    if (sweep_done<MODE>(st, a)) return;
    for_points4(g, p0, p1, [&](int p, const float4 v) { src.visit(P, q, st, p, v); });
  });
}

template <int MODE>
__device__ __forceinline__ void sweep_finish(const SweepArgs& a, const SweepQuery& q, SweepState<MODE>& st) {
  if constexpr (MODE == kCount) {
    a.count[q.oi] = st.cnt;
  } else if constexpr (MODE == kSaliency) {
    double s = 0.0;
    if (st.cnt >= a.min_nb && st.cnt > 0) {
      const double k = (double)st.cnt;
      double u[9];
      for (int j = 0; j < 9; ++j) u[j] = st.m[j] / k;
      double c[6];
      c[0] = u[3] - u[0] * u[0];
      c[1] = u[4] - u[0] * u[1];
      c[2] = u[5] - u[0] * u[2];
      c[3] = u[6] - u[1] * u[1];
      c[4] = u[7] - u[1] * u[2];
      c[5] = u[8] - u[2] * u[2];
      bool zero = true;  // Eigen's isZero(): every |entry| <= 1e-12
      for (int j = 0; j < 6; ++j) zero = zero && (fabs(c[j]) <= 1e-12);
      if (!zero) {
        double ev[3];
        eigen3_values(c, ev);
        const double e1 = ev[2], e2 = ev[1], e3 = ev[0];
        if (e2 / e1 < a.g21 && e3 / e2 < a.g32) s = e3;  // NaN ratios compare false
      }
    }
    a.s_out[q.oi] = s;
    a.count[q.oi] = st.cnt;
  } else {
    a.flag[q.oi] = (st.si > 0.0 && st.cnt >= a.min_nb && !st.beaten) ? 1 : 0;
  }
}

template <int MODE>
__device__ __forceinline__ void sweep_begin(const SweepArgs& a, const SweepQuery& q, SweepState<MODE>& st) {
  if constexpr (MODE == kNms) st.si = a.s_in[q.oi];
}

// ---- lane form: a lane per cell-sorted point
template <bool F64, int MODE>
__global__ void __launch_bounds__(kBlock) k_sweep_lane(GridView g, RadParams P, SweepArgs a) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= g.n) return;
  SweepQuery q;
  sweep_query<F64>(g, (int)t, q);
  int cx, cy, cz;
  grid_cell(g, q.qf.x, q.qf.y, q.qf.z, cx, cy, cz);
  SweepState<MODE> st;
  sweep_begin<MODE>(a, q, st);
  sweep_lane<F64, MODE>(g, P, a, q, cx, cy, cz, st);
  sweep_finish<MODE>(a, q, st);
}

// ---- tile form: one wave per block, 64 consecutive cell-sorted queries
template <bool F64, int MODE>
__global__ void __launch_bounds__(kTile) k_sweep_tile(GridView g, RadParams P, SweepArgs a, int tile_min) {
  __shared__ float4 sh_v[kTile];
  __shared__ double sh_e[F64 ? 3 * kTile : 1];  // x[64] y[64] z[64]
  __shared__ double sh_s[MODE == kNms ? kTile : 1];
  const int lane = threadIdx.x;
  const int64_t t = (int64_t)blockIdx.x * kTile + lane;
  const bool valid = t < g.n;
  SweepQuery q;
  SweepState<MODE> st;
  int cx = 0, cy = 0, cz = 0, cell = -1;
  if (valid) {
    sweep_query<F64>(g, (int)t, q);
    grid_cell(g, q.qf.x, q.qf.y, q.qf.z, cx, cy, cz);
    cell = cx + g.nx * (cy + g.ny * cz);
    sweep_begin<MODE>(a, q, st);
  }
  bool walk = false;  // this lane's cell has too few queries here: the lane form
  unsigned long long todo = __ballot(valid);
  while (todo) {  // wave-uniform: one turn per distinct cell of the wave's queries
    const int lead = __ffsll(todo) - 1;
    const int c = __builtin_amdgcn_readfirstlane(__shfl(cell, lead, 64));
    const bool mine = valid && cell == c;
    const unsigned long long mask = __ballot(mine);
    todo &= ~mask;
    if (__popcll(mask) < tile_min) {
      walk = walk || mine;
      continue;
    }
    const int ccx = __builtin_amdgcn_readfirstlane(__shfl(cx, lead, 64));
    const int ccy = __builtin_amdgcn_readfirstlane(__shfl(cy, lead, 64));
    const int ccz = __builtin_amdgcn_readfirstlane(__shfl(cz, lead, 64));
    for_cube_rows(g, ccx, ccy, ccz, 1, [&](int p0, int p1) {
      for (int base = p0; base < p1; base += kTile) {
        if (!__ballot(mine && !sweep_done<MODE>(st, a))) return;
        const int m = min(kTile, p1 - base);
        __syncthreads();  // the readers of the previous chunk are through
        if (lane < m) {
          const float4 v = g.pts[base + lane];
          sh_v[lane] = v;
          if constexpr (F64) {
            const double4 e = g.pts64[base + lane];
            sh_e[lane] = e.x;
            sh_e[kTile + lane] = e.y;
            sh_e[2 * kTile + lane] = e.z;
          }
          if constexpr (MODE == kNms) sh_s[lane] = a.s_in[__float_as_int(v.w)];
        }
        __syncthreads();
        if (mine) {
          for (int j = 0; j < m; ++j) {
            const float4 v = sh_v[j];
            const float d = dist2_f32(q.qf, v.x, v.y, v.z);
            if (!(d <= P.hi)) continue;
            double ex = (double)v.x, ey = (double)v.y, ez = (double)v.z;
            if constexpr (F64) {
              if (MODE == kSaliency || !(d <= P.lo)) {
                ex = sh_e[j];
                ey = sh_e[kTile + j];
                ez = sh_e[2 * kTile + j];
              }
            }
            if (!(d <= P.lo)) {
              const double dx = q.qx - ex, dy = q.qy - ey, dz = q.qz - ez;
              double r = dx * dx;
              r = r + dy * dy;
              r = r + dz * dz;
              if (!(r < P.r2)) continue;
            }
            double sv = 0.0;
            if constexpr (MODE == kNms) sv = sh_s[j];
            sweep_take<MODE>(st, a, ex, ey, ez, sv);
          }
        }
      }
    });
  }
  if (walk) sweep_lane<F64, MODE>(g, P, a, q, cx, cy, cz, st);
  if (valid) sweep_finish<MODE>(a, q, st);
}

// fixed-order float64 sum of sqrt(d2[i * k + col]) over the rows with cnt[i] >
// col: one block; a thread adds its rows in ascending order, block_sum_f64 the threads
__global__ void __launch_bounds__(kBlock) k_nn_distance_sum(const double* __restrict__ d2,
                                                            const int32_t* __restrict__ cnt, int64_t n, int k,
                                                            int col, double* __restrict__ out) {
  __shared__ double sh[kBlock / 64];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kBlock)
    if (cnt[i] > col) acc += sqrt(fmax(d2[i * k + col], 0.0));
  const double r = block_sum_f64<kBlock>(acc, sh);
  if (threadIdx.x == 0) *out = r;
}

// ------------------------------------------------------------------- host
constexpr double kKpOcc = 1.0;
constexpr int kKpCapMult = 4;

struct KpWs {
  char* grid;
  size_t grid_bytes;
  uint8_t* flags;  // nms only
  int32_t* ctmp;
  int64_t* cnt;
};

template <bool F64>
static size_t kp_carve(Arena& ar, int64_t n, bool nms, KpWs* w) {
  n = std::max<int64_t>(n, 1);
  w->grid_bytes = F64 ? grid64_ws_bytes(n, kKpCapMult) : grid_ws_bytes(n, kKpCapMult);
  w->grid = ar.take<char>(w->grid_bytes);
  w->flags = nullptr;
  w->ctmp = nullptr;
  w->cnt = nullptr;
  if (nms) {
    w->flags = ar.take<uint8_t>(n + 16);
    w->ctmp = ar.take<int32_t>(compact_workspace_ints(n));
    w->cnt = ar.take<int64_t>(2);
  }
  return ar.used;
}

template <bool F64>
static size_t kp_ws_bytes(int64_t n, bool nms) {
  if (n <= 0 || n >= ((int64_t)1 << 31)) return 0;
  Arena ar(nullptr, 0);
  KpWs w;
  return kp_carve<F64>(ar, n, nms, &w) + 1024;
}

static bool kp_lane_form() {
  const char* e = getenv("O3DX_ISS_FORM");
  return !(e && std::strcmp(e, "tile") == 0);
}

template <bool F64, class T>
static int kp_grid(const T* xyz, int64_t n, double min_h, const KpWs& w, hipStream_t s, GridBuild* G) {
  if constexpr (F64)
    return grid64_build(xyz, n, kKpOcc, min_h, w.grid, w.grid_bytes, s, G, nullptr, kKpCapMult);
  else  // ordered: the in-cell order (ascending index) fixes the moments' summation order
    return grid_build(xyz, n, kKpOcc, min_h, w.grid, w.grid_bytes, s, G, nullptr, nullptr, false, kKpCapMult, true);
}

// the grid (h >= radius + slack), the filter bounds and one sweep
template <bool F64, int MODE, class T>
static int kp_sweep(const char* who, const T* xyz, int64_t n, double radius, SweepArgs a, const KpWs& w,
                    hipStream_t s) {
  GridBuild G;
  auto need_h = [&]() { return radius + (double)G.view.slack + (double)G.view.d64; };
  {
    KTimer kt("kp_grid", s);
    O3DX_TRY((kp_grid<F64, T>(xyz, n, radius * (1.0 + 1e-3), w, s, &G)));
    if (!((double)G.view.h >= need_h())) {
      O3DX_TRY((kp_grid<F64, T>(xyz, n, need_h() * (1.0 + 1e-3), w, s, &G)));
      if (!((double)G.view.h >= need_h()))
        return fail(O3DX_EIO, "%s: no grid with cells >= radius (h = %g, radius = %g, slack = %g)", who,
                    (double)G.view.h, radius, (double)G.view.slack + (double)G.view.d64);
    }
  }
  const GridView g = G.view;
  RadParams P;
  P.r2 = radius * radius;
  {  // as cluster.hip's DbParams: relative 1e-6 around the float32 d^2, d64 around the frame
    const double d64 = (double)g.d64, rin = radius - d64, rout = radius + d64;
    const double lo = rin > 0.0 ? rin * rin * (1.0 - 1e-6) : -1.0, hi = rout * rout * (1.0 + 1e-6);
    P.lo = lo > 1e-30 ? std::nextafterf((float)std::min(lo, 3e38), -INFINITY) : -1.0f;
    P.hi = hi > 1e-30 ? std::nextafterf((float)std::min(hi, 3e38), INFINITY) : 1e-30f;
    if (!(hi < 3e38)) P.hi = INFINITY;
  }
  const char* tn = MODE == kCount ? "kp_count" : (MODE == kSaliency ? "kp_saliency" : "kp_nms");
  {
    KTimer kt(tn, s);
    if (kp_lane_form())
      hipLaunchKernelGGL((k_sweep_lane<F64, MODE>), dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                         g, P, a);
    else
      hipLaunchKernelGGL((k_sweep_tile<F64, MODE>), dim3((unsigned)((n + kTile - 1) / kTile)), dim3(kTile), 0, s, g,
                         P, a, kTileMin);
  }
  O3DX_HIP(hipGetLastError());
  return 0;
}

static int kp_check(const char* who, const void* xyz, int64_t n, double radius) {
  if (n <= 0 || n >= ((int64_t)1 << 31)) return fail(O3DX_EINVAL, "%s: n = %lld outside [1, 2^31)", who, (long long)n);
  if (!(radius > 0.0) || !std::isfinite(radius)) return fail(O3DX_EINVAL, "%s: radius must be finite and > 0", who);
  if (!xyz) return fail(O3DX_EINVAL, "%s: null points", who);
  return 0;
}

template <bool F64, class T>
static int radius_count_run(const char* who, const T* xyz, int64_t n, double radius, int cap, int32_t* count,
                            void* ws, size_t ws_bytes, void* stream) {
  O3DX_TRY(kp_check(who, xyz, n, radius));
  if (!count) return fail(O3DX_EINVAL, "%s: null count", who);
  if (!ws || ws_bytes < kp_ws_bytes<F64>(n, false)) return fail(O3DX_ENOMEM, "%s: workspace too small", who);
  Arena ar(ws, ws_bytes);
  KpWs w;
  kp_carve<F64>(ar, n, false, &w);
  O3DX_ARENA_CHECK(ar);
  SweepArgs a = {};
  a.count = count;
  a.cap = cap > 0 ? cap : 0x7fffffff;
  return kp_sweep<F64, kCount, T>(who, xyz, n, radius, a, w, as_stream(stream));
}

template <bool F64, class T>
static int iss_saliency_run(const char* who, const T* xyz, int64_t n, double radius, double g21, double g32,
                            int min_nb, double* s_out, int32_t* count, void* ws, size_t ws_bytes, void* stream) {
  O3DX_TRY(kp_check(who, xyz, n, radius));
  if (!s_out || !count) return fail(O3DX_EINVAL, "%s: null s or count", who);
  if (!ws || ws_bytes < kp_ws_bytes<F64>(n, false)) return fail(O3DX_ENOMEM, "%s: workspace too small", who);
  Arena ar(ws, ws_bytes);
  KpWs w;
  kp_carve<F64>(ar, n, false, &w);
  O3DX_ARENA_CHECK(ar);
  SweepArgs a = {};
  a.count = count;
  a.s_out = s_out;
  a.min_nb = min_nb;
  a.g21 = g21;
  a.g32 = g32;
  return kp_sweep<F64, kSaliency, T>(who, xyz, n, radius, a, w, as_stream(stream));
}

template <bool F64, class T>
static int iss_nms_run(const char* who, const T* xyz, int64_t n, const double* s_in, double radius, int min_nb,
                       int32_t* idx_out, int64_t* count_host, void* ws, size_t ws_bytes, void* stream) {
  O3DX_TRY(kp_check(who, xyz, n, radius));
  if (!s_in || !idx_out || !count_host) return fail(O3DX_EINVAL, "%s: null s, idx_out or count_host", who);
  if (!ws || ws_bytes < kp_ws_bytes<F64>(n, true)) return fail(O3DX_ENOMEM, "%s: workspace too small", who);
  hipStream_t s = as_stream(stream);
  Arena ar(ws, ws_bytes);
  KpWs w;
  kp_carve<F64>(ar, n, true, &w);
  O3DX_ARENA_CHECK(ar);
  SweepArgs a = {};
  a.s_in = s_in;
  a.flag = w.flags;
  a.min_nb = min_nb;
  O3DX_TRY((kp_sweep<F64, kNms, T>(who, xyz, n, radius, a, w, s)));
  O3DX_TRY(compact_flags(w.flags, n, idx_out, nullptr, w.cnt, w.ctmp, s));
  O3DX_TRY(read_back(count_host, w.cnt, sizeof(int64_t), s));
  return 0;
}

}  // namespace o3dx

using namespace o3dx;

extern "C" size_t o3dx_radius_count_workspace_bytes(int64_t n) { return kp_ws_bytes<false>(n, false); }
extern "C" size_t o3dx_radius_count_f64_workspace_bytes(int64_t n) { return kp_ws_bytes<true>(n, false); }
extern "C" size_t o3dx_iss_saliency_workspace_bytes(int64_t n) { return kp_ws_bytes<false>(n, false); }
extern "C" size_t o3dx_iss_saliency_f64_workspace_bytes(int64_t n) { return kp_ws_bytes<true>(n, false); }
extern "C" size_t o3dx_iss_nms_workspace_bytes(int64_t n) { return kp_ws_bytes<false>(n, true); }
extern "C" size_t o3dx_iss_nms_f64_workspace_bytes(int64_t n) { return kp_ws_bytes<true>(n, true); }

extern "C" int o3dx_radius_count(const float* xyz, int64_t n, double radius, int cap, int32_t* count, void* ws,
                                 size_t ws_bytes, void* stream) {
  return radius_count_run<false>("o3dx_radius_count", xyz, n, radius, cap, count, ws, ws_bytes, stream);
}
extern "C" int o3dx_radius_count_f64(const double* xyz, int64_t n, double radius, int cap, int32_t* count, void* ws,
                                     size_t ws_bytes, void* stream) {
  return radius_count_run<true>("o3dx_radius_count_f64", xyz, n, radius, cap, count, ws, ws_bytes, stream);
}

extern "C" int o3dx_iss_saliency(const float* xyz, int64_t n, double radius, double gamma_21, double gamma_32,
                                 int min_neighbors, double* s, int32_t* count, void* ws, size_t ws_bytes,
                                 void* stream) {
  return iss_saliency_run<false>("o3dx_iss_saliency", xyz, n, radius, gamma_21, gamma_32, min_neighbors, s, count, ws,
                                 ws_bytes, stream);
}
extern "C" int o3dx_iss_saliency_f64(const double* xyz, int64_t n, double radius, double gamma_21, double gamma_32,
                                     int min_neighbors, double* s, int32_t* count, void* ws, size_t ws_bytes,
                                     void* stream) {
  return iss_saliency_run<true>("o3dx_iss_saliency_f64", xyz, n, radius, gamma_21, gamma_32, min_neighbors, s, count,
                                ws, ws_bytes, stream);
}

extern "C" int o3dx_iss_nms(const float* xyz, int64_t n, const double* s, double radius, int min_neighbors,
                            int32_t* idx_out, int64_t* count_host, void* ws, size_t ws_bytes, void* stream) {
  return iss_nms_run<false>("o3dx_iss_nms", xyz, n, s, radius, min_neighbors, idx_out, count_host, ws, ws_bytes,
                            stream);
}
extern "C" int o3dx_iss_nms_f64(const double* xyz, int64_t n, const double* s, double radius, int min_neighbors,
                                int32_t* idx_out, int64_t* count_host, void* ws, size_t ws_bytes, void* stream) {
  return iss_nms_run<true>("o3dx_iss_nms_f64", xyz, n, s, radius, min_neighbors, idx_out, count_host, ws, ws_bytes,
                           stream);
}

extern "C" int o3dx_nn_distance_sum(const double* d2, const int32_t* cnt, int64_t n, int k, int col,
                                    double* sum_host, void* ws, size_t ws_bytes, void* stream) {
  if (n < 0 || k < 1 || col < 0 || col >= k || !sum_host || (n > 0 && (!d2 || !cnt)))
    return fail(O3DX_EINVAL, "o3dx_nn_distance_sum: bad args");
  if (!ws || ws_bytes < 256) return fail(O3DX_ENOMEM, "o3dx_nn_distance_sum: workspace too small");
  hipStream_t s = as_stream(stream);
  double* out = reinterpret_cast<double*>(ws);
  hipLaunchKernelGGL(k_nn_distance_sum, dim3(1), dim3(kBlock), 0, s, d2, cnt, n, k, col, out);
  O3DX_HIP(hipGetLastError());
  return read_back(sum_host, out, sizeof(double), s);
}
