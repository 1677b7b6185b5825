// fpfh.hip — FPFH features (Open3D ComputeFPFHFeature, restated in DESIGN.md
// §4.11) and the 33-D nearest-feature matcher (gfx950).
//
// FPFH: the neighbour lists are taken once (o3dx_knn_search) and two kernels
// run over them, one wave per point, one lane per list position (a list holds
// at most O3DX_MAX_KNN = 64 entries, the wave's width).
//   k_spfh   lane l computes the pair feature of (point, list[l]) in float64
//            and votes into 33 integer LDS counters; the row leaves as 33 uint8
//            counts + the list length (36 B instead of 132 B of float32).
//   k_fpfh   the list's rows are gathered into LDS (lane p fetches row p);
//            then lane b owns bin b, walks the list in order and adds
//            count * inc_j / d^2 in float64.  No float atomics anywhere.
// Matcher: one lane per source row (33 registers), the target rows staged in
// LDS and read as wave-wide broadcasts; direct differences in float32.
#include "common.hpp"

namespace o3dx {

constexpr int kFeatDim = 33;
constexpr int kSpfhRow = 36;          // bytes per SPFH row: 33 counts, m, 2 x 0
constexpr int kWavesPerBlock = kBlock / 64;

struct PairF {
  double f0, f1, f2;
};

// Open3D ComputePairFeatures in float64, no contraction (-ffp-contract=off).
__device__ __forceinline__ PairF pair_feature(const double p1[3], const double n1_[3], const double p2[3],
                                              const double n2_[3]) {
  PairF r{0.0, 0.0, 0.0};
  double dp[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
  const double d = sqrt((dp[0] * dp[0] + dp[1] * dp[1]) + dp[2] * dp[2]);
  if (d == 0.0) return r;
  double n1[3] = {n1_[0], n1_[1], n1_[2]}, n2[3] = {n2_[0], n2_[1], n2_[2]};
  const double a1 = ((n1[0] * dp[0] + n1[1] * dp[1]) + n1[2] * dp[2]) / d;
  const double a2 = ((n2[0] * dp[0] + n2[1] * dp[1]) + n2[2] * dp[2]) / d;
  double f2;
  if (acos(fabs(a1)) > acos(fabs(a2))) {  // on the acos values; a NaN keeps the roles
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double t = n1[a];
      n1[a] = n2[a];
      n2[a] = t;
      dp[a] = -dp[a];
    }
    f2 = -a2;
  } else {
    f2 = a1;
  }
  double v[3] = {dp[1] * n1[2] - dp[2] * n1[1], dp[2] * n1[0] - dp[0] * n1[2], dp[0] * n1[1] - dp[1] * n1[0]};
  const double vn = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  if (vn == 0.0) return r;
#pragma unroll
  for (int a = 0; a < 3; ++a) v[a] /= vn;
  const double w[3] = {n1[1] * v[2] - n1[2] * v[1], n1[2] * v[0] - n1[0] * v[2], n1[0] * v[1] - n1[1] * v[0]};
  r.f1 = (v[0] * n2[0] + v[1] * n2[1]) + v[2] * n2[2];
  r.f0 = atan2((w[0] * n2[0] + w[1] * n2[1]) + w[2] * n2[2], (n1[0] * n2[0] + n1[1] * n2[1]) + n1[2] * n2[2]);
  r.f2 = f2;
  return r;
}

__device__ __forceinline__ int bin11(double x) {  // floor, clamped to 0..10 (NaN -> 0)
  return (int)fmin(fmax(floor(x), 0.0), 10.0);
}

// Pass 1: SPFH rows.  One wave per point; lane l takes list position l
// (position 0 is skipped whatever it holds).
__global__ void __launch_bounds__(kBlock) k_spfh(const float* __restrict__ xyz, const float* __restrict__ nrm,
                                                 int64_t n, int K, const int32_t* __restrict__ idx,
                                                 const int32_t* __restrict__ cnt, uint32_t* __restrict__ rows) {
  __shared__ uint32_t bins[kWavesPerBlock][kSpfhRow];
  const int w = threadIdx.x >> 6, l = lane_id();
  const int64_t i = (int64_t)blockIdx.x * kWavesPerBlock + w;
  const bool live = i < n;
  if (l < kSpfhRow) bins[w][l] = 0;
  __syncthreads();
  int m = 0;
  if (live) {
    m = min(max(cnt[i], 0), K);
    if (l >= 1 && l < m) {
      const int64_t j = idx[i * K + l];
      if (j >= 0 && j < n) {
        double p1[3], n1[3], p2[3], n2[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          p1[a] = (double)xyz[3 * i + a];
          n1[a] = (double)nrm[3 * i + a];
          p2[a] = (double)xyz[3 * j + a];
          n2[a] = (double)nrm[3 * j + a];
        }
        const PairF f = pair_feature(p1, n1, p2, n2);
        const int h0 = bin11(11.0 * (f.f0 + M_PI) / (2.0 * M_PI));
        const int h1 = bin11(11.0 * (f.f1 + 1.0) * 0.5);
        const int h2 = bin11(11.0 * (f.f2 + 1.0) * 0.5);
        atomicAdd(&bins[w][h0], 1u);  // integer LDS ballots: order-free
        atomicAdd(&bins[w][11 + h1], 1u);
        atomicAdd(&bins[w][22 + h2], 1u);
      }
    }
  }
  __syncthreads();
  if (live && l < kSpfhRow / 4) {
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int k = 4 * l + b;
      const uint32_t c = k < kFeatDim ? bins[w][k] : (k == kFeatDim ? (uint32_t)m : 0u);
      v |= (c & 0xffu) << (8 * b);
    }
    rows[i * (kSpfhRow / 4) + l] = v;
  }
}

// Pass 2: lane b owns bin b and walks the list in order.
__global__ void __launch_bounds__(kBlock) k_fpfh(int64_t n, int K, const int32_t* __restrict__ idx,
                                                 const double* __restrict__ d2, const int32_t* __restrict__ cnt,
                                                 const uint8_t* __restrict__ rows, float* __restrict__ out) {
  __shared__ double sh[kWavesPerBlock][kFeatDim];
  __shared__ uint32_t nb[kWavesPerBlock][64 * (kSpfhRow / 4)];
  const int w = threadIdx.x >> 6, l = lane_id();
  const int64_t i = (int64_t)blockIdx.x * kWavesPerBlock + w;
  const bool live = i < n;
  const int m = live ? min(max(cnt[i], 0), K) : 0;
  int jl = 0;
  double dl = 0.0;
  if (l < m) {
    jl = idx[i * K + l];
    dl = d2[i * K + l];
    if (jl < 0 || jl >= n) {  // (never from o3dx_knn_search; keeps the gather in bounds)
      jl = 0;
      dl = 0.0;
    }
  }
  // the list's rows into LDS first, lane p fetching row p as 9 dwords (all of
  // the wave's gathers in flight at once; the walk below then reads LDS
  // instead of waiting on one global row per step).  Lane stride 9 dwords:
  // conflict-free.
  if (l < m) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(rows) + (int64_t)jl * (kSpfhRow / 4);
#pragma unroll
    for (int k = 0; k < kSpfhRow / 4; ++k) nb[w][l * (kSpfhRow / 4) + k] = src[k];
  }
  __syncthreads();
  const uint8_t* mine = reinterpret_cast<const uint8_t*>(nb[w]);
  double acc = 0.0;
  for (int p = 1; p < m; ++p) {  // m is wave-uniform
    const double d = __shfl(dl, p, 64);
    const int byte = l < kSpfhRow ? (int)mine[p * kSpfhRow + l] : 0;
    const int mj = __shfl(byte, kFeatDim, 64);
    const double inc = mj > 1 ? 100.0 / (double)(mj - 1) : 0.0;
    const double val = ((double)byte * inc) / d;
    acc += d != 0.0 ? val : 0.0;
  }
  if (l < kFeatDim) sh[w][l] = acc;
  __syncthreads();
  if (live && l < kFeatDim) {
    double res = 0.0;
    if (m > 1) {
      const int g = (l / 11) * 11;
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 11; ++k) s += sh[w][g + k];
      if (s != 0.0) s = 100.0 / s;
      const double own = (double)rows[i * kSpfhRow + l] * (100.0 / (double)(m - 1));
      res = acc * s + own;
    }
    out[i * kFeatDim + l] = (float)res;
  }
}

// ---------------------------------------------------------------- matcher
constexpr int kMatchTile = 128;   // target rows per LDS tile
constexpr int kMatchStride = 36;  // floats per staged row (16-B aligned rows)

// blockIdx.x: 64 source rows (lane = row); blockIdx.y: a chunk of targets
// [chunk * per, ...).  Wave w of the block takes rows [32 w, 32 w + 32) of each
// staged tile.  Partial (d2, index) per (chunk, source row).
__global__ void __launch_bounds__(kBlock) k_match(const float* __restrict__ A, int64_t ns,
                                                  const float* __restrict__ B, int64_t nt, int64_t per,
                                                  float* __restrict__ pd, int32_t* __restrict__ pi) {
  __shared__ __attribute__((aligned(16))) float tile[kMatchTile * kMatchStride];
  __shared__ float bd[kWavesPerBlock][64];
  __shared__ int32_t bi[kWavesPerBlock][64];
  const int w = threadIdx.x >> 6, l = lane_id();
  const int64_t row = (int64_t)blockIdx.x * 64 + l;
  const int64_t t0 = (int64_t)blockIdx.y * per, t1 = min(nt, t0 + per);
  float a[kFeatDim];
#pragma unroll
  for (int c = 0; c < kFeatDim; ++c) a[c] = row < ns ? A[row * kFeatDim + c] : 0.0f;
  float best = INFINITY;
  int32_t besti = (int32_t)t0;
  for (int64_t base = t0; base < t1; base += kMatchTile) {
    const int rows = (int)min<int64_t>(kMatchTile, t1 - base);
    __syncthreads();
    for (int e = threadIdx.x; e < rows * kFeatDim; e += kBlock) {
      const int r = e / kFeatDim, c = e - r * kFeatDim;
      tile[r * kMatchStride + c] = B[(base + r) * kFeatDim + c];
    }
    __syncthreads();
    const int r1 = min(rows, 32 * (w + 1));
    for (int r = 32 * w; r < r1; ++r) {
      const float4* q = reinterpret_cast<const float4*>(tile + r * kMatchStride);
      float s = 0.0f;
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        const float4 b = q[v];
        const float e0 = a[4 * v] - b.x, e1 = a[4 * v + 1] - b.y, e2 = a[4 * v + 2] - b.z, e3 = a[4 * v + 3] - b.w;
        s += e0 * e0;
        s += e1 * e1;
        s += e2 * e2;
        s += e3 * e3;
      }
      const float e32 = a[32] - tile[r * kMatchStride + 32];
      s += e32 * e32;
      if (s < best) {  // ascending target index within the wave: strict <
        best = s;
        besti = (int32_t)(base + r);
      }
    }
  }
  bd[w][l] = best;
  bi[w][l] = besti;
  __syncthreads();
  if (w == 0 && row < ns) {
#pragma unroll
    for (int v = 1; v < kWavesPerBlock; ++v) {
      const float d = bd[v][l];
      const int32_t k = bi[v][l];
      if (d < best || (d == best && k < besti)) {
        best = d;
        besti = k;
      }
    }
    pd[(int64_t)blockIdx.y * ns + row] = best;
    pi[(int64_t)blockIdx.y * ns + row] = besti;
  }
}

__global__ void __launch_bounds__(kBlock) k_match_fold(const float* __restrict__ pd, const int32_t* __restrict__ pi,
                                                       int64_t ns, int chunks, int32_t* __restrict__ idx_out,
                                                       float* __restrict__ d2_out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= ns) return;
  float best = pd[i];
  int32_t besti = pi[i];
  for (int c = 1; c < chunks; ++c) {
    const float d = pd[(int64_t)c * ns + i];
    const int32_t k = pi[(int64_t)c * ns + i];
    if (d < best || (d == best && k < besti)) {
      best = d;
      besti = k;
    }
  }
  idx_out[i] = besti;
  if (d2_out) d2_out[i] = best;
}

// target chunks per source block: enough blocks to fill the device, no chunk
// below one tile
static int match_chunks(int64_t ns, int64_t nt) {
  const int64_t sb = (ns + 63) / 64;
  int64_t c = (2048 + sb - 1) / std::max<int64_t>(sb, 1);
  c = std::min<int64_t>(c, (nt + kMatchTile - 1) / kMatchTile);
  return (int)std::min<int64_t>(std::max<int64_t>(c, 1), 1024);
}

struct FpfhWs {
  int32_t* idx;
  double* d2;
  int32_t* cnt;
  uint32_t* rows;
  void* knn;
  size_t knn_bytes;
};

static size_t fpfh_carve(Arena& ar, int64_t n, int K, FpfhWs* w) {
  const size_t nn = (size_t)std::max<int64_t>(n, 1);
  w->d2 = ar.take<double>(nn * K);
  w->idx = ar.take<int32_t>(nn * K);
  w->cnt = ar.take<int32_t>(nn);
  w->rows = ar.take<uint32_t>(nn * (kSpfhRow / 4));
  w->knn_bytes = o3dx_knn_workspace_bytes(n);
  w->knn = ar.take<char>(w->knn_bytes);
  return ar.used;
}

}  // namespace o3dx

using namespace o3dx;

extern "C" size_t o3dx_fpfh_workspace_bytes(int64_t n, int knn) {
  Arena ar(nullptr, 0);
  FpfhWs w;
  return fpfh_carve(ar, std::max<int64_t>(n, 0), std::min(std::max(knn, 1), O3DX_MAX_KNN), &w) + 1024;
}

extern "C" int o3dx_fpfh(const float* xyz, const float* normals, int64_t n, int mode, int knn, double radius,
                         float* out, uint8_t* spfh_out, void* ws, size_t ws_bytes, void* stream) {
  if (n < 0 || (n > 0 && (!xyz || !normals || !out))) return fail(O3DX_EINVAL, "o3dx_fpfh: bad arguments");
  if (mode == O3DX_SEARCH_RADIUS)
    return fail(O3DX_ENOTSUP, "o3dx_fpfh: a radius search has unbounded lists; use KNN or HYBRID");
  if (mode != O3DX_SEARCH_KNN && mode != O3DX_SEARCH_HYBRID)
    return fail(O3DX_EINVAL, "o3dx_fpfh: unknown search mode %d", mode);
  if (knn < 1 || knn > O3DX_MAX_KNN)
    return fail(O3DX_EINVAL, "o3dx_fpfh: knn / max_nn must be in 1..O3DX_MAX_KNN (%d), got %d", O3DX_MAX_KNN, knn);
  if (mode == O3DX_SEARCH_HYBRID && !(radius > 0.0)) return fail(O3DX_EINVAL, "o3dx_fpfh: radius must be > 0");
  if (n == 0) return 0;
  if (!ws || ws_bytes < o3dx_fpfh_workspace_bytes(n, knn)) return fail(O3DX_ENOMEM, "o3dx_fpfh: workspace too small");
  Arena ar(ws, ws_bytes);
  FpfhWs w;
  fpfh_carve(ar, n, knn, &w);
  O3DX_ARENA_CHECK(ar);
  hipStream_t s = as_stream(stream);
  O3DX_TRY(o3dx_knn_search(xyz, n, xyz, n, mode, knn, radius, w.idx, w.d2, w.cnt, w.knn, w.knn_bytes, stream));
  const unsigned g = (unsigned)((n + kWavesPerBlock - 1) / kWavesPerBlock);
  {
    KTimer kt("fpfh_spfh", s);
    hipLaunchKernelGGL(k_spfh, dim3(g), dim3(kBlock), 0, s, xyz, normals, n, knn, w.idx, w.cnt, w.rows);
  }
  {
    KTimer kt("fpfh_gather", s);
    hipLaunchKernelGGL(k_fpfh, dim3(g), dim3(kBlock), 0, s, n, knn, w.idx, w.d2, w.cnt, (const uint8_t*)w.rows, out);
  }
  O3DX_HIP(hipGetLastError());
  if (spfh_out)
    O3DX_HIP(hipMemcpyAsync(spfh_out, w.rows, (size_t)n * kSpfhRow, hipMemcpyDeviceToDevice, s));
  return host_wait(s);  // the workspace is the caller's again
}

extern "C" size_t o3dx_feature_match_workspace_bytes(int64_t ns, int64_t nt) {
  ns = std::max<int64_t>(ns, 1);
  nt = std::max<int64_t>(nt, 1);
  const size_t c = (size_t)match_chunks(ns, nt);
  return 2 * Arena::align(c * ns * sizeof(float) + 1) + 1024;
}

extern "C" int o3dx_feature_match(const float* A, int64_t ns, const float* B, int64_t nt, int32_t* idx_out,
                                  float* d2_out, void* ws, size_t ws_bytes, void* stream) {
  if (ns < 0 || nt < 0 || (ns > 0 && (!A || !idx_out)) || (nt > 0 && !B))
    return fail(O3DX_EINVAL, "o3dx_feature_match: bad arguments");
  if (ns == 0) return 0;
  if (nt == 0) return fail(O3DX_EINVAL, "o3dx_feature_match: no target features");
  if (nt > INT32_MAX) return fail(O3DX_EINVAL, "o3dx_feature_match: nt must be < 2^31");
  if (!ws || ws_bytes < o3dx_feature_match_workspace_bytes(ns, nt))
    return fail(O3DX_ENOMEM, "o3dx_feature_match: workspace too small");
  const int chunks = match_chunks(ns, nt);
  // whole tiles per chunk, so that every chunk starts on a tile boundary
  int64_t per = (nt + chunks - 1) / chunks;
  per = (per + kMatchTile - 1) / kMatchTile * kMatchTile;
  const int used = (int)((nt + per - 1) / per);
  Arena ar(ws, ws_bytes);
  float* pd = ar.take<float>((size_t)used * ns);
  int32_t* pi = ar.take<int32_t>((size_t)used * ns);
  O3DX_ARENA_CHECK(ar);
  hipStream_t s = as_stream(stream);
  KTimer kt("feature_match", s);
  hipLaunchKernelGGL(k_match, dim3((unsigned)((ns + 63) / 64), (unsigned)used), dim3(kBlock), 0, s, A, ns, B, nt, per,
                     pd, pi);
  hipLaunchKernelGGL(k_match_fold, dim3(grid_for(ns)), dim3(kBlock), 0, s, pd, pi, ns, used, idx_out, d2_out);
  O3DX_HIP(hipGetLastError());
  return 0;
}
