// globalreg.hip — RANSAC on correspondences (Open3D
// RegistrationRANSACBasedOnCorrespondence, restated in DESIGN.md §4.11): the
// host side of a round (batched Umeyama of the samples, the checkers) and the
// sweep that scores every surviving hypothesis against all correspondences.
// The design is ransac.hip's: exact integer inlier counts for every
// hypothesis in one launch (float32 distance, float64 re-decision inside a
// guard band of the threshold), sum d^2 in fixed-order float64 only for the
// hypotheses the sequential rule can consult.
#include <vector>

#include "common.hpp"

namespace o3dx {

// one hypothesis on the device: the float64 rows of [R | t], their float32
// roundings and the magnitudes the guard band needs
struct CorrHyp {
  double T[12];
  float Tf[12];
  float rmax, tmax;  // max |R_ij|, max |t_i|
  float pad[2];
};

struct CorrPair {  // a gathered correspondence (float32 inputs)
  float px, py, pz, qx, qy, qz;
};

__global__ void __launch_bounds__(kBlock) k_corr_gather(const float* __restrict__ src, const float* __restrict__ tgt,
                                                        const int32_t* __restrict__ corr, int64_t c,
                                                        CorrPair* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= c) return;
  const int64_t i = corr[2 * k], j = corr[2 * k + 1];
  out[k] = CorrPair{src[3 * i], src[3 * i + 1], src[3 * i + 2], tgt[3 * j], tgt[3 * j + 1], tgt[3 * j + 2]};
}

// |T p - q| in the pinned float64 order
__device__ __forceinline__ double corr_dist64(const double* T, const CorrPair& v) {
  const double x = v.px, y = v.py, z = v.pz;
  const double dx = (((T[0] * x + T[1] * y) + T[2] * z) + T[3]) - (double)v.qx;
  const double dy = (((T[4] * x + T[5] * y) + T[6] * z) + T[7]) - (double)v.qy;
  const double dz = (((T[8] * x + T[9] * y) + T[10] * z) + T[11]) - (double)v.qz;
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

// blockIdx.x: hypothesis; blockIdx.y: a slice of the correspondences.
// float32 error of each difference component: <= 5 roundings of magnitude
// <= S = rmax (|x| + |y| + |z|) + tmax + |q|_inf, plus the rounding of T itself
// (2^-24 S); of the norm: sqrt(3) times that plus 3 roundings of d.  The band
// below (32 S + 16 d) 2^-24 covers it several times over; inside it the
// float64 decision stands.
__global__ void __launch_bounds__(kBlock) k_corr_count(const CorrPair* __restrict__ pq, int64_t c,
                                                       const CorrHyp* __restrict__ hyp, double max_d,
                                                       uint32_t* __restrict__ counts) {
  __shared__ CorrHyp H;
  __shared__ int part[kBlock / 64];
  if (threadIdx.x < sizeof(CorrHyp) / 4)
    reinterpret_cast<uint32_t*>(&H)[threadIdx.x] = reinterpret_cast<const uint32_t*>(hyp + blockIdx.x)[threadIdx.x];
  __syncthreads();
  const float thr = (float)max_d;
  const float* T = H.Tf;
  int cnt = 0;
  for (int64_t k = (int64_t)blockIdx.y * kBlock + threadIdx.x; k < c; k += (int64_t)gridDim.y * kBlock) {
    const CorrPair v = pq[k];
    const float dx = (((T[0] * v.px + T[1] * v.py) + T[2] * v.pz) + T[3]) - v.qx;
    const float dy = (((T[4] * v.px + T[5] * v.py) + T[6] * v.pz) + T[7]) - v.qy;
    const float dz = (((T[8] * v.px + T[9] * v.py) + T[10] * v.pz) + T[11]) - v.qz;
    const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
    const float S = H.rmax * ((fabsf(v.px) + fabsf(v.py)) + fabsf(v.pz)) + H.tmax +
                    fmaxf(fmaxf(fabsf(v.qx), fabsf(v.qy)), fabsf(v.qz));
    const float band = (32.0f * S + 16.0f * (d + thr)) * 5.9604645e-08f;
    bool in = d < thr;
    if (!(fabsf(d - thr) > band)) in = corr_dist64(H.T, v) < max_d;  // (a NaN lands here too)
    cnt += in ? 1 : 0;
  }
  cnt = wave_sum(cnt);
  if (lane_id() == 0) part[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < kBlock / 64; ++w) t += part[w];
    if (t) atomicAdd(&counts[blockIdx.x], (uint32_t)t);  // integer: order-free
  }
}

// sum d * d over the inliers of hypothesis blockIdx.x, float64: each thread
// its strided share in order, then the block's fixed-order fold
__global__ void __launch_bounds__(kBlock) k_corr_error2(const CorrPair* __restrict__ pq, int64_t c,
                                                        const CorrHyp* __restrict__ hyp, double max_d,
                                                        double* __restrict__ sums, int64_t* __restrict__ counts) {
  __shared__ CorrHyp H;
  __shared__ double sh[kBlock / 64];
  __shared__ int part[kBlock / 64];
  if (threadIdx.x < sizeof(CorrHyp) / 4)
    reinterpret_cast<uint32_t*>(&H)[threadIdx.x] = reinterpret_cast<const uint32_t*>(hyp + blockIdx.x)[threadIdx.x];
  __syncthreads();
  double acc = 0.0;
  int cnt = 0;
  for (int64_t k = threadIdx.x; k < c; k += kBlock) {
    const double d = corr_dist64(H.T, pq[k]);
    if (d < max_d) {
      acc += d * d;
      ++cnt;
    }
  }
  cnt = wave_sum(cnt);
  if (lane_id() == 0) part[threadIdx.x >> 6] = cnt;
  const double r = block_sum_f64<kBlock>(acc, sh);
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < kBlock / 64; ++w) t += part[w];
    sums[blockIdx.x] = r;
    counts[blockIdx.x] = t;
  }
}

static_assert(sizeof(CorrHyp) == 160, "CorrHyp layout");
static_assert(sizeof(CorrHyp) / 4 <= kBlock, "CorrHyp is copied by one block");

struct CorrWs {
  CorrPair* pq;
  CorrHyp* hyp;
  uint32_t* counts;
  double* sums;
  int64_t* cnt64;
};

static size_t corr_carve(Arena& ar, int64_t c, int H, CorrWs* w) {
  const size_t cc = (size_t)std::max<int64_t>(c, 1), hh = (size_t)std::max(H, 1);
  w->pq = ar.take<CorrPair>(cc);
  w->hyp = ar.take<CorrHyp>(hh);
  w->counts = ar.take<uint32_t>(hh);
  w->sums = ar.take<double>(hh);
  w->cnt64 = ar.take<int64_t>(hh);
  return ar.used;
}

static void pack_hyps(const double* T, int H, std::vector<CorrHyp>& out) {
  out.resize((size_t)H);
  for (int h = 0; h < H; ++h) {
    CorrHyp& c = out[(size_t)h];
    std::memset(&c, 0, sizeof(c));
    double rm = 0.0, tm = 0.0;
    for (int a = 0; a < 12; ++a) {
      c.T[a] = T[16 * h + a];
      c.Tf[a] = (float)c.T[a];
      if (a % 4 == 3) tm = std::max(tm, std::fabs(c.T[a]));
      else rm = std::max(rm, std::fabs(c.T[a]));
    }
    // rounded up: the band may only widen
    c.rmax = std::nextafterf((float)rm, INFINITY);
    c.tmax = std::nextafterf((float)tm, INFINITY);
  }
}

static int corr_args(const char* fn, const float* src, const float* tgt, const int32_t* corr, int64_t c,
                     const double* T, int H, double max_d) {
  if (c < 0 || H < 0 || (c > 0 && (!src || !tgt || !corr)) || (H > 0 && !T))
    return fail(O3DX_EINVAL, "%s: bad arguments", fn);
  if (!(max_d > 0.0)) return fail(O3DX_EINVAL, "%s: max_distance must be > 0", fn);
  return 0;
}

static inline double norm3(double x, double y, double z) { return std::sqrt((x * x + y * y) + z * z); }

}  // namespace o3dx

using namespace o3dx;

extern "C" int o3dx_umeyama_from_samples(const double* coords, int H, int rn, double* T_out) {
  if (H < 0 || rn < 1 || (H > 0 && (!coords || !T_out)))
    return fail(O3DX_EINVAL, "o3dx_umeyama_from_samples: bad arguments");
  for (int h = 0; h < H; ++h) {
    const double* s = coords + (size_t)h * rn * 6;
    // the point-to-point sums about the anchor a = the first target point
    double sums[O3DX_ICP_NSUMS] = {0};
    const double a[3] = {s[3], s[4], s[5]};
    for (int k = 0; k < rn; ++k) {
      const double p[3] = {s[6 * k] - a[0], s[6 * k + 1] - a[1], s[6 * k + 2] - a[2]};
      const double q[3] = {s[6 * k + 3] - a[0], s[6 * k + 4] - a[1], s[6 * k + 5] - a[2]};
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) sums[3 * i + j] += q[i] * p[j];
        sums[9 + i] += p[i];
        sums[12 + i] += q[i];
      }
      sums[15] += (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
    }
    for (int i = 0; i < 3; ++i) sums[16 + i] = a[i];
    sums[28] = (double)rn;
    const int rc = o3dx_icp_solve_point_to_point(sums, 0, T_out + (size_t)16 * h);
    if (rc < 0) return rc;
  }
  return 0;
}

extern "C" int o3dx_corr_check(const double* coords, int H, int rn, const double* T, double edge_s, double dist_t,
                               uint8_t* pass) {
  if (H < 0 || rn < 1 || (H > 0 && (!coords || !pass)) || (H > 0 && dist_t >= 0.0 && !T))
    return fail(O3DX_EINVAL, "o3dx_corr_check: bad arguments");
  for (int h = 0; h < H; ++h) {
    const double* s = coords + (size_t)h * rn * 6;
    bool ok = true;
    if (edge_s >= 0.0)
      for (int i = 0; i < rn && ok; ++i)
        for (int j = i + 1; j < rn && ok; ++j) {
          const double ds = norm3(s[6 * i] - s[6 * j], s[6 * i + 1] - s[6 * j + 1], s[6 * i + 2] - s[6 * j + 2]);
          const double dt = norm3(s[6 * i + 3] - s[6 * j + 3], s[6 * i + 4] - s[6 * j + 4], s[6 * i + 5] - s[6 * j + 5]);
          if (ds < dt * edge_s || dt < ds * edge_s) ok = false;
        }
    if (ok && dist_t >= 0.0) {
      const double* M = T + (size_t)16 * h;
      for (int k = 0; k < rn && ok; ++k) {
        const double x = s[6 * k], y = s[6 * k + 1], z = s[6 * k + 2];
        const double dx = (((M[0] * x + M[1] * y) + M[2] * z) + M[3]) - s[6 * k + 3];
        const double dy = (((M[4] * x + M[5] * y) + M[6] * z) + M[7]) - s[6 * k + 4];
        const double dz = (((M[8] * x + M[9] * y) + M[10] * z) + M[11]) - s[6 * k + 5];
        if (norm3(dx, dy, dz) > dist_t) ok = false;
      }
    }
    pass[h] = ok ? 1 : 0;
  }
  return 0;
}

extern "C" size_t o3dx_corr_count_workspace_bytes(int64_t c, int H) {
  Arena ar(nullptr, 0);
  CorrWs w;
  return corr_carve(ar, c, H, &w) + 1024;
}

extern "C" int o3dx_corr_count(const float* src, const float* tgt, const int32_t* corr, int64_t c, const double* T,
                               int H, double max_d, int64_t* counts_host, void* ws, size_t ws_bytes, void* stream) {
  O3DX_TRY(corr_args("o3dx_corr_count", src, tgt, corr, c, T, H, max_d));
  if (H > 0 && !counts_host) return fail(O3DX_EINVAL, "o3dx_corr_count: bad arguments");
  if (H == 0) return 0;
  if (c == 0) {
    for (int h = 0; h < H; ++h) counts_host[h] = 0;
    return 0;
  }
  if (!ws || ws_bytes < o3dx_corr_count_workspace_bytes(c, H))
    return fail(O3DX_ENOMEM, "o3dx_corr_count: workspace too small");
  Arena ar(ws, ws_bytes);
  CorrWs w;
  corr_carve(ar, c, H, &w);
  O3DX_ARENA_CHECK(ar);
  hipStream_t s = as_stream(stream);
  std::vector<CorrHyp> hyps;
  pack_hyps(T, H, hyps);
  O3DX_HIP(hipMemcpyAsync(w.hyp, hyps.data(), hyps.size() * sizeof(CorrHyp), hipMemcpyHostToDevice, s));
  O3DX_HIP(hipMemsetAsync(w.counts, 0, (size_t)H * sizeof(uint32_t), s));
  hipLaunchKernelGGL(k_corr_gather, dim3(grid_for(c)), dim3(kBlock), 0, s, src, tgt, corr, c, w.pq);
  {
    // slices of the correspondences: enough blocks for the device when there
    // are few hypotheses, at least eight correspondences per lane
    const int64_t want = (4096 + H - 1) / H;
    const unsigned gy = (unsigned)std::min<int64_t>(std::max<int64_t>(std::min<int64_t>(want, (c + 8 * kBlock - 1) / (8 * kBlock)), 1), 1024);
    KTimer kt("corr_count", s);
    hipLaunchKernelGGL(k_corr_count, dim3((unsigned)H, gy), dim3(kBlock), 0, s, w.pq, c, w.hyp, max_d, w.counts);
  }
  O3DX_HIP(hipGetLastError());
  std::vector<uint32_t> out((size_t)H);
  O3DX_TRY(read_back(out.data(), w.counts, (size_t)H * sizeof(uint32_t), s));
  for (int h = 0; h < H; ++h) counts_host[h] = (int64_t)out[(size_t)h];
  return 0;
}

extern "C" int o3dx_corr_error2(const float* src, const float* tgt, const int32_t* corr, int64_t c, const double* T,
                                int H, double max_d, double* sums_host, int64_t* counts_host, void* ws,
                                size_t ws_bytes, void* stream) {
  O3DX_TRY(corr_args("o3dx_corr_error2", src, tgt, corr, c, T, H, max_d));
  if (H > 0 && !sums_host) return fail(O3DX_EINVAL, "o3dx_corr_error2: bad arguments");
  if (H == 0) return 0;
  if (c == 0) {
    for (int h = 0; h < H; ++h) {
      sums_host[h] = 0.0;
      if (counts_host) counts_host[h] = 0;
    }
    return 0;
  }
  if (!ws || ws_bytes < o3dx_corr_count_workspace_bytes(c, H))
    return fail(O3DX_ENOMEM, "o3dx_corr_error2: workspace too small");
  Arena ar(ws, ws_bytes);
  CorrWs w;
  corr_carve(ar, c, H, &w);
  O3DX_ARENA_CHECK(ar);
  hipStream_t s = as_stream(stream);
  std::vector<CorrHyp> hyps;
  pack_hyps(T, H, hyps);
  O3DX_HIP(hipMemcpyAsync(w.hyp, hyps.data(), hyps.size() * sizeof(CorrHyp), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_corr_gather, dim3(grid_for(c)), dim3(kBlock), 0, s, src, tgt, corr, c, w.pq);
  {
    KTimer kt("corr_error2", s);
    hipLaunchKernelGGL(k_corr_error2, dim3((unsigned)H), dim3(kBlock), 0, s, w.pq, c, w.hyp, max_d, w.sums, w.cnt64);
  }
  O3DX_HIP(hipGetLastError());
  if (counts_host) {
    O3DX_HIP(hipMemcpyAsync(counts_host, w.cnt64, (size_t)H * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  }
  return read_back(sums_host, w.sums, (size_t)H * sizeof(double), s);
}
