// las.hip — LAS (ASPRS laser scan format 1.0-1.4, uncompressed) point records
// decoded and encoded on the device.
//
// Replaces the laspy record handling behind the reference's LAS methods
// (reference open3dpypro/PointCloud.py:496-567): read_las / read_las_gen take
// lp.x / lp.y / lp.z (X * scale + offset in float64), lp.red .. / 2^16,
// lp.intensity and lp.raw_classification out of the packed records
// (PointCloud.py:523-547); get_lasdata / save_las / append_save_las quantise
// the coordinates and fill the records (PointCloud.py:499-521, 549-565).  The
// host (las_io.py) parses and writes the public header and moves the record
// block between the file and HBM in one copy; these kernels touch every
// record once, one lane per record.  The stride is the header's record length
// (26, 34, ...: rarely a multiple of 4), so every access is byte-exact.
// Byte work, HBM bound.
#include "common.hpp"

namespace o3dx {

// leading layout of a point format: X, Y, Z int32 at 0, 4, 8 and the intensity
// at 12 in all of them
struct LasLayout {
  int min_len;  // the format's record length without extra bytes
  int cls_off;  // classification byte
  int rgb_off;  // red, green, blue u16 (-1: the format has no colour)
};

static bool las_layout(int fmt, LasLayout* l) {
  static const LasLayout kTable[11] = {{20, 15, -1}, {28, 15, -1}, {26, 15, 20}, {34, 15, 28},
                                       {57, 15, -1}, {63, 15, 28}, {30, 16, -1}, {36, 16, 30},
                                       {38, 16, 30}, {59, 16, -1}, {67, 16, 30}};
  if (fmt < 0 || fmt > 10) return false;
  *l = kTable[fmt];
  return true;
}

template <class T>
__device__ __forceinline__ T las_load(const uint8_t* p) {
  T v;
  __builtin_memcpy(&v, p, sizeof(T));
  return v;
}

template <class T>
__device__ __forceinline__ void las_store(uint8_t* p, T v) {
  __builtin_memcpy(p, &v, sizeof(T));
}

struct LasAffine {
  double scale[3], offset[3];
};

__global__ void __launch_bounds__(kBlock) k_las_unpack(const uint8_t* __restrict__ rec, int64_t n, int64_t stride,
                                                       int cls_off, int rgb_off, LasAffine t,
                                                       double* __restrict__ xyz64, float* __restrict__ xyz32,
                                                       uint16_t* __restrict__ intensity, uint8_t* __restrict__ cls,
                                                       float* __restrict__ rgb, uint32_t* __restrict__ flags) {
  bool wide = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint8_t* p = rec + i * stride;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      // one multiply, then one add (-ffp-contract=off: never an fma)
      const double v = (double)las_load<int32_t>(p + 4 * a) * t.scale[a] + t.offset[a];
      const float f = (float)v;
      if (xyz64) xyz64[3 * i + a] = v;
      if (xyz32) xyz32[3 * i + a] = f;
      wide |= ((double)f != v) && (v == v);
    }
    if (intensity) intensity[i] = las_load<uint16_t>(p + 12);
    if (cls) cls[i] = p[cls_off];
    if (rgb) {
#pragma unroll
      for (int a = 0; a < 3; ++a) rgb[3 * i + a] = (float)las_load<uint16_t>(p + rgb_off + 2 * a) / 65536.0f;
    }
  }
  // one atomic per wave at most, none once the bit is seen set
  if (flags && __any(wide) && lane_id() == 0 && !(*(volatile uint32_t*)flags & O3DX_LAS_FLAG_NOT_F32))
    atomicOr(flags, O3DX_LAS_FLAG_NOT_F32);
}

__global__ void k_las_stats_init(int64_t* stats) {
  if (threadIdx.x < 3) stats[threadIdx.x] = INT32_MAX;
  else if (threadIdx.x < 6) stats[threadIdx.x] = INT32_MIN;
  else if (threadIdx.x < 8) stats[threadIdx.x] = 0;
}

// numpy's (c * 255).astype(np.uint8) for a colour in [0, 1]: the product in
// float64, truncated
__device__ __forceinline__ uint16_t las_colour(float c) {
  const double v = (double)c * 255.0;
  return (v == v) ? (uint16_t)(uint8_t)(long long)v : (uint16_t)0;
}

template <class T>
__global__ void __launch_bounds__(kBlock) k_las_pack(const T* __restrict__ xyz, int64_t n, int64_t stride, int cls_off,
                                                     int rgb_off, LasAffine t, const float* __restrict__ rgb,
                                                     const uint16_t* __restrict__ intensity,
                                                     const uint8_t* __restrict__ cls, uint8_t* __restrict__ rec,
                                                     int64_t* __restrict__ stats) {
  int mn[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, mx[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  int n_over = 0, n_bad = 0;
  const int64_t nblk = (n + kBlock - 1) / kBlock;
  for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {
    // the block's records are one byte range: cleared with wide stores by the
    // whole block, then every lane writes its record's fields
    const int64_t r0 = b * kBlock, r1 = std::min<int64_t>(n, r0 + kBlock);
    {
      uint8_t* z = rec + r0 * stride;
      const size_t bytes = (size_t)((r1 - r0) * stride);
      const size_t head = std::min(bytes, (size_t)((16 - (reinterpret_cast<uintptr_t>(z) & 15)) & 15));
      const size_t nv = (bytes - head) / 16;
      uint4* q = reinterpret_cast<uint4*>(z + head);
      for (size_t k = threadIdx.x; k < nv; k += kBlock) q[k] = make_uint4(0, 0, 0, 0);
      for (size_t k = threadIdx.x; k < head; k += kBlock) z[k] = 0;
      for (size_t k = head + nv * 16 + threadIdx.x; k < bytes; k += kBlock) z[k] = 0;
    }
    __syncthreads();  // the clears are ordered before the field stores below
    const int64_t i = r0 + threadIdx.x;
    if (i < r1) {
      uint8_t* p = rec + i * stride;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double v = (double)xyz[3 * i + a];
        const double q = rint((v - t.offset[a]) / t.scale[a]);  // ties to even: np.round
        int X = 0;
        if (!(fabs(q) <= 1.7976931348623157e308)) {  // NaN or infinite
          ++n_bad;
        } else if (q < -2147483648.0 || q > 2147483647.0) {
          ++n_over;
        } else {
          X = (int)q;
          mn[a] = min(mn[a], X);
          mx[a] = max(mx[a], X);
        }
        las_store<int32_t>(p + 4 * a, X);
      }
      if (intensity) las_store<uint16_t>(p + 12, intensity[i]);
      if (cls) p[cls_off] = cls[i];
      if (rgb) {
#pragma unroll
        for (int a = 0; a < 3; ++a) las_store<uint16_t>(p + rgb_off + 2 * a, las_colour(rgb[3 * i + a]));
      }
    }
  }
  // wave reduction, the block's four waves through LDS, then one vector atomic
  // per word and block (thousands of same-address atomics serialise in L2)
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    mn[a] = wave_min(mn[a]);
    mx[a] = wave_max(mx[a]);
  }
  n_over = wave_sum(n_over);
  n_bad = wave_sum(n_bad);
  __shared__ int sh[kBlock / 64][8];
  if (lane_id() == 0) {
    int* r = sh[threadIdx.x >> 6];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      r[a] = mn[a];
      r[3 + a] = mx[a];
    }
    r[6] = n_over;
    r[7] = n_bad;
  }
  __syncthreads();
  const int c = threadIdx.x;
  if (c < 8) {
    int v = sh[0][c];
    for (int w = 1; w < kBlock / 64; ++w) v = c < 3 ? min(v, sh[w][c]) : c < 6 ? max(v, sh[w][c]) : v + sh[w][c];
    if (c < 3) {
      if (v != INT32_MAX) atomicMin((long long*)&stats[c], (long long)v);
    } else if (c < 6) {
      if (v != INT32_MIN) atomicMax((long long*)&stats[c], (long long)v);
    } else if (v) {
      atomicAdd((unsigned long long*)&stats[c], (unsigned long long)v);
    }
  }
}

static int las_affine(const double* scale, const double* offset, LasAffine* t, const char* who) {
  if (!scale || !offset) return fail(O3DX_EINVAL, "%s: null scale / offset", who);
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(scale[a]) || scale[a] == 0.0 || !std::isfinite(offset[a]))
      return fail(O3DX_EINVAL, "%s: scale must be finite and non-zero, offset finite (axis %d)", who, a);
    t->scale[a] = scale[a];
    t->offset[a] = offset[a];
  }
  return 0;
}

}  // namespace o3dx

using namespace o3dx;

extern "C" int o3dx_las_unpack(const uint8_t* rec, int64_t n, int64_t stride, int point_format, const double* scale,
                               const double* offset, double* xyz64_out, float* xyz32_out, uint16_t* intensity_out,
                               uint8_t* cls_out, float* rgb_out, uint32_t* flags, void* stream) {
  LasLayout l;
  if (!las_layout(point_format, &l)) return fail(O3DX_EINVAL, "o3dx_las_unpack: point format %d (0..10)", point_format);
  if (n < 0 || stride < l.min_len || stride > 65535 || (n > 0 && !rec))
    return fail(O3DX_EINVAL, "o3dx_las_unpack: bad arguments (n %lld, stride %lld, format %d needs >= %d)",
                (long long)n, (long long)stride, point_format, l.min_len);
  if (rgb_out && l.rgb_off < 0)
    return fail(O3DX_EINVAL, "o3dx_las_unpack: point format %d has no colour", point_format);
  LasAffine t;
  O3DX_TRY(las_affine(scale, offset, &t, "o3dx_las_unpack"));
  hipStream_t s = as_stream(stream);
  if (flags) O3DX_HIP(hipMemsetAsync(flags, 0, sizeof(uint32_t), s));
  if (n == 0) return 0;
  KTimer kt("las_unpack", s);
  hipLaunchKernelGGL(k_las_unpack, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, s, rec, n, stride, l.cls_off,
                     l.rgb_off, t, xyz64_out, xyz32_out, intensity_out, cls_out, rgb_out, flags);
  O3DX_HIP(hipGetLastError());
  return 0;
}

extern "C" int o3dx_las_pack(const void* xyz, int xyz_f64, int64_t n, int64_t stride, int point_format,
                             const double* scale, const double* offset, const float* rgb, const uint16_t* intensity,
                             const uint8_t* cls, uint8_t* rec_out, int64_t* stats, void* stream) {
  LasLayout l;
  const bool writable = las_layout(point_format, &l) && point_format != 4 && point_format != 5 && point_format <= 8;
  if (!writable) return fail(O3DX_EINVAL, "o3dx_las_pack: point format %d (0..3, 6..8)", point_format);
  if (n < 0 || stride < l.min_len || stride > 65535 || (n > 0 && (!xyz || !rec_out)) || !stats)
    return fail(O3DX_EINVAL, "o3dx_las_pack: bad arguments (n %lld, stride %lld, format %d needs >= %d)",
                (long long)n, (long long)stride, point_format, l.min_len);
  if (rgb && l.rgb_off < 0) return fail(O3DX_EINVAL, "o3dx_las_pack: point format %d has no colour", point_format);
  LasAffine t;
  O3DX_TRY(las_affine(scale, offset, &t, "o3dx_las_pack"));
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(k_las_stats_init, dim3(1), dim3(64), 0, s, stats);
  O3DX_HIP(hipGetLastError());
  if (n == 0) return 0;
  KTimer kt("las_pack", s);
  const dim3 grid(grid_for(n, kBlock, 2048)), block(kBlock);
  if (xyz_f64)
    hipLaunchKernelGGL(k_las_pack<double>, grid, block, 0, s, (const double*)xyz, n, stride, l.cls_off, l.rgb_off, t,
                       rgb, intensity, cls, rec_out, stats);
  else
    hipLaunchKernelGGL(k_las_pack<float>, grid, block, 0, s, (const float*)xyz, n, stride, l.cls_off, l.rgb_off, t, rgb,
                       intensity, cls, rec_out, stats);
  O3DX_HIP(hipGetLastError());
  return 0;
}
