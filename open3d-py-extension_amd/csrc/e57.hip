// e57.hip — E57 (ASTM E2807) files checked, decoded and encoded on the device.
//
// Replaces the pye57 / libE57 byte work behind the reference's E57 methods
// (reference open3dpypro/PointCloud.py:569-703, open3dpypro/E57File.py).  The
// host (e57_io.py) parses the file header, the XML and the packet headers and
// hands over, per prototype field, a segment table {stream byte offset,
// logical file offset, length}; the file's bytes are in HBM once, paged as on
// disk (1020 payload bytes + a big-endian CRC32C per 1024-byte page).
//   k_e57_crc_pages  every page's checksum against its trailer
//   k_e57_unpack     records straight from the paged bytes, one lane per record
//   k_e57_pack       one scan's packets, one lane per output word (gather form)
//   k_e57_seal       logical bytes into pages, each with its trailer
// Byte work, HBM bound; include/o3dx.h "E57 IO" states the rules.
#include "common.hpp"

namespace o3dx {

constexpr int kE57Page = 1024;
constexpr int kE57Payload = 1020;
constexpr int kE57MaxFields = 10;      // one per O3DX_E57_ROLE_*
constexpr int kE57MaxPackFields = 13;  // x y z, intensity, r g b, row, column, normal x y z + 1
constexpr int kE57MaxHead = 6 + 2 * kE57MaxPackFields;

// ------------------------------------------------------------------ CRC32C
// Castagnoli, reflected 0x82F63B78; slice-by-8 tables (row 0: the byte table)
struct CrcTables {
  uint32_t t[8][256];
};
constexpr CrcTables make_crc_tables() {
  CrcTables r{};
  for (int i = 0; i < 256; ++i) {
    uint32_t c = (uint32_t)i;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
    r.t[0][i] = c;
  }
  for (int k = 1; k < 8; ++k)
    for (int i = 0; i < 256; ++i) r.t[k][i] = r.t[0][r.t[k - 1][i] & 0xffu] ^ (r.t[k - 1][i] >> 8);
  return r;
}
__device__ const CrcTables kCrc = make_crc_tables();

// A tile is 64 pages, one per lane of the block's single wave.  A staged page
// takes 257 words: at 256 every lane's word i would sit on one LDS bank, at
// 257 lane l's word i is on bank (l + i) mod 32 — conflict-free in each
// 32-lane half.  64 x 1028 B + 8 KiB of tables = 73,984 B: two blocks per CU.
constexpr int kCrcLanes = 64;
constexpr int kCrcStride = 257;

__device__ __forceinline__ void crc_stage_tables(uint32_t* tab) {
  const uint32_t* g = &kCrc.t[0][0];
  for (int i = threadIdx.x; i < 8 * 256; i += kCrcLanes) tab[i] = g[i];
}

// CRC32C of the 255 payload words of one staged page
__device__ __forceinline__ uint32_t crc_walk(const uint32_t* __restrict__ pg, const uint32_t* __restrict__ tab) {
  uint32_t crc = 0xffffffffu;
  for (int i = 0; i < 254; i += 2) {
    const uint32_t a = crc ^ pg[i], b = pg[i + 1];
    crc = tab[7 * 256 + (a & 0xff)] ^ tab[6 * 256 + ((a >> 8) & 0xff)] ^ tab[5 * 256 + ((a >> 16) & 0xff)] ^
          tab[4 * 256 + (a >> 24)] ^ tab[3 * 256 + (b & 0xff)] ^ tab[2 * 256 + ((b >> 8) & 0xff)] ^
          tab[1 * 256 + ((b >> 16) & 0xff)] ^ tab[b >> 24];
  }
  const uint32_t a = crc ^ pg[254];
  crc = tab[3 * 256 + (a & 0xff)] ^ tab[2 * 256 + ((a >> 8) & 0xff)] ^ tab[1 * 256 + ((a >> 16) & 0xff)] ^
        tab[a >> 24];
  return ~crc;
}

__global__ void k_e57_crc_init(int64_t* out2) {
  if (threadIdx.x == 0) out2[0] = 0;
  if (threadIdx.x == 1) out2[1] = INT64_MAX;
}

__global__ void __launch_bounds__(kCrcLanes) k_e57_crc_pages(const uint8_t* __restrict__ file, int64_t n_pages,
                                                             int64_t* __restrict__ out2) {
  __shared__ uint32_t tab[8 * 256];
  __shared__ uint32_t buf[kCrcLanes * kCrcStride];
  crc_stage_tables(tab);
  const int l = threadIdx.x;
  const int64_t tiles = (n_pages + kCrcLanes - 1) / kCrcLanes;
  int bad = 0;
  int64_t first = INT64_MAX;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t base = tile * kCrcLanes;
    const int np = (int)std::min<int64_t>(kCrcLanes, n_pages - base);
    // coalesced: one page per wave instruction, 16 B per lane
    const uint4* g = reinterpret_cast<const uint4*>(file + base * kE57Page);
#pragma unroll 4
    for (int k = 0; k < np; ++k) {
      const uint4 v = g[k * 64 + l];
      uint32_t* d = buf + k * kCrcStride + 4 * l;
      d[0] = v.x;
      d[1] = v.y;
      d[2] = v.z;
      d[3] = v.w;
    }
    __syncthreads();
    if (l < np) {
      const uint32_t* pg = buf + l * kCrcStride;
      const uint32_t want = __builtin_bswap32(pg[255]);  // the trailer is big-endian
      if (crc_walk(pg, tab) != want) {
        ++bad;
        first = std::min<int64_t>(first, base + l);
      }
    }
    __syncthreads();
  }
  bad = wave_sum(bad);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) first = std::min<int64_t>(first, __shfl_xor(first, o, 64));
  if (l == 0 && bad) {
    atomicAdd((unsigned long long*)&out2[0], (unsigned long long)bad);
    atomicMin((long long*)&out2[1], (long long)first);
  }
}

__global__ void __launch_bounds__(kCrcLanes) k_e57_seal(const uint32_t* __restrict__ logical, int64_t logical_words,
                                                        uint32_t* __restrict__ paged, int64_t n_pages) {
  __shared__ uint32_t tab[8 * 256];
  __shared__ uint32_t buf[kCrcLanes * kCrcStride];
  crc_stage_tables(tab);
  const int l = threadIdx.x;
  const int64_t tiles = (n_pages + kCrcLanes - 1) / kCrcLanes;
  // 16-byte accesses when both buffers allow them (a tile is 65,280 logical and 65,536 paged bytes)
  const bool wide = ((reinterpret_cast<uintptr_t>(logical) | reinterpret_cast<uintptr_t>(paged)) & 15) == 0;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t base = tile * kCrcLanes;
    const int np = (int)std::min<int64_t>(kCrcLanes, n_pages - base);
    const int64_t w0 = base * 255;
    if (wide && w0 + kCrcLanes * 255 <= logical_words) {
      // a whole tile: 64 x 1020 bytes, 16 B per lane (the tile's start is 16-byte aligned)
      const uint4* g = reinterpret_cast<const uint4*>(logical + w0);
#pragma unroll 5
      for (int q = l; q < kCrcLanes * 255 / 4; q += kCrcLanes) {
        const uint4 v = g[q];
        const int t = 4 * q;
        buf[(t / 255) * kCrcStride + t % 255] = v.x;
        buf[((t + 1) / 255) * kCrcStride + (t + 1) % 255] = v.y;
        buf[((t + 2) / 255) * kCrcStride + (t + 2) % 255] = v.z;
        buf[((t + 3) / 255) * kCrcStride + (t + 3) % 255] = v.w;
      }
    } else {
#pragma unroll 4
      for (int t = l; t < np * 255; t += kCrcLanes) {
        const int64_t wi = w0 + t;
        buf[(t / 255) * kCrcStride + t % 255] = wi < logical_words ? logical[wi] : 0u;  // the last page's padding
      }
    }
    __syncthreads();
    if (l < np) {
      uint32_t* pg = buf + l * kCrcStride;
      pg[255] = __builtin_bswap32(crc_walk(pg, tab));
    }
    __syncthreads();
    if (wide) {
      uint4* out = reinterpret_cast<uint4*>(paged + base * 256);
#pragma unroll 4
      for (int q = l; q < np * 64; q += kCrcLanes) {  // one page per wave instruction
        const uint32_t* s = buf + (q >> 6) * kCrcStride + 4 * (q & 63);
        out[q] = make_uint4(s[0], s[1], s[2], s[3]);
      }
    } else {
      uint32_t* out = paged + base * 256;
      for (int t = l; t < np * 256; t += kCrcLanes) out[t] = buf[(t >> 8) * kCrcStride + (t & 255)];
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------- unpack
struct E57UnpackField {
  int role, kind, bits, seg_count;
  int64_t minimum, seg_begin;
  double scale, offset;
};
struct E57UnpackArgs {
  int nf, has_pose;
  double pose[12];
  E57UnpackField f[kE57MaxFields];
};

template <class T>
__device__ __forceinline__ T e57_load(const uint8_t* p) {
  T v;
  __builtin_memcpy(&v, p, sizeof(T));
  return v;
}

// The last segment row whose stream offset is <= s (-1: none).  A writer's
// packets are nearly equal, so the row is guessed by interpolation, bracketed
// by doubling steps from the guess, then found by binary search in the
// bracket: a few reads for a regular file, O(log rows) for any table.
__device__ __forceinline__ int e57_segment_of(const int64_t* __restrict__ seg, int count, int64_t s) {
  if (count <= 0 || seg[0] > s) return -1;
  const int last = count - 1;
  const int64_t total = seg[3 * last] + seg[3 * last + 2];
  int g = last;
  if (total > 0 && s < total)  // a float guess is enough: the steps below correct it
    g = std::min(last, std::max(0, (int)(((float)s / (float)total) * (float)count)));
  int lo, hi;
  if (seg[3 * g] <= s) {
    lo = g;
    hi = last;
    for (int step = 1; lo + step <= last; step <<= 1) {
      if (seg[3 * (lo + step)] <= s) {
        lo += step;
      } else {
        hi = lo + step - 1;
        break;
      }
    }
  } else {
    lo = 0;  // seg[0] <= s
    hi = g - 1;
    for (int step = 1; hi - step > 0; step <<= 1) {
      if (seg[3 * (hi - step)] <= s) {
        lo = hi - step;
        break;
      }
      hi -= step + 1;
    }
  }
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg[3 * mid] <= s) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The `bits` bits of record r of one field: stream bit r * bits, LSB first.
// Contiguous bytes are read at once; otherwise every byte is fetched on its
// own (a value may straddle a page trailer and a segment end).  A byte
// outside the table or the file sets *range and reads as 0.
__device__ __forceinline__ uint64_t e57_fetch(const uint8_t* __restrict__ file, int64_t file_bytes,
                                              const int64_t* __restrict__ seg, int seg_count, uint64_t r, int bits,
                                              bool* range) {
  if (bits == 0) return 0;
  const uint64_t bit = r * (uint64_t)bits;
  int64_t s = (int64_t)(bit >> 3);
  const int sh = (int)(bit & 7);
  const int nbytes = (sh + bits + 7) >> 3;  // <= 9
  const int j0 = e57_segment_of(seg, seg_count, s);
  int j = j0 < 0 ? 0 : j0;
  int64_t end = 0, phys = 0;
  bool live = false;
  if (j0 >= 0) {
    end = seg[3 * j] + seg[3 * j + 2];
    const int64_t lg = seg[3 * j + 1] + (s - seg[3 * j]);
    phys = lg + 4 * (lg / kE57Payload);
    live = true;
  }
  uint64_t low = 0;
  uint32_t top = 0;
  if (live && s + nbytes <= end && phys >= 0 && (phys & (kE57Page - 1)) + nbytes <= kE57Payload &&
      phys + 9 <= file_bytes) {
    // the usual case: the value's bytes are contiguous in one segment and one page
    low = e57_load<uint64_t>(file + phys);
    if (nbytes > 8) top = file[phys + 8];
    uint64_t v = low >> sh;
    if (sh) v |= (uint64_t)top << (64 - sh);
    if (bits < 64) v &= (1ull << bits) - 1ull;
    return v;
  }
  for (int k = 0; k < nbytes; ++k, ++s) {
    while (live && s >= end) {  // the next segment of the stream
      if (++j >= seg_count) {
        live = false;
        break;
      }
      end = seg[3 * j] + seg[3 * j + 2];
      const int64_t lg = seg[3 * j + 1] + (s - seg[3 * j]);
      phys = lg + 4 * (lg / kE57Payload);
    }
    uint32_t byte = 0;
    if (live && (uint64_t)phys < (uint64_t)file_bytes) byte = file[phys];
    else *range = true;
    if (k < 8) low |= (uint64_t)byte << (8 * k);
    else top = byte;
    ++phys;
    if ((phys & (kE57Page - 1)) == kE57Payload) phys += 4;  // over the page trailer
  }
  uint64_t v = low >> sh;
  if (sh) v |= (uint64_t)top << (64 - sh);
  if (bits < 64) v &= (1ull << bits) - 1ull;
  return v;
}

__global__ void __launch_bounds__(kBlock) k_e57_unpack(const uint8_t* __restrict__ file, int64_t file_bytes,
                                                       const int64_t* __restrict__ seg, E57UnpackArgs a, int64_t r0,
                                                       int64_t n, double* __restrict__ xyz64, float* __restrict__ xyz32,
                                                       uint8_t* __restrict__ rgb, float* __restrict__ intensity,
                                                       uint16_t* __restrict__ row, uint16_t* __restrict__ col,
                                                       int8_t* __restrict__ invalid, uint32_t* __restrict__ flags) {
  bool wide = false, range = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double x = 0.0, y = 0.0, z = 0.0;
    for (int k = 0; k < a.nf; ++k) {
      const E57UnpackField& f = a.f[k];
      const uint64_t raw = e57_fetch(file, file_bytes, seg + 3 * f.seg_begin, f.seg_count, (uint64_t)(r0 + i), f.bits,
                                     &range);
      int64_t iv = 0;
      double dv;
      float fv;
      if (f.kind == O3DX_E57_KIND_F32) {
        fv = __uint_as_float((uint32_t)raw);
        dv = (double)fv;  // exact
      } else if (f.kind == O3DX_E57_KIND_F64) {
        dv = __longlong_as_double((long long)raw);
        fv = (float)dv;
      } else {
        iv = (int64_t)((uint64_t)f.minimum + raw);
        if (f.kind == O3DX_E57_KIND_INT) {
          dv = (double)iv;
          fv = (float)iv;  // one rounding, as numpy's int64 -> float32
        } else {
          dv = (double)iv * f.scale + f.offset;  // one multiply, then one add (-ffp-contract=off)
          fv = (float)dv;
        }
      }
      switch (f.role) {
        case O3DX_E57_ROLE_X: x = dv; break;
        case O3DX_E57_ROLE_Y: y = dv; break;
        case O3DX_E57_ROLE_Z: z = dv; break;
        case O3DX_E57_ROLE_INTENSITY: intensity[i] = fv; break;
        case O3DX_E57_ROLE_RED:
        case O3DX_E57_ROLE_GREEN:
        case O3DX_E57_ROLE_BLUE: rgb[3 * i + (f.role - O3DX_E57_ROLE_RED)] = (uint8_t)iv; break;
        case O3DX_E57_ROLE_ROW: row[i] = (uint16_t)iv; break;
        case O3DX_E57_ROLE_COLUMN: col[i] = (uint16_t)iv; break;
        default: invalid[i] = (int8_t)iv; break;
      }
    }
    if (xyz64 || xyz32 || flags) {
      double p[3] = {x, y, z};
      if (a.has_pose) {
        const double* m = a.pose;
        p[0] = ((m[0] * x + m[1] * y) + m[2] * z) + m[9];
        p[1] = ((m[3] * x + m[4] * y) + m[5] * z) + m[10];
        p[2] = ((m[6] * x + m[7] * y) + m[8] * z) + m[11];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float f32 = (float)p[c];
        if (xyz64) xyz64[3 * i + c] = p[c];
        if (xyz32) xyz32[3 * i + c] = f32;
        wide |= ((double)f32 != p[c]) && (p[c] == p[c]);
      }
    }
  }
  if (flags) {
    // one atomic per wave and bit at most, none once the bit is seen set
    const uint32_t seen = *(volatile uint32_t*)flags;
    uint32_t add = 0;
    if (__any(wide) && !(seen & O3DX_E57_FLAG_NOT_F32)) add |= O3DX_E57_FLAG_NOT_F32;
    if (__any(range) && !(seen & O3DX_E57_FLAG_RANGE)) add |= O3DX_E57_FLAG_RANGE;
    if (add && lane_id() == 0) atomicOr(flags, add);
  }
}

// --------------------------------------------------------------------- pack
struct E57PackField {
  const void* src;
  int64_t stride, first, minimum;
  int kind, bits;
  int off_full, off_last, len_full, len_last;
};
struct E57PackArgs {
  int nf, head;
  int full_bytes, last_bytes;
  int64_t R, packets, last_rec;
  uint8_t head_full[kE57MaxHead + 2], head_last[kE57MaxHead + 2];
  E57PackField f[kE57MaxPackFields];
};

// the unsigned bit field of record i of a source column
__device__ __forceinline__ uint64_t e57_source(const E57PackField& f, int64_t i) {
  const int64_t e = f.first + i * f.stride;
  uint64_t v;
  if (f.kind == O3DX_E57_SRC_F32) {
    v = __float_as_uint(((const float*)f.src)[e]);
  } else if (f.kind == O3DX_E57_SRC_F64) {
    v = (uint64_t)__double_as_longlong(((const double*)f.src)[e]);
  } else if (f.kind == O3DX_E57_SRC_COLOUR) {
    // numpy's (c * 255).astype(np.uint8) for a colour in [0, 1]: the product in float64, truncated
    const double c = (double)((const float*)f.src)[e] * 255.0;
    v = (c == c) ? (uint64_t)(uint8_t)(long long)c : 0ull;
  } else {
    v = (uint64_t)((const int64_t*)f.src)[e] - (uint64_t)f.minimum;
  }
  return f.bits < 64 ? v & ((1ull << f.bits) - 1ull) : v;
}

// bits [bit_lo, bit_lo + nb) (nb <= 32) of a field's stream inside one packet,
// gathered from the records that overlap them
__device__ __forceinline__ uint32_t e57_gather(const E57PackField& f, int64_t rec0, int nrec, int bit_lo, int nb) {
  // positions inside one packet fit 32 bits (a stream is < 65,536 bytes)
  uint64_t acc = 0;
  const unsigned first = (unsigned)bit_lo / (unsigned)f.bits;
  int rel = (int)(first * (unsigned)f.bits) - bit_lo;  // <= 0 for the first record
  for (int r = (int)first; r < nrec && rel < nb; ++r, rel += f.bits) {
    const uint64_t v = e57_source(f, rec0 + r);
    acc |= rel >= 0 ? v << rel : v >> (-rel);
  }
  return (uint32_t)(nb < 32 ? acc & ((1ull << nb) - 1ull) : acc);
}

__device__ __forceinline__ int e57_field_at(const E57PackArgs& a, bool last, int o, int* off, int* len) {
  for (int k = 0; k < a.nf; ++k) {
    const int of = last ? a.f[k].off_last : a.f[k].off_full, ln = last ? a.f[k].len_last : a.f[k].len_full;
    if (o >= of && o < of + ln) {
      *off = of;
      *len = ln;
      return k;
    }
  }
  return -1;
}

__global__ void __launch_bounds__(kBlock) k_e57_pack(E57PackArgs a, int64_t words, uint32_t* __restrict__ out) {
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b0 = 4 * w;
    const uint32_t wf = (uint32_t)a.full_bytes >> 2;  // words per full packet; 32-bit division where it fits
    const int64_t p = std::min<int64_t>(w <= 0xffffffffll ? (int64_t)((uint32_t)w / wf) : w / wf, a.packets - 1);
    const int o = (int)(b0 - p * a.full_bytes);
    const bool last = p == a.packets - 1;
    const int64_t rec0 = p * a.R;
    const int nrec = (int)(last ? a.last_rec : a.R);
    const uint8_t* head = last ? a.head_last : a.head_full;
    int off = 0, len = 0;
    const int k = o >= a.head ? e57_field_at(a, last, o, &off, &len) : -1;
    uint32_t word = 0;
    if (k >= 0 && o + 4 <= off + len) {
      word = e57_gather(a.f[k], rec0, nrec, (o - off) * 8, 32);
    } else {
      for (int b = 0; b < 4; ++b) {  // a word across the header, two streams or the padding
        const int ob = o + b;
        uint32_t byte = 0;
        if (ob < a.head) {
          byte = head[ob];
        } else {
          const int kb = e57_field_at(a, last, ob, &off, &len);
          if (kb >= 0) byte = e57_gather(a.f[kb], rec0, nrec, (ob - off) * 8, 8);
        }
        word |= byte << (8 * b);
      }
    }
    out[w] = word;
  }
}

}  // namespace o3dx

using namespace o3dx;

extern "C" int o3dx_e57_crc_pages(const uint8_t* file, int64_t n_pages, int64_t* out2, void* stream) {
  if (n_pages < 0 || !out2 || (n_pages > 0 && !file) || (reinterpret_cast<uintptr_t>(file) & 15))
    return fail(O3DX_EINVAL, "o3dx_e57_crc_pages: bad arguments (pages %lld; the bytes must be 16-byte aligned)",
                (long long)n_pages);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(k_e57_crc_init, dim3(1), dim3(64), 0, s, out2);
  O3DX_HIP(hipGetLastError());
  if (n_pages == 0) return 0;
  KTimer kt("e57_crc_pages", s);
  const int64_t tiles = (n_pages + kCrcLanes - 1) / kCrcLanes;
  hipLaunchKernelGGL(k_e57_crc_pages, dim3(grid_for(tiles, 1, 4096)), dim3(kCrcLanes), 0, s, file, n_pages, out2);
  O3DX_HIP(hipGetLastError());
  return 0;
}

extern "C" int o3dx_e57_seal(const uint8_t* logical, int64_t logical_bytes, uint8_t* paged, int64_t n_pages,
                             void* stream) {
  if (logical_bytes < 0 || n_pages < 0 || (logical_bytes & 3) || (logical_bytes > 0 && !logical) ||
      (n_pages > 0 && !paged) || logical_bytes > n_pages * kE57Payload ||
      ((reinterpret_cast<uintptr_t>(logical) | reinterpret_cast<uintptr_t>(paged)) & 3))
    return fail(O3DX_EINVAL,
                "o3dx_e57_seal: bad arguments (%lld logical bytes, a multiple of 4 and 4-byte aligned, into %lld "
                "pages)", (long long)logical_bytes, (long long)n_pages);
  if (n_pages == 0) return 0;
  hipStream_t s = as_stream(stream);
  KTimer kt("e57_seal", s);
  const int64_t tiles = (n_pages + kCrcLanes - 1) / kCrcLanes;
  hipLaunchKernelGGL(k_e57_seal, dim3(grid_for(tiles, 1, 4096)), dim3(kCrcLanes), 0, s, (const uint32_t*)logical,
                     logical_bytes / 4, (uint32_t*)paged, n_pages);
  O3DX_HIP(hipGetLastError());
  return 0;
}

extern "C" int o3dx_e57_unpack(const uint8_t* file, int64_t file_bytes, int n_fields, const int64_t* desc,
                               const double* affine, const int64_t* seg, int64_t seg_rows, int64_t r0, int64_t n,
                               const double* pose, double* xyz64_out, float* xyz32_out, uint8_t* rgb_out,
                               float* intensity_out, uint16_t* row_out, uint16_t* col_out, int8_t* invalid_out,
                               uint32_t* flags, void* stream) {
  if (n_fields < 1 || n_fields > kE57MaxFields || !desc || !affine || file_bytes < 0 || (file_bytes > 0 && !file) ||
      seg_rows < 0 || (seg_rows > 0 && !seg) || r0 < 0 || n < 0 || r0 > (INT64_MAX >> 7) - n)
    return fail(O3DX_EINVAL, "o3dx_e57_unpack: bad arguments (%d fields, records [%lld, +%lld))", n_fields,
                (long long)r0, (long long)n);
  E57UnpackArgs a;
  a.nf = 0;
  a.has_pose = pose ? 1 : 0;
  for (int c = 0; c < 12; ++c) a.pose[c] = pose ? pose[c] : 0.0;
  unsigned seen = 0;
  for (int k = 0; k < n_fields; ++k) {
    const int64_t* d = desc + 6 * k;
    E57UnpackField f;
    f.role = (int)d[0];
    f.kind = (int)d[1];
    f.bits = (int)d[2];
    f.minimum = d[3];
    f.seg_begin = d[4];
    f.seg_count = (int)d[5];
    f.scale = affine[2 * k];
    f.offset = affine[2 * k + 1];
    if (d[0] < 0 || d[0] > O3DX_E57_ROLE_INVALID || (seen >> f.role & 1u))
      return fail(O3DX_EINVAL, "o3dx_e57_unpack: field %d has role %lld (0..%d, each once)", k, (long long)d[0],
                  O3DX_E57_ROLE_INVALID);
    seen |= 1u << f.role;
    const bool kind_ok = (f.kind == O3DX_E57_KIND_F32 && d[2] == 32) || (f.kind == O3DX_E57_KIND_F64 && d[2] == 64) ||
                         ((f.kind == O3DX_E57_KIND_INT || f.kind == O3DX_E57_KIND_SCALED) && d[2] >= 0 && d[2] <= 64);
    if (!kind_ok) return fail(O3DX_EINVAL, "o3dx_e57_unpack: field %d has kind %d with %lld bits", k, f.kind,
                              (long long)d[2]);
    if (f.role >= O3DX_E57_ROLE_RED && f.kind != O3DX_E57_KIND_INT)
      return fail(O3DX_EINVAL, "o3dx_e57_unpack: field %d (role %d) must be an Integer field", k, f.role);
    if (d[4] < 0 || d[5] < 0 || d[5] > INT32_MAX || d[4] > seg_rows - d[5])
      return fail(O3DX_EINVAL, "o3dx_e57_unpack: field %d segments [%lld, +%lld) leave the table of %lld rows", k,
                  (long long)d[4], (long long)d[5], (long long)seg_rows);
    // a column nobody asked for is not decoded
    const bool used = f.role <= O3DX_E57_ROLE_Z ? (xyz64_out || xyz32_out || flags)
                      : f.role == O3DX_E57_ROLE_INTENSITY ? intensity_out != nullptr
                      : f.role <= O3DX_E57_ROLE_BLUE ? rgb_out != nullptr
                      : f.role == O3DX_E57_ROLE_ROW ? row_out != nullptr
                      : f.role == O3DX_E57_ROLE_COLUMN ? col_out != nullptr : invalid_out != nullptr;
    if (used) a.f[a.nf++] = f;
  }
  const unsigned xyz = 7u, col3 = 7u << O3DX_E57_ROLE_RED;
  if (((xyz64_out || xyz32_out) && (seen & xyz) != xyz) || (rgb_out && (seen & col3) != col3) ||
      (intensity_out && !(seen >> O3DX_E57_ROLE_INTENSITY & 1u)) || (row_out && !(seen >> O3DX_E57_ROLE_ROW & 1u)) ||
      (col_out && !(seen >> O3DX_E57_ROLE_COLUMN & 1u)) || (invalid_out && !(seen >> O3DX_E57_ROLE_INVALID & 1u)))
    return fail(O3DX_EINVAL, "o3dx_e57_unpack: an output column was given without its field(s) (roles seen %#x)", seen);
  hipStream_t s = as_stream(stream);
  if (flags) O3DX_HIP(hipMemsetAsync(flags, 0, sizeof(uint32_t), s));
  if (n == 0) return 0;
  KTimer kt("e57_unpack", s);
  hipLaunchKernelGGL(k_e57_unpack, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, s, file, file_bytes, seg, a, r0,
                     n, xyz64_out, xyz32_out, rgb_out, intensity_out, row_out, col_out, invalid_out, flags);
  O3DX_HIP(hipGetLastError());
  return 0;
}

extern "C" int o3dx_e57_pack(int n_fields, const int64_t* desc, const void* const* src, const int64_t* stride,
                             int64_t n, int64_t records_per_packet, int64_t full_bytes, int64_t last_bytes,
                             const uint8_t* head_full, const uint8_t* head_last, uint8_t* out, void* stream) {
  const int64_t R = records_per_packet;
  if (n_fields < 1 || n_fields > kE57MaxPackFields || !desc || !src || !stride || n < 0 || R < 8 || (R & 7) ||
      !head_full || !head_last)
    return fail(O3DX_EINVAL, "o3dx_e57_pack: bad arguments (%d fields, n %lld, %lld records per packet: a multiple "
                "of 8)", n_fields, (long long)n, (long long)R);
  if (n == 0) return 0;
  E57PackArgs a;
  a.nf = n_fields;
  a.head = 6 + 2 * n_fields;
  a.R = R;
  a.packets = (n + R - 1) / R;
  a.last_rec = n - (a.packets - 1) * R;
  if (full_bytes < a.head || full_bytes > 65536 || (full_bytes & 3) || last_bytes < a.head || last_bytes > full_bytes ||
      (last_bytes & 3) || !out || (reinterpret_cast<uintptr_t>(out) & 3))
    return fail(O3DX_EINVAL, "o3dx_e57_pack: packets of %lld / %lld bytes (multiples of 4, header %d .. 65536; the "
                "output 4-byte aligned)", (long long)full_bytes, (long long)last_bytes, a.head);
  a.full_bytes = (int)full_bytes;
  a.last_bytes = (int)last_bytes;
  for (int c = 0; c < a.head; ++c) {
    a.head_full[c] = head_full[c];
    a.head_last[c] = head_last[c];
  }
  int64_t at_full = a.head, at_last = a.head;
  for (int k = 0; k < n_fields; ++k) {
    const int64_t* d = desc + 6 * k;
    E57PackField& f = a.f[k];
    const int64_t bits = d[1], len_full = R / 8 * bits, len_last = (a.last_rec * bits + 7) / 8;
    const bool kind_ok = (d[0] == O3DX_E57_SRC_F32 && bits == 32) || (d[0] == O3DX_E57_SRC_F64 && bits == 64) ||
                         (d[0] == O3DX_E57_SRC_COLOUR && bits == 8) || (d[0] == O3DX_E57_SRC_I64 && bits >= 0 &&
                                                                        bits <= 64);
    if (!kind_ok) return fail(O3DX_EINVAL, "o3dx_e57_pack: field %d has source %lld with %lld bits", k,
                              (long long)d[0], (long long)bits);
    if (d[3] < at_full || d[3] + len_full > full_bytes || d[4] < at_last || d[5] != len_last ||
        d[4] + len_last > last_bytes || (bits > 0 && !src[k]) || stride[2 * k] < 0 || stride[2 * k + 1] < 0)
      return fail(O3DX_EINVAL, "o3dx_e57_pack: field %d stream at %lld / %lld (%lld / %lld bytes) leaves its packet "
                  "or overlaps the field before", k, (long long)d[3], (long long)d[4], (long long)len_full,
                  (long long)d[5]);
    f.src = src[k];
    f.stride = stride[2 * k];
    f.first = stride[2 * k + 1];
    f.minimum = d[2];
    f.kind = (int)d[0];
    f.bits = (int)bits;
    f.off_full = (int)d[3];
    f.off_last = (int)d[4];
    f.len_full = (int)len_full;
    f.len_last = (int)len_last;
    at_full = d[3] + len_full;
    at_last = d[4] + len_last;
  }
  const int64_t words = ((a.packets - 1) * full_bytes + last_bytes) / 4;
  hipStream_t s = as_stream(stream);
  KTimer kt("e57_pack", s);
  hipLaunchKernelGGL(k_e57_pack, dim3(grid_for(words, kBlock, 16384)), dim3(kBlock), 0, s, a, words, (uint32_t*)out);
  O3DX_HIP(hipGetLastError());
  return 0;
}
