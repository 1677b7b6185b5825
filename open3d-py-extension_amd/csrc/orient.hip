// orient.hip — Euclidean minimum spanning tree and consistent normal
// orientation on the device (Open3D OrientNormalsConsistentTangentPlane(k);
// reference open3dpypro/PointCloud.py:69-70, estimate_normals(method="poisson")).
//
// The rule (include/o3dx.h states it in full), made deterministic by one strict
// total order on undirected edges, (w, min(i,j), max(i,j)):
//   1. kNN arcs (i, knn[i][*]) from the caller's lists;
//   2. EMST: the minimum spanning tree of the complete graph under
//      w = d^2(i,j) in float64, ((dx dx) + dy dy) + dz dz (dist2_f64);
//   3. the Riemannian graph = the union of 1 and 2;
//   4. the MST of that graph under w = 1 - |dot(n_i, n_j)|, float64;
//   5. root = lowest index of maximal z, flipped iff its nz < 0; along the
//      tree a child is flipped iff dot(parent as oriented, child) < 0;
//   6. flipped normals have their three sign bits toggled.
//
// Both trees are Boruvka rounds.  Per round every component takes its smallest
// outgoing edge in two phases — a 64-bit atomicMin on the order-preserving bits
// of w (best_w), then an atomicMin on the packed (lo, hi) among the edges equal
// to that minimum (best_e) — and the winners are united.  Under a strict total
// order the chosen edges close no cycle except the pair that chose each other,
// which is recorded once.
//   EMST: a lane per cell-sorted point searches the grid.hpp grid shell by shell
//     for its nearest point of another component.  It stops once the shell's
//     lower bound strictly exceeds its best or the component's current best
//     (which only decreases during the launch); cells whose points all lie in
//     the searcher's component are skipped through a per-cell label.  A first
//     pass over shells 0..1 only posts bounds, so the full pass starts pruned.
//   normal MST: a lane per point over its k arcs, then a lane per EMST edge;
//     weights on the fly from the normals.  Duplicate arcs carry the same key.
//   signs: the union-find carries a parity in the top bit of the parent word
//     (flip[x] ^ flip[parent[x]]); a root is linked by one CAS with the parity
//     between the two roots.  After the last round parity(i -> root) is the
//     number of dot < 0 edges on the tree path, mod 2: the propagation is one
//     launch, whatever the tree's depth.
// Links go from the larger index to the smaller, so find strictly descends.
// Inside a launch the shared words (parent, best_w, best_e) are touched only by
// agent-scope atomics; no float atomics; no loop waits for another thread;
// every loop has a bound and raises *err past it.
#include <hipcub/hipcub.hpp>

#include "grid.hpp"

namespace o3dx {
namespace {

typedef unsigned long long u64;
constexpr u64 kNone = ~0ull;
constexpr int kOrMaxRounds = 40;    // ceil(log2 n) <= 31 rounds halve the components
constexpr double kOrOcc = 2.0;      // mean points per occupied cell of the EMST grid
constexpr int kOrCapMult = 4;

// order-preserving map of a float64 onto unsigned integers
__device__ __forceinline__ u64 key_of(double w) {
  const u64 b = (u64)__double_as_longlong(w);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ u64 pack_edge(int i, int j) {
  const int lo = min(i, j), hi = max(i, j);
  return ((u64)(uint32_t)lo << 32) | (u64)(uint32_t)hi;
}
__device__ __forceinline__ u64 ld64(const u64* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// atomicMin, skipped when the word is already no larger (it only decreases)
__device__ __forceinline__ void post_min(u64* p, u64 v) {
  if (v < ld64(p)) atomicMin(p, v);
}

// ------------------------------------------------ union-find with parity
// word = parent index | parity << 31; a root is (x, parity 0).  No path
// shortening: a path, once built, never changes, so the parity read along it
// stays valid whatever the other threads link meanwhile.
__device__ __forceinline__ int puf_find(const uint32_t* parent, int x, int64_t bound, int* err, uint32_t* par) {
  uint32_t acc = 0;
  for (int64_t it = 0; it <= bound; ++it) {
    const uint32_t w = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int p = (int)(w & 0x7fffffffu);
    if (p >= x) {  // a root (p == x); p > x cannot be: reported, not followed
      if (p > x) atomicOr(err, 1);
      *par = acc;
      return x;
    }
    acc ^= w >> 31;
    x = p;
  }
  atomicOr(err, 1);
  *par = acc;
  return x;
}

// Unites the components of a and b with flip[a] ^ flip[b] = bit.  A failed CAS
// means the root was linked by another thread: the retry starts from the two
// roots seen (bit then relates them), and the larger of them has a parent now.
__device__ __forceinline__ void puf_unite(uint32_t* parent, int a, int b, uint32_t bit, int64_t bound, int* err) {
  for (int64_t it = 0; it <= bound; ++it) {
    uint32_t pa, pb;
    int ra = puf_find(parent, a, bound, err, &pa);
    int rb = puf_find(parent, b, bound, err, &pb);
    if (ra == rb) return;
    bit ^= pa ^ pb;
    if (ra < rb) {
      const int t = ra;
      ra = rb;
      rb = t;
    }
    const uint32_t old = atomicCAS(parent + ra, (uint32_t)ra, (uint32_t)rb | (bit << 31));
    if (old == (uint32_t)ra) return;
    a = ra;
    b = rb;
  }
  atomicOr(err, 1);
}

struct Bor {
  int64_t n;
  uint32_t* parent;  // n
  int32_t* comp;     // n: the component (its root) of every point, final between launches
  uint8_t* par;      // n: parity of the point against its root
  u64* best_w;       // n, per root: key of the smallest outgoing weight
  u64* best_e;       // n, per root: the smallest (lo, hi) among the edges of that weight
  int32_t* ctr;      // {edges recorded, err}
};

__global__ void __launch_bounds__(kBlock) k_bor_init(Bor B) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < B.n) {
    B.parent[i] = (uint32_t)i;
    B.comp[i] = (int32_t)i;
    B.par[i] = 0;
    B.best_w[i] = kNone;
    B.best_e[i] = kNone;
  }
  if (i == 0) {
    B.ctr[0] = 0;
    B.ctr[1] = 0;
  }
}

__device__ __forceinline__ double normal_dot(const float* __restrict__ nrm, int i, int j) {
  const double ax = (double)nrm[3 * (int64_t)i], ay = (double)nrm[3 * (int64_t)i + 1], az = (double)nrm[3 * (int64_t)i + 2];
  const double bx = (double)nrm[3 * (int64_t)j], by = (double)nrm[3 * (int64_t)j + 1], bz = (double)nrm[3 * (int64_t)j + 2];
  double r = ax * bx;
  r = r + ay * by;
  r = r + az * bz;
  return r;
}

// A lane per point; the roots with an outgoing edge record it (the pair that
// chose the same edge: the smaller root does) and unite.  nrm != null: the
// link carries the edge's parity between the two roots.
__global__ void __launch_bounds__(kBlock) k_bor_unite(Bor B, const float* __restrict__ nrm, u64* __restrict__ edges) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= B.n) return;
  const int c = (int)t;
  if (B.comp[c] != c) return;
  const u64 e = B.best_e[c];  // final: written by the launch before
  if (e == kNone) return;
  const int lo = (int)(e >> 32), hi = (int)(e & 0xffffffffu);
  if (lo < 0 || hi < 0 || lo >= B.n || hi >= B.n) {
    atomicOr(B.ctr + 1, 1);
    return;
  }
  const int cl = B.comp[lo], ch = B.comp[hi];
  const int c2 = cl == c ? ch : cl;
  if (c2 == c || (cl != c && ch != c)) {
    atomicOr(B.ctr + 1, 1);
    return;
  }
  if (B.best_e[c2] != e || c < c2) {
    const int pos = atomicAdd(B.ctr, 1);
    if (pos < B.n - 1)
      edges[pos] = e;
    else
      atomicOr(B.ctr + 1, 1);
  }
  uint32_t bit = 0;
  if (nrm) bit = (normal_dot(nrm, lo, hi) < 0.0 ? 1u : 0u) ^ B.par[lo] ^ B.par[hi];
  puf_unite(B.parent, c, c2, bit, 2 * B.n + 2, B.ctr + 1);
}

// comp / par from the final parent[] (only read here), the bests reset
__global__ void __launch_bounds__(kBlock) k_bor_relabel(Bor B) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= B.n) return;
  uint32_t p;
  const int r = puf_find(B.parent, (int)i, B.n + 1, B.ctr + 1, &p);
  B.comp[i] = r;
  B.par[i] = (uint8_t)p;
  B.best_w[i] = kNone;
  B.best_e[i] = kNone;
}

// every path one link long again
__global__ void __launch_bounds__(kBlock) k_bor_flatten(Bor B) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= B.n) return;
  B.parent[i] = (uint32_t)B.comp[i] | ((uint32_t)B.par[i] << 31);
}

// ------------------------------------------------------------------ EMST
struct EmstArr {
  int32_t* comp_s;     // n: comp in cell-sorted order
  int32_t* cell_comp;  // per cell: the component all its points share, -1 when they differ
  u64* cand_w;         // n, by original index: this point's best outgoing edge
  u64* cand_e;
};

__global__ void __launch_bounds__(kBlock) k_emst_comp_sorted(GridView g, const int32_t* __restrict__ comp,
                                                             int32_t* __restrict__ comp_s) {
  const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (s >= g.n) return;
  comp_s[s] = comp[__float_as_int(g.pts[s].w)];
}

__global__ void __launch_bounds__(kBlock) k_emst_cell_comp(GridView g, int64_t ncells,
                                                           const int32_t* __restrict__ comp_s,
                                                           int32_t* __restrict__ cell_comp) {
  const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (c >= ncells) return;
  const int p0 = g.start[c], p1 = g.start[c + 1];
  int lab = -1;
  if (p0 < p1) {
    lab = comp_s[p0];
    for (int p = p0 + 1; p < p1; ++p)
      if (comp_s[p] != lab) {
        lab = -1;
        break;
      }
  }
  cell_comp[c] = lab;
}

// The nearest point of another component by (d^2, lo, hi).  For a fixed i the
// order of (min(i,j), max(i,j)) over j is the order of j.  rcap >= 0: shells
// 0..rcap only and nothing stored (any edge found bounds the component's
// best); rcap < 0: the full search, the candidate stored.
__global__ void __launch_bounds__(kBlock) k_emst_search(GridView g, Bor B, EmstArr E, int rcap) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= g.n) return;
  const int s = (int)t;
  const float4 qf = g.pts[s];
  const int oi = __float_as_int(qf.w);
  const int mc = E.comp_s[s];
  const double qx = (double)qf.x, qy = (double)qf.y, qz = (double)qf.z;
  int cx, cy, cz;
  grid_cell(g, qf.x, qf.y, qf.z, cx, cy, cz);
  int rmax = shell_rmax(g, cx, cy, cz);
  if (rcap >= 0) rmax = min(rmax, rcap);
  double bd = INFINITY;
  int bj = -1;
  for (int r = 0; r <= rmax; ++r) {
    for_shell(g, cx, cy, cz, r, [&](int c) {
      if (E.cell_comp[c] == mc) return;
      const int p1 = g.start[c + 1];
      for (int p = g.start[c]; p < p1; ++p) {
        if (E.comp_s[p] == mc) continue;
        const float4 v = g.pts[p];
        const double d = dist2_f64(qx, qy, qz, v);
        const int j = __float_as_int(v.w);
        if (bj < 0 || d < bd || (d == bd && j < bj)) {
          bd = d;
          bj = j;
        }
      }
    });
    const double R = cube_reach(g, qx, qy, qz, cx, cy, cz, r) - (double)g.slack;
    if (R > 0.0) {  // every point not seen yet has d^2 >= R^2
      const double R2 = R * R;
      if (bj >= 0 && bd < R2) break;
      if (key_of(R2) > ld64(B.best_w + mc)) break;  // kNone is above every key
    }
  }
  const u64 kw = bj >= 0 ? key_of(bd) : kNone;
  if (bj >= 0) post_min(B.best_w + mc, kw);
  if (rcap < 0) {
    E.cand_w[oi] = kw;
    E.cand_e[oi] = bj >= 0 ? pack_edge(oi, bj) : kNone;
  }
}

// phase 2: among the candidates equal to the component's minimum, the smallest (lo, hi)
__global__ void __launch_bounds__(kBlock) k_emst_pick(Bor B, EmstArr E) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= B.n) return;
  const u64 kw = E.cand_w[i];
  if (kw == kNone) return;
  const int c = B.comp[i];
  if (kw == B.best_w[c]) post_min(B.best_e + c, E.cand_e[i]);  // best_w: final, only read here
}

// ------------------------------------------------------------- normal MST
// Lanes [0, n): point i's arcs (i, knn[i][*]); lanes [n, 2n - 1): the EMST
// edges.  PHASE 1 posts the weights, PHASE 2 the (lo, hi) of the arcs equal
// to a component's minimum.  An arc is offered to both of its components.
template <int PHASE>
__device__ __forceinline__ void nmst_arc(const Bor& B, const float* __restrict__ nrm, int i, int j, int ci, u64& own_w,
                                         u64& own_e) {
  const int cj = B.comp[j];
  if (ci == cj) return;
  const double w = 1.0 - fabs(normal_dot(nrm, i, j));
  const u64 kw = key_of(w);
  if (PHASE == 1) {
    own_w = min(own_w, kw);
    post_min(B.best_w + cj, kw);
  } else {
    const u64 e = pack_edge(i, j);
    if (kw == B.best_w[ci]) own_e = min(own_e, e);
    if (kw == B.best_w[cj]) post_min(B.best_e + cj, e);
  }
}

template <int PHASE>
__global__ void __launch_bounds__(kBlock) k_nmst_scan(Bor B, const float* __restrict__ nrm,
                                                      const int32_t* __restrict__ knn, int k,
                                                      const u64* __restrict__ emst) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= 2 * B.n - 1) return;
  u64 own_w = kNone, own_e = kNone;
  int ci;
  if (t < B.n) {
    const int i = (int)t;
    ci = B.comp[i];
    for (int a = 0; a < k; ++a) {
      const int j = knn[t * k + a];
      if (j < 0 || j >= B.n || j == i) continue;
      nmst_arc<PHASE>(B, nrm, i, j, ci, own_w, own_e);
    }
  } else {
    const u64 e = emst[t - B.n];
    const int lo = (int)(e >> 32), hi = (int)(e & 0xffffffffu);
    if (lo < 0 || hi < 0 || lo >= B.n || hi >= B.n) return;
    ci = B.comp[lo];
    nmst_arc<PHASE>(B, nrm, lo, hi, ci, own_w, own_e);
  }
  if (PHASE == 1) {
    if (own_w != kNone) post_min(B.best_w + ci, own_w);
  } else {
    if (own_e != kNone) post_min(B.best_e + ci, own_e);
  }
}

// ------------------------------------------------------------------ signs
__device__ __forceinline__ uint32_t fkey32(float z) {
  const uint32_t b = (uint32_t)__float_as_int(z + 0.0f);  // -0 -> +0
  return (b >> 31) ? ~b : (b | 0x80000000u);
}

// the maximal z, lowest index: the maximum of (key(z), ~i)
__global__ void __launch_bounds__(kBlock) k_orient_zmax(const float* __restrict__ xyz, int64_t n, u64* zmax) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  u64 v = 0;
  if (i < n) v = ((u64)fkey32(xyz[3 * i + 2]) << 32) | (u64)(0xffffffffu - (uint32_t)i);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  if (lane_id() == 0 && v > ld64(zmax)) atomicMax(zmax, v);
}

__global__ void __launch_bounds__(kBlock) k_orient_flip(int64_t n, const uint8_t* __restrict__ par, const u64* zmax,
                                                        float* nrm, uint8_t* __restrict__ flipped) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t root = (int64_t)(0xffffffffu - (uint32_t)(*zmax & 0xffffffffu));
  if (root < 0 || root >= n) return;  // (n >= 1: never)
  const uint32_t f = (uint32_t)par[i] ^ (uint32_t)par[root] ^ (nrm[3 * root + 2] < 0.0f ? 1u : 0u);
  if (flipped) flipped[i] = (uint8_t)f;
  if (f && i != root) {
    uint32_t* w = reinterpret_cast<uint32_t*>(nrm + 3 * i);
    w[0] ^= 0x80000000u;
    w[1] ^= 0x80000000u;
    w[2] ^= 0x80000000u;
  }
}

// the root's own normal after every other lane has read its nz (a launch of its own)
__global__ void k_orient_flip_root(int64_t n, const u64* zmax, float* nrm) {
  const int64_t root = (int64_t)(0xffffffffu - (uint32_t)(*zmax & 0xffffffffu));
  if (root < 0 || root >= n) return;
  if (nrm[3 * root + 2] < 0.0f) {
    uint32_t* w = reinterpret_cast<uint32_t*>(nrm + 3 * root);
    w[0] ^= 0x80000000u;
    w[1] ^= 0x80000000u;
    w[2] ^= 0x80000000u;
  }
}

__global__ void __launch_bounds__(kBlock) k_edges_unpack(const u64* __restrict__ packed, int64_t m,
                                                         int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= m) return;
  const u64 e = packed[i];
  out[2 * i] = (int32_t)(e >> 32);
  out[2 * i + 1] = (int32_t)(e & 0xffffffffu);
}

// ------------------------------------------------------------------- host
static size_t or_sort_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceRadixSort::SortKeys(nullptr, b, (const u64*)nullptr, (u64*)nullptr, (int)std::max<int64_t>(n, 1));
  return b;
}

struct OrWs {
  Bor B;
  EmstArr E;
  u64 *emst, *tree, *sorted, *zmax;
  char* sort_tmp;
  size_t sort_bytes;
  char* grid;
  size_t grid_bytes;
};

static size_t or_carve(Arena& ar, int64_t n, bool orient, OrWs* w) {
  n = std::max<int64_t>(n, 1);
  w->B.n = n;
  w->B.parent = ar.take<uint32_t>(n);
  w->B.comp = ar.take<int32_t>(n);
  w->B.par = ar.take<uint8_t>(n);
  w->B.best_w = ar.take<u64>(n);
  w->B.best_e = ar.take<u64>(n);
  w->B.ctr = ar.take<int32_t>(4);
  w->zmax = ar.take<u64>(1);
  w->E.comp_s = ar.take<int32_t>(n);
  w->E.cell_comp = ar.take<int32_t>(std::max<int64_t>((int64_t)kOrCapMult * n, 4096) + 1);
  w->E.cand_w = ar.take<u64>(n);
  w->E.cand_e = ar.take<u64>(n);
  w->emst = ar.take<u64>(n);
  w->tree = orient ? ar.take<u64>(n) : nullptr;
  w->sorted = ar.take<u64>(n);
  w->sort_bytes = or_sort_bytes(n);
  w->sort_tmp = ar.take<char>(w->sort_bytes);
  w->grid_bytes = grid_ws_bytes(n, kOrCapMult);
  w->grid = ar.take<char>(w->grid_bytes);
  return ar.used;
}

static size_t or_ws_bytes(int64_t n, bool orient) {
  if (n <= 0 || n >= ((int64_t)1 << 31)) return 0;
  Arena ar(nullptr, 0);
  OrWs w;
  return or_carve(ar, n, orient, &w) + 1024;
}

// the round's tail: unite, relabel, flatten; then {edges so far, err}
static int bor_finish_round(const char* who, const Bor& B, const float* nrm, u64* edges, hipStream_t s, int32_t res[2]) {
  const dim3 gn((unsigned)((B.n + kBlock - 1) / kBlock)), bk(kBlock);
  hipLaunchKernelGGL(k_bor_unite, gn, bk, 0, s, B, nrm, edges);
  hipLaunchKernelGGL(k_bor_relabel, gn, bk, 0, s, B);
  hipLaunchKernelGGL(k_bor_flatten, gn, bk, 0, s, B);
  O3DX_HIP(hipGetLastError());
  O3DX_TRY(read_back(res, B.ctr, 2 * sizeof(int32_t), s));
  if (res[1] != 0) return fail(O3DX_EIO, "%s: the union-find exceeded its iteration bound or met a bad edge", who);
  return 0;
}

// sorted (lo, hi) rows of m packed edges
static int edges_out(const OrWs& w, const u64* packed, int64_t m, int32_t* out, hipStream_t s) {
  if (m <= 0 || !out) return 0;
  size_t sb = w.sort_bytes;
  O3DX_HIP(hipcub::DeviceRadixSort::SortKeys(w.sort_tmp, sb, packed, w.sorted, (int)m, 0, 64, s));
  hipLaunchKernelGGL(k_edges_unpack, dim3((unsigned)((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, w.sorted, m, out);
  O3DX_HIP(hipGetLastError());
  return 0;
}

// the EMST's n - 1 packed edges into w.emst (unordered)
static int emst_stage(const char* who, const float* xyz, int64_t n, OrWs& w, hipStream_t s) {
  const Bor& B = w.B;
  const dim3 gn((unsigned)((n + kBlock - 1) / kBlock)), bk(kBlock);
  hipLaunchKernelGGL(k_bor_init, gn, bk, 0, s, B);
  O3DX_HIP(hipGetLastError());
  if (n == 1) return 0;
  GridBuild G;
  {
    KTimer kt("emst_grid", s);
    O3DX_TRY(grid_build(xyz, n, kOrOcc, 0.0, w.grid, w.grid_bytes, s, &G, nullptr, nullptr, false, kOrCapMult, false));
  }
  const GridView g = G.view;
  const int64_t ncells = (int64_t)g.nx * g.ny * g.nz;
  if (ncells > std::max<int64_t>((int64_t)kOrCapMult * n, 4096))
    return fail(O3DX_EIO, "%s: the grid has more cells than its capacity", who);
  const dim3 gc((unsigned)((ncells + kBlock - 1) / kBlock));
  int32_t res[2] = {0, 0}, prev = 0;
  for (int round = 0; round < kOrMaxRounds; ++round) {
    KTimer kt("emst_round", s);
    hipLaunchKernelGGL(k_emst_comp_sorted, gn, bk, 0, s, g, B.comp, w.E.comp_s);
    hipLaunchKernelGGL(k_emst_cell_comp, gc, bk, 0, s, g, ncells, w.E.comp_s, w.E.cell_comp);
    if (round > 0) hipLaunchKernelGGL(k_emst_search, gn, bk, 0, s, g, B, w.E, 1);
    hipLaunchKernelGGL(k_emst_search, gn, bk, 0, s, g, B, w.E, -1);
    hipLaunchKernelGGL(k_emst_pick, gn, bk, 0, s, B, w.E);
    O3DX_TRY(bor_finish_round(who, B, nullptr, w.emst, s, res));
    if (res[0] == n - 1) return 0;
    if (res[0] <= prev || res[0] > n - 1) break;
    prev = res[0];
  }
  return fail(O3DX_EIO, "%s: the EMST has %d edges, expected %lld", who, res[0], (long long)(n - 1));
}

}  // namespace
}  // namespace o3dx

using namespace o3dx;

extern "C" size_t o3dx_emst_workspace_bytes(int64_t n) { return or_ws_bytes(n, false); }
extern "C" size_t o3dx_orient_normals_workspace_bytes(int64_t n, int k) {
  return k < 1 ? 0 : or_ws_bytes(n, true);
}

extern "C" int o3dx_emst(const float* xyz, int64_t n, const int32_t* knn_idx, int k, int32_t* edges_out_dev, void* ws,
                         size_t ws_bytes, void* stream) {
  const char* who = "o3dx_emst";
  (void)knn_idx;
  if (n <= 0 || n >= ((int64_t)1 << 31)) return fail(O3DX_EINVAL, "%s: n = %lld outside [1, 2^31)", who, (long long)n);
  if (k < 0) return fail(O3DX_EINVAL, "%s: k must be >= 0", who);
  if (!xyz || (n > 1 && !edges_out_dev)) return fail(O3DX_EINVAL, "%s: null points or edges", who);
  if (!ws || ws_bytes < or_ws_bytes(n, false)) return fail(O3DX_ENOMEM, "%s: workspace too small", who);
  hipStream_t s = as_stream(stream);
  Arena ar(ws, ws_bytes);
  OrWs w;
  or_carve(ar, n, false, &w);
  O3DX_ARENA_CHECK(ar);
  O3DX_TRY(emst_stage(who, xyz, n, w, s));
  {
    KTimer kt("emst_sort", s);
    O3DX_TRY(edges_out(w, w.emst, n - 1, edges_out_dev, s));
  }
  return host_wait(s);
}

extern "C" int o3dx_orient_normals_tangent_plane(const float* xyz, int64_t n, const int32_t* knn_idx, int k,
                                                 float* normals, int32_t* tree_out, uint8_t* flipped_out, void* ws,
                                                 size_t ws_bytes, void* stream) {
  const char* who = "o3dx_orient_normals_tangent_plane";
  if (n <= 0 || n >= ((int64_t)1 << 31)) return fail(O3DX_EINVAL, "%s: n = %lld outside [1, 2^31)", who, (long long)n);
  if (k < 1) return fail(O3DX_EINVAL, "%s: k must be >= 1", who);
  if (!xyz || !knn_idx || !normals) return fail(O3DX_EINVAL, "%s: null points, neighbour lists or normals", who);
  if (!ws || ws_bytes < or_ws_bytes(n, true)) return fail(O3DX_ENOMEM, "%s: workspace too small", who);
  hipStream_t s = as_stream(stream);
  Arena ar(ws, ws_bytes);
  OrWs w;
  or_carve(ar, n, true, &w);
  O3DX_ARENA_CHECK(ar);
  const Bor& B = w.B;
  const dim3 gn((unsigned)((n + kBlock - 1) / kBlock)), bk(kBlock);

  O3DX_TRY(emst_stage(who, xyz, n, w, s));

  // the MST of the kNN arcs + the EMST edges under 1 - |dot|
  hipLaunchKernelGGL(k_bor_init, gn, bk, 0, s, B);
  if (n > 1) {
    const dim3 ga((unsigned)((2 * n - 1 + kBlock - 1) / kBlock));
    int32_t res[2] = {0, 0}, prev = 0;
    bool done = false;
    for (int round = 0; round < kOrMaxRounds && !done; ++round) {
      KTimer kt("nmst_round", s);
      hipLaunchKernelGGL(k_nmst_scan<1>, ga, bk, 0, s, B, normals, knn_idx, k, w.emst);
      hipLaunchKernelGGL(k_nmst_scan<2>, ga, bk, 0, s, B, normals, knn_idx, k, w.emst);
      O3DX_TRY(bor_finish_round(who, B, normals, w.tree, s, res));
      done = res[0] == n - 1;
      if (!done && (res[0] <= prev || res[0] > n - 1)) break;
      prev = res[0];
    }
    if (!done)
      return fail(O3DX_EIO, "%s: the normal tree has %d edges, expected %lld (non-finite normals?)", who, res[0],
                  (long long)(n - 1));
  }
  {
    KTimer kt("orient_flip", s);
    O3DX_HIP(hipMemsetAsync(w.zmax, 0, sizeof(u64), s));
    hipLaunchKernelGGL(k_orient_zmax, gn, bk, 0, s, xyz, n, w.zmax);
    hipLaunchKernelGGL(k_orient_flip, gn, bk, 0, s, n, B.par, w.zmax, normals, flipped_out);
    hipLaunchKernelGGL(k_orient_flip_root, dim3(1), dim3(1), 0, s, n, w.zmax, normals);
    O3DX_HIP(hipGetLastError());
  }
  if (tree_out) {
    KTimer kt("orient_sort", s);
    O3DX_TRY(edges_out(w, w.tree, n - 1, tree_out, s));
  }
  return host_wait(s);
}
