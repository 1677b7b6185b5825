// unionfind.hpp — the lock-free union-find over a global int32 parent[] array
// shared by DBSCAN (cluster.hip) and the image labelling (raster.hip).
#pragma once

#include <type_traits>

#include "common.hpp"

namespace o3dx {

// ------------------------------------------------------------- union-find
// parent[x] <= x always (links go from the larger index to the smaller), so
// find strictly descends and ends at a root; within the union launch every
// access to parent[] is an agent-scope atomic (the XCDs' L2s are private: a
// plain load could be served stale).  No loop waits for another thread: each
// has an iteration bound from n and raises *err past it.
__device__ __forceinline__ int uf_load(const int32_t* parent, int x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// HALVE (the union launch): a visited non-root is pointed at its grandparent
// with an atomic min — parent[x] only ever decreases to another member of x's
// tree, a root (parent[r] == r) is never touched, so the links' CAS on roots
// and the descent are unaffected; it keeps the trees shallow (measured:
// profiles/dbscan_time.txt).
template <bool HALVE = false>
__device__ __forceinline__ int uf_find(typename std::conditional<HALVE, int32_t, const int32_t>::type* parent, int x,
                                       int64_t bound, int* err) {
  for (int64_t it = 0; it <= bound; ++it) {
    const int p = uf_load(parent, x);
    if (p >= x) {  // a root (p == x); p > x cannot be: reported, not followed
      if (p > x) atomicOr(err, 1);
      return x;
    }
    if constexpr (HALVE) {
      const int gp = uf_load(parent, p);
      if (gp < p) atomicMin(parent + x, gp);
    }
    x = p;
  }
  atomicOr(err, 1);
  return x;
}

// Unites the components of a and b; returns the smaller end of the last step
// (a member of the united component, its root unless another thread linked it
// since).  A failed CAS continues from the value it returned (< the index it
// tried), so a + b strictly decreases on every retry.
__device__ __forceinline__ int uf_unite(int32_t* parent, int a, int b, int64_t bound, int* err) {
  for (int64_t it = 0; it <= bound; ++it) {
    if (a == b) return a;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicCAS(parent + a, a, b);
    if (old == a) return b;
    if (old > a) {
      atomicOr(err, 1);
      return b;
    }
    a = old;
  }
  atomicOr(err, 1);
  return b;
}

}  // namespace o3dx
