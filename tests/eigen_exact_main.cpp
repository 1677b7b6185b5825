// Stand-alone host check of csrc/eigen3.hpp: the product formulation of the
// normals' finish (selects + shared-divisor exact division) against the *_ref
// text, bit for bit (memcmp: signed zeros and NaN payloads count).
// Built and run by tests/test_eigen_exact_host.py; prints one line per case
// family "<family> cases=<n> diff=<n>" and exits 1 when any case differs.
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "eigen3.hpp"

using namespace o3dx;

static uint64_t g_s = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (g_s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static double uni() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }  // [0, 1)
static double sym() { return 2.0 * uni() - 1.0; }
static double from_bits(uint64_t b) {
  double d;
  memcpy(&d, &b, 8);
  return d;
}
// a double with the given biased exponent and a mantissa of one of four
// kinds: random, all ones but a few low bits, all zeros but a few low bits, zero
static double shaped(unsigned bexp, int kind) {
  uint64_t man = rnd() & 0xfffffffffffffull;
  if (kind == 1) man |= 0xfffffffffffffull & ~(rnd() & 0xffull);
  if (kind == 2) man &= 0xffull;
  if (kind == 3) man = 0;
  return from_bits((rnd() & 0x8000000000000000ull) | ((uint64_t)(bexp & 0x7ff) << 52) | man);
}

static long g_total_cases = 0, g_total_diff = 0;
static void report(const char* family, long cases, long diff) {
  printf("%s cases=%ld diff=%ld\n", family, cases, diff);
  g_total_cases += cases;
  g_total_diff += diff;
}

// ------------------------------------------------------------------ quotients
static long g_fast = 0;  // quotients that took the three-instruction form
template <int N>
static long check_div(const double (&a)[N], double b) {
  double q[N], r[N];
  div_shared<N>(a, b, q);
  bool ok = exp_in_range(b);
  for (int i = 0; i < N; ++i) {
    volatile double ai = a[i], bi = b;  // the plain division, kept out of the optimiser's reach
    r[i] = ai / bi;
    ok = ok && exp_in_range(a[i]);
  }
  if (ok) g_fast += N;
  long d = 0;
  for (int i = 0; i < N; ++i) d += memcmp(&q[i], &r[i], 8) != 0;
  return d;
}

static void quotients() {
  long n = 0, d = 0;
  // moment sums over a small integer count
  for (int k = 3; k <= 200; ++k)
    for (int i = 0; i < 3000; ++i) {
      const double a[3] = {sym() * k, sym() * sym() * k, ldexp(sym(), (int)(rnd() % 40) - 20) * k};
      d += check_div<3>(a, (double)k);
      n += 3;
    }
  report("quot_small_int", n, d);
  // random pairs, a quarter with near-all-ones mantissas, exponents inside the guard
  n = d = 0;
  for (int i = 0; i < 1500000; ++i) {
    const int ka = (int)(rnd() & 3) == 0 ? 1 : (int)(rnd() % 3 == 0 ? 2 : 0);
    const int kb = (int)(rnd() & 3) == 0 ? 1 : (int)(rnd() % 5 == 0 ? 3 : 0);
    const double b = shaped(1023 - 60 + (unsigned)(rnd() % 121), kb);
    const double a[3] = {shaped(1023 - 60 + (unsigned)(rnd() % 121), ka), shaped(1023 - 60 + (unsigned)(rnd() % 121), ka),
                         shaped(1023 - 60 + (unsigned)(rnd() % 121), 0)};
    d += check_div<3>(a, b);
    n += 3;
  }
  report("quot_random", n, d);
  // the whole exponent range: |a / b| near both ends, subnormal and overflowing quotients and residuals
  n = d = 0;
  for (int i = 0; i < 1000000; ++i) {
    const double b = shaped((unsigned)(rnd() % 2048), (int)(rnd() & 3));
    const double a[1] = {shaped((unsigned)(rnd() % 2048), (int)(rnd() & 3))};
    d += check_div<1>(a, b);
    n += 1;
  }
  report("quot_full_range", n, d);
  // the guard's edges: exponents at and next to kExpLo / kExpHi
  n = d = 0;
  const int edge[8] = {kExpLo - 1, kExpLo, kExpLo + 1, kExpHi - 1, kExpHi, kExpHi + 1, 1, 2046};
  for (int i = 0; i < 200000; ++i) {
    const double b = shaped((unsigned)edge[rnd() % 8], (int)(rnd() & 3));
    const double a[3] = {shaped((unsigned)edge[rnd() % 8], (int)(rnd() & 3)), shaped((unsigned)edge[rnd() % 8], 1),
                         shaped(1023, 0)};
    d += check_div<3>(a, b);
    n += 3;
  }
  report("quot_guard_edges", n, d);
  // special values, every pair
  n = d = 0;
  std::vector<double> sp;
  const double mags[] = {0.0, from_bits(1), from_bits(0xfffffffffffffull), DBL_MIN, DBL_MAX, HUGE_VAL, 1.0, 3.0, 30.0,
                         from_bits(0x3fefffffffffffffull), from_bits(0x3ff0000000000001ull), ldexp(1.0, -480),
                         ldexp(1.0, 481), ldexp(1.0, -481), ldexp(1.0, 482), ldexp(1.0, -1000), ldexp(1.0, 1000)};
  for (double m : mags) {
    sp.push_back(m);
    sp.push_back(-m);
  }
  sp.push_back(from_bits(0x7ff8000000000000ull));
  sp.push_back(from_bits(0xfff8000000000001ull));
  sp.push_back(from_bits(0x7ff800000000beefull));
  for (double b : sp)
    for (double a0 : sp)
      for (double a1 : sp) {
        const double a[3] = {a0, a1, 7.0};
        d += check_div<3>(a, b);
        const double s[1] = {a0};
        d += check_div<1>(s, b);
        n += 4;
      }
  report("quot_special", n, d);
}

// --------------------------------------------------------------------- solver
static long cmp_solver(const double c[6]) {
  double o[3], r[3];
  fast_eigen3x3(c, o);
  fast_eigen3x3_ref(c, r);
  return memcmp(o, r, sizeof o) != 0;
}
static long cmp_moments(const double m[9], int k) {
  double c[6], cr[6], o[3], r[3];
  moments_cov(m, k, c);
  moments_cov_ref(m, k, cr);
  fast_eigen3x3(c, o);
  fast_eigen3x3_ref(cr, r);
  return (memcmp(c, cr, sizeof c) != 0) || (memcmp(o, r, sizeof o) != 0);
}
static double pick_scale() {
  switch (rnd() % 8) {
    case 0: return ldexp(1.0, 40);
    case 1: return ldexp(1.0, -40);
    case 2: return ldexp(1.0, (int)(rnd() % 1400) - 700);  // through the guard's edges and beyond
    default: return 1.0;
  }
}
static void outer_add(double c[6], const double v[3], double w) {
  c[0] += w * v[0] * v[0]; c[1] += w * v[0] * v[1]; c[2] += w * v[0] * v[2];
  c[3] += w * v[1] * v[1]; c[4] += w * v[1] * v[2]; c[5] += w * v[2] * v[2];
}
static void small_ints(double v[3]) {
  for (int i = 0; i < 3; ++i) v[i] = (double)((int)(rnd() % 7) - 3);
}
// a few non-zero entries moved by an ulp or two.  (A zero stays: next to it
// lie the subnormals, and a matrix whose largest entry is one overflows in the
// normalisation to NaNs of both signs.)
static void nudge(double c[6]) {
  for (int j = 0; j < 6; ++j)
    if ((rnd() & 3) == 0 && c[j] != 0) {
      int steps = (int)(rnd() % 5) - 2;
      for (; steps > 0; --steps) c[j] = nextafter(c[j], HUGE_VAL);
      for (; steps < 0; ++steps) c[j] = nextafter(c[j], -HUGE_VAL);
    }
}

static void solver() {
  const int kPer = 200000;
  long d;
  // random SPD
  d = 0;
  for (int i = 0; i < 2 * kPer; ++i) {
    double c[6] = {0, 0, 0, 0, 0, 0};
    for (int t = 0; t < 3; ++t) {
      const double v[3] = {sym(), sym(), sym()};
      outer_add(c, v, t == 2 ? ldexp(1.0, -(int)(rnd() % 30)) : 1.0);  // thin slabs too
    }
    const double s = pick_scale();
    for (double& x : c) x *= s;
    d += cmp_solver(c);
  }
  report("solver_spd", 2 * kPer, d);
  // rank 1 and rank 2, random and small-integer directions
  d = 0;
  for (int i = 0; i < 2 * kPer; ++i) {
    double c[6] = {0, 0, 0, 0, 0, 0};
    const int rank = 1 + (int)(rnd() & 1);
    for (int t = 0; t < rank; ++t) {
      double v[3] = {sym(), sym(), sym()};
      if (rnd() & 1) small_ints(v);
      outer_add(c, v, 1.0);
    }
    const double s = pick_scale();
    for (double& x : c) x *= s;
    d += cmp_solver(c);
  }
  report("solver_rank12", 2 * kPer, d);
  // all zero (both signs) and diagonal (norm == 0), equal entries included
  d = 0;
  for (int i = 0; i < kPer; ++i) {
    double c[6] = {0, 0, 0, 0, 0, 0};
    if (i >= 64) {
      const double a = uni(), b = uni(), s = pick_scale();
      const double e[3] = {a, (rnd() & 1) ? a : b, (rnd() & 3) == 0 ? a : uni()};
      c[0] = e[rnd() % 3] * s; c[3] = e[rnd() % 3] * s; c[5] = e[rnd() % 3] * s;
      if ((rnd() & 7) == 0) c[rnd() % 6] = 0.0;
      if ((rnd() & 15) == 0) c[0] = -c[0];
    } else {
      for (int j = 0; j < 6; ++j) c[j] = ((i >> j) & 1) ? -0.0 : 0.0;
    }
    d += cmp_solver(c);
  }
  report("solver_zero_diag", kPer, d);
  // two and three equal eigenvalues (half_det = +-1): a I + b v v^T with exact
  // small-integer v, and the same nudged by an ulp or two
  d = 0;
  for (int i = 0; i < 2 * kPer; ++i) {
    const double a = (rnd() & 7) == 0 ? 0.0 : (double)(rnd() % 16) * 0.25;
    double v[3];
    small_ints(v);
    double c[6] = {a, 0, 0, a, 0, a};
    const int kind = (int)(rnd() % 4);
    outer_add(c, v, kind == 0 ? 0.0 : kind == 1 ? -0.125 : (double)(1 + rnd() % 4) * 0.5);
    if (rnd() & 1) nudge(c);
    const double s = pick_scale();
    for (double& x : c) x *= s;
    d += cmp_solver(c);
  }
  report("solver_equal_eigs", 2 * kPer, d);
  // half_det = 0: eigenvalues q - t, q, q + t (q I + t (u u^T - w w^T) for
  // orthogonal integer u, w of equal length), exact and nudged
  d = 0;
  for (int i = 0; i < kPer; ++i) {
    const double q = (double)(rnd() % 9) * 0.5, t = (double)(1 + rnd() % 8) * 0.25;
    static const double uw[4][2][3] = {{{1, 1, 0}, {1, -1, 0}}, {{1, 0, 1}, {1, 0, -1}}, {{0, 1, 1}, {0, 1, -1}},
                                       {{1, 1, 1}, {1, -1, 0}}};
    const int p = (int)(rnd() % 4);
    double c[6] = {q, 0, 0, q, 0, q};
    outer_add(c, uw[p][0], t / ddot(uw[p][0], uw[p][0]));
    outer_add(c, uw[p][1], -t / ddot(uw[p][1], uw[p][1]));
    if (rnd() & 1) nudge(c);
    const double s = pick_scale();
    for (double& x : c) x *= s;
    d += cmp_solver(c);
  }
  report("solver_half_det_zero", kPer, d);
  // imax ties and |e0[0]| == |e0[1]|: matrices symmetric under a permutation
  // of the axes, [[a,b,c],[b,a,c],[c,c,e]] and its relabellings, a I + b 1 1^T
  d = 0;
  for (int i = 0; i < 2 * kPer; ++i) {
    const bool ints = rnd() & 1;
    const double a = ints ? (double)(rnd() % 9) : uni() + 1.0, b = ints ? (double)((int)(rnd() % 7) - 3) : sym();
    const double cc = (rnd() & 3) == 0 ? b : (ints ? (double)((int)(rnd() % 7) - 3) : sym());
    const double e = (rnd() & 3) == 0 ? a : (ints ? (double)(rnd() % 9) : uni() + 1.0);
    double c[6];
    switch (rnd() % 3) {
      case 0: c[0] = a; c[1] = b; c[2] = cc; c[3] = a; c[4] = cc; c[5] = e; break;   // x <-> y
      case 1: c[0] = a; c[1] = cc; c[2] = b; c[3] = e; c[4] = cc; c[5] = a; break;   // x <-> z
      default: c[0] = e; c[1] = cc; c[2] = cc; c[3] = a; c[4] = b; c[5] = a; break;  // y <-> z
    }
    if ((rnd() & 7) == 0) nudge(c);
    const double s = pick_scale();
    for (double& x : c) x *= s;
    d += cmp_solver(c);
  }
  report("solver_ties", 2 * kPer, d);
  // indefinite matrices of any sign with zeros of either sign among the
  // entries.  (The exponents stay where no product of three entries
  // overflows: once two NaNs of different sign meet in one operation, which
  // of them comes out is the operand order the compiler chose, not the
  // formulation's.)
  d = 0;
  for (int i = 0; i < kPer; ++i) {
    double c[6];
    for (double& x : c) {
      const unsigned r = (unsigned)(rnd() % 16);
      x = r == 0 ? 0.0 : r == 1 ? -0.0 : shaped(1023 - 80 + (unsigned)(rnd() % 161), (int)(rnd() & 3));
    }
    d += cmp_solver(c);
  }
  report("solver_indefinite", kPer, d);
}

// ---------------------------------------------------------------- moment sets
static void moments() {
  const int ks[5] = {3, 4, 30, 31, 64};
  const char* names[5] = {"mom_unit_cube", "mom_offset_5e5", "mom_identical", "mom_collinear", "mom_axis_plane"};
  for (int fam = 0; fam < 5; ++fam) {
    long n = 0, d = 0;
    for (int i = 0; i < 100000; ++i) {
      const int k = ks[rnd() % 5];
      const float o[3] = {(float)uni(), (float)uni(), (float)uni()};
      const float dir[3] = {(float)sym(), (float)sym(), (float)sym()};
      const int axis = (int)(rnd() % 3);
      const float level = (rnd() & 1) ? 0.0f : (float)sym();
      double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      for (int j = 0; j < k; ++j) {
        float p[3] = {(float)uni(), (float)uni(), (float)uni()};
        if (fam == 1)
          for (float& x : p) x = 5e5f + x;
        if (fam == 2)
          for (int a = 0; a < 3; ++a) p[a] = o[a];
        if (fam == 3) {
          const float t = (float)sym();
          for (int a = 0; a < 3; ++a) p[a] = o[a] + t * dir[a];
        }
        if (fam == 4) p[axis] = level;
        const double x = p[0], y = p[1], z = p[2];
        m[0] += x; m[1] += y; m[2] += z;
        m[3] = fma(x, x, m[3]); m[4] = fma(x, y, m[4]); m[5] = fma(x, z, m[5]);
        m[6] = fma(y, y, m[6]); m[7] = fma(y, z, m[7]); m[8] = fma(z, z, m[8]);
      }
      d += cmp_moments(m, k);
      ++n;
    }
    report(names[fam], n, d);
  }
}

int main() {
  quotients();
  printf("quot_fast_path=%ld\n", g_fast);
  const long nq = g_total_cases;
  solver();
  moments();
  printf("total quotients=%ld solver_and_moment_cases=%ld diff=%ld\n", nq, g_total_cases - nq, g_total_diff);
  return g_total_diff ? 1 : 0;
}
