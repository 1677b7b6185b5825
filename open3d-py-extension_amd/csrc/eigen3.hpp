// eigen3.hpp — the normals' per-query finish in float64: Open3D's raw-moment
// covariance (ComputeCovariance) and FastEigen3x3 (Eberly's robust symmetric
// 3x3 solver, smallest eigenvector), usable on host and device.
//
// Two formulations that give the same bits:
//   *_ref  Open3D's text restated: an arm per case, a division per quotient.
//          The yardstick; only the check entry (o3dx_normal_finish_check) and
//          the host test use it.
//   plain  the product path: one copy of each arm chosen by selects, and
//          quotients that share a divisor taken through one reciprocal
//          (ExactDiv).  Every lane performs the same IEEE operations on the
//          same operands in the same order as *_ref; what a lane discards may
//          be anything.
// Build with -ffp-contract=off: every fma here is written out.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define O3DX_HD __host__ __device__
#else
#define O3DX_HD
#endif

namespace o3dx {

O3DX_HD inline void dcross(const double u[3], const double v[3], double o[3]) {
  o[0] = u[1] * v[2] - u[2] * v[1];
  o[1] = u[2] * v[0] - u[0] * v[2];
  o[2] = u[0] * v[1] - u[1] * v[0];
}
O3DX_HD inline double ddot(const double u[3], const double v[3]) {
  return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2];
}

// ------------------------------------------------------------ *_ref (yardstick)
// Open3D ComputeEigenvector0
O3DX_HD inline void eigvec0_ref(const double A[3][3], double e, double out[3]) {
  double r0[3] = {A[0][0] - e, A[0][1], A[0][2]};
  double r1[3] = {A[0][1], A[1][1] - e, A[1][2]};
  double r2[3] = {A[0][2], A[1][2], A[2][2] - e};
  double a[3], b[3], c[3];
  dcross(r0, r1, a);
  dcross(r0, r2, b);
  dcross(r1, r2, c);
  double d0 = ddot(a, a), d1 = ddot(b, b), d2 = ddot(c, c);
  double dmax = d0;
  int imax = 0;
  if (d1 > dmax) {
    dmax = d1;
    imax = 1;
  }
  if (d2 > dmax) imax = 2;
  if (imax == 0) {
    double s = sqrt(d0);
    out[0] = a[0] / s; out[1] = a[1] / s; out[2] = a[2] / s;
  } else if (imax == 1) {
    double s = sqrt(d1);
    out[0] = b[0] / s; out[1] = b[1] / s; out[2] = b[2] / s;
  } else {
    double s = sqrt(d2);
    out[0] = c[0] / s; out[1] = c[1] / s; out[2] = c[2] / s;
  }
}

// Open3D ComputeEigenvector1
O3DX_HD inline void eigvec1_ref(const double A[3][3], const double e0[3], double e1v, double out[3]) {
  double U[3], V[3];
  if (fabs(e0[0]) > fabs(e0[1])) {
    double inv = 1.0 / sqrt(e0[0] * e0[0] + e0[2] * e0[2]);
    U[0] = -e0[2] * inv; U[1] = 0; U[2] = e0[0] * inv;
  } else {
    double inv = 1.0 / sqrt(e0[1] * e0[1] + e0[2] * e0[2]);
    U[0] = 0; U[1] = e0[2] * inv; U[2] = -e0[1] * inv;
  }
  dcross(e0, U, V);
  double AU[3] = {A[0][0] * U[0] + A[0][1] * U[1] + A[0][2] * U[2], A[0][1] * U[0] + A[1][1] * U[1] + A[1][2] * U[2],
                  A[0][2] * U[0] + A[1][2] * U[1] + A[2][2] * U[2]};
  double AV[3] = {A[0][0] * V[0] + A[0][1] * V[1] + A[0][2] * V[2], A[0][1] * V[0] + A[1][1] * V[1] + A[1][2] * V[2],
                  A[0][2] * V[0] + A[1][2] * V[1] + A[2][2] * V[2]};
  double m00 = U[0] * AU[0] + U[1] * AU[1] + U[2] * AU[2] - e1v;
  double m01 = U[0] * AV[0] + U[1] * AV[1] + U[2] * AV[2];
  double m11 = V[0] * AV[0] + V[1] * AV[1] + V[2] * AV[2] - e1v;
  double a00 = fabs(m00), a01 = fabs(m01), a11 = fabs(m11);
  if (a00 >= a11) {
    if (fmax(a00, a01) > 0) {
      if (a00 >= a01) {
        m01 /= m00; m00 = 1 / sqrt(1 + m01 * m01); m01 *= m00;
      } else {
        m00 /= m01; m01 = 1 / sqrt(1 + m00 * m00); m00 *= m01;
      }
      for (int i = 0; i < 3; ++i) out[i] = m01 * U[i] - m00 * V[i];
    } else {
      for (int i = 0; i < 3; ++i) out[i] = U[i];
    }
  } else {
    if (fmax(a11, a01) > 0) {
      if (a11 >= a01) {
        m01 /= m11; m11 = 1 / sqrt(1 + m01 * m01); m01 *= m11;
      } else {
        m11 /= m01; m01 = 1 / sqrt(1 + m11 * m11); m11 *= m01;
      }
      for (int i = 0; i < 3; ++i) out[i] = m11 * U[i] - m01 * V[i];
    } else {
      for (int i = 0; i < 3; ++i) out[i] = U[i];
    }
  }
}

// Open3D FastEigen3x3 (Eberly's robust symmetric 3x3 solver): smallest eigenvector.
// c = {xx, xy, xz, yy, yz, zz}
O3DX_HD inline void fast_eigen3x3_ref(const double c[6], double out[3]) {
  double A[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}};
  double max_coeff = A[0][0];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) max_coeff = fmax(max_coeff, A[i][j]);
  if (max_coeff == 0) {
    out[0] = out[1] = out[2] = 0;
    return;
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[i][j] /= max_coeff;
  double norm = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
  if (norm > 0) {
    double q = (A[0][0] + A[1][1] + A[2][2]) / 3;
    double b00 = A[0][0] - q, b11 = A[1][1] - q, b22 = A[2][2] - q;
    double p = sqrt((b00 * b00 + b11 * b11 + b22 * b22 + norm * 2) / 6);
    double c00 = b11 * b22 - A[1][2] * A[1][2];
    double c01 = A[0][1] * b22 - A[1][2] * A[0][2];
    double c02 = A[0][1] * A[1][2] - b11 * A[0][2];
    double det = (b00 * c00 - A[0][1] * c01 + A[0][2] * c02) / (p * p * p);
    double half_det = fmin(fmax(det * 0.5, -1.0), 1.0);
    double angle = acos(half_det) / (double)3;
    const double two_thirds_pi = 2.09439510239319549;
    double beta2 = cos(angle) * 2;
    double beta0 = cos(angle + two_thirds_pi) * 2;
    double beta1 = -(beta0 + beta2);
    double ev0 = q + p * beta0, ev1 = q + p * beta1, ev2 = q + p * beta2;
    double ea[3], eb[3];
    if (half_det >= 0) {
      eigvec0_ref(A, ev2, ea);
      if (ev2 < ev0 && ev2 < ev1) {
        out[0] = ea[0]; out[1] = ea[1]; out[2] = ea[2];
        return;
      }
      eigvec1_ref(A, ea, ev1, eb);
      if (ev1 < ev0 && ev1 < ev2) {
        out[0] = eb[0]; out[1] = eb[1]; out[2] = eb[2];
        return;
      }
      dcross(eb, ea, out);  // evec0 = evec1 x evec2
    } else {
      eigvec0_ref(A, ev0, ea);
      if (ev0 < ev1 && ev0 < ev2) {
        out[0] = ea[0]; out[1] = ea[1]; out[2] = ea[2];
        return;
      }
      eigvec1_ref(A, ea, ev1, eb);
      if (ev1 < ev0 && ev1 < ev2) {
        out[0] = eb[0]; out[1] = eb[1]; out[2] = eb[2];
        return;
      }
      dcross(ea, eb, out);  // evec2 = evec0 x evec1
    }
  } else {
    if (A[0][0] < A[1][1] && A[0][0] < A[2][2]) {
      out[0] = 1; out[1] = 0; out[2] = 0;
    } else if (A[1][1] < A[0][0] && A[1][1] < A[2][2]) {
      out[0] = 0; out[1] = 1; out[2] = 0;
    } else {
      out[0] = 0; out[1] = 0; out[2] = 1;
    }
  }
}

// Open3D ComputeCovariance's tail: nine raw moments {x, y, z, xx, xy, xz, yy,
// yz, zz} of k points -> c = {xx, xy, xz, yy, yz, zz}
O3DX_HD inline void moments_cov_ref(const double m[9], int k, double c[6]) {
  double u[9];
  for (int j = 0; j < 9; ++j) u[j] = m[j] / (double)k;
  c[0] = u[3] - u[0] * u[0];
  c[3] = u[6] - u[1] * u[1];
  c[5] = u[8] - u[2] * u[2];
  c[1] = u[4] - u[0] * u[1];
  c[2] = u[5] - u[0] * u[2];
  c[4] = u[7] - u[1] * u[2];
}

// ------------------------------------------------- exact shared-divisor division
// N quotients a[i] / b through one reciprocal.  With y = RN(1/b) (an ordinary
// division, correctly rounded by definition), q0 = RN(a y), r = a - q0 b
// (exact in one fma) and q = RN(q0 + r y), q is the correctly rounded a / b
// (Markstein's final-step theorem): the division's own bits, in three
// float64 instructions instead of the eleven or so of a division expansion.
//
// The identity needs finite, normal, non-zero operands and a quotient and a
// residual that neither overflow nor underflow; a zero numerator would also
// lose its sign (r = +0 turns a -0 quotient into +0).  The guard keeps both
// biased exponents within [kExpLo, kExpHi] = 2^-480 .. 2^481: then
// |a / b| lies in 2^+-962, y is normal, and the residual's last bit, at least
// 2^(ea - 106), is far above the subnormals.  Zeros, subnormals, infinities
// and NaNs have exponent field 0 or 2047 and fail it.  Lanes that fail take
// the ordinary divisions (rare: degenerate neighbourhoods).
constexpr int kExpLo = 1023 - 480, kExpHi = 1023 + 480;

O3DX_HD inline bool exp_in_range(double v) {
  uint64_t bits;
  __builtin_memcpy(&bits, &v, 8);
  const unsigned e = (unsigned)(bits >> 52) & 0x7ffu;
  return e - (unsigned)kExpLo <= (unsigned)(kExpHi - kExpLo);
}

template <int N>
O3DX_HD inline void div_shared(const double* a, double b, double* q) {  // a, q: N values, distinct arrays
  const double y = 1.0 / b;
  bool ok = exp_in_range(b);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < N; ++i) {
    const double q0 = a[i] * y;
    const double r = fma(-q0, b, a[i]);
    q[i] = fma(r, y, q0);
    ok = ok && exp_in_range(a[i]);
  }
  if (__builtin_expect(!ok, 0)) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < N; ++i) q[i] = a[i] / b;
  }
}

// ------------------------------------------------------------- the product path
O3DX_HD inline void moments_cov(const double m[9], int k, double c[6]) {
  const double a[9] = {m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8]};
  double u[9];
  div_shared<9>(a, (double)k, u);
  c[0] = u[3] - u[0] * u[0];
  c[3] = u[6] - u[1] * u[1];
  c[5] = u[8] - u[2] * u[2];
  c[1] = u[4] - u[0] * u[1];
  c[2] = u[5] - u[0] * u[2];
  c[4] = u[7] - u[1] * u[2];
}

// ComputeEigenvector0: the largest of the three row cross products, chosen
// by selects; one sqrt and one set of three quotients
O3DX_HD inline void eigvec0(const double A[3][3], double e, double out[3]) {
  double r0[3] = {A[0][0] - e, A[0][1], A[0][2]};
  double r1[3] = {A[0][1], A[1][1] - e, A[1][2]};
  double r2[3] = {A[0][2], A[1][2], A[2][2] - e};
  double a[3], b[3], c[3];
  dcross(r0, r1, a);
  dcross(r0, r2, b);
  dcross(r1, r2, c);
  const double d0 = ddot(a, a), d1 = ddot(b, b), d2 = ddot(c, c);
  const bool s1 = d1 > d0;
  const double dmax = s1 ? d1 : d0;
  const bool s2 = d2 > dmax;
  const double d = s2 ? d2 : dmax;
  double v[3];
  for (int i = 0; i < 3; ++i) v[i] = s2 ? c[i] : (s1 ? b[i] : a[i]);
  const double s = sqrt(d);
  div_shared<3>(v, s, out);
}

// ComputeEigenvector1: U's two forms and the four arms of the 2x2 kernel
// share one 1/sqrt, one division and one 1/sqrt
O3DX_HD inline void eigvec1(const double A[3][3], const double e0[3], double e1v, double out[3]) {
  double U[3], V[3];
  {
    const bool x = fabs(e0[0]) > fabs(e0[1]);
    const double h = x ? e0[0] : e0[1];
    const double inv = 1.0 / sqrt(h * h + e0[2] * e0[2]);
    const double t = (x ? -e0[2] : e0[2]) * inv;
    const double w = (x ? e0[0] : -e0[1]) * inv;
    U[0] = x ? t : 0.0;
    U[1] = x ? 0.0 : t;
    U[2] = w;
  }
  dcross(e0, U, V);
  double AU[3] = {A[0][0] * U[0] + A[0][1] * U[1] + A[0][2] * U[2], A[0][1] * U[0] + A[1][1] * U[1] + A[1][2] * U[2],
                  A[0][2] * U[0] + A[1][2] * U[1] + A[2][2] * U[2]};
  double AV[3] = {A[0][0] * V[0] + A[0][1] * V[1] + A[0][2] * V[2], A[0][1] * V[0] + A[1][1] * V[1] + A[1][2] * V[2],
                  A[0][2] * V[0] + A[1][2] * V[1] + A[2][2] * V[2]};
  const double m00 = U[0] * AU[0] + U[1] * AU[1] + U[2] * AU[2] - e1v;
  const double m01 = U[0] * AV[0] + U[1] * AV[1] + U[2] * AV[2];
  const double m11 = V[0] * AV[0] + V[1] * AV[1] + V[2] * AV[2] - e1v;
  const double a00 = fabs(m00), a01 = fabs(m01), a11 = fabs(m11);
  const bool first = a00 >= a11;         // the diagonal entry the arm works on: m00, else m11
  const double md = first ? m00 : m11, ad = first ? a00 : a11;
  const bool any = fmax(ad, a01) > 0;
  const bool dg = ad >= a01;             // divide by the diagonal entry, else by m01
  const double t = (dg ? m01 : md) / (dg ? md : m01);
  const double s = 1 / sqrt(1 + t * t);
  const double ts = t * s;
  const double nd = dg ? s : ts, n01 = dg ? ts : s;  // the new (diagonal, m01)
  const double cu = first ? n01 : nd, cv = first ? nd : n01;
  for (int i = 0; i < 3; ++i) {
    const double o = cu * U[i] - cv * V[i];
    out[i] = any ? o : U[i];
  }
}

O3DX_HD inline void fast_eigen3x3(const double c[6], double out[3]) {
  double max_coeff = c[0];
  for (int j = 1; j < 6; ++j) max_coeff = fmax(max_coeff, c[j]);  // max is order-free up to a zero's sign
  if (max_coeff == 0) {
    out[0] = out[1] = out[2] = 0;
    return;
  }
  double n[6];
  {
    const double a[6] = {c[0], c[1], c[2], c[3], c[4], c[5]};
    div_shared<6>(a, max_coeff, n);
  }
  const double A[3][3] = {{n[0], n[1], n[2]}, {n[1], n[3], n[4]}, {n[2], n[4], n[5]}};
  double norm = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
  if (norm > 0) {
    double q = (A[0][0] + A[1][1] + A[2][2]) / 3;
    double b00 = A[0][0] - q, b11 = A[1][1] - q, b22 = A[2][2] - q;
    double p = sqrt((b00 * b00 + b11 * b11 + b22 * b22 + norm * 2) / 6);
    double c00 = b11 * b22 - A[1][2] * A[1][2];
    double c01 = A[0][1] * b22 - A[1][2] * A[0][2];
    double c02 = A[0][1] * A[1][2] - b11 * A[0][2];
    double det = (b00 * c00 - A[0][1] * c01 + A[0][2] * c02) / (p * p * p);
    double half_det = fmin(fmax(det * 0.5, -1.0), 1.0);
    double angle = acos(half_det) / (double)3;
    const double two_thirds_pi = 2.09439510239319549;
    double beta2 = cos(angle) * 2;
    double beta0 = cos(angle + two_thirds_pi) * 2;
    double beta1 = -(beta0 + beta2);
    double ev0 = q + p * beta0, ev1 = q + p * beta1, ev2 = q + p * beta2;
    // half_det >= 0: start from the largest eigenvalue (ev2), else from the
    // smallest (ev0); eo is the other end
    const bool pos = half_det >= 0;
    const double es = pos ? ev2 : ev0, eo = pos ? ev0 : ev2;
    double ea[3], eb[3];
    eigvec0(A, es, ea);
    if (es < eo && es < ev1) {
      out[0] = ea[0]; out[1] = ea[1]; out[2] = ea[2];
      return;
    }
    eigvec1(A, ea, ev1, eb);
    double u[3], v[3];  // evec0 = evec1 x evec2, or evec2 = evec0 x evec1
    for (int i = 0; i < 3; ++i) {
      u[i] = pos ? eb[i] : ea[i];
      v[i] = pos ? ea[i] : eb[i];
    }
    double x[3];
    dcross(u, v, x);
    const bool mid = ev1 < ev0 && ev1 < ev2;
    for (int i = 0; i < 3; ++i) out[i] = mid ? eb[i] : x[i];
  } else {
    const bool d0 = A[0][0] < A[1][1] && A[0][0] < A[2][2];
    const bool d1 = A[1][1] < A[0][0] && A[1][1] < A[2][2];
    out[0] = d0 ? 1 : 0;
    out[1] = (!d0 && d1) ? 1 : 0;
    out[2] = (!d0 && !d1) ? 1 : 0;
  }
}

// ------------------------------------------------------------ all three eigenvalues
// Eberly's non-iterative solve as above, the three eigenvalues instead of the
// smallest eigenvector: ev[0] <= ev[1] <= ev[2] (beta0 <= beta1 <= beta2 by
// construction).  Scaled by the largest |entry|, so a matrix whose diagonal
// rounded below zero keeps its order.  Error: a few ulps of the largest
// |entry| on each value (the ISS saliency, keypoint.hip).
O3DX_HD inline void eigen3_values(const double c[6], double ev[3]) {
  double mc = fabs(c[0]);
  for (int j = 1; j < 6; ++j) mc = fmax(mc, fabs(c[j]));
  if (!(mc > 0)) {  // the zero matrix (or NaN entries)
    ev[0] = ev[1] = ev[2] = mc;
    return;
  }
  const double a00 = c[0] / mc, a01 = c[1] / mc, a02 = c[2] / mc, a11 = c[3] / mc, a12 = c[4] / mc, a22 = c[5] / mc;
  const double norm = a01 * a01 + a02 * a02 + a12 * a12;
  double e0, e1, e2;
  if (norm > 0) {
    const double q = (a00 + a11 + a22) / 3;
    const double b00 = a00 - q, b11 = a11 - q, b22 = a22 - q;
    const double p = sqrt((b00 * b00 + b11 * b11 + b22 * b22 + norm * 2) / 6);
    const double c00 = b11 * b22 - a12 * a12;
    const double c01 = a01 * b22 - a12 * a02;
    const double c02 = a01 * a12 - b11 * a02;
    const double det = (b00 * c00 - a01 * c01 + a02 * c02) / (p * p * p);
    const double half_det = fmin(fmax(det * 0.5, -1.0), 1.0);
    const double angle = acos(half_det) / (double)3;
    const double two_thirds_pi = 2.09439510239319549;
    const double beta2 = cos(angle) * 2;
    const double beta0 = cos(angle + two_thirds_pi) * 2;
    const double beta1 = -(beta0 + beta2);
    e0 = q + p * beta0;
    e1 = q + p * beta1;
    e2 = q + p * beta2;
  } else {  // diagonal: its entries, sorted
    e0 = fmin(a00, fmin(a11, a22));
    e1 = fmax(fmin(a00, a11), fmin(fmax(a00, a11), a22));
    e2 = fmax(a00, fmax(a11, a22));
  }
  ev[0] = e0 * mc;
  ev[1] = e1 * mc;
  ev[2] = e2 * mc;
}

}  // namespace o3dx
