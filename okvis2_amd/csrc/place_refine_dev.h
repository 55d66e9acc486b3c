// place_refine_dev.h -- the solver of the refinement of Frontend::verifyRecognisedPlace's pose
// (okvis_frontend/src/Frontend.cpp:399-527) as ONE sequence of IEEE-754 operations that compiles for the host and for
// gfx950: tests/place_refine_ref.py transcribed line by line (quaternion_from_matrix, start_pose, normalized, product,
// plus, cholesky_solve and the body of refine's loop).  The stand-alone program tests/cpp/place_refine_step_main.cpp and
// the per-multiframe kernels of k_place_refine.hip are both this header; the tests hold them to the restatement byte
// for byte.  What is NOT here is the evaluation of the terms (place_term_dev.h, device only): the solver sees a point
// only through a PlaceRefineEval (0.5 sum rho, g, the upper triangle of A, the counts).
//
// The loop is a state machine over one PlaceRefineRecord per multiframe with two entry points:
//   refine_adopt_start(record, evaluation)   the evaluation at the start pose: the finite test (status 4), n_terms == 0
//                                            (status 3), S = 1 / (1 + sqrt(A_jj)), radius 1e4, nu 2
//   refine_advance(record, evaluation)       if a candidate is pending: the non-finite cost test, the quality against
//                                            1e-3 and the acceptance with its radius and function-tolerance updates, or
//                                            the rejection.  Then the loop: the four end tests in the restatement's
//                                            order, ++it, the scaled system, the Cholesky solve, the model change, the
//                                            parameter tolerance and plus, until a candidate needs an evaluation
//                                            (pending = 1) or the multiframe has ended (status >= 0).  An invalid step
//                                            uses up an iteration without an evaluation.
//
// Expression order: every operation is a separate IEEE operation in the restatement's order (the library is built with
// -ffp-contract=off: no FMA).  The order of okvfe_set_fp64_reduction (the template argument kTree) applies to the
// 3-term sum of plus and the 4-term sum of normalized only; every other sum runs left to right from its first term (the
// dot products from 0.0).  log, sin, cos and sinc are elementary_fixed.h.  Every array has a compile-time size and every
// loop a compile-time trip count, so that the device form keeps its state in registers.
// The two DEFINED DEVIATIONS from ceres and PARITY UNPINNED are those of the restatement (include/okvfe.h states them).
#pragma once
#include <stdint.h>

#include "elementary_fixed.h"

#if defined(__HIPCC__)
#define OKVFE_PR_HD __host__ __device__ inline __attribute__((always_inline))
#define OKVFE_PR_UNROLL _Pragma("unroll")
#else
#define OKVFE_PR_HD inline
#define OKVFE_PR_UNROLL
#endif

namespace okvfe {

constexpr int kRefineRunning = -1;  // PlaceRefineRecord::status while the loop goes on; 0..4 are the call's status values
constexpr int kRefineMaxIterations = 64;

struct PlaceRefineEval {  // what an evaluation at a pose hands to the solver (accumulate() of the restatement)
  double cost;            // 0.5 sum of rho0
  double g[6];
  double a[21];           // the upper triangle of A, row by row: (0,0) (0,1) .. (0,5) (1,1) ..
  int32_t n_terms, n_singular;
};
static_assert(sizeof(PlaceRefineEval) == 232, "28 doubles and two counts");

struct PlaceRefineRecord {
  double x[7], cost, cost0, g[6], a[21];
  double S[6], radius, nu;
  double xc[7], model_change;
  double start[7];
  int32_t function_tolerance, it, n_acc, status, pending, n_terms, bad_best, pad;
};
static_assert(sizeof(PlaceRefineRecord) == 59 * 8 + 8 * 4, "well under 1 KB per multiframe");

OKVFE_PR_HD bool refine_finite(double v) {
  unsigned long long bits;
  __builtin_memcpy(&bits, &v, 8);
  return (bits & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}
OKVFE_PR_HD double refine_abs(double v) { return v < 0.0 ? -v : (v == 0.0 ? 0.0 : v); }
OKVFE_PR_HD double refine_sqrt(double v) { return __builtin_sqrt(v); }
template <bool kTree>
OKVFE_PR_HD double refine_sum3(double a, double b, double c) {
  if constexpr (kTree) return a + (b + c);
  return (a + b) + c;
}
template <bool kTree>
OKVFE_PR_HD double refine_sum4(double a, double b, double c, double d) {
  if constexpr (kTree) return (a + b) + (c + d);
  return ((a + b) + c) + d;
}
// index of (i, j), i <= j, in the row-by-row upper triangle
OKVFE_PR_HD constexpr int refine_upper(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }

// Eigen's Quaterniond(Matrix3d) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<Other, 3, 3>) of the
// rotation of a row-major 3 x 4 hypothesis: (x, y, z, w), not normalised
OKVFE_PR_HD void quaternion_from_matrix(const double* Hm /* 3 x 4, row-major */, double q[4]) {
#define OKVFE_PR_C(i, j) Hm[4 * (i) + (j)]
  double t = (OKVFE_PR_C(0, 0) + OKVFE_PR_C(1, 1)) + OKVFE_PR_C(2, 2);
  q[0] = 0.0; q[1] = 0.0; q[2] = 0.0; q[3] = 0.0;
  if (t > 0.0) {
    t = refine_sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (OKVFE_PR_C(2, 1) - OKVFE_PR_C(1, 2)) * t;
    q[1] = (OKVFE_PR_C(0, 2) - OKVFE_PR_C(2, 0)) * t;
    q[2] = (OKVFE_PR_C(1, 0) - OKVFE_PR_C(0, 1)) * t;
  } else if (!(OKVFE_PR_C(1, 1) > OKVFE_PR_C(0, 0)) && !(OKVFE_PR_C(2, 2) > OKVFE_PR_C(0, 0))) {  // i = 0, j = 1, k = 2
    t = refine_sqrt(((OKVFE_PR_C(0, 0) - OKVFE_PR_C(1, 1)) - OKVFE_PR_C(2, 2)) + 1.0);
    q[0] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (OKVFE_PR_C(2, 1) - OKVFE_PR_C(1, 2)) * t;
    q[1] = (OKVFE_PR_C(1, 0) + OKVFE_PR_C(0, 1)) * t;
    q[2] = (OKVFE_PR_C(2, 0) + OKVFE_PR_C(0, 2)) * t;
  } else if (OKVFE_PR_C(1, 1) > OKVFE_PR_C(0, 0) && !(OKVFE_PR_C(2, 2) > OKVFE_PR_C(1, 1))) {     // i = 1, j = 2, k = 0
    t = refine_sqrt(((OKVFE_PR_C(1, 1) - OKVFE_PR_C(2, 2)) - OKVFE_PR_C(0, 0)) + 1.0);
    q[1] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (OKVFE_PR_C(0, 2) - OKVFE_PR_C(2, 0)) * t;
    q[2] = (OKVFE_PR_C(2, 1) + OKVFE_PR_C(1, 2)) * t;
    q[0] = (OKVFE_PR_C(0, 1) + OKVFE_PR_C(1, 0)) * t;
  } else {                                                                                          // i = 2, j = 0, k = 1
    t = refine_sqrt(((OKVFE_PR_C(2, 2) - OKVFE_PR_C(0, 0)) - OKVFE_PR_C(1, 1)) + 1.0);
    q[2] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (OKVFE_PR_C(1, 0) - OKVFE_PR_C(0, 1)) * t;
    q[0] = (OKVFE_PR_C(0, 2) + OKVFE_PR_C(2, 0)) * t;
    q[1] = (OKVFE_PR_C(1, 2) + OKVFE_PR_C(2, 1)) * t;
  }
#undef OKVFE_PR_C
}

// Transformation(Matrix4d) (okvis_kinematics implementation/Transformation.hpp:141-151) of a row-major 3 x 4 hypothesis:
// t its last column, q Eigen's conversion
OKVFE_PR_HD void start_pose(const double* Hm, double x[7]) {
  x[0] = Hm[3]; x[1] = Hm[7]; x[2] = Hm[11];
  quaternion_from_matrix(Hm, x + 3);
}

// Eigen's normalized(): divided by sqrt(squaredNorm()) iff that is > 0
template <bool kTree>
OKVFE_PR_HD void normalized(const double q[4], double o[4]) {
  const double n2 = refine_sum4<kTree>(q[0] * q[0], q[1] * q[1], q[2] * q[2], q[3] * q[3]);
  if (n2 > 0) {
    const double n = refine_sqrt(n2);
    o[0] = q[0] / n; o[1] = q[1] / n; o[2] = q[2] / n; o[3] = q[3] / n;
  } else {
    o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3];
  }
}

// Eigen's a * b of (x, y, z, w) quaternions, each sum left to right
OKVFE_PR_HD void product(const double a[4], const double b[4], double o[4]) {
  const double ax = a[0], ay = a[1], az = a[2], aw = a[3];
  const double bx = b[0], by = b[1], bz = b[2], bw = b[3];
  o[0] = ((aw * bx + ax * bw) + ay * bz) - az * by;
  o[1] = ((aw * by + ay * bw) + az * bx) - ax * bz;
  o[2] = ((aw * bz + az * bw) + ax * by) - ay * bx;
  o[3] = ((aw * bw - ax * bx) - ay * by) - az * bz;
}

// PoseManifold::plus (okvis_ceres/src/PoseLocalParameterization.cpp:49-70 with deltaQ and sinc, Transformation.hpp:50-71);
// false: a half-angle beyond pi / 4 (or a NaN) is an invalid step and o is not written
template <bool kTree>
OKVFE_PR_HD bool plus(const double x[7], const double d[6], double o[7]) {
  const double half = 0.5 * refine_sqrt(refine_sum3<kTree>(d[3] * d[3], d[4] * d[4], d[5] * d[5]));
  if (!(half <= 7.85398163397448278999e-01)) return false;
  const double f = sinc_fixed(half) * 0.5;
  const double dq[4] = {f * d[3], f * d[4], f * d[5], cos_fixed(half)};
  double qn[4], qp[4];
  normalized<kTree>(x + 3, qn);
  product(dq, qn, qp);
  normalized<kTree>(qp, o + 3);
  o[0] = x[0] + d[0]; o[1] = x[1] + d[1]; o[2] = x[2] + d[2];
  return true;
}

// M d = b by L L^T in one written-out order; M symmetric, given by its upper triangle (refine_upper).  false: a pivot
// that is not > 0, or a d that is not finite
OKVFE_PR_HD bool cholesky_solve(const double M[21], const double b[6], double d[6]) {
  double L[6][6], y[6];
OKVFE_PR_UNROLL
  for (int j = 0; j < 6; ++j) {
    double v = M[refine_upper(j, j)];
OKVFE_PR_UNROLL
    for (int k = 0; k < j; ++k) v = v - L[j][k] * L[j][k];
    if (!(v > 0.0)) return false;
    L[j][j] = refine_sqrt(v);
OKVFE_PR_UNROLL
    for (int i = j + 1; i < 6; ++i) {
      v = M[refine_upper(j, i)];
OKVFE_PR_UNROLL
      for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
      L[i][j] = v / L[j][j];
    }
  }
OKVFE_PR_UNROLL
  for (int i = 0; i < 6; ++i) {
    double v = b[i];
OKVFE_PR_UNROLL
    for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
    y[i] = v / L[i][i];
  }
  bool finite = true;
OKVFE_PR_UNROLL
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
OKVFE_PR_UNROLL
    for (int k = i + 1; k < 6; ++k) v = v - L[k][i] * d[k];
    d[i] = v / L[i][i];
    finite = finite && refine_finite(d[i]);
  }
  return finite;
}

OKVFE_PR_HD bool refine_eval_finite(const PlaceRefineEval& e) {
  bool ok = refine_finite(e.cost);
OKVFE_PR_UNROLL
  for (int j = 0; j < 6; ++j) ok = ok && refine_finite(e.g[j]);
OKVFE_PR_UNROLL
  for (int j = 0; j < 21; ++j) ok = ok && refine_finite(e.a[j]);
  return ok;
}

OKVFE_PR_HD void refine_take_point(PlaceRefineRecord& r, const PlaceRefineEval& e) {
  r.cost = e.cost;
OKVFE_PR_UNROLL
  for (int j = 0; j < 6; ++j) r.g[j] = e.g[j];
OKVFE_PR_UNROLL
  for (int j = 0; j < 21; ++j) r.a[j] = e.a[j];
}

// a fresh record at the start pose x (bad_best: the winner's index lies outside the hypothesis list and x is NaN)
OKVFE_PR_HD void refine_init(PlaceRefineRecord& r, const double x[7], bool bad_best) {
  const double nan = elementary_nan();
OKVFE_PR_UNROLL
  for (int j = 0; j < 7; ++j) {
    r.x[j] = x[j]; r.start[j] = x[j]; r.xc[j] = x[j];
  }
  r.cost = nan; r.cost0 = nan;
OKVFE_PR_UNROLL
  for (int j = 0; j < 6; ++j) { r.g[j] = nan; r.S[j] = nan; }
OKVFE_PR_UNROLL
  for (int j = 0; j < 21; ++j) r.a[j] = nan;
  r.radius = 1.0e4; r.nu = 2.0; r.model_change = nan;
  r.function_tolerance = 0; r.it = 0; r.n_acc = 0; r.status = kRefineRunning; r.pending = 0; r.n_terms = 0;
  r.bad_best = bad_best ? 1 : 0; r.pad = 0;
}

// the evaluation at the start pose
OKVFE_PR_HD void refine_adopt_start(PlaceRefineRecord& r, const PlaceRefineEval& e) {
  refine_take_point(r, e);
  r.cost0 = e.cost;
  r.n_terms = e.n_terms;
  r.it = 0; r.n_acc = 0; r.pending = 0;
  if (r.bad_best || !refine_eval_finite(e)) {
    r.status = 4;
  } else if (e.n_terms == 0) {
    r.status = 3;
  } else {
OKVFE_PR_UNROLL
    for (int j = 0; j < 6; ++j) r.S[j] = 1.0 / (1.0 + refine_sqrt(r.a[refine_upper(j, j)]));
  }
  r.radius = 1.0e4;
  r.nu = 2.0;
  r.function_tolerance = 0;
}

// e: the evaluation at r.xc where r.pending is set; not read otherwise
template <bool kTree>
OKVFE_PR_HD void refine_advance(PlaceRefineRecord& r, const PlaceRefineEval& e, int max_iterations) {
  if (r.status != kRefineRunning) return;
  if (r.pending) {
    r.pending = 0;
    const double cost_c = e.cost;
    bool accepted = false;
    double quality = 0.0;
    if (refine_finite(cost_c)) {
      quality = (r.cost - cost_c) / r.model_change;
      accepted = quality > 1.0e-3;
    }
    if (accepted) {
      r.n_acc = r.n_acc + 1;
      const double t = 2.0 * quality - 1.0;
      const double shrink = 1.0 - (t * t) * t;
      const double third = 1.0 / 3.0;
      const double grown = r.radius / (shrink > third ? shrink : third);
      r.radius = grown < 1.0e16 ? grown : 1.0e16;
      r.nu = 2.0;
      r.function_tolerance = refine_abs(r.cost - cost_c) <= 1.0e-6 * r.cost ? 1 : 0;
OKVFE_PR_UNROLL
      for (int j = 0; j < 7; ++j) r.x[j] = r.xc[j];
      refine_take_point(r, e);
      if (!refine_eval_finite(e)) r.status = 4;
    } else {
      r.radius = r.radius / r.nu;
      r.nu = 2.0 * r.nu;
    }
  }
  // (bounded: every pass either ends the multiframe, returns, or counts an iteration towards max_iterations)
  while (r.status == kRefineRunning) {
    double gmax = refine_abs(r.g[0]);
OKVFE_PR_UNROLL
    for (int j = 1; j < 6; ++j) {
      const double v = refine_abs(r.g[j]);
      gmax = v > gmax ? v : gmax;
    }
    if (gmax <= 1.0e-10) { r.status = 1; break; }
    if (r.function_tolerance) { r.status = 1; break; }
    if (r.radius < 1.0e-32) { r.status = 4; break; }
    if (r.it >= max_iterations) { r.status = 2; break; }
    r.it = r.it + 1;
    double As[21], M[21], gs[6], b[6], ds[6], d[6];
OKVFE_PR_UNROLL
    for (int i = 0; i < 6; ++i)
OKVFE_PR_UNROLL
      for (int j = i; j < 6; ++j) {
        As[refine_upper(i, j)] = (r.S[i] * r.a[refine_upper(i, j)]) * r.S[j];
        M[refine_upper(i, j)] = As[refine_upper(i, j)];
      }
OKVFE_PR_UNROLL
    for (int j = 0; j < 6; ++j) {
      gs[j] = r.S[j] * r.g[j];
      b[j] = -gs[j];
      const double ajj = As[refine_upper(j, j)];
      const double lo = 1.0e-6 > ajj ? 1.0e-6 : ajj;    // max(As_jj, 1e-6), As_jj first
      const double hi = 1.0e32 < lo ? 1.0e32 : lo;      // min(.., 1e32)
      M[refine_upper(j, j)] = ajj + hi / r.radius;
    }
    bool valid = cholesky_solve(M, b, ds);
    if (valid) {
OKVFE_PR_UNROLL
      for (int j = 0; j < 6; ++j) d[j] = r.S[j] * ds[j];
      double gd = 0.0, dAd = 0.0;
OKVFE_PR_UNROLL
      for (int j = 0; j < 6; ++j) gd = gd + gs[j] * ds[j];
      double Ad[6];
OKVFE_PR_UNROLL
      for (int i = 0; i < 6; ++i) {
        double v = 0.0;
OKVFE_PR_UNROLL
        for (int j = 0; j < 6; ++j) v = v + As[i <= j ? refine_upper(i, j) : refine_upper(j, i)] * ds[j];
        Ad[i] = v;
      }
OKVFE_PR_UNROLL
      for (int j = 0; j < 6; ++j) dAd = dAd + ds[j] * Ad[j];
      r.model_change = -(gd + 0.5 * dAd);
      if (!(r.model_change > 0.0)) valid = false;
    }
    if (valid) {
      double dd = 0.0, xx = 0.0;
OKVFE_PR_UNROLL
      for (int j = 0; j < 6; ++j) dd = dd + d[j] * d[j];
OKVFE_PR_UNROLL
      for (int j = 0; j < 7; ++j) xx = xx + r.x[j] * r.x[j];
      if (refine_sqrt(dd) <= 1.0e-8 * (refine_sqrt(xx) + 1.0e-8)) { r.status = 1; break; }
      double xc[7];
      valid = plus<kTree>(r.x, d, xc);
      if (valid) {
OKVFE_PR_UNROLL
        for (int j = 0; j < 7; ++j) r.xc[j] = xc[j];
        r.pending = 1;
        return;
      }
    }
    r.radius = r.radius / r.nu;
    r.nu = 2.0 * r.nu;
  }
}

}  // namespace okvfe
