// place_refine_dev.h -- the solver of the refinement of Frontend::verifyRecognisedPlace's pose
// (okvis_frontend/src/Frontend.cpp:399-527) as ONE sequence of IEEE-754 operations that compiles for the host and for
// gfx950: tests/place_refine_ref.py transcribed line by line (quaternion_from_matrix, start_pose, plus, cholesky_solve
// and the body of refine's loop; its normalized and product are fp64_ops.h's quat_normalized and quat_product).  The stand-alone program tests/cpp/place_refine_step_main.cpp and
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
#include "fp64_ops.h"

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

OKVFE_FP64_HD double refine_abs(double v) { return v < 0.0 ? -v : (v == 0.0 ? 0.0 : v); }
// index of (i, j), i <= j, in the row-by-row upper triangle
OKVFE_FP64_HD constexpr int refine_upper(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }

// Eigen's Quaterniond(Matrix3d) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<Other, 3, 3>) of the
// rotation of a row-major 3 x 4 hypothesis: (x, y, z, w), not normalised
OKVFE_FP64_HD void quaternion_from_matrix(const double* Hm /* 3 x 4, row-major */, double q[4]) {
#define OKVFE_PR_C(i, j) Hm[4 * (i) + (j)]
  double t = (OKVFE_PR_C(0, 0) + OKVFE_PR_C(1, 1)) + OKVFE_PR_C(2, 2);
  q[0] = 0.0; q[1] = 0.0; q[2] = 0.0; q[3] = 0.0;
  if (t > 0.0) {
    t = fp64::sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (OKVFE_PR_C(2, 1) - OKVFE_PR_C(1, 2)) * t;
    q[1] = (OKVFE_PR_C(0, 2) - OKVFE_PR_C(2, 0)) * t;
    q[2] = (OKVFE_PR_C(1, 0) - OKVFE_PR_C(0, 1)) * t;
  } else if (!(OKVFE_PR_C(1, 1) > OKVFE_PR_C(0, 0)) && !(OKVFE_PR_C(2, 2) > OKVFE_PR_C(0, 0))) {  // i = 0, j = 1, k = 2
    t = fp64::sqrt(((OKVFE_PR_C(0, 0) - OKVFE_PR_C(1, 1)) - OKVFE_PR_C(2, 2)) + 1.0);
    q[0] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (OKVFE_PR_C(2, 1) - OKVFE_PR_C(1, 2)) * t;
    q[1] = (OKVFE_PR_C(1, 0) + OKVFE_PR_C(0, 1)) * t;
    q[2] = (OKVFE_PR_C(2, 0) + OKVFE_PR_C(0, 2)) * t;
  } else if (OKVFE_PR_C(1, 1) > OKVFE_PR_C(0, 0) && !(OKVFE_PR_C(2, 2) > OKVFE_PR_C(1, 1))) {     // i = 1, j = 2, k = 0
    t = fp64::sqrt(((OKVFE_PR_C(1, 1) - OKVFE_PR_C(2, 2)) - OKVFE_PR_C(0, 0)) + 1.0);
    q[1] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (OKVFE_PR_C(0, 2) - OKVFE_PR_C(2, 0)) * t;
    q[2] = (OKVFE_PR_C(2, 1) + OKVFE_PR_C(1, 2)) * t;
    q[0] = (OKVFE_PR_C(0, 1) + OKVFE_PR_C(1, 0)) * t;
  } else {                                                                                          // i = 2, j = 0, k = 1
    t = fp64::sqrt(((OKVFE_PR_C(2, 2) - OKVFE_PR_C(0, 0)) - OKVFE_PR_C(1, 1)) + 1.0);
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
OKVFE_FP64_HD void start_pose(const double* Hm, double x[7]) {
  x[0] = Hm[3]; x[1] = Hm[7]; x[2] = Hm[11];
  quaternion_from_matrix(Hm, x + 3);
}

// PoseManifold::plus (okvis_ceres/src/PoseLocalParameterization.cpp:49-70 with deltaQ and sinc, Transformation.hpp:50-71);
// false: a half-angle beyond pi / 4 (or a NaN) is an invalid step and o is not written
template <bool kTree>
OKVFE_FP64_HD bool plus(const double x[7], const double d[6], double o[7]) {
  const double half = 0.5 * fp64::sqrt(fp64::sum3<kTree>(d[3] * d[3], d[4] * d[4], d[5] * d[5]));
  if (!(half <= 7.85398163397448278999e-01)) return false;
  const double f = sinc_fixed(half) * 0.5;
  const double dq[4] = {f * d[3], f * d[4], f * d[5], cos_fixed(half)};
  double qn[4], qp[4];
  fp64::quat_normalized<kTree>(x + 3, qn);
  fp64::quat_product(dq, qn, qp);
  fp64::quat_normalized<kTree>(qp, o + 3);
  o[0] = x[0] + d[0]; o[1] = x[1] + d[1]; o[2] = x[2] + d[2];
  return true;
}

// M d = b by L L^T in one written-out order; M symmetric, given by its upper triangle (refine_upper).  false: a pivot
// that is not > 0, or a d that is not finite
OKVFE_FP64_HD bool cholesky_solve(const double M[21], const double b[6], double d[6]) {
  double L[6][6], y[6];
OKVFE_FP64_UNROLL
  for (int j = 0; j < 6; ++j) {
    double v = M[refine_upper(j, j)];
OKVFE_FP64_UNROLL
    for (int k = 0; k < j; ++k) v = v - L[j][k] * L[j][k];
    if (!(v > 0.0)) return false;
    L[j][j] = fp64::sqrt(v);
OKVFE_FP64_UNROLL
    for (int i = j + 1; i < 6; ++i) {
      v = M[refine_upper(j, i)];
OKVFE_FP64_UNROLL
      for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
      L[i][j] = v / L[j][j];
    }
  }
OKVFE_FP64_UNROLL
  for (int i = 0; i < 6; ++i) {
    double v = b[i];
OKVFE_FP64_UNROLL
    for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
    y[i] = v / L[i][i];
  }
  bool finite = true;
OKVFE_FP64_UNROLL
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
OKVFE_FP64_UNROLL
    for (int k = i + 1; k < 6; ++k) v = v - L[k][i] * d[k];
    d[i] = v / L[i][i];
    finite = finite && fp64::finite(d[i]);
  }
  return finite;
}

OKVFE_FP64_HD bool refine_eval_finite(const PlaceRefineEval& e) {
  bool ok = fp64::finite(e.cost);
OKVFE_FP64_UNROLL
  for (int j = 0; j < 6; ++j) ok = ok && fp64::finite(e.g[j]);
OKVFE_FP64_UNROLL
  for (int j = 0; j < 21; ++j) ok = ok && fp64::finite(e.a[j]);
  return ok;
}

OKVFE_FP64_HD void refine_take_point(PlaceRefineRecord& r, const PlaceRefineEval& e) {
  r.cost = e.cost;
OKVFE_FP64_UNROLL
  for (int j = 0; j < 6; ++j) r.g[j] = e.g[j];
OKVFE_FP64_UNROLL
  for (int j = 0; j < 21; ++j) r.a[j] = e.a[j];
}

// a fresh record at the start pose x (bad_best: the winner's index lies outside the hypothesis list and x is NaN)
OKVFE_FP64_HD void refine_init(PlaceRefineRecord& r, const double x[7], bool bad_best) {
  const double nan = elementary_nan();
OKVFE_FP64_UNROLL
  for (int j = 0; j < 7; ++j) {
    r.x[j] = x[j]; r.start[j] = x[j]; r.xc[j] = x[j];
  }
  r.cost = nan; r.cost0 = nan;
OKVFE_FP64_UNROLL
  for (int j = 0; j < 6; ++j) { r.g[j] = nan; r.S[j] = nan; }
OKVFE_FP64_UNROLL
  for (int j = 0; j < 21; ++j) r.a[j] = nan;
  r.radius = 1.0e4; r.nu = 2.0; r.model_change = nan;
  r.function_tolerance = 0; r.it = 0; r.n_acc = 0; r.status = kRefineRunning; r.pending = 0; r.n_terms = 0;
  r.bad_best = bad_best ? 1 : 0; r.pad = 0;
}

// the evaluation at the start pose
OKVFE_FP64_HD void refine_adopt_start(PlaceRefineRecord& r, const PlaceRefineEval& e) {
  refine_take_point(r, e);
  r.cost0 = e.cost;
  r.n_terms = e.n_terms;
  r.it = 0; r.n_acc = 0; r.pending = 0;
  if (r.bad_best || !refine_eval_finite(e)) {
    r.status = 4;
  } else if (e.n_terms == 0) {
    r.status = 3;
  } else {
OKVFE_FP64_UNROLL
    for (int j = 0; j < 6; ++j) r.S[j] = 1.0 / (1.0 + fp64::sqrt(r.a[refine_upper(j, j)]));
  }
  r.radius = 1.0e4;
  r.nu = 2.0;
  r.function_tolerance = 0;
}

// e: the evaluation at r.xc where r.pending is set; not read otherwise
template <bool kTree>
OKVFE_FP64_HD void refine_advance(PlaceRefineRecord& r, const PlaceRefineEval& e, int max_iterations) {
  if (r.status != kRefineRunning) return;
  if (r.pending) {
    r.pending = 0;
    const double cost_c = e.cost;
    bool accepted = false;
    double quality = 0.0;
    if (fp64::finite(cost_c)) {
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
OKVFE_FP64_UNROLL
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
OKVFE_FP64_UNROLL
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
OKVFE_FP64_UNROLL
    for (int i = 0; i < 6; ++i)
OKVFE_FP64_UNROLL
      for (int j = i; j < 6; ++j) {
        As[refine_upper(i, j)] = (r.S[i] * r.a[refine_upper(i, j)]) * r.S[j];
        M[refine_upper(i, j)] = As[refine_upper(i, j)];
      }
OKVFE_FP64_UNROLL
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
OKVFE_FP64_UNROLL
      for (int j = 0; j < 6; ++j) d[j] = r.S[j] * ds[j];
      double gd = 0.0, dAd = 0.0;
OKVFE_FP64_UNROLL
      for (int j = 0; j < 6; ++j) gd = gd + gs[j] * ds[j];
      double Ad[6];
OKVFE_FP64_UNROLL
      for (int i = 0; i < 6; ++i) {
        double v = 0.0;
OKVFE_FP64_UNROLL
        for (int j = 0; j < 6; ++j) v = v + As[i <= j ? refine_upper(i, j) : refine_upper(j, i)] * ds[j];
        Ad[i] = v;
      }
OKVFE_FP64_UNROLL
      for (int j = 0; j < 6; ++j) dAd = dAd + ds[j] * Ad[j];
      r.model_change = -(gd + 0.5 * dAd);
      if (!(r.model_change > 0.0)) valid = false;
    }
    if (valid) {
      double dd = 0.0, xx = 0.0;
OKVFE_FP64_UNROLL
      for (int j = 0; j < 6; ++j) dd = dd + d[j] * d[j];
OKVFE_FP64_UNROLL
      for (int j = 0; j < 7; ++j) xx = xx + r.x[j] * r.x[j];
      if (fp64::sqrt(dd) <= 1.0e-8 * (fp64::sqrt(xx) + 1.0e-8)) { r.status = 1; break; }
      double xc[7];
      valid = plus<kTree>(r.x, d, xc);
      if (valid) {
OKVFE_FP64_UNROLL
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
