// radtan8_distortion.h -- the ONE product copy of the 8-coefficient radial-tangential distortion
// (OpenCV's "rational" model, okvis::cameras::RadialTangentialDistortion8), value and 2x2 point
// Jacobian.  Included by host_tables.cpp (host: awareness maps, overlap masks, host back-projection)
// and camera_dev.h (device: keypoint back-projection, landmark / motion-stereo projection).
//
// FP64 bit-equality with the reference depends only on the operation tree (no FMA: the library is
// built with -ffp-contract=off), so the expressions below keep the reference's grouping
// (RadialTangentialDistortion8.hpp:108-222): the rational factor num / den with
//   num = 1 + rho (k1 + rho (k2 + k3 rho)),  den = 1 + rho (k4 + rho (k5 + k6 rho)),
// and the quotient-rule Jacobian with its two divisions per entry (J(0,1) and J(1,0) are different
// expressions).  Named subterms are the same subtrees as in the reference; `* 1.0` factors are left
// out (exact).  Coefficients k[8] = k1 k2 p1 p2 k3 k4 k5 k6 (getIntrinsics order).
#pragma once

#include "atan_fixed.h"  // OKVFE_HD

namespace okvfe {

// Returns false for rho = |u|^2 > 9 (the reference's guard against the model's fold-over; out / J
// are then left untouched).  J row-major {J00, J01, J10, J11}; may be null.
// kPastFold: the same value is returned, but out / J are written past the guard as well: the
// formulas below evaluated at u, for a caller that ignores the status as ReprojectionError does
// (the reference reads indeterminate memory there; tests/radtan8_ref.py project defines it so).
template <bool kPastFold = false>
OKVFE_HD bool radtan8_distort(double u0, double u1, const double* k, double out[2], double* J) {
  const double k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4], k4 = k[5], k5 = k[6], k6 = k[7];
  const double mx = u0 * u0;
  const double my = u1 * u1;
  const double mxy = u0 * u1;
  const double rho = mx + my;
  const bool fold = rho > 9.0;
  if (fold && !kPastFold) return false;
  const double qn = k2 + k3 * rho;  // inner terms of the numerator / denominator polynomials
  const double pn = k1 + rho * qn;
  const double num = rho * pn + 1.0;
  const double qd = k5 + k6 * rho;
  const double pd = k4 + rho * qd;
  const double den = rho * pd + 1.0;
  const double rad = num / den;
  out[0] = u0 * rad + 2.0 * p1 * mxy + p2 * (rho + 2.0 * mx);
  out[1] = u1 * rad + 2.0 * p2 * mxy + p1 * (rho + 2.0 * my);
  if (!J) return !fold;
  const double den2 = den * den;
  // d num / d u_j and d den / d u_j
  const double dn0 = rho * (u0 * qn * 2.0 + k3 * u0 * rho * 2.0) + u0 * pn * 2.0;
  const double dn1 = rho * (u1 * qn * 2.0 + k3 * u1 * rho * 2.0) + u1 * pn * 2.0;
  const double dd0 = rho * (u0 * qd * 2.0 + k6 * u0 * rho * 2.0) + u0 * pd * 2.0;
  const double dd1 = rho * (u1 * qd * 2.0 + k6 * u1 * rho * 2.0) + u1 * pd * 2.0;
  J[0] = p1 * u1 * 2.0 + p2 * u0 * 6.0 + num / den + (u0 * dn0) / den - u0 * dd0 * num / den2;
  J[1] = p1 * u0 * 2.0 + p2 * u1 * 2.0 + (u0 * dn1) / den - u0 * dd1 * num / den2;
  J[2] = p1 * u0 * 2.0 + p2 * u1 * 2.0 + (u1 * dn0) / den - u1 * dd0 * num / den2;
  J[3] = p1 * u1 * 6.0 + p2 * u0 * 2.0 + num / den + (u1 * dn1) / den - u1 * dd1 * num / den2;
  return !fold;
}

}  // namespace okvfe
