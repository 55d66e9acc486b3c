// camera_dev.h -- device-side pinhole camera model (FP64), shared by k_describe.hip and k_match.hip.
// Restates okvis::cameras::PinholeCamera<D>::backProject / project and the distortion models
// (okvis_cv/include/okvis/cameras/implementation/PinholeCamera.hpp:241-283,574-593,
//  RadialTangentialDistortion.hpp:90-135,214-252, EquidistantDistortion.hpp:87-171,319-351,
//  RadialTangentialDistortion8.hpp:108-222,326-364 via radtan8_distortion.h).
// Component-wise, sums left to right, no FMA (-ffp-contract=off).
//
// Attribution: the distortion formulas in distort() below (radial-tangential value + Jacobian, and
// the machine-generated equidistant Jacobian with its temporaries t2..t25) keep the reference's
// operation order on purpose -- FP64 bit-exactness depends on it -- and are therefore a close
// transcription of RadialTangentialDistortion.hpp:111-135 and EquidistantDistortion.hpp:128-171,
// which are Copyright (c) 2015 Autonomous Systems Lab / ETH Zurich, (c) 2020 Smart Robotics Lab /
// Imperial College London, (c) 2024 Smart Robotics Lab / Technical University of Munich,
// distributed under the BSD 3-Clause licence (see the licence header of those files; the
// conditions -- retain the copyright notice, the list of conditions and the disclaimer; no
// endorsement with the holders' names -- apply to this fragment).
#pragma once

#include "atan_fixed.h"
#include "equidistant_jacobian.h"
#include "okvfe_internal.h"
#include "radtan8_distortion.h"

namespace okvfe {
namespace cam {

// kRT8: the form that also knows OKVFE_DIST_RADTAN8 (radtan8_distortion.h).  The host launches it only
// when a camera slot of the call holds such a camera, so the kernels of the other three models keep
// their code (and registers) exactly.  distort returns false where the model fails (RADTAN8, rho > 9).
// kPastFold: out / J are written there as well (radtan8_distortion.h), for project_jacobian below.
template <bool kRT8 = false, bool kPastFold = false>
__device__ inline bool distort(const DeviceCamera& c, double u0, double u1, double out[2], double J[4]) {
  if constexpr (kRT8) {
    if (c.distortion == OKVFE_DIST_RADTAN8) return radtan8_distort<kPastFold>(u0, u1, c.d, out, J);
  }
  if (c.distortion == OKVFE_DIST_NONE) {
    out[0] = u0; out[1] = u1;
    J[0] = 1.0; J[1] = 0.0; J[2] = 0.0; J[3] = 1.0;
    return true;
  }
  if (c.distortion == OKVFE_DIST_RADTAN) {
    const double k1 = c.d[0], k2 = c.d[1], p1 = c.d[2], p2 = c.d[3];
    const double mx_u = u0 * u0;
    const double my_u = u1 * u1;
    const double mxy_u = u0 * u1;
    const double rho_u = mx_u + my_u;
    const double rad_dist_u = k1 * rho_u + k2 * rho_u * rho_u;
    out[0] = u0 + u0 * rad_dist_u + 2.0 * p1 * mxy_u + p2 * (rho_u + 2.0 * mx_u);
    out[1] = u1 + u1 * rad_dist_u + 2.0 * p2 * mxy_u + p1 * (rho_u + 2.0 * my_u);
    J[0] = 1 + rad_dist_u + k1 * 2.0 * mx_u + k2 * rho_u * 4 * mx_u + 2.0 * p1 * u1 + 6 * p2 * u0;
    J[2] = k1 * 2.0 * u0 * u1 + k2 * 4 * rho_u * u0 * u1 + p1 * 2.0 * u0 + 2.0 * p2 * u1;
    J[1] = J[2];
    J[3] = 1 + rad_dist_u + k1 * 2.0 * my_u + k2 * rho_u * 4 * my_u + 6 * p1 * u1 + 2.0 * p2 * u0;
    return true;
  }
  // equidistant; atan_fixed: the same operation sequence as on the host (atan_fixed.h)
  const double k1 = c.d[0], k2 = c.d[1], k3 = c.d[2], k4 = c.d[3];
  const double r = sqrt(u0 * u0 + u1 * u1);
  const double theta = atan_fixed(r);
  const double theta2 = theta * theta;
  const double theta4 = theta2 * theta2;
  const double theta6 = theta4 * theta2;
  const double theta8 = theta4 * theta4;
  const double thetad = theta * (1.0 + k1 * theta2 + k2 * theta4 + k3 * theta6 + k4 * theta8);
  const double scaling = (r > 1e-8) ? thetad / r : 1.0;
  out[0] = scaling * u0;
  out[1] = scaling * u1;
  if (r > 1e-8) {
    equidistant_jacobian(u0, u1, k1, k2, k3, k4, [](double v) { return sqrt(v); }, J);  // equidistant_jacobian.h
  } else {
    J[0] = 1.0; J[1] = 0.0; J[2] = 0.0; J[3] = 1.0;
  }
  return true;
}

// Gauss-Newton undistortion: 5 steps for the radial-tangential models, 20 for equidistant; success at
// chi2 < 1e-6 (RADTAN8: 1e-4), early stop at 1e-15.  A RADTAN8 step whose distort fails ends the
// iteration with the back-projection invalid (okvfe.h, OKVFE_DIST_RADTAN8).
template <bool kRT8 = false>
__device__ inline bool backproject(const DeviceCamera& c, double px, double py, double dir[3]) {
  const double pd0 = (px - c.cu) * c.one_over_fu;
  const double pd1 = (py - c.cv) * c.one_over_fv;
  bool success = false;
  double x0 = pd0, x1 = pd1;
  if (c.distortion == OKVFE_DIST_NONE) {
    success = true;
  } else {
    const bool rt8 = kRT8 && c.distortion == OKVFE_DIST_RADTAN8;
    const int n = c.distortion == OKVFE_DIST_RADTAN || rt8 ? 5 : 20;
    const double chi2_ok = rt8 ? 1e-4 : 1e-6;
    for (int i = 0; i < n; ++i) {
      double xt[2], E[4];
      if (!distort<kRT8>(c, x0, x1, xt, E)) {
        success = false;
        break;
      }
      const double e0 = pd0 - xt[0], e1 = pd1 - xt[1];
      const double a = E[0] * E[0] + E[2] * E[2];
      const double b = E[0] * E[1] + E[2] * E[3];
      const double cc = E[1] * E[0] + E[3] * E[2];
      const double d = E[1] * E[1] + E[3] * E[3];
      const double det = a * d - b * cc;
      const double invdet = 1.0 / det;
      const double i00 = d * invdet, i01 = -b * invdet, i10 = -cc * invdet, i11 = a * invdet;
      const double b00 = i00 * E[0] + i01 * E[1];
      const double b01 = i00 * E[2] + i01 * E[3];
      const double b10 = i10 * E[0] + i11 * E[1];
      const double b11 = i10 * E[2] + i11 * E[3];
      const double du0 = b00 * e0 + b01 * e1;
      const double du1 = b10 * e0 + b11 * e1;
      x0 += du0;
      x1 += du1;
      const double chi2 = e0 * e0 + e1 * e1;
      if (chi2 < chi2_ok) success = true;
      if (chi2 < 1e-15) {
        success = true;
        break;
      }
    }
  }
  dir[0] = x0;
  dir[1] = x1;
  dir[2] = 1.0;
  return success;
}


// PinholeCamera::project without Jacobian; status 0 = Successful, 1 = OutsideImage, 3 = Behind,
// 4 = Invalid (PinholeCamera.hpp:241-283, CameraBase.hpp:97-106)
template <bool kRT8 = false>
__device__ inline int project(const DeviceCamera& c, int w, int h, const double p[3], double pt[2]) {
  if (fabs(p[2]) < 1.0e-12) return 4;
  const double rz = 1.0 / p[2];
  double dist[2], J[4];
  if (!distort<kRT8>(c, p[0] * rz, p[1] * rz, dist, J)) return 4;
  pt[0] = c.fu * dist[0] + c.cu;
  pt[1] = c.fv * dist[1] + c.cv;
  if (pt[0] < 0.0 || pt[1] < 0.0) return 1;
  if (pt[0] >= (double)w || pt[1] >= (double)h) return 1;
  return p[2] > 0.0 ? 0 : 3;
}

// PinholeCamera::project with the 2 x 3 point Jacobian J23 (row-major; PinholeCamera.hpp:296-374), for callers that
// ignore the status as ReprojectionError.hpp:133 does.  The same statuses.  Status 4 of a singular depth
// (fabs(p[2]) < 1.0e-12, :302-304) returns before anything is written, as the reference does; status 4 of a distortion
// failure (RADTAN8, rho > 9) comes with pt and J23 of the model's formulas evaluated past their guard, where the
// reference leaves imagePoint2 and distortionJacobian indeterminate (:339-358).
template <bool kRT8 = false>
__device__ inline int project_jacobian(const DeviceCamera& c, int w, int h, const double p[3], double pt[2],
                                       double J23[6]) {
  if (fabs(p[2]) < 1.0e-12) return 4;
  const double rz = 1.0 / p[2];
  const double rz2 = rz * rz;
  double dist[2], D[4];
  const bool ok = distort<kRT8, true>(c, p[0] * rz, p[1] * rz, dist, D);
  J23[0] = c.fu * D[0] * rz;
  J23[1] = c.fu * D[1] * rz;
  J23[2] = -c.fu * (p[0] * D[0] + p[1] * D[1]) * rz2;
  J23[3] = c.fv * D[2] * rz;
  J23[4] = c.fv * D[3] * rz;
  J23[5] = -c.fv * (p[0] * D[2] + p[1] * D[3]) * rz2;
  pt[0] = c.fu * dist[0] + c.cu;
  pt[1] = c.fv * dist[1] + c.cv;
  if (!ok) return 4;
  if (pt[0] < 0.0 || pt[1] < 0.0) return 1;
  if (pt[0] >= (double)w || pt[1] >= (double)h) return 1;
  return p[2] > 0.0 ? 0 : 3;
}

}  // namespace cam
}  // namespace okvfe
