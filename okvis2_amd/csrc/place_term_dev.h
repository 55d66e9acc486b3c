// place_term_dev.h -- one term of Frontend::verifyRecognisedPlace's ceres problem and of its Hessian H
// (okvis_ceres/include/okvis/ceres/implementation/ReprojectionError.hpp:99-183 with jacobians[0] only): the residual and
// J0_minimal at a pose T_Sold_Snew.  Shared, text unchanged, by place_hessian_kernel (k_place_hessian.hip) and
// place_refine_eval_kernel (k_place_refine.hip).  Device only.
// FP64, 3- and 4-term sums (fp64_ops.h) in the order of okvfe_set_fp64_reduction (a template argument), no FMA.  The
// matrix products are full: the zeros of T_CS, J, Jh and the square-root information are multiplied and added, so that a
// non-finite operand spreads as it does in Eigen.
// PARITY UNPINNED: Eigen's Quaternion::normalize() and toRotationMatrix() (Eigen is not in the tree), restated from the
// published source (Eigen/src/Geometry/Quaternion.h, Eigen/src/Core/Dot.h).
#pragma once
#include "camera_dev.h"
#include "fp64_ops.h"
#include "okvfe_internal.h"

namespace okvfe {

// q.normalize() and q.toRotationMatrix() of a PoseParameterBlock's (qx, qy, qz, qw) (ReprojectionError.hpp:101-103,
// :110-112, :115, :120): Eigen divides by sqrt(z) iff z = squaredNorm() > 0, so a zero or NaN quaternion stays as it is
template <bool kTree>
__device__ inline void quaternion_rotation(const double* q, double R[9]) {
  double x = q[0], y = q[1], z = q[2], w = q[3];
  const double n2 = fp64::sum4<kTree>(x * x, y * y, z * z, w * w);
  if (n2 > 0) {
    const double n = sqrt(n2);
    x = x / n; y = y / n; z = z / n; w = w / n;
  }
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz;         R[2] = txz + twy;
  R[3] = txy + twz;         R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;         R[7] = tyz + twx;         R[8] = 1.0 - (txx + tyy);
}

// the inverse of the pose (t, q) as a full 4 x 4 matrix (ReprojectionError.hpp:115-124): the rotation transposed, the
// translation (-C^T) t, the last row of the identity
template <bool kTree>
__device__ inline void inverse_transform(const double* pose /* t[3], qx qy qz qw */, double T[16]) {
  double C[9];
  quaternion_rotation<kTree>(pose + 3, C);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T[4 * i + j] = C[3 * j + i];
    T[4 * i + 3] = fp64::sum3<kTree>((-C[i]) * pose[0], (-C[3 + i]) * pose[1], (-C[6 + i]) * pose[2]);
  }
  T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
}

// ReprojectionError.hpp:125-162 for one term: hp_W of the landmark, the keypoint (measurement and size), T_SW and t_WS
// of the multiframe, T_CS and the intrinsics of the camera.  r = the weighted error, J = J0_minimal (2 x 6 row-major).
// Returns true where the result is the defined NaN (okvfe.h): a singular depth or a size that is no positive finite number.
template <bool kTree, bool kRT8>
__device__ __forceinline__ bool hessian_term(const DeviceCamera& cam, int w, int h, const double* T_SW, const double* t_WS,
                                             const double* T_CS, const double* hp_W, const okvfe_keypoint& kp, double r[2],
                                             double J[12]) {
  double hp_S[4], hp_C[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    hp_S[i] = fp64::sum4<kTree>(T_SW[4 * i] * hp_W[0], T_SW[4 * i + 1] * hp_W[1], T_SW[4 * i + 2] * hp_W[2],
                           T_SW[4 * i + 3] * hp_W[3]);                                      // :125
#pragma unroll
  for (int i = 0; i < 4; ++i)
    hp_C[i] = fp64::sum4<kTree>(T_CS[4 * i] * hp_S[0], T_CS[4 * i + 1] * hp_S[1], T_CS[4 * i + 2] * hp_S[2],
                           T_CS[4 * i + 3] * hp_S[3]);                                      // :126
  // projectHomogeneous (PinholeCamera.hpp:506-526): the head negated when w < 0, its Jacobian not negated back
  double head[3] = {hp_C[0], hp_C[1], hp_C[2]};
  if (hp_C[3] < 0) {
    head[0] = -head[0]; head[1] = -head[1]; head[2] = -head[2];
  }
  const double nan = __longlong_as_double(0x7FF8000000000000LL);
  double pt[2] = {nan, nan}, J23[6] = {nan, nan, nan, nan, nan, nan};
  const bool singular = fabs(head[2]) < 1.0e-12;  // PinholeCamera.hpp:302-304: nothing is written
  (void)cam::project_jacobian<kRT8>(cam, w, h, head, pt, J23);  // the status is ignored (ReprojectionError.hpp:133)
  const double Jh[2][4] = {{J23[0], J23[1], J23[2], 0.0}, {J23[3], J23[4], J23[5], 0.0}};  // :523-524
  // squareRootInformation_ of 64 / (size size) I (Frontend.cpp:464, ReprojectionError.hpp:75-76)
  const double size = (double)kp.size;
  const bool bad_size = !(size > 0.0 && size < __longlong_as_double(0x7FF0000000000000LL));
  const double s = sqrt(64.0 / (size * size));
  const double S[2][2] = {{s, 0.0}, {0.0, s}};
  double Jw[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) Jw[i][j] = S[i][0] * Jh[0][j] + S[i][1] * Jh[1][j];         // :134
  const double e[2] = {(double)kp.x - pt[0], (double)kp.y - pt[1]};                         // :139
  r[0] = S[0][0] * e[0] + S[0][1] * e[1];                                                   // :142
  r[1] = S[1][0] * e[0] + S[1][1] * e[1];
  // J of :155-159: [C_SW hp_W[3] | -C_SW crossMx(p)] over a zero row; C_SW is the rotation of T_SW
  const double p[3] = {hp_W[0] - t_WS[0] * hp_W[3], hp_W[1] - t_WS[1] * hp_W[3], hp_W[2] - t_WS[2] * hp_W[3]};
  const double X[3][3] = {{0.0, -p[2], p[1]}, {p[2], 0.0, -p[0]}, {-p[1], p[0], 0.0}};       // operators.hpp crossMx
  double Jp[4][6];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Jp[i][j] = T_SW[4 * i + j] * hp_W[3];
      Jp[i][3 + j] = fp64::sum3<kTree>((-T_SW[4 * i]) * X[0][j], (-T_SW[4 * i + 1]) * X[1][j], (-T_SW[4 * i + 2]) * X[2][j]);
    }
#pragma unroll
  for (int j = 0; j < 6; ++j) Jp[3][j] = 0.0;
  // J0_minimal = (Jh_weighted T_CS) J (:163)
  double A[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      A[i][j] = fp64::sum4<kTree>(Jw[i][0] * T_CS[j], Jw[i][1] * T_CS[4 + j], Jw[i][2] * T_CS[8 + j], Jw[i][3] * T_CS[12 + j]);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j)
      J[6 * i + j] = fp64::sum4<kTree>(A[i][0] * Jp[0][j], A[i][1] * Jp[1][j], A[i][2] * Jp[2][j], A[i][3] * Jp[3][j]);
  if (singular || bad_size) {
    r[0] = nan; r[1] = nan;
#pragma unroll
    for (int j = 0; j < 12; ++j) J[j] = nan;
    return true;
  }
  return false;
}

}  // namespace okvfe
