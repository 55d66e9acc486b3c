// imu_dev.h -- ImuError::propagation (okvis_ceres/src/ImuError.cpp:557-779) as ONE sequence of IEEE-754 operations that
// compiles for the host and for gfx950: the pose guess every frame starts from, its 15 x 15 Jacobian F and covariance P,
// and per camera T_WC = T_WS T_SC (ThreadedSlam.cpp:434-444) with the extraction direction
// T_WC.inverse().C() * (0, 0, -1) (Frontend.cpp:246-251).  The host entry okvfe_imu_propagation (capi_imu.cpp), the
// stand-alone program tests/cpp/imu_propagation_main.cpp and the kernels of k_imu.hip are all this header;
// tests/imu_ref.py restates it in numpy, and the tests hold all of them to that restatement byte for byte.
//
//   the loop             :601-743 as written: the dt <= 0 skip, the end < nexttime interpolation, the !hasStarted
//                        interpolation, both saturation tests (strict >, sigma *= 100), break on nexttime == t_end
//   time                 okvis_time: a timestamp is (uint32 sec, uint32 nsec); Time - Time goes through the
//                        Duration(int32, int32) constructor, which normalises; toSec() = double(sec) + 1e-9 * double(nsec)
//   sinc, rightJacobian  okvis_kinematics implementation/Transformation.hpp:50-62, :74-87; crossMx operators.hpp:60-73
//   Transformation       the constructor and set() normalise the quaternion (:131-138, :239-244); inverse :207-210;
//                        operator* :261-264
//
// Expression order: Eigen expressions in source order, left to right, one operation at a time (the library is built with
// -ffp-contract=off: no FMA).  3-term sums and the 4-term sums of squaredNorm() follow okvfe_set_fp64_reduction (the
// template argument kTree; fp64_ops.h, with Eigen's quaternion product, whose sums run left to right, and normalized()).  The 15-term sums of
// F_delta P_delta F_delta^T ((F_delta P_delta) first) and of T P_delta T^T run in ascending k from the first product; the
// switch does not apply to them.  Zeros are multiplied and added, so a non-finite operand spreads as it does in Eigen.
// PARITY UNPINNED: Eigen's own evaluation order of these expressions, its products, normalized(), inverse() and
// toRotationMatrix() are restated from the published sources (Eigen is not in the tree).
//
// DEFINED DEVIATIONS from the reference:
//   * cos and sinc of theta_half, and cos and sin of Phi in rightJacobian, are cos_fixed, sinc_fixed and sin_fixed
//     (elementary_fixed.h): within 1 ulp of libm for |x| <= pi / 4 and NaN beyond.  The NaN spreads into the outputs, and
//     n_out_of_range counts the intervals in which one of them was called outside its domain (a NaN argument included).
//     At 200 Hz that takes a rate above 157 rad/s.
//   * The reference reads element it + 1 before it knows that it exists.  Here it is read only where it exists; the
//     iteration of the last element, which no input with t_start < t_end reaches, ends the loop.
//   * t_end <= t_start: zero increments and n_propagated = 0.
//   * front().timeStamp > t_start (the reference's assertion) is status bit 1, an empty sample list status bit 2; nothing
//     but status and n_out_of_range (= 0) is written for such a multiframe.
//   * back().timeStamp < t_end: n_propagated = -1 as in the reference, pose and speed_and_bias are the inputs unchanged
//     (the per-camera outputs are those of that pose); F and P are not written.
#pragma once
#include <stdint.h>

#include "elementary_fixed.h"
#include "fp64_ops.h"

namespace okvfe {

constexpr int kImuSampleDoubles = 8;  // (sec, nsec) as two uint32 in the first double's bytes, gyro[3], accel[3], unused
constexpr int kImuStateDoubles = 18;  // t_start, t_end (each as a sample's first double), T_WS[7], speedAndBias[9]
constexpr int kImuStatusFrontAfterStart = 1, kImuStatusEmpty = 2;

struct ImuParams {  // okvfe_imu_params
  double a_max, g_max, sigma_g_c, sigma_a_c, sigma_gw_c, sigma_aw_c, g;
};

struct ImuTime {
  uint32_t sec, nsec;
};

OKVFE_FP64_HD ImuTime imu_time(const double* first) {
  unsigned long long bits;
  __builtin_memcpy(&bits, first, 8);
  ImuTime t;
  t.sec = (uint32_t)(bits & 0xFFFFFFFFull);
  t.nsec = (uint32_t)(bits >> 32);
  return t;
}
OKVFE_FP64_HD bool imu_time_lt(ImuTime a, ImuTime b) { return a.sec < b.sec || (a.sec == b.sec && a.nsec < b.nsec); }
OKVFE_FP64_HD bool imu_time_eq(ImuTime a, ImuTime b) { return a.sec == b.sec && a.nsec == b.nsec; }
// (a - b).toSec(): Time.hpp:85-88, Duration.cpp:55-73, Duration::toSec
OKVFE_FP64_HD double imu_time_diff(ImuTime a, ImuTime b) {
  long long s = (long long)(int32_t)a.sec - (long long)(int32_t)b.sec;
  long long n = (long long)(int32_t)a.nsec - (long long)(int32_t)b.nsec;
  while (n > 1000000000LL) {
    n -= 1000000000LL;
    ++s;
  }
  while (n < 0) {
    n += 1000000000LL;
    --s;
  }
  return (double)(int32_t)s + 1e-9 * (double)(int32_t)n;
}

OKVFE_FP64_HD double imu_abs(double x) { return __builtin_fabs(x); }

// 3 x 3 matrices are row-major double[9]; no output aliases an input
template <bool kTree>
OKVFE_FP64_HD void imu_matvec(const double* M, const double* v, double* o) {
OKVFE_FP64_UNROLL
  for (int i = 0; i < 3; ++i) o[i] = fp64::sum3<kTree>(M[3 * i] * v[0], M[3 * i + 1] * v[1], M[3 * i + 2] * v[2]);
}
template <bool kTree>
OKVFE_FP64_HD void imu_matmul(const double* A, const double* B, double* O) {
OKVFE_FP64_UNROLL
  for (int i = 0; i < 3; ++i)
OKVFE_FP64_UNROLL
    for (int j = 0; j < 3; ++j) O[3 * i + j] = fp64::sum3<kTree>(A[3 * i] * B[j], A[3 * i + 1] * B[3 + j], A[3 * i + 2] * B[6 + j]);
}
template <bool kTree>
OKVFE_FP64_HD double imu_norm3(const double* v) {
  return sqrt(fp64::sum3<kTree>(v[0] * v[0], v[1] * v[1], v[2] * v[2]));
}
// operators.hpp:60-73
OKVFE_FP64_HD void imu_cross_mx(const double* v, double* X) {
  X[0] = 0.0;   X[1] = -v[2]; X[2] = v[1];
  X[3] = v[2];  X[4] = 0.0;   X[5] = -v[0];
  X[6] = -v[1]; X[7] = v[0];  X[8] = 0.0;
}
// q.toRotationMatrix() of (x, y, z, w), not normalised first (Eigen/src/Geometry/Quaternion.h)
OKVFE_FP64_HD void imu_to_rotation(const double* q, double* R) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz;         R[2] = txz + twy;
  R[3] = txy + twz;         R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;         R[7] = tyz + twx;         R[8] = 1.0 - (txx + tyy);
}
// Eigen's inverse(): conjugate().coeffs() / squaredNorm() iff that is > 0, else zeros
template <bool kTree>
OKVFE_FP64_HD void imu_q_inverse(const double* q, double* o) {
  const double n2 = fp64::sum4<kTree>(q[0] * q[0], q[1] * q[1], q[2] * q[2], q[3] * q[3]);
  if (n2 > 0) {
    o[0] = (-q[0]) / n2; o[1] = (-q[1]) / n2; o[2] = (-q[2]) / n2; o[3] = q[3] / n2;
  } else {
    o[0] = 0.0; o[1] = 0.0; o[2] = 0.0; o[3] = 0.0;
  }
}

// Transformation.hpp:74-87.  Returns true where cos_fixed / sin_fixed were called outside their domain.
template <bool kTree>
OKVFE_FP64_HD bool imu_right_jacobian(const double* phi_vec, double* R) {
  const double Phi = imu_norm3<kTree>(phi_vec);
  double Px[9], Px2[9];
  imu_cross_mx(phi_vec, Px);
  imu_matmul<kTree>(Px, Px, Px2);
  if (Phi < 1.0e-4) {
    const double c_6th = 1.66666666666666657415e-01;  // 1.0 / 6.0
OKVFE_FP64_UNROLL
    for (int e = 0; e < 9; ++e) R[e] = (e % 4 == 0 ? 1.0 : 0.0) + (-0.5 * Px[e] + c_6th * Px2[e]);
    return false;
  }
  const double Phi2 = Phi * Phi;
  const double Phi3 = Phi2 * Phi;
  const double a = (-(1.0 - cos_fixed(Phi))) / Phi2;
  const double b = (Phi - sin_fixed(Phi)) / Phi3;
OKVFE_FP64_UNROLL
  for (int e = 0; e < 9; ++e) R[e] = (e % 4 == 0 ? 1.0 : 0.0) + (a * Px[e] + b * Px2[e]);
  return !(Phi <= 7.85398163397448278999e-01);
}

// the eight 3 x 3 blocks in which F_delta (:692-702) and F (:756-765) differ from the identity
struct ImuBlocks {
  double b0_3[9], b0_6[9], b0_9[9], b0_12[9], b3_9[9], b6_3[9], b6_9[9], b6_12[9];
};
// M (15 x 15 row-major, the identity outside these blocks) with the blocks put in
OKVFE_FP64_HD void imu_put_blocks(const ImuBlocks& B, double* M) {
OKVFE_FP64_UNROLL
  for (int i = 0; i < 3; ++i)
OKVFE_FP64_UNROLL
    for (int j = 0; j < 3; ++j) {
      M[15 * i + 3 + j] = B.b0_3[3 * i + j];
      M[15 * i + 6 + j] = B.b0_6[3 * i + j];
      M[15 * i + 9 + j] = B.b0_9[3 * i + j];
      M[15 * i + 12 + j] = B.b0_12[3 * i + j];
      M[15 * (3 + i) + 9 + j] = B.b3_9[3 * i + j];
      M[15 * (6 + i) + 3 + j] = B.b6_3[3 * i + j];
      M[15 * (6 + i) + 9 + j] = B.b6_9[3 * i + j];
      M[15 * (6 + i) + 12 + j] = B.b6_12[3 * i + j];
    }
}
// T of :772-775 (the identity with C_WS_0 three times on the diagonal), into an identity
OKVFE_FP64_HD void imu_put_T(const double* C, double* M) {
OKVFE_FP64_UNROLL
  for (int b = 0; b < 3; ++b)
OKVFE_FP64_UNROLL
    for (int i = 0; i < 3; ++i)
OKVFE_FP64_UNROLL
      for (int j = 0; j < 3; ++j) M[15 * (3 * b + i) + 3 * b + j] = C[3 * i + j];
}
// one entry of a 15 x 15 product: the 15 terms a[k sa] b[k sb] in ascending k from the first product
OKVFE_FP64_HD double imu_dot15(const double* a, int sa, const double* b, int sb) {
  double acc = a[0] * b[0];
  for (int k = 1; k < 15; ++k) acc = acc + a[k * sa] * b[k * sb];
  return acc;
}
// the noise of :708-727 for diagonal entry e of P_delta
struct ImuNoise {
  double dalpha, v, p, b_g, b_a;
};
OKVFE_FP64_HD double imu_noise_of(const ImuNoise& N, int e) {
  return e < 3 ? N.p : e < 6 ? N.dalpha : e < 9 ? N.v : e < 12 ? N.b_g : N.b_a;
}

// The covariance of the host: P_delta, F_delta P_delta and F_delta in plain arrays.  (The kernel's policy keeps the three
// in LDS and gives a fixed lane to every group of entries; each entry is the same imu_dot15.)
struct ImuCovNone {
  OKVFE_FP64_HD void begin() {}
  OKVFE_FP64_HD void step(const ImuBlocks&, const ImuNoise&) {}
  OKVFE_FP64_HD void finish(const double*, double*) {}
};
struct ImuCovHost {
  double P[225], FP[225], F[225];
  void identity(double* M) {
    for (int e = 0; e < 225; ++e) M[e] = e % 16 == 0 ? 1.0 : 0.0;
  }
  void begin() {
    for (int e = 0; e < 225; ++e) P[e] = 0.0;
    identity(F);
  }
  void step(const ImuBlocks& B, const ImuNoise& N) {
    imu_put_blocks(B, F);
    for (int e = 0; e < 225; ++e) FP[e] = imu_dot15(F + 15 * (e / 15), 1, P + e % 15, 15);
    for (int e = 0; e < 225; ++e) P[e] = imu_dot15(FP + 15 * (e / 15), 1, F + 15 * (e % 15), 1);
    for (int e = 0; e < 15; ++e) P[16 * e] = P[16 * e] + imu_noise_of(N, e);
  }
  void finish(const double* C_WS_0, double* out) {
    identity(F);
    imu_put_T(C_WS_0, F);
    for (int e = 0; e < 225; ++e) FP[e] = imu_dot15(F + 15 * (e / 15), 1, P + e % 15, 15);
    for (int e = 0; e < 225; ++e) out[e] = imu_dot15(FP + 15 * (e / 15), 1, F + 15 * (e % 15), 1);
  }
};

struct ImuOut {
  int32_t status, n_out_of_range, n_propagated;
  bool wrote_state;     // pose and speed_and_bias (and the per-camera outputs) are written
  bool wrote_jacobian;  // ... and F, P: the propagation ran
  double pose[7], speed_and_bias[9];
  double Delta_t;
  ImuBlocks F;          // kJac: F's blocks (b0_6 = I Delta_t)
};

// One multiframe.  samples: n records of kImuSampleDoubles; state: kImuStateDoubles.  kJac: the sub-Jacobians are
// accumulated and o.F is filled; kCov (needs kJac): cov sees every interval's F_delta and noise.  P itself is
// cov.finish(C_WS_0, out), which the caller runs where o.wrote_jacobian.
template <bool kTree, bool kJac, bool kCov, class Cov>
OKVFE_FP64_HD void imu_propagate(const ImuParams& prm, const double* samples, int n, const double* state, Cov& cov,
                                ImuOut& o, double* C_WS_0) {
  static_assert(kJac || !kCov, "the covariance needs the sub-Jacobians");
  o.status = 0; o.n_out_of_range = 0; o.n_propagated = 0; o.wrote_state = false; o.wrote_jacobian = false;
  o.Delta_t = 0.0;
  if (n <= 0) {
    o.status = kImuStatusEmpty;
    return;
  }
  const ImuTime t_start = imu_time(state), t_end = imu_time(state + 1);
  if (imu_time_lt(t_start, imu_time(samples))) {  // :570, the assertion
    o.status = kImuStatusFrontAfterStart;
    return;
  }
OKVFE_FP64_UNROLL
  for (int e = 0; e < 7; ++e) o.pose[e] = state[2 + e];
OKVFE_FP64_UNROLL
  for (int e = 0; e < 9; ++e) o.speed_and_bias[e] = state[9 + e];
  o.wrote_state = true;
  if (imu_time_lt(imu_time(samples + (long long)(n - 1) * kImuSampleDoubles), t_end)) {  // :572
    o.n_propagated = -1;
    return;
  }
  o.wrote_jacobian = true;
  const double* sb = o.speed_and_bias;
  imu_to_rotation(o.pose + 3, C_WS_0);
  double Delta_q[4] = {0.0, 0.0, 0.0, 1.0};
  double C_integral[9], C_doubleintegral[9], cross[9], dalpha_db_g[9], dv_db_g[9], dp_db_g[9];
  double acc_integral[3] = {0.0, 0.0, 0.0}, acc_doubleintegral[3] = {0.0, 0.0, 0.0};
OKVFE_FP64_UNROLL
  for (int e = 0; e < 9; ++e) {
    C_integral[e] = 0.0; C_doubleintegral[e] = 0.0; cross[e] = 0.0; dalpha_db_g[e] = 0.0; dv_db_g[e] = 0.0; dp_db_g[e] = 0.0;
  }
  if constexpr (kCov) cov.begin();
  double Delta_t = 0.0;
  bool has_started = false;
  int i = 0, n_oor = 0;
  ImuTime time = t_start;
  const int n_loop = imu_time_lt(t_start, t_end) ? n - 1 : 0;  // (the last element's iteration only ends the loop)
  for (int it = 0; it < n_loop; ++it) {
    const double* s0 = samples + (long long)it * kImuSampleDoubles;
    const double* s1 = s0 + kImuSampleDoubles;
    double omega_S_0[3] = {s0[1], s0[2], s0[3]}, acc_S_0[3] = {s0[4], s0[5], s0[6]};
    double omega_S_1[3] = {s1[1], s1[2], s1[3]}, acc_S_1[3] = {s1[4], s1[5], s1[6]};
    const ImuTime t0 = imu_time(s0);
    ImuTime nexttime = imu_time(s1);
    double dt = imu_time_diff(nexttime, time);
    if (imu_time_lt(t_end, nexttime)) {  // :618
      const double interval = imu_time_diff(nexttime, t0);
      nexttime = t_end;
      dt = imu_time_diff(nexttime, time);
      const double r = dt / interval;
OKVFE_FP64_UNROLL
      for (int k = 0; k < 3; ++k) {
        omega_S_1[k] = (1.0 - r) * omega_S_0[k] + r * omega_S_1[k];
        acc_S_1[k] = (1.0 - r) * acc_S_0[k] + r * acc_S_1[k];
      }
    }
    if (dt <= 0.0) continue;
    Delta_t = Delta_t + dt;
    if (!has_started) {  // :632
      has_started = true;
      const double r = dt / imu_time_diff(nexttime, t0);
OKVFE_FP64_UNROLL
      for (int k = 0; k < 3; ++k) {
        omega_S_0[k] = r * omega_S_0[k] + (1.0 - r) * omega_S_1[k];
        acc_S_0[k] = r * acc_S_0[k] + (1.0 - r) * acc_S_1[k];
      }
    }
    double sigma_g_c = prm.sigma_g_c, sigma_a_c = prm.sigma_a_c;
    if (imu_abs(omega_S_0[0]) > prm.g_max || imu_abs(omega_S_0[1]) > prm.g_max || imu_abs(omega_S_0[2]) > prm.g_max ||
        imu_abs(omega_S_1[0]) > prm.g_max || imu_abs(omega_S_1[1]) > prm.g_max || imu_abs(omega_S_1[2]) > prm.g_max)
      sigma_g_c = sigma_g_c * 100.0;
    if (imu_abs(acc_S_0[0]) > prm.a_max || imu_abs(acc_S_0[1]) > prm.a_max || imu_abs(acc_S_0[2]) > prm.a_max ||
        imu_abs(acc_S_1[0]) > prm.a_max || imu_abs(acc_S_1[1]) > prm.a_max || imu_abs(acc_S_1[2]) > prm.a_max)
      sigma_a_c = sigma_a_c * 100.0;
    // orientation (:664-671)
    double omega_S_true[3], acc_S_true[3], dq[4], Delta_q_1[4];
OKVFE_FP64_UNROLL
    for (int k = 0; k < 3; ++k) omega_S_true[k] = 0.5 * (omega_S_0[k] + omega_S_1[k]) - sb[3 + k];
    const double theta_half = (imu_norm3<kTree>(omega_S_true) * 0.5) * dt;
    const double sinc_theta_half = sinc_fixed(theta_half);
    const double cos_theta_half = cos_fixed(theta_half);
    bool oor = !(theta_half <= 7.85398163397448278999e-01);
OKVFE_FP64_UNROLL
    for (int k = 0; k < 3; ++k) dq[k] = ((sinc_theta_half * omega_S_true[k]) * 0.5) * dt;
    dq[3] = cos_theta_half;
    fp64::quat_product(Delta_q, dq, Delta_q_1);
    // rotation matrix integrals (:673-680)
    double C[9], C_1[9], CC[9], half_CC[9], quarter_CC[9], half_acc[3], quarter_acc[3];
    imu_to_rotation(Delta_q, C);
    imu_to_rotation(Delta_q_1, C_1);
OKVFE_FP64_UNROLL
    for (int k = 0; k < 3; ++k) acc_S_true[k] = 0.5 * (acc_S_0[k] + acc_S_1[k]) - sb[6 + k];
OKVFE_FP64_UNROLL
    for (int e = 0; e < 9; ++e) {
      CC[e] = C[e] + C_1[e];
      half_CC[e] = 0.5 * CC[e];
      quarter_CC[e] = 0.25 * CC[e];
    }
    imu_matvec<kTree>(half_CC, acc_S_true, half_acc);
    imu_matvec<kTree>(quarter_CC, acc_S_true, quarter_acc);
    double acc_integral_1[3];
OKVFE_FP64_UNROLL
    for (int k = 0; k < 3; ++k) {
      half_acc[k] = half_acc[k] * dt;
      quarter_acc[k] = (quarter_acc[k] * dt) * dt;
      acc_integral_1[k] = acc_integral[k] + half_acc[k];
      acc_doubleintegral[k] = acc_doubleintegral[k] + (acc_integral[k] * dt + quarter_acc[k]);
    }
    double phi_vec[3];
OKVFE_FP64_UNROLL
    for (int k = 0; k < 3; ++k) phi_vec[k] = omega_S_true[k] * dt;
    if constexpr (!kJac) {
      const double Phi = imu_norm3<kTree>(phi_vec);  // rightJacobian's argument: only whether it is in the domain
      oor = oor || (!(Phi < 1.0e-4) && !(Phi <= 7.85398163397448278999e-01));
    } else {
      double C_integral_1[9];
OKVFE_FP64_UNROLL
      for (int e = 0; e < 9; ++e) {
        C_integral_1[e] = C_integral[e] + half_CC[e] * dt;
        C_doubleintegral[e] = C_doubleintegral[e] + (C_integral[e] * dt + (quarter_CC[e] * dt) * dt);
      }
      // Jacobian parts (:683-688)
OKVFE_FP64_UNROLL
      for (int e = 0; e < 9; ++e) dalpha_db_g[e] = dalpha_db_g[e] + dt * C_1[e];
      double rj[9], dq_inv[4], R_inv[9], cross_1[9], acc_S_x[9], t0m[9], t1m[9], t2m[9], S[9], dv_db_g_1[9];
      oor = imu_right_jacobian<kTree>(phi_vec, rj) || oor;
      imu_q_inverse<kTree>(dq, dq_inv);
      imu_to_rotation(dq_inv, R_inv);
      imu_matmul<kTree>(R_inv, cross, cross_1);
OKVFE_FP64_UNROLL
      for (int e = 0; e < 9; ++e) cross_1[e] = cross_1[e] + rj[e] * dt;
      imu_cross_mx(acc_S_true, acc_S_x);
      imu_matmul<kTree>(C, acc_S_x, t0m);
      imu_matmul<kTree>(t0m, cross, t1m);
      imu_matmul<kTree>(C_1, acc_S_x, t0m);
      imu_matmul<kTree>(t0m, cross_1, t2m);
      const double half_dt = 0.5 * dt, quarter_dt2 = (0.25 * dt) * dt;
      ImuBlocks Fd;
OKVFE_FP64_UNROLL
      for (int e = 0; e < 9; ++e) {
        S[e] = t1m[e] + t2m[e];
        dv_db_g_1[e] = dv_db_g[e] + half_dt * S[e];
        const double dp_inc = dt * dv_db_g[e] + quarter_dt2 * S[e];
        dp_db_g[e] = dp_db_g[e] + dp_inc;
        if constexpr (kCov) {  // :692-702
          Fd.b0_6[e] = (e % 4 == 0 ? 1.0 : 0.0) * dt;
          Fd.b0_9[e] = dp_inc;
          Fd.b0_12[e] = (-C_integral[e]) * dt + (quarter_CC[e] * dt) * dt;
          Fd.b3_9[e] = (-dt) * C_1[e];
          Fd.b6_9[e] = half_dt * S[e];
          Fd.b6_12[e] = (-0.5 * CC[e]) * dt;
        }
      }
      if constexpr (kCov) {
        double v[3], X[9];
OKVFE_FP64_UNROLL
        for (int k = 0; k < 3; ++k) v[k] = acc_integral[k] * dt + quarter_acc[k];
        imu_cross_mx(v, X);
OKVFE_FP64_UNROLL
        for (int e = 0; e < 9; ++e) Fd.b0_3[e] = -X[e];
        imu_cross_mx(half_acc, X);
OKVFE_FP64_UNROLL
        for (int e = 0; e < 9; ++e) Fd.b6_3[e] = -X[e];
        ImuNoise N;  // :708-724
        N.dalpha = (dt * sigma_g_c) * sigma_g_c;
        N.v = (dt * sigma_a_c) * prm.sigma_a_c;
        N.p = ((0.5 * dt) * dt) * N.v;
        N.b_g = (dt * prm.sigma_gw_c) * prm.sigma_gw_c;
        N.b_a = (dt * prm.sigma_aw_c) * prm.sigma_aw_c;
        cov.step(Fd, N);
      }
OKVFE_FP64_UNROLL
      for (int e = 0; e < 9; ++e) {
        C_integral[e] = C_integral_1[e];
        cross[e] = cross_1[e];
        dv_db_g[e] = dv_db_g_1[e];
      }
    }
    if (oor) ++n_oor;
    // memory shift (:731-741)
OKVFE_FP64_UNROLL
    for (int k = 0; k < 4; ++k) Delta_q[k] = Delta_q_1[k];
OKVFE_FP64_UNROLL
    for (int k = 0; k < 3; ++k) acc_integral[k] = acc_integral_1[k];
    time = nexttime;
    ++i;
    if (imu_time_eq(nexttime, t_end)) break;
  }
  // the epilogue (:745-777)
  const double z2 = fp64::sum3<kTree>(0.0 * 0.0, 0.0 * 0.0, 6371009.0 * 6371009.0);
  const double zn = sqrt(z2);
  const double g_W[3] = {prm.g * (0.0 / zn), prm.g * (0.0 / zn), prm.g * (6371009.0 / zn)};
  double Ca[3], Cv[3], q_new[4];
  imu_matvec<kTree>(C_WS_0, acc_doubleintegral, Ca);
  imu_matvec<kTree>(C_WS_0, acc_integral, Cv);
  fp64::quat_product(o.pose + 3, Delta_q, q_new);
OKVFE_FP64_UNROLL
  for (int k = 0; k < 3; ++k) {
    o.pose[k] = ((o.pose[k] + sb[k] * Delta_t) + Ca[k]) - ((0.5 * g_W[k]) * Delta_t) * Delta_t;
    o.speed_and_bias[k] = sb[k] + (Cv[k] - g_W[k] * Delta_t);
  }
  fp64::quat_normalized<kTree>(q_new, o.pose + 3);
  o.n_propagated = i;
  o.n_out_of_range = n_oor;
  o.Delta_t = Delta_t;
  if constexpr (kJac) {  // :756-765
    double X[9], nC[9];
    imu_cross_mx(Ca, X);
OKVFE_FP64_UNROLL
    for (int e = 0; e < 9; ++e) {
      o.F.b0_3[e] = -X[e];
      o.F.b0_6[e] = (e % 4 == 0 ? 1.0 : 0.0) * Delta_t;
      nC[e] = -C_WS_0[e];
    }
    imu_cross_mx(Cv, X);
OKVFE_FP64_UNROLL
    for (int e = 0; e < 9; ++e) o.F.b6_3[e] = -X[e];
    imu_matmul<kTree>(C_WS_0, dp_db_g, o.F.b0_9);
    imu_matmul<kTree>(nC, C_doubleintegral, o.F.b0_12);
    imu_matmul<kTree>(nC, dalpha_db_g, o.F.b3_9);
    imu_matmul<kTree>(C_WS_0, dv_db_g, o.F.b6_9);
    imu_matmul<kTree>(nC, C_integral, o.F.b6_12);
  }
}

// T_WC = T_WS * T_SC (Transformation.hpp:261-264, whose constructor normalises) and
// extractionDir = T_WC.inverse().C() * (0, 0, -1) (Frontend.cpp:246-251) as float
template <bool kTree>
OKVFE_FP64_HD void imu_camera(const double* T_WS, const double* T_SC, double* T_WC, float* gravity_C) {
  double C_WS[9], r[3], q[4], qi[4], qn[4], C_inv[9], d[3];
  imu_to_rotation(T_WS + 3, C_WS);
  imu_matvec<kTree>(C_WS, T_SC, r);
  fp64::quat_product(T_WS + 3, T_SC + 3, q);
  fp64::quat_normalized<kTree>(q, T_WC + 3);
OKVFE_FP64_UNROLL
  for (int k = 0; k < 3; ++k) T_WC[k] = r[k] + T_WS[k];
  imu_q_inverse<kTree>(T_WC + 3, qi);
  fp64::quat_normalized<kTree>(qi, qn);
  imu_to_rotation(qn, C_inv);
  const double down[3] = {0.0, 0.0, -1.0};
  imu_matvec<kTree>(C_inv, down, d);
OKVFE_FP64_UNROLL
  for (int k = 0; k < 3; ++k) gravity_C[k] = (float)d[k];
}

// F (15 x 15 row-major) from its blocks
OKVFE_FP64_HD void imu_write_jacobian(const ImuBlocks& B, double* F) {
  for (int e = 0; e < 225; ++e) F[e] = e % 16 == 0 ? 1.0 : 0.0;
  imu_put_blocks(B, F);
}

// The outputs of a call (okvfe_imu_result_device): one record per multiframe; jacobian, covariance, T_WC and gravity_C
// may be null.
struct ImuResultPtrs {
  double *pose, *speed_and_bias;
  int32_t *n_propagated, *status, *n_out_of_range;
  double *jacobian, *covariance, *T_WC;
  float* gravity_C;
};
// everything of multiframe m but P.  T_SC: n_cams x 7 doubles.
template <bool kTree, bool kJac>
OKVFE_FP64_HD void imu_store(const ImuResultPtrs& R, long long m, int n_cams, const double* T_SC, const ImuOut& o) {
  R.status[m] = o.status;
  R.n_out_of_range[m] = o.n_out_of_range;
  if (!o.wrote_state) return;
  R.n_propagated[m] = o.n_propagated;
  for (int e = 0; e < 7; ++e) R.pose[7 * m + e] = o.pose[e];
  for (int e = 0; e < 9; ++e) R.speed_and_bias[9 * m + e] = o.speed_and_bias[e];
  if constexpr (kJac) {
    if (R.jacobian && o.wrote_jacobian) imu_write_jacobian(o.F, R.jacobian + 225 * m);
  }
  if (!R.T_WC && !R.gravity_C) return;
  for (int c = 0; c < n_cams; ++c) {
    double T_WC[7];
    float g[3];
    imu_camera<kTree>(o.pose, T_SC + 7 * c, T_WC, g);
    const long long row = m * n_cams + c;
    if (R.T_WC)
      for (int e = 0; e < 7; ++e) R.T_WC[7 * row + e] = T_WC[e];
    if (R.gravity_C)
      for (int e = 0; e < 3; ++e) R.gravity_C[3 * row + e] = g[e];
  }
}

// The host loop: multiframe m of a batch in the layout of okvfe_imu_propagation_blocks_device, every pointer a host pointer.
// The form follows the outputs asked for, as the kernels' does.
template <bool kTree>
inline void imu_host_multiframe(const ImuParams& prm, const double* samples, const int32_t* sample_begin,
                                const double* states, long long m, int n_cams, const double* T_SC,
                                const ImuResultPtrs& R) {
  const double* s = samples + (long long)sample_begin[m] * kImuSampleDoubles;
  const int n = sample_begin[m + 1] - sample_begin[m];
  const double* st = states + m * kImuStateDoubles;
  ImuOut o;
  double C_WS_0[9];
  if (R.covariance) {
    ImuCovHost cov;
    imu_propagate<kTree, true, true>(prm, s, n, st, cov, o, C_WS_0);
    if (o.wrote_jacobian) cov.finish(C_WS_0, R.covariance + 225 * m);
    imu_store<kTree, true>(R, m, n_cams, T_SC, o);
  } else if (R.jacobian) {
    ImuCovNone cov;
    imu_propagate<kTree, true, false>(prm, s, n, st, cov, o, C_WS_0);
    imu_store<kTree, true>(R, m, n_cams, T_SC, o);
  } else {
    ImuCovNone cov;
    imu_propagate<kTree, false, false>(prm, s, n, st, cov, o, C_WS_0);
    imu_store<kTree, false>(R, m, n_cams, T_SC, o);
  }
}

}  // namespace okvfe
