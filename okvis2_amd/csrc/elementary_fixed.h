// elementary_fixed.h -- FP64 log, sin and cos as ONE fixed sequence of IEEE-754 operations each, compiling for the host
// and for gfx950: what the Cauchy loss and PoseManifold::plus of the refinement of Frontend::verifyRecognisedPlace
// (okvis_frontend/src/Frontend.cpp:399-527) need (place_refine_dev.h, k_place_refine.hip), and the IMU propagation (imu_dev.h).
//
// Why: a refinement on the device is to be held byte for byte to a numpy restatement (tests/place_refine_ref.py); the
// device math library's log, sin and cos differ from a host libm in the last bit for some arguments.  As in atan_fixed.h the
// same sequence of + - * / and integer bit operations runs on both sides (no FMA: the library is built with
// -ffp-contract=off; no table that could be reordered).  tests/elementary_ref.py restates the three in numpy,
// tests/test_elementary_fixed_host.py compares a host program built from this header with it byte for byte.
//
// The constants are the doubles nearest to 1 / k!, 1 / (2 k + 1), sqrt(2) and pi / 4, written with 21 digits; ln2_hi is
// the double nearest to ln 2 with the low 32 bits of its mantissa cleared (k ln2_hi is exact), ln2_lo the double nearest
// to ln 2 - ln2_hi.
//
//   sin_fixed(x), cos_fixed(x)   |x| <= pi / 4 (the double 0.78539816339744828): the Taylor polynomials through x^17 and
//                                x^18 in Horner form (truncation error below 1e-19); NaN outside that range and for NaN.
//   sinc_fixed(x)                okvis::kinematics::sinc (okvis_kinematics implementation/Transformation.hpp:50-62) with
//                                sin_fixed: sin(x) / x where fabs(x) > 1.0e-6, else the reference's polynomial as written.
//   log_fixed(x)                 x >= 1: x = 2^k m with m in [sqrt(1/2), sqrt(2)) by bit operations, f = (m - 1) / (m + 1),
//                                log m = 2 f + 2 f (f^2 / 3 + ... + f^20 / 21) (11 terms of the series: the next one is
//                                below 1e-17 relative), the result k ln2_hi + (k ln2_lo + log m).  NaN for NaN and for
//                                x < 1, +inf for +inf.
//
// Measured against glibc's sin, cos and log on a dense sample of the domains (tests/test_elementary_fixed_host.py, which
// holds these as bounds): sin_fixed and cos_fixed differ from libm by at most 1 ulp, log_fixed by at most 2 ulp (the
// quotient f and the two-term sum each round once).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define OKVFE_HD __host__ __device__ inline
#else
#define OKVFE_HD inline
#endif

namespace okvfe {

OKVFE_HD double elementary_nan() {
  const unsigned long long bits = 0x7FF8000000000000ull;
  double v;
  __builtin_memcpy(&v, &bits, 8);
  return v;
}

OKVFE_HD double sin_fixed(double x) {
  const double s3 = -1.66666666666666657415e-01, s5 = 8.33333333333333321769e-03, s7 = -1.98412698412698412526e-04,
               s9 = 2.75573192239858925110e-06, s11 = -2.50521083854417202239e-08, s13 = 1.60590438368216133409e-10,
               s15 = -7.64716373181981640551e-13, s17 = 2.81145725434552059811e-15;
  const double ax = x < 0.0 ? -x : x;
  if (!(ax <= 7.85398163397448278999e-01)) return elementary_nan();
  const double z = x * x;
  const double p = s3 + z * (s5 + z * (s7 + z * (s9 + z * (s11 + z * (s13 + z * (s15 + z * s17))))));
  return x + x * (z * p);
}

OKVFE_HD double cos_fixed(double x) {
  const double c4 = 4.16666666666666643537e-02, c6 = -1.38888888888888894189e-03, c8 = 2.48015873015873015658e-05,
               c10 = -2.75573192239858882758e-07, c12 = 2.08767569878681001866e-09, c14 = -1.14707455977297245073e-11,
               c16 = 4.77947733238738525345e-14, c18 = -1.56192069685862252711e-16;
  const double ax = x < 0.0 ? -x : x;
  if (!(ax <= 7.85398163397448278999e-01)) return elementary_nan();
  const double z = x * x;
  const double q = c4 + z * (c6 + z * (c8 + z * (c10 + z * (c12 + z * (c14 + z * (c16 + z * c18))))));
  return 1.0 - (0.5 * z - (z * z) * q);
}

// Transformation.hpp:50-62; a NaN or an |x| beyond pi / 4 gives NaN
OKVFE_HD double sinc_fixed(double x) {
  const double ax = x < 0.0 ? -x : x;
  if (ax > 1.0e-6) return sin_fixed(x) / x;
  const double c_2 = 1.66666666666666657415e-01, c_4 = 8.33333333333333321769e-03, c_6 = 1.98412698412698412526e-04;
  const double x_2 = x * x;
  const double x_4 = x_2 * x_2;
  const double x_6 = (x_2 * x_2) * x_2;
  return ((1.0 - c_2 * x_2) + c_4 * x_4) - c_6 * x_6;
}

OKVFE_HD double log_fixed(double x) {
  const double ln2_hi = 6.93146705627441406250e-01, ln2_lo = 4.74932503903167255529e-07;
  const double l3 = 3.33333333333333314830e-01, l5 = 2.00000000000000011102e-01, l7 = 1.42857142857142849213e-01,
               l9 = 1.11111111111111104943e-01, l11 = 9.09090909090909116141e-02, l13 = 7.69230769230769273470e-02,
               l15 = 6.66666666666666657415e-02, l17 = 5.88235294117647050660e-02, l19 = 5.26315789473684181310e-02,
               l21 = 4.76190476190476164042e-02;
  if (!(x >= 1.0)) return elementary_nan();
  unsigned long long bits;
  __builtin_memcpy(&bits, &x, 8);
  if (bits == 0x7FF0000000000000ull) return x;
  int k = (int)(bits >> 52) - 1023;
  bits = (bits & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull;  // m in [1, 2)
  double m;
  __builtin_memcpy(&m, &bits, 8);
  if (m >= 1.41421356237309514547e+00) {
    m = m * 0.5;
    k = k + 1;
  }
  const double f = (m - 1.0) / (m + 1.0);
  const double z = f * f;
  const double p = l3 + z * (l5 + z * (l7 + z * (l9 + z * (l11 + z * (l13 + z * (l15 + z * (l17 + z * (l19 + z * l21))))))));
  const double f2 = 2.0 * f;
  const double series = f2 + f2 * (z * p);
  const double dk = (double)k;
  return dk * ln2_hi + (dk * ln2_lo + series);
}

}  // namespace okvfe
