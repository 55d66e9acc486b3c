// fp64_ops.h -- the FP64 operations whose order is the parity contract, each ONCE, compiling for the host (g++ or hipcc)
// and for gfx950: the 3- and 4-term sums in the two orders of okvfe_set_fp64_reduction, Eigen's quaternion product and
// normalized(), the bit-test finite and sqrt.  HIP-free: the stand-alone host programs under tests/cpp/ compile it
// through imu_dev.h, place_refine_dev.h and ransac_hyp_dev.h, and tests/cpp/fp64_ops_main.cpp on its own.
//
//   Eigen's order   x0 + (x1 + x2) and (x0 + x1) + (x2 + x3): the unrolled non-vectorised redux (redux_novec_unroller
//                   splits at Length / 2); the default
//   left to right   (x0 + x1) + x2 and ((x0 + x1) + x2) + x3
//
// The batched kernels take the order as the template argument kTree (the host launches the instantiation for the order
// in force, okvfe_internal.h: fp64_left_to_right()); k_match.hip and k_map.hip read a device symbol and pass it to
// sum3_select.  The library is built with -ffp-contract=off: every operation below is a separate IEEE operation.
#pragma once

#if defined(__HIPCC__)
#define OKVFE_FP64_HD __host__ __device__ inline __attribute__((always_inline))
#define OKVFE_FP64_UNROLL _Pragma("unroll")
#define OKVFE_FP64_NOUNROLL _Pragma("unroll 1")
#else
#define OKVFE_FP64_HD inline
#define OKVFE_FP64_UNROLL
#define OKVFE_FP64_NOUNROLL
#endif

namespace okvfe {
namespace fp64 {

// no NaN and no infinity, by the exponent bits (no libm, no fast-math assumption)
OKVFE_FP64_HD bool finite(double v) {
  unsigned long long bits;
  __builtin_memcpy(&bits, &v, 8);
  return (bits & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}
OKVFE_FP64_HD double sqrt(double v) { return __builtin_sqrt(v); }

template <bool kTree>
OKVFE_FP64_HD double sum3(double p0, double p1, double p2) {
  if constexpr (kTree) return p0 + (p1 + p2);
  return (p0 + p1) + p2;
}
template <bool kTree>
OKVFE_FP64_HD double sum4(double p0, double p1, double p2, double p3) {
  if constexpr (kTree) return (p0 + p1) + (p2 + p3);
  return ((p0 + p1) + p2) + p3;
}
// sum3 with the order as a value (on the device: a symbol's scalar load): uniform branch-free select
OKVFE_FP64_HD double sum3_select(bool tree, double p0, double p1, double p2) {
  const double u = tree ? p1 : p0, v = tree ? p2 : p1, w = tree ? p0 : p2;
  const double s = u + v;
  return tree ? w + s : s + w;  // (addition commutes bit-exactly: one add either way)
}

// Eigen's a * b of (x, y, z, w) quaternions, each sum left to right
OKVFE_FP64_HD void quat_product(const double a[4], const double b[4], double o[4]) {
  const double ax = a[0], ay = a[1], az = a[2], aw = a[3];
  const double bx = b[0], by = b[1], bz = b[2], bw = b[3];
  o[0] = ((aw * bx + ax * bw) + ay * bz) - az * by;
  o[1] = ((aw * by + ay * bw) + az * bx) - ax * bz;
  o[2] = ((aw * bz + az * bw) + ax * by) - ay * bx;
  o[3] = ((aw * bw - ax * bx) - ay * by) - az * bz;
}
// Eigen's normalized(): divided by sqrt(squaredNorm()) iff that is > 0, so a zero or NaN quaternion stays as it is
template <bool kTree>
OKVFE_FP64_HD void quat_normalized(const double q[4], double o[4]) {
  const double n2 = sum4<kTree>(q[0] * q[0], q[1] * q[1], q[2] * q[2], q[3] * q[3]);
  if (n2 > 0) {
    const double n = sqrt(n2);
    o[0] = q[0] / n; o[1] = q[1] / n; o[2] = q[2] / n; o[3] = q[3] / n;
  } else {
    o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3];
  }
}

}  // namespace fp64
}  // namespace okvfe
