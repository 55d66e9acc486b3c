// ransac2d2d_hyp_dev.h -- the hypotheses of the relative RANSAC (Frontend::runRansac2d2d, Frontend.cpp:2281-2394) as ONE
// sequence of IEEE-754 operations that compiles for the host and for gfx950: tests/ransac2d2d_hyp_ref.py transcribed
// line by line.  okvfe_twopt_rotation_hypothesis, okvfe_fivept_hypothesis, the stand-alone program
// tests/cpp/ransac2d2d_hyp_main.cpp and the kernel of k_ransac2d2d_hyp.hip are all this header; the tests hold them to
// the restatement byte for byte.  Only + - * /, sqrt and comparisons; no libm.  The library is built with
// -ffp-contract=off: every operation below is a separate IEEE operation.
//
// A DEFINED ALGORITHM, PARITY UNPINNED: opengv (not in the reference tree) samples with rand() and solves with
// twopt_rotationOnly and Stewenius' five-point; what is here is stated in include/okvfe.h and follows no other
// implementation bit for bit.
//
//   hyp2_sample       N distinct list positions of hypothesis h with the splitmix64 draw of ransac_hyp_dev.h, under the
//                     key (pair key 128 + camera 2 + problem), problem 0 = rotation only (draws 0, 1), 1 = relative
//                     pose (draws 0 .. 7): t = r(j, n - j), then over the chosen positions in ascending order t += 1
//                     where x <= t.  No rejection loop.
//   twopt_rotation    M = T1 T2^T of the triads e1 = f_0, e3 = f_0 x f_1 normalised, e2 = e3 x e1 (b1 ~ M b2).
//   fivept_hypothesis Nister's five-point over samples 0 .. 4, samples 5 .. 7 choose among the candidates:
//     null space   Q (5 x 9), row i = b1_i (x) b2_i; Gauss-Jordan with full pivoting (largest |a| over the rows not yet
//                  used and the columns not yet used, the first in row-major order on ties; a zero or non-finite pivot:
//                  invalid; every other row minus (its entry / pivot) times the pivot row, then the pivot row over the
//                  pivot); the free columns f_0 < .. < f_3 give X, Y, Z, W: 1 at f_k, -a[s][f_k] at the pivot column
//                  of row s, 0 elsewhere.  E = x X + y Y + z Z + W.
//     constraints  det E, then the nine entries of (E E^T - 1/2 tr(E E^T) I) E row-major, as polynomials over the
//                  columns x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1.  An entry of E
//                  is a 4-vector over (x, y, z, 1), a product of two a 10-vector over (x^2 xy xz x y^2 yz y z^2 z 1);
//                  a product starts from zeros and adds a_i b_j in the order i outer, j inner.
//     elimination  Gauss-Jordan on the first ten columns with partial pivoting (largest |a| of the column over the rows
//                  not yet used, the first on ties; a zero or non-finite pivot: invalid).
//     polynomial   rows (x^2z) - z (x^2), (y^2z) - z (y^2), (xyz) - z (xy) give B(z), 3 x 3 with columns of degree
//                  3, 3, 4; det B along the first row has degree 10.
//     real roots   a_10 zero or non-finite: invalid.  bound = 1 + max |a_i / a_10|.  The roots of the d-th derivative
//                  (d = 9 .. 0) are bracketed by those of the (d+1)-th and +-bound; an interval whose ends have values of
//                  strictly opposite sign is bisected until the midpoint equals an end, at most kHypMaxBisections steps
//                  (the half that keeps the sign change; a midpoint whose value has the sign class of the upper end
//                  becomes the upper end); the root is the upper end.  Ascending, at most 10.  A root of even
//                  multiplicity has no sign change and is NOT found; an end whose value is exactly 0 has none either.
//                  No Newton polish, no cut of the steps.
//     per root     (x, y, 1) ~ the cross product of the pair of B(z) rows with the largest |third component| (pairs
//                  (0,1), (0,2), (1,2), the first on ties); E follows.
//     decomposition  Horn: T = 1/2 tr(E E^T) I - E E^T = b b^T; b = the row of T with the largest diagonal entry (the
//                  first on ties; not > 0: the root gives nothing) over the square root of that entry;
//                  R-/+ = (cof(E) -/+ [b]x E) / (b.b); candidates (R-, +b^), (R-, -b^), (R+, +b^), (R+, -b^), b^ = b / |b|.
//     choice       the sum (the caller's functor: the consensus call's relative_pose_distance over samples 5, 6, 7,
//                  left to right) of every candidate of every root, roots ascending, candidates in the order above;
//                  the smallest wins, the first on ties, a NaN or an infinite sum never.
// The work arrays (kFiveptWork doubles) are the caller's: LDS on the device, the stack on the host.  Every loop has a
// compile-time trip count or cap.
#pragma once
#include <stdint.h>

#include "fp64_ops.h"
#include "ransac_hyp_dev.h"

namespace okvfe {
namespace {

// ---- the sampler ----------------------------------------------------------------------------------------------------
constexpr int kHyp2RotSamples = 2, kHyp2RelSamples = 8, kHyp2MinCorrespondences = 10;  // Frontend.cpp:2300
OKVFE_FP64_HD uint64_t hyp2_key(uint64_t pair_key, int cam, int problem) {
  return pair_key * 128ull + (uint64_t)cam * 2ull + (uint64_t)problem;
}
// N distinct positions of [0, n), n >= N
template <int N>
OKVFE_FP64_HD void hyp2_sample(uint64_t seed, uint64_t key, int h, int n, int pos[N]) {
  int s[N];  // the chosen positions, ascending (static indices only: the loops are unrolled)
  OKVFE_FP64_UNROLL
  for (int j = 0; j < N; ++j) {
    int t = hyp_draw(seed, key, h, j, n - j);
    OKVFE_FP64_UNROLL
    for (int i = 0; i < j; ++i)
      if (s[i] <= t) t += 1;
    pos[j] = t;
    int v = t;
    OKVFE_FP64_UNROLL
    for (int i = 0; i < j; ++i)
      if (v < s[i]) {
        const int w = s[i];
        s[i] = v;
        v = w;
      }
    s[j] = v;
  }
}

// ---- rotation only --------------------------------------------------------------------------------------------------
OKVFE_FP64_HD double hyp2_abs(double v) { return v < 0.0 ? -v : v; }

// e1 = f0, e3 = f0 x f1 normalised, e2 = e3 x e1; false: the cross product has squared norm 0
OKVFE_FP64_HD bool twopt_triad(const double* f0, const double* f1, double* E) {
  E[0] = f0[0]; E[1] = f0[1]; E[2] = f0[2];
  hyp_cross(f0, f1, E + 6);
  const double n2 = hyp_dot(E + 6, E + 6);
  if (n2 == 0.0) return false;
  const double n = fp64::sqrt(n2);
  E[6] = E[6] / n; E[7] = E[7] / n; E[8] = E[8] / n;
  hyp_cross(E + 6, E, E + 3);
  return true;
}
// b1, b2: 2 x 3 -> M (9 doubles, zeros when invalid)
OKVFE_FP64_HD bool twopt_rotation(const double* b1, const double* b2, double* M) {
  double T1[9], T2[9];
  for (int i = 0; i < 9; ++i) M[i] = 0.0;
  if (!twopt_triad(b1, b1 + 3, T1)) return false;
  if (!twopt_triad(b2, b2 + 3, T2)) return false;
  double R[9];
  bool ok = true;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      R[3 * i + j] = (T1[i] * T2[j] + T1[3 + i] * T2[3 + j]) + T1[6 + i] * T2[6 + j];
      ok = ok && fp64::finite(R[3 * i + j]);
    }
  if (!ok) return false;
  for (int i = 0; i < 9; ++i) M[i] = R[i];
  return true;
}

// ---- relative pose --------------------------------------------------------------------------------------------------
// the work arrays of one solve, in doubles
constexpr int kF5A = 0;      // 10 x 20 (the 5 x 9 null-space system first, the derivative chain and its roots last)
constexpr int kF5Lin = 200;  // 9 entries of E x (X, Y, Z, W)
constexpr int kF5D = 236;    // E E^T, 6 x 10 (B(z) and the polynomial in z last)
constexpr int kF5T1 = 296, kF5T2 = 306, kF5C = 316;  // two quadratics and a cubic
constexpr int kFiveptWork = 336;
// inside kF5A, after the elimination: the derivative d at kF5Der(d), 11 - d coefficients; two lists of ten roots
OKVFE_FP64_HD int f5_der(int d) { return 11 * d - (d * (d - 1)) / 2; }
constexpr int kF5Roots = 65;
// inside kF5D: B(z) row r at kF5D + 13 r: px[4], py[4], pc[5], constant term first; the polynomial at kF5D + 39
constexpr int kF5Poly = kF5D + 39;

// the monomial of a product: (x, y, z, 1)_i (x, y, z, 1)_j among (x^2 xy xz x y^2 yz y z^2 z 1), and that times
// (x, y, z, 1)_l among the 20 columns; four and five bits per entry
OKVFE_FP64_HD int f5_qidx(int i, int j) { return (int)((0x9863875265413210ull >> (4 * (4 * i + j))) & 15ull); }
OKVFE_FP64_HD int f5_cidx(int q, int l) {
  const int e = 4 * q + l;
  const unsigned long long w = e < 12 ? 0x5a9044a06229040ull : e < 24 ? 0x734c83982362d25ull
                               : e < 36 ? 0x945cb8c1aa7b8e9ull : 0x9c9ecull;
  return (int)((w >> (5 * (e % 12))) & 31ull);
}
OKVFE_FP64_HD void f5_mul_ll(const double* p, const double* q, double* out) {
  for (int k = 0; k < 10; ++k) out[k] = 0.0;
  OKVFE_FP64_UNROLL
  for (int i = 0; i < 4; ++i) {
    OKVFE_FP64_UNROLL
    for (int j = 0; j < 4; ++j) {
      const int k = f5_qidx(i, j);
      out[k] = out[k] + p[i] * q[j];
    }
  }
}
OKVFE_FP64_HD void f5_mul_ql(const double* q, const double* l, double* out) {
  for (int k = 0; k < 20; ++k) out[k] = 0.0;
  OKVFE_FP64_UNROLL
  for (int i = 0; i < 10; ++i) {
    OKVFE_FP64_UNROLL
    for (int j = 0; j < 4; ++j) {
      const int k = f5_cidx(i, j);
      out[k] = out[k] + q[i] * l[j];
    }
  }
}
// out = a(z) b(z), na and nb coefficients, constant term first
OKVFE_FP64_HD void f5_pmul(const double* a, int na, const double* b, int nb, double* out) {
  for (int k = 0; k < na + nb - 1; ++k) out[k] = 0.0;
  for (int i = 0; i < na; ++i)
    for (int j = 0; j < nb; ++j) out[i + j] = out[i + j] + a[i] * b[j];
}
// q[m] z^m + .. + q[0], m <= 10
OKVFE_FP64_HD double f5_horner(const double* q, int m, double z) {
  double v = q[m];
  for (int i = 0; i < 10; ++i)
    if (i < m) v = v * z + q[m - 1 - i];
  return v;
}
OKVFE_FP64_HD int f5_sym(int i, int k) {  // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
  const int a = i < k ? i : k, b = i < k ? k : i;
  return a == 0 ? b : a == 1 ? 2 + b : 5;
}

// the null space of the five epipolar constraints into ws[kF5Lin ..]; false: a failed pivot
OKVFE_FP64_HD bool f5_null_space(const double* b1, const double* b2, double* ws) {
  double* Q = ws + kF5A;
  for (int i = 0; i < 5; ++i)
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) Q[9 * i + 3 * a + b] = b1[3 * i + a] * b2[3 * i + b];
  int used = 0;    // bit c: column c is a pivot column
  int pivcol = 0;  // four bits per row
  for (int s = 0; s < 5; ++s) {
    double best = -1.0;
    int br = -1, bc = -1;
    for (int r = s; r < 5; ++r)
      for (int c = 0; c < 9; ++c) {
        if ((used >> c) & 1) continue;
        const double a = hyp2_abs(Q[9 * r + c]);
        if (a > best) {
          best = a;
          br = r;
          bc = c;
        }
      }
    if (br < 0) return false;
    const double piv = Q[9 * br + bc];
    if (piv == 0.0 || !fp64::finite(piv)) return false;
    for (int j = 0; j < 9; ++j) {
      const double u = Q[9 * br + j], v = Q[9 * s + j];
      Q[9 * br + j] = v;
      Q[9 * s + j] = u;
    }
    for (int r = 0; r < 5; ++r) {  // (a row equal to the pivot row has the factor 1 and becomes exactly zero)
      if (r == s) continue;
      const double f = Q[9 * r + bc] / piv;
      for (int j = 0; j < 9; ++j) Q[9 * r + j] = Q[9 * r + j] - f * Q[9 * s + j];
    }
    for (int j = 0; j < 9; ++j) Q[9 * s + j] = Q[9 * s + j] / piv;
    used |= 1 << bc;
    pivcol |= bc << (4 * s);
  }
  double* lin = ws + kF5Lin;
  for (int i = 0; i < 36; ++i) lin[i] = 0.0;
  int k = 0;
  for (int c = 0; c < 9; ++c) {
    if ((used >> c) & 1) continue;
    lin[4 * c + k] = 1.0;
    for (int s = 0; s < 5; ++s) lin[4 * ((pivcol >> (4 * s)) & 15) + k] = -Q[9 * s + c];
    k += 1;
  }
  return true;
}

// the ten cubic constraints into ws[kF5A ..]
OKVFE_FP64_HD void f5_constraints(double* ws) {
  double* A = ws + kF5A;
  const double* lin = ws + kF5Lin;
  double *D = ws + kF5D, *T1 = ws + kF5T1, *T2 = ws + kF5T2, *C = ws + kF5C;
  // det E = e0 (e4 e8 - e5 e7) - e1 (e3 e8 - e5 e6) + e2 (e3 e7 - e4 e6)
  OKVFE_FP64_NOUNROLL
  for (int t = 0; t < 3; ++t) {
    const int a = t == 0 ? 4 : 3, b = t == 2 ? 7 : 8, c = t == 0 ? 5 : t == 1 ? 5 : 4, d = t == 0 ? 7 : 6;
    f5_mul_ll(lin + 4 * a, lin + 4 * b, T1);
    f5_mul_ll(lin + 4 * c, lin + 4 * d, T2);
    for (int k = 0; k < 10; ++k) T1[k] = T1[k] - T2[k];
    if (t == 0) {
      f5_mul_ql(T1, lin + 0, A);
    } else {
      f5_mul_ql(T1, lin + 4 * t, C);
      for (int k = 0; k < 20; ++k) A[k] = t == 1 ? A[k] - C[k] : A[k] + C[k];
    }
  }
  // E E^T, its trace, Lambda = E E^T - 1/2 tr I
  OKVFE_FP64_NOUNROLL
  for (int i = 0; i < 3; ++i) {
    OKVFE_FP64_NOUNROLL
    for (int j = i; j < 3; ++j) {
      double* d = D + 10 * f5_sym(i, j);
      f5_mul_ll(lin + 4 * (3 * i), lin + 4 * (3 * j), d);
      f5_mul_ll(lin + 4 * (3 * i + 1), lin + 4 * (3 * j + 1), T1);
      for (int k = 0; k < 10; ++k) d[k] = d[k] + T1[k];
      f5_mul_ll(lin + 4 * (3 * i + 2), lin + 4 * (3 * j + 2), T1);
      for (int k = 0; k < 10; ++k) d[k] = d[k] + T1[k];
    }
  }
  for (int k = 0; k < 10; ++k) T2[k] = 0.5 * ((D[k] + D[30 + k]) + D[50 + k]);
  for (int k = 0; k < 10; ++k) {
    D[k] = D[k] - T2[k];
    D[30 + k] = D[30 + k] - T2[k];
    D[50 + k] = D[50 + k] - T2[k];
  }
  OKVFE_FP64_NOUNROLL
  for (int i = 0; i < 3; ++i) {
    OKVFE_FP64_NOUNROLL
    for (int j = 0; j < 3; ++j) {
      double* row = A + 20 * (1 + 3 * i + j);
      f5_mul_ql(D + 10 * f5_sym(i, 0), lin + 4 * j, row);
      f5_mul_ql(D + 10 * f5_sym(i, 1), lin + 4 * (3 + j), C);
      for (int k = 0; k < 20; ++k) row[k] = row[k] + C[k];
      f5_mul_ql(D + 10 * f5_sym(i, 2), lin + 4 * (6 + j), C);
      for (int k = 0; k < 20; ++k) row[k] = row[k] + C[k];
    }
  }
}

// Gauss-Jordan on the first ten columns; false: a failed pivot
OKVFE_FP64_HD bool f5_eliminate(double* ws) {
  double* A = ws + kF5A;
  for (int c = 0; c < 10; ++c) {
    double best = -1.0;
    int br = -1;
    for (int r = c; r < 10; ++r) {
      const double a = hyp2_abs(A[20 * r + c]);
      if (a > best) {
        best = a;
        br = r;
      }
    }
    if (br < 0) return false;
    const double piv = A[20 * br + c];
    if (piv == 0.0 || !fp64::finite(piv)) return false;
    for (int j = 0; j < 20; ++j) {
      const double u = A[20 * br + j], v = A[20 * c + j];
      A[20 * br + j] = v;
      A[20 * c + j] = u;
    }
    for (int r = 0; r < 10; ++r) {
      if (r == c) continue;
      const double f = A[20 * r + c] / piv;
      for (int j = 0; j < 20; ++j) A[20 * r + j] = A[20 * r + j] - f * A[20 * c + j];
    }
    for (int j = 0; j < 20; ++j) A[20 * c + j] = A[20 * c + j] / piv;
  }
  return true;
}

// B(z) into ws[kF5D ..] and det B into ws[kF5Poly ..] (11 coefficients, constant term first)
OKVFE_FP64_HD void f5_polynomial(double* ws) {
  const double* A = ws + kF5A;
  double* B = ws + kF5D;
  for (int r = 0; r < 3; ++r) {
    const double* a = A + 20 * (4 + 2 * r) + 10;  // x^2z, y^2z, xyz
    const double* b = A + 20 * (5 + 2 * r) + 10;  // x^2, y^2, xy
    double* o = B + 13 * r;
    o[0] = a[2]; o[1] = a[1] - b[2]; o[2] = a[0] - b[1]; o[3] = -b[0];
    o[4] = a[5]; o[5] = a[4] - b[5]; o[6] = a[3] - b[4]; o[7] = -b[3];
    o[8] = a[9]; o[9] = a[8] - b[9]; o[10] = a[7] - b[8]; o[11] = a[6] - b[7]; o[12] = -b[6];
  }
  double *P = ws + kF5Poly, *T1 = ws + kF5T1, *T2 = ws + kF5T2, *C = ws + kF5C;  // (T1, T2 are adjacent: 8 <= 10 each)
  const double *r0 = B, *r1 = B + 13, *r2 = B + 26;
  // det = B00 (B11 B22 - B12 B21) - B01 (B10 B22 - B12 B20) + B02 (B10 B21 - B11 B20)
  f5_pmul(r1 + 4, 4, r2 + 8, 5, T1);
  f5_pmul(r1 + 8, 5, r2 + 4, 4, T2);
  for (int k = 0; k < 8; ++k) T1[k] = T1[k] - T2[k];
  f5_pmul(r0, 4, T1, 8, P);
  f5_pmul(r1, 4, r2 + 8, 5, T1);
  f5_pmul(r1 + 8, 5, r2, 4, T2);
  for (int k = 0; k < 8; ++k) T1[k] = T1[k] - T2[k];
  f5_pmul(r0 + 4, 4, T1, 8, C);
  for (int k = 0; k < 11; ++k) P[k] = P[k] - C[k];
  f5_pmul(r1, 4, r2 + 4, 4, T1);
  f5_pmul(r1 + 4, 4, r2, 4, T2);
  for (int k = 0; k < 7; ++k) T1[k] = T1[k] - T2[k];
  f5_pmul(r0 + 8, 5, T1, 7, C);
  for (int k = 0; k < 11; ++k) P[k] = P[k] + C[k];
}

// the real roots of ws[kF5Poly ..] by the derivative chain (inside kF5A, which is dead by now); -> their number, the
// roots ascending at ws[kF5A + kF5Roots ..]; -1: the leading coefficient is zero or not finite
OKVFE_FP64_HD int f5_real_roots(double* ws) {
  const double* P = ws + kF5Poly;
  double* der = ws + kF5A;
  const double lead = P[10];
  if (lead == 0.0 || !fp64::finite(lead)) return -1;
  double mx = 0.0;
  for (int i = 0; i < 10; ++i) {
    const double a = hyp2_abs(P[i] / lead);
    if (a > mx) mx = a;
  }
  const double bound = 1.0 + mx;
  for (int i = 0; i < 11; ++i) der[i] = P[i];
  for (int d = 1; d < 10; ++d) {
    const double* from = der + f5_der(d - 1);
    double* to = der + f5_der(d);
    for (int i = 0; i < 11 - d; ++i) to[i] = from[i + 1] * (double)(i + 1);
  }
  int np = 0;
  for (int d = 9; d >= 0; --d) {
    const double* q = der + f5_der(d);
    const int m = 10 - d;
    const double* prev = der + kF5Roots + 10 * ((d + 1) & 1);
    double* cur = der + kF5Roots + 10 * (d & 1);
    int nc = 0;
    for (int k = 0; k < 11; ++k) {
      if (k > np) break;
      double lo = k == 0 ? -bound : prev[k - 1];
      double hi = k == np ? bound : prev[k];
      const double flo = f5_horner(q, m, lo), fhi = f5_horner(q, m, hi);
      if (!((flo < 0.0 && fhi > 0.0) || (flo > 0.0 && fhi < 0.0))) continue;
      const bool up = fhi > 0.0;
      for (int it = 0; it < kHypMaxBisections; ++it) {
        const double mid = (lo + hi) / 2.0;
        if (mid == lo || mid == hi) break;
        const double fm = f5_horner(q, m, mid);
        if ((fm > 0.0) == up) hi = mid; else lo = mid;
      }
      cur[nc] = hi;
      nc += 1;
    }
    np = nc;
  }
  return np;  // (d == 0 wrote the even list: kF5Roots)
}

struct FiveptState {
  double H[12], best;
  int found;
};

// one real root: E, its decomposition, the four candidates against samples 5 .. 7
template <class Dist>
OKVFE_FP64_HD void f5_consider(const double* ws, double z, const double* b1, const double* b2, const double* s1,
                             const double* s2, FiveptState& S, const Dist& dist) {
  const double* B = ws + kF5D;
  const double* lin = ws + kF5Lin;
  double v[3][3];
  OKVFE_FP64_UNROLL
  for (int r = 0; r < 3; ++r) {
    v[r][0] = f5_horner(B + 13 * r, 3, z);
    v[r][1] = f5_horner(B + 13 * r + 4, 3, z);
    v[r][2] = f5_horner(B + 13 * r + 8, 4, z);
  }
  double c[3] = {0.0, 0.0, 0.0}, c01[3], c02[3], c12[3];
  hyp_cross(v[0], v[1], c01);
  hyp_cross(v[0], v[2], c02);
  hyp_cross(v[1], v[2], c12);
  double best = -1.0;
  c[0] = c01[0]; c[1] = c01[1]; c[2] = c01[2];
  if (hyp2_abs(c01[2]) > best) best = hyp2_abs(c01[2]);
  if (hyp2_abs(c02[2]) > best) {
    best = hyp2_abs(c02[2]);
    c[0] = c02[0]; c[1] = c02[1]; c[2] = c02[2];
  }
  if (hyp2_abs(c12[2]) > best) {
    best = hyp2_abs(c12[2]);
    c[0] = c12[0]; c[1] = c12[1]; c[2] = c12[2];
  }
  const double x = c[0] / c[2], y = c[1] / c[2];
  double E[9];
  OKVFE_FP64_UNROLL
  for (int e = 0; e < 9; ++e) E[e] = ((x * lin[4 * e] + y * lin[4 * e + 1]) + z * lin[4 * e + 2]) + lin[4 * e + 3];
  // T = 1/2 tr(E E^T) I - E E^T
  double G[9];
  OKVFE_FP64_UNROLL
  for (int i = 0; i < 3; ++i) {
    OKVFE_FP64_UNROLL
    for (int j = 0; j < 3; ++j) G[3 * i + j] = hyp_dot(E + 3 * i, E + 3 * j);
  }
  const double half = 0.5 * ((G[0] + G[4]) + G[8]);
  const double t0 = half - G[0], t1 = half - G[4], t2 = half - G[8];
  double b[3], tk = t0;
  b[0] = t0; b[1] = -G[1]; b[2] = -G[2];
  if (t1 > tk) {
    tk = t1;
    b[0] = -G[3]; b[1] = t1; b[2] = -G[5];
  }
  if (t2 > tk) {
    tk = t2;
    b[0] = -G[6]; b[1] = -G[7]; b[2] = t2;
  }
  if (!(tk > 0.0)) return;
  const double sk = fp64::sqrt(tk);
  b[0] = b[0] / sk; b[1] = b[1] / sk; b[2] = b[2] / sk;
  const double bb = hyp_dot(b, b), nb = fp64::sqrt(bb);
  const double bh[3] = {b[0] / nb, b[1] / nb, b[2] / nb};
  double cof[9], bxe[9];
  hyp_cross(E + 3, E + 6, cof);
  hyp_cross(E + 6, E, cof + 3);
  hyp_cross(E, E + 3, cof + 6);
  OKVFE_FP64_UNROLL
  for (int j = 0; j < 3; ++j) {
    bxe[j] = b[1] * E[6 + j] - b[2] * E[3 + j];
    bxe[3 + j] = b[2] * E[j] - b[0] * E[6 + j];
    bxe[6 + j] = b[0] * E[3 + j] - b[1] * E[j];
  }
  OKVFE_FP64_NOUNROLL
  for (int cand = 0; cand < 4; ++cand) {
    double H[12];
    const bool minus = cand < 2, pos = (cand & 1) == 0;
    OKVFE_FP64_UNROLL
    for (int i = 0; i < 3; ++i) {
      OKVFE_FP64_UNROLL
      for (int j = 0; j < 3; ++j)
        H[4 * i + j] = (minus ? cof[3 * i + j] - bxe[3 * i + j] : cof[3 * i + j] + bxe[3 * i + j]) / bb;
      H[4 * i + 3] = pos ? bh[i] : -bh[i];
    }
    const double d = dist(H, b1 + 15, b2 + 15, s1, s2);
    if (d < S.best) {
      S.best = d;
      S.found = 1;
      for (int i = 0; i < 12; ++i) S.H[i] = H[i];
    }
  }
}

// b1 / b2: 8 x 3 unit bearings of the older / current frame (rows 0 .. 4 are solved, rows 5 .. 7 choose); s1 / s2: the
// sigmas of rows 5 .. 7; ws: kFiveptWork doubles.  dist(H, b1_5.., b2_5.., s1, s2): the sum over the three rows of the
// consensus' distance under [R | t] = H.  -> H (12 doubles, zeros when invalid), *n_roots; returns the validity.
template <class Dist>
OKVFE_FP64_HD bool fivept_hypothesis(const double* b1, const double* b2, const double* s1, const double* s2, double* ws,
                                   double* H, int* n_roots, const Dist& dist) {
  for (int i = 0; i < 12; ++i) H[i] = 0.0;
  *n_roots = 0;
  if (!f5_null_space(b1, b2, ws)) return false;
  f5_constraints(ws);
  if (!f5_eliminate(ws)) return false;
  f5_polynomial(ws);
  const int n = f5_real_roots(ws);
  const double* roots = ws + kF5A + kF5Roots;
  if (n <= 0) return false;
  *n_roots = n;
  FiveptState S;
  for (int i = 0; i < 12; ++i) S.H[i] = 0.0;
  S.best = __builtin_inf();
  S.found = 0;
  OKVFE_FP64_NOUNROLL
  for (int k = 0; k < 10; ++k) {
    if (k >= n) break;
    f5_consider(ws, roots[k], b1, b2, s1, s2, S, dist);
  }
  bool valid = S.found != 0;
  for (int i = 0; i < 12; ++i) valid = valid && fp64::finite(S.H[i]);
  if (valid)
    for (int i = 0; i < 12; ++i) H[i] = S.H[i];
  return valid;
}

}  // namespace
}  // namespace okvfe
