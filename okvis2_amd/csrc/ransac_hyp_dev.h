// ransac_hyp_dev.h -- the pose hypotheses of the absolute-pose RANSAC (Frontend::runRansac3d2d, Frontend.cpp:2208-2261,
// and Frontend::verifyRecognisedPlace, :372-397) as ONE sequence of IEEE-754 operations that compiles for the host and
// for gfx950: tests/ransac_hyp_ref.py transcribed line by line.  okvfe_p3p_hypothesis, the stand-alone program
// tests/cpp/ransac_hyp_main.cpp and the kernel of k_ransac_hyp.hip are all this header; the tests hold them to the
// restatement byte for byte.  Only + - * /, sqrt and comparisons; no libm, nothing of elementary_fixed.h.  The library
// is built with -ffp-contract=off: every operation below is a separate IEEE operation.
//
// A DEFINED ALGORITHM, PARITY UNPINNED: opengv (not in the reference tree) samples with rand() and solves gp3p; what
// is here is stated in include/okvfe.h and follows no other implementation.
//
//   hyp_sample     counter-based sampler.  z = seed + (key 512 + h 8 + j + 1) 0x9E3779B97F4A7C15 through the splitmix64
//                  finaliser; r(j, range) = ((z >> 32) range) >> 32.  i0 = r(0, n) over the camera-major list; its
//                  camera owns [b, e), n_c = e - b; fewer than four: one sample drawn, invalid.  Draws 1..3:
//                  t = r(j, n_c - j), then for every already chosen position x of the camera in ascending order
//                  t += (x <= t): the draws are distinct without a rejection loop.
//   p3p_hypothesis samples 0..2 through Grunert's P3P (the quartic in v = s3 / s1), sample 3 chooses among the
//                  solutions with the consensus' distance (the caller's functor: it follows okvfe_set_fp64_reduction;
//                  every sum of the solver itself runs left to right).
// Real roots of the quartic A4 v^4 + .. + A0: A4 == 0 or a non-finite coefficient: none.  B..E = A3..A0 / A4, the
// depressed quartic y^4 + p y^2 + q y + r with v = y - B / 4.  q == 0: w = (-p +- sqrt(p p - 4 r)) / 2, y = +-sqrt(w)
// for w >= 0, in the order +sqrt(w+), -sqrt(w+), +sqrt(w-), -sqrt(w-).  Otherwise Ferrari: the positive root m of
// g(m) = ((8 m + 8 p) m + (2 p p - 8 r)) m - q q by bisection on [0, hi], hi doubled from 1 until g(hi) > 0, at most
// kHypMaxDoublings times (then: no root), bisected until the midpoint equals an end, at most kHypMaxBisections steps,
// m = the upper end; s = sqrt(2 m), t0 = p / 2 + m, u0 = q / (2 s); y = (s +- sqrt(s s - 4 (t0 + u0))) / 2 and
// y = (-s +- sqrt(s s - 4 (t0 - u0))) / 2, each pair only if its discriminant is >= 0, in this order, + before -.
// Equal roots are listed as often as they occur.  Every root takes three Newton steps on the original quartic (a step
// whose derivative is exactly zero leaves v as it is).  ROOT ORDER IS SOLUTION ORDER.
// A root counts (n_solutions) iff v > 0 && u > 0 && s1^2 > 0 (a NaN fails):
// u = ((k - 1) v v - 2 k cb v + 1 + k) / (2 (cg - v ca)), s1^2 = b^2 / (1 + v v - 2 v cb).
// Pose of a solution: Q_i = s_i f_i; R_CW from the orthonormal triads e1 = (X2 - X1) / |..|, e3 = e1 x (X3 - X1)
// normalised, e2 = e3 x e1 of Q and of P (no SVD); t_CW = Q1 - R_CW P1; inverted; T_WS = T_WC T_SC^-1.
// Choice: the smallest distance of sample 3 under the solution, the first on ties; a NaN or an infinite distance never
// wins.  Invalid (12 zeros): no solution, no finite distance, a non-finite output.
#pragma once
#include <stdint.h>

#include "fp64_ops.h"

namespace okvfe {
namespace {

constexpr int kHypMaxDoublings = 64;    // hi = 2^64 at the most
constexpr int kHypMaxBisections = 128;

// ---- the sampler ----------------------------------------------------------------------------------------------------
OKVFE_FP64_HD uint64_t hyp_hash(uint64_t seed, uint64_t key, int h, int j) {
  uint64_t z = seed + (key * 512ull + (uint64_t)h * 8ull + (uint64_t)j + 1ull) * 0x9E3779B97F4A7C15ull;
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
OKVFE_FP64_HD int hyp_draw(uint64_t seed, uint64_t key, int h, int j, int range) {
  return (int)(((hyp_hash(seed, key, h, j) >> 32) * (uint64_t)range) >> 32);
}

// The four list positions of hypothesis h of the multiframe with sample key `key`; n: correspondences of the multiframe;
// range_of(i, &b, &e): the range of the camera that owns position i.  -> positions drawn: 0 (n == 0), 1 (the camera
// has fewer than four correspondences) or 4; the positions not drawn are -1.
template <class RangeOf>
OKVFE_FP64_HD int hyp_sample(uint64_t seed, uint64_t key, int h, int n, const RangeOf& range_of, int pos[4]) {
  pos[0] = -1; pos[1] = -1; pos[2] = -1; pos[3] = -1;
  if (n <= 0) return 0;
  const int i0 = hyp_draw(seed, key, h, 0, n);
  int b = 0, e = 0;
  range_of(i0, &b, &e);
  pos[0] = i0;
  const int nc = e - b;
  if (nc < 4) return 1;
  int s0 = i0 - b, s1 = 0, s2 = 0;  // the chosen positions inside the camera, ascending
  {
    int t = hyp_draw(seed, key, h, 1, nc - 1);
    if (s0 <= t) t += 1;
    pos[1] = b + t;
    if (t < s0) { s1 = s0; s0 = t; } else { s1 = t; }
  }
  {
    int t = hyp_draw(seed, key, h, 2, nc - 2);
    if (s0 <= t) t += 1;
    if (s1 <= t) t += 1;
    pos[2] = b + t;
    if (t < s0) { s2 = s1; s1 = s0; s0 = t; } else if (t < s1) { s2 = s1; s1 = t; } else { s2 = t; }
  }
  {
    int t = hyp_draw(seed, key, h, 3, nc - 3);
    if (s0 <= t) t += 1;
    if (s1 <= t) t += 1;
    if (s2 <= t) t += 1;
    pos[3] = b + t;
  }
  return 4;
}

// ---- the solver -----------------------------------------------------------------------------------------------------
OKVFE_FP64_HD double hyp_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
OKVFE_FP64_HD void hyp_cross(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
OKVFE_FP64_HD void hyp_unit(double* a) {
  const double n = fp64::sqrt(hyp_dot(a, a));
  a[0] = a[0] / n; a[1] = a[1] / n; a[2] = a[2] / n;
}
// e1 = (X2 - X1) / |..|, e3 = e1 x (X3 - X1) normalised, e2 = e3 x e1: E[0..2] = e1, E[3..5] = e2, E[6..8] = e3
OKVFE_FP64_HD void hyp_triad(const double* X1, const double* X2, const double* X3, double* E) {
  double d[3];
  for (int i = 0; i < 3; ++i) {
    E[i] = X2[i] - X1[i];
    d[i] = X3[i] - X1[i];
  }
  hyp_unit(E);
  hyp_cross(E, d, E + 6);
  hyp_unit(E + 6);
  hyp_cross(E + 6, E, E + 3);
}

struct P3pProblem {
  double P[3][3], f[3][3];   // samples 0..2: world points and bearings
  double p3[3], f3[3], sigma3;  // sample 3
  double C[9], r[3];         // T_SC of the samples' camera
  double a2, b2, c2, ca, cb, cg, k;
  double A[5];               // A0 .. A4
  double Ew[9];              // the triad of the world points
};

struct P3pState {
  double H[12], best;
  int n_solutions, found;
};

// one root of the quartic, already polished: the test, the pose, the distance of sample 3, the choice
template <class Dist>
OKVFE_FP64_HD void p3p_consider(const P3pProblem& Q, double v, P3pState& S, const Dist& dist) {
  const double u = ((((Q.k - 1.0) * v) * v - ((2.0 * Q.k) * Q.cb) * v) + 1.0 + Q.k) / (2.0 * (Q.cg - v * Q.ca));
  const double s1sq = Q.b2 / ((1.0 + v * v) - (2.0 * v) * Q.cb);
  if (!(v > 0.0 && u > 0.0 && s1sq > 0.0)) return;
  S.n_solutions += 1;
  const double s1 = fp64::sqrt(s1sq), s2 = u * s1, s3 = v * s1;
  double X[3][3], Ec[9], R[9], t[3], H[12];
  for (int i = 0; i < 3; ++i) {
    X[0][i] = s1 * Q.f[0][i];
    X[1][i] = s2 * Q.f[1][i];
    X[2][i] = s3 * Q.f[2][i];
  }
  hyp_triad(X[0], X[1], X[2], Ec);
  for (int i = 0; i < 3; ++i)   // R_CW = e1c e1w^T + e2c e2w^T + e3c e3w^T
    for (int j = 0; j < 3; ++j) R[3 * i + j] = (Ec[i] * Q.Ew[j] + Ec[3 + i] * Q.Ew[3 + j]) + Ec[6 + i] * Q.Ew[6 + j];
  for (int i = 0; i < 3; ++i)   // t_CW = Q1 - R_CW P1
    t[i] = X[0][i] - ((R[3 * i] * Q.P[0][0] + R[3 * i + 1] * Q.P[0][1]) + R[3 * i + 2] * Q.P[0][2]);
  for (int i = 0; i < 3; ++i) {
    // R_WC = R_CW^T, t_WC = -(R_CW^T t_CW); R_WS = R_WC C_SC^T, t_WS = t_WC - R_WS r_SC
    const double twc = -((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]);
    for (int j = 0; j < 3; ++j) H[4 * i + j] = (R[i] * Q.C[3 * j] + R[3 + i] * Q.C[3 * j + 1]) + R[6 + i] * Q.C[3 * j + 2];
    H[4 * i + 3] = twc - ((H[4 * i] * Q.r[0] + H[4 * i + 1] * Q.r[1]) + H[4 * i + 2] * Q.r[2]);
  }
  const double d = dist(H, Q.p3, Q.C, Q.r, Q.f3, Q.sigma3);
  if (d < S.best) {
    S.best = d;
    S.found = 1;
    for (int i = 0; i < 12; ++i) S.H[i] = H[i];
  }
}

// a root y of the depressed quartic: back to v, three Newton steps on the original quartic, then p3p_consider
template <class Dist>
OKVFE_FP64_HD void p3p_root(const P3pProblem& Q, double y, double shift, P3pState& S, const Dist& dist) {
  double v = y - shift;
  for (int it = 0; it < 3; ++it) {
    const double f = (((Q.A[4] * v + Q.A[3]) * v + Q.A[2]) * v + Q.A[1]) * v + Q.A[0];
    const double fp = (((4.0 * Q.A[4]) * v + 3.0 * Q.A[3]) * v + 2.0 * Q.A[2]) * v + Q.A[1];
    if (fp != 0.0) v = v - f / fp;
  }
  p3p_consider(Q, v, S, dist);
}

// P / f: four world points / unit bearings (rows), sigma3 of the fourth; C, r: T_SC of their camera.
// dist(H, p, C_SC, r_SC, b, sigma): the distance of the consensus (FrameAbsolutePoseSacProblem.hpp:140-165) of point p with
// bearing b under the hypothesis H (3 x 4 row-major), in the order of the sums in force.  In the library it is the
// consensus kernel's own invert_hypothesis + ransac_distance (k_ransac.hip); this header holds no copy of it.
// -> H (12 doubles, zeros when invalid), *n_solutions; returns the validity.
template <class Dist>
OKVFE_FP64_HD bool p3p_hypothesis(const double* P /* 4 x 3 */, const double* f /* 4 x 3 */, double sigma3, const double* C,
                                const double* r, double* H, int* n_solutions, const Dist& dist) {
  P3pProblem Q;
  for (int i = 0; i < 3; ++i) {
    for (int s = 0; s < 3; ++s) {
      Q.P[s][i] = P[3 * s + i];
      Q.f[s][i] = f[3 * s + i];
    }
    Q.p3[i] = P[9 + i];
    Q.f3[i] = f[9 + i];
    Q.r[i] = r[i];
  }
  for (int i = 0; i < 9; ++i) Q.C[i] = C[i];
  Q.sigma3 = sigma3;
  P3pState S;
  for (int i = 0; i < 12; ++i) {
    S.H[i] = 0.0;
    H[i] = 0.0;
  }
  S.best = __builtin_inf();
  S.n_solutions = 0;
  S.found = 0;
  *n_solutions = 0;

  double d23[3], d13[3], d12[3];
  for (int i = 0; i < 3; ++i) {
    d23[i] = Q.P[1][i] - Q.P[2][i];
    d13[i] = Q.P[0][i] - Q.P[2][i];
    d12[i] = Q.P[0][i] - Q.P[1][i];
  }
  const double a2 = hyp_dot(d23, d23), b2 = hyp_dot(d13, d13), c2 = hyp_dot(d12, d12);
  const double ca = hyp_dot(Q.f[1], Q.f[2]), cb = hyp_dot(Q.f[0], Q.f[2]), cg = hyp_dot(Q.f[0], Q.f[1]);
  const double k = (a2 - c2) / b2, k2 = (a2 + c2) / b2;
  const double rc = c2 / b2, ra = a2 / b2;
  Q.a2 = a2; Q.b2 = b2; Q.c2 = c2; Q.ca = ca; Q.cb = cb; Q.cg = cg; Q.k = k;
  Q.A[4] = (k - 1.0) * (k - 1.0) - ((4.0 * rc) * ca) * ca;
  {
    const double t1 = (k * (1.0 - k)) * cb, t2 = ((1.0 - k2) * ca) * cg, t3 = (((2.0 * rc) * ca) * ca) * cb;
    Q.A[3] = 4.0 * ((t1 - t2) + t3);
  }
  {
    const double t1 = k * k - 1.0, t2 = ((2.0 * k) * k) * (cb * cb), t3 = (2.0 * ((b2 - c2) / b2)) * (ca * ca);
    const double t4 = (((4.0 * k2) * ca) * cb) * cg, t5 = (2.0 * ((b2 - a2) / b2)) * (cg * cg);
    Q.A[2] = 2.0 * ((((t1 + t2) + t3) - t4) + t5);
  }
  {
    const double t1 = ((-k) * (1.0 + k)) * cb, t2 = (((2.0 * ra) * cg) * cg) * cb, t3 = ((1.0 - k2) * ca) * cg;
    Q.A[1] = 4.0 * ((t1 + t2) - t3);
  }
  Q.A[0] = (1.0 + k) * (1.0 + k) - ((4.0 * ra) * cg) * cg;
  bool ok = Q.A[4] != 0.0;
  for (int i = 0; i < 5; ++i) ok = ok && fp64::finite(Q.A[i]);
  if (!ok) return false;
  hyp_triad(Q.P[0], Q.P[1], Q.P[2], Q.Ew);

  const double B = Q.A[3] / Q.A[4], Cq = Q.A[2] / Q.A[4], D = Q.A[1] / Q.A[4], E = Q.A[0] / Q.A[4];
  const double BB = B * B;
  const double p = Cq - (3.0 * BB) / 8.0;
  const double q = (D - (B * Cq) / 2.0) + (BB * B) / 8.0;
  const double rr = ((E - (B * D) / 4.0) + (BB * Cq) / 16.0) - ((3.0 * BB) * BB) / 256.0;
  const double shift = B / 4.0;
  const double none = __builtin_nan("");  // a root that does not exist: it fails every test of p3p_consider
  double y0 = none, y1 = none, y2 = none, y3 = none;
  if (q == 0.0) {
    const double disc = p * p - 4.0 * rr;
    if (disc >= 0.0) {
      const double sd = fp64::sqrt(disc);
      const double w1 = ((-p) + sd) / 2.0, w2 = ((-p) - sd) / 2.0;
      if (w1 >= 0.0) {
        y0 = fp64::sqrt(w1);
        y1 = -y0;
      }
      if (w2 >= 0.0) {
        y2 = fp64::sqrt(w2);
        y3 = -y2;
      }
    }
  } else {
    const double g1 = 8.0 * p, g2 = (2.0 * p) * p - 8.0 * rr, g3 = q * q;
    double lo = 0.0, hi = 1.0;
    int doublings = 0;
    bool bracket = (((8.0 * hi + g1) * hi + g2) * hi - g3) > 0.0;
    while (!bracket && doublings < kHypMaxDoublings) {
      hi = hi * 2.0;
      doublings += 1;
      bracket = (((8.0 * hi + g1) * hi + g2) * hi - g3) > 0.0;
    }
    if (bracket) {
      for (int it = 0; it < kHypMaxBisections; ++it) {
        const double mid = (lo + hi) / 2.0;
        if (mid == lo || mid == hi) break;
        if ((((8.0 * mid + g1) * mid + g2) * mid - g3) > 0.0) hi = mid; else lo = mid;
      }
      const double m = hi;
      const double s = fp64::sqrt(2.0 * m), t0 = p / 2.0 + m, u0 = q / (2.0 * s);
      const double disc1 = s * s - 4.0 * (t0 + u0), disc2 = s * s - 4.0 * (t0 - u0);
      if (disc1 >= 0.0) {
        const double sd = fp64::sqrt(disc1);
        y0 = (s + sd) / 2.0;
        y1 = (s - sd) / 2.0;
      }
      if (disc2 >= 0.0) {
        const double sd = fp64::sqrt(disc2);
        y2 = ((-s) + sd) / 2.0;
        y3 = ((-s) - sd) / 2.0;
      }
    }
  }
  OKVFE_FP64_NOUNROLL
  for (int i = 0; i < 4; ++i)  // (one copy of the pose chain in the code; selects, not an indexed array in memory)
    p3p_root(Q, i == 0 ? y0 : i == 1 ? y1 : i == 2 ? y2 : y3, shift, S, dist);
  *n_solutions = S.n_solutions;
  bool valid = S.found != 0;
  for (int i = 0; i < 12; ++i) valid = valid && fp64::finite(S.H[i]);
  if (valid)
    for (int i = 0; i < 12; ++i) H[i] = S.H[i];
  return valid;
}

}  // namespace
}  // namespace okvfe
