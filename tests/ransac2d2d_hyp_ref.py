"""Reference of okvfe_twopt_rotation_hypothesis, okvfe_fivept_hypothesis and okvfe_ransac2d2d_hypotheses_blocks_device:
the float64 restatement of okvis2_amd/csrc/ransac2d2d_hyp_dev.h, one IEEE operation per line -- the counter-based
sampler (ransac_hyp_ref.draw under the folded key), the rotation from two triads, Nister's five-point (null space by
Gauss-Jordan with full pivoting, the ten cubic constraints, the elimination, det B(z), its real roots by the
derivative chain and capped bisection, Horn's closed-form decomposition) and the choice among the candidates by the
consensus' own distance over samples 5 .. 7 (ransac2d2d_ref.relative_distances: the only part that follows the order
of the FP64 sums).  The correspondences are ransac2d2d_ref.correspondences.  A DEFINED ALGORITHM: opengv's sampler is
rand() and its solvers twopt_rotationOnly and Stewenius' five-point; nothing here claims parity with them
(include/okvfe.h states the deviations).

The scalar arithmetic runs on Python floats (IEEE binary64, one operation per operator, no contraction); a division
by zero and a square root go through numpy so that they give the IEEE result instead of an exception.

A census counts the branches taken.  Test infrastructure only."""
import math

import numpy as np

import ransac2d2d_ref as R2
from ransac_hyp_ref import MAX_BISECTIONS, draw

M64 = (1 << 64) - 1
MIN_CORR = R2.MIN_CORR
ROT_SAMPLES, REL_SAMPLES = 2, 8
INF = float("inf")

CENSUS = ("below_10", "rot_valid", "rot_zero_cross", "rot_nonfinite", "rel_valid", "null_pivot", "elim_pivot",
          "bad_lead", "no_root", "no_finite_sum", "rel_nonfinite", "tie", "t_not_positive", "bisection_cap",
          "roots0", "roots1", "roots2", "roots3", "roots4", "roots5", "roots6", "roots7", "roots8", "roots9",
          "roots10", "nan_bearing", "fallback_bearing")


def new_census():
    return dict.fromkeys(CENSUS, 0)


def _count(census, key, n=1):
    if census is not None:
        census[key] += int(n)


def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))


def _sqrt(a):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(a)))


def _finite(v):
    return not (math.isnan(v) or math.isinf(v))


# ---- the sampler ---------------------------------------------------------------------------------------------------
def fold_key(pair_key, cam, problem):
    """problem 0: rotation only, 1: relative pose"""
    return (pair_key * 128 + cam * 2 + problem) & M64


def sample(seed, key, h, n, count):
    """`count` distinct positions of [0, n), n >= count"""
    chosen, pos = [], []
    for j in range(count):
        t = draw(seed, key, h, j, n - j)
        for x in sorted(chosen):
            if x <= t:
                t += 1
        chosen.append(t)
        pos.append(t)
    return pos


# ---- rotation only -------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _triad(f0, f1):
    e3 = _cross(f0, f1)
    n2 = _dot(e3, e3)
    if n2 == 0.0:
        return None
    n = _sqrt(n2)
    e3 = [_div(e3[0], n), _div(e3[1], n), _div(e3[2], n)]
    return list(f0), _cross(e3, f0), e3


def twopt(b1, b2, census=None):
    """b1, b2: [2, 3].  -> (M [9], valid)"""
    b1 = [[float(v) for v in row] for row in np.asarray(b1, np.float64).reshape(2, 3)]
    b2 = [[float(v) for v in row] for row in np.asarray(b2, np.float64).reshape(2, 3)]
    T1 = _triad(b1[0], b1[1])
    T2 = _triad(b2[0], b2[1]) if T1 is not None else None
    if T1 is None or T2 is None:
        _count(census, "rot_zero_cross")
        return np.zeros(9), 0
    M = [(T1[0][i] * T2[0][j] + T1[1][i] * T2[1][j]) + T1[2][i] * T2[2][j] for i in range(3) for j in range(3)]
    if not all(_finite(v) for v in M):
        _count(census, "rot_nonfinite")
        return np.zeros(9), 0
    _count(census, "rot_valid")
    return np.array(M), 1


# ---- relative pose -------------------------------------------------------------------------------------------------
LIN = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0))
QUAD = ((2, 0, 0), (1, 1, 0), (1, 0, 1), (1, 0, 0), (0, 2, 0), (0, 1, 1), (0, 1, 0), (0, 0, 2), (0, 0, 1), (0, 0, 0))
CUBIC = ((3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
         (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0))
_add = lambda a, b: tuple(x + y for x, y in zip(a, b))
QIDX = [[QUAD.index(_add(a, b)) for b in LIN] for a in LIN]
CIDX = [[CUBIC.index(_add(q, l)) for l in LIN] for q in QUAD]
SYM = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}


def _sym(i, k):
    return SYM[(min(i, k), max(i, k))]


def _mul_ll(p, q):
    out = [0.0] * 10
    for i in range(4):
        for j in range(4):
            k = QIDX[i][j]
            out[k] = out[k] + p[i] * q[j]
    return out


def _mul_ql(q, l):
    out = [0.0] * 20
    for i in range(10):
        for j in range(4):
            k = CIDX[i][j]
            out[k] = out[k] + q[i] * l[j]
    return out


def _pmul(a, b):
    out = [0.0] * (len(a) + len(b) - 1)
    for i in range(len(a)):
        for j in range(len(b)):
            out[i + j] = out[i + j] + a[i] * b[j]
    return out


def _horner(q, m, z):
    v = q[m]
    for i in range(m):
        v = v * z + q[m - 1 - i]
    return v


def null_space(b1, b2, pivots=None):
    """-> lin[9][4]: entry e of (X, Y, Z, W), or None (a failed pivot); pivots: a list that receives the pivots"""
    Q = [[b1[i][a] * b2[i][b] for a in range(3) for b in range(3)] for i in range(5)]
    used, pivcol = [False] * 9, []
    for s in range(5):
        best, br, bc = -1.0, -1, -1
        for r in range(s, 5):
            for c in range(9):
                if used[c]:
                    continue
                a = abs(Q[r][c])
                if a > best:
                    best, br, bc = a, r, c
        if br < 0:
            return None
        piv = Q[br][bc]
        if pivots is not None:
            pivots.append(piv)
        if piv == 0.0 or not _finite(piv):
            return None
        Q[br], Q[s] = Q[s], Q[br]
        for r in range(5):
            if r == s:
                continue
            f = _div(Q[r][bc], piv)
            Q[r] = [Q[r][j] - f * Q[s][j] for j in range(9)]
        Q[s] = [_div(u, piv) for u in Q[s]]
        used[bc] = True
        pivcol.append(bc)
    lin = [[0.0] * 4 for _ in range(9)]
    k = 0
    for c in range(9):
        if used[c]:
            continue
        lin[c][k] = 1.0
        for s in range(5):
            lin[pivcol[s]][k] = -Q[s][c]
        k += 1
    return lin


def constraints(lin):
    """-> A[10][20]"""
    A = []
    # det E = e0 (e4 e8 - e5 e7) - e1 (e3 e8 - e5 e6) + e2 (e3 e7 - e4 e6)
    row = None
    for t, (a, b, c, d) in enumerate(((4, 8, 5, 7), (3, 8, 5, 6), (3, 7, 4, 6))):
        T1 = _mul_ll(lin[a], lin[b])
        T2 = _mul_ll(lin[c], lin[d])
        T1 = [T1[k] - T2[k] for k in range(10)]
        C = _mul_ql(T1, lin[t])
        if t == 0:
            row = C
        elif t == 1:
            row = [row[k] - C[k] for k in range(20)]
        else:
            row = [row[k] + C[k] for k in range(20)]
    A.append(row)
    D = [None] * 6
    for i in range(3):
        for j in range(i, 3):
            d = _mul_ll(lin[3 * i], lin[3 * j])
            T1 = _mul_ll(lin[3 * i + 1], lin[3 * j + 1])
            d = [d[k] + T1[k] for k in range(10)]
            T1 = _mul_ll(lin[3 * i + 2], lin[3 * j + 2])
            d = [d[k] + T1[k] for k in range(10)]
            D[_sym(i, j)] = d
    half = [0.5 * ((D[0][k] + D[3][k]) + D[5][k]) for k in range(10)]
    for s in (0, 3, 5):
        D[s] = [D[s][k] - half[k] for k in range(10)]
    for i in range(3):
        for j in range(3):
            row = _mul_ql(D[_sym(i, 0)], lin[j])
            C = _mul_ql(D[_sym(i, 1)], lin[3 + j])
            row = [row[k] + C[k] for k in range(20)]
            C = _mul_ql(D[_sym(i, 2)], lin[6 + j])
            row = [row[k] + C[k] for k in range(20)]
            A.append(row)
    return A


def eliminate(A, pivots=None):
    """Gauss-Jordan on the first ten columns, in place; False: a failed pivot; pivots: a list that receives the pivots"""
    for c in range(10):
        best, br = -1.0, -1
        for r in range(c, 10):
            a = abs(A[r][c])
            if a > best:
                best, br = a, r
        if br < 0:
            return False
        piv = A[br][c]
        if pivots is not None:
            pivots.append(piv)
        if piv == 0.0 or not _finite(piv):
            return False
        A[br], A[c] = A[c], A[br]
        for r in range(10):
            if r == c:
                continue
            f = _div(A[r][c], piv)
            A[r] = [A[r][j] - f * A[c][j] for j in range(20)]
        A[c] = [_div(u, piv) for u in A[c]]
    return True


def polynomial(A):
    """-> (B: three rows of (px [4], py [4], pc [5]), P [11]), constant terms first"""
    B = []
    for r in range(3):
        a, b = A[4 + 2 * r][10:], A[5 + 2 * r][10:]
        B.append(([a[2], a[1] - b[2], a[0] - b[1], -b[0]], [a[5], a[4] - b[5], a[3] - b[4], -b[3]],
                  [a[9], a[8] - b[9], a[7] - b[8], a[6] - b[7], -b[6]]))
    r0, r1, r2 = B
    sub = lambda u, v: [u[k] - v[k] for k in range(len(u))]
    P = _pmul(r0[0], sub(_pmul(r1[1], r2[2]), _pmul(r1[2], r2[1])))
    C = _pmul(r0[1], sub(_pmul(r1[0], r2[2]), _pmul(r1[2], r2[0])))
    P = [P[k] - C[k] for k in range(11)]
    C = _pmul(r0[2], sub(_pmul(r1[0], r2[1]), _pmul(r1[1], r2[0])))
    P = [P[k] + C[k] for k in range(11)]
    return B, P


def real_roots(P, census=None):
    """-> the real roots ascending, or None (the leading coefficient is zero or not finite)"""
    lead = P[10]
    if lead == 0.0 or not _finite(lead):
        return None
    mx = 0.0
    for i in range(10):
        a = abs(_div(P[i], lead))
        if a > mx:
            mx = a
    bound = 1.0 + mx
    der = [list(P)]
    for d in range(1, 10):
        der.append([der[d - 1][i + 1] * float(i + 1) for i in range(11 - d)])
    prev = []
    for d in range(9, -1, -1):
        q, m = der[d], 10 - d
        cur = []
        for k in range(len(prev) + 1):
            lo = -bound if k == 0 else prev[k - 1]
            hi = bound if k == len(prev) else prev[k]
            flo, fhi = _horner(q, m, lo), _horner(q, m, hi)
            if not ((flo < 0.0 and fhi > 0.0) or (flo > 0.0 and fhi < 0.0)):
                continue
            up = fhi > 0.0
            for it in range(MAX_BISECTIONS):
                mid = (lo + hi) / 2.0
                if mid == lo or mid == hi:
                    break
                fm = _horner(q, m, mid)
                if (fm > 0.0) == up:
                    hi = mid
                else:
                    lo = mid
            else:
                _count(census, "bisection_cap")
            cur.append(hi)
        prev = cur
    return prev


def candidates(lin, B, z, census=None):
    """the (up to four) [R | t] of one root, in candidate order; E first"""
    v = [[_horner(B[r][0], 3, z), _horner(B[r][1], 3, z), _horner(B[r][2], 4, z)] for r in range(3)]
    c01, c02, c12 = _cross(v[0], v[1]), _cross(v[0], v[2]), _cross(v[1], v[2])
    best, c = -1.0, c01
    if abs(c01[2]) > best:
        best = abs(c01[2])
    if abs(c02[2]) > best:
        best, c = abs(c02[2]), c02
    if abs(c12[2]) > best:
        best, c = abs(c12[2]), c12
    x, y = _div(c[0], c[2]), _div(c[1], c[2])
    E = [((x * lin[e][0] + y * lin[e][1]) + z * lin[e][2]) + lin[e][3] for e in range(9)]
    rows = [E[0:3], E[3:6], E[6:9]]
    G = [[_dot(rows[i], rows[j]) for j in range(3)] for i in range(3)]
    half = 0.5 * ((G[0][0] + G[1][1]) + G[2][2])
    t0, t1, t2 = half - G[0][0], half - G[1][1], half - G[2][2]
    tk, b = t0, [t0, -G[0][1], -G[0][2]]
    if t1 > tk:
        tk, b = t1, [-G[1][0], t1, -G[1][2]]
    if t2 > tk:
        tk, b = t2, [-G[2][0], -G[2][1], t2]
    if not tk > 0.0:
        _count(census, "t_not_positive")
        return E, []
    sk = _sqrt(tk)
    b = [_div(b[0], sk), _div(b[1], sk), _div(b[2], sk)]
    bb = _dot(b, b)
    nb = _sqrt(bb)
    bh = [_div(b[0], nb), _div(b[1], nb), _div(b[2], nb)]
    cof = _cross(rows[1], rows[2]) + _cross(rows[2], rows[0]) + _cross(rows[0], rows[1])
    bxe = [0.0] * 9
    for j in range(3):
        bxe[j] = b[1] * E[6 + j] - b[2] * E[3 + j]
        bxe[3 + j] = b[2] * E[j] - b[0] * E[6 + j]
        bxe[6 + j] = b[0] * E[3 + j] - b[1] * E[j]
    out = []
    for cand in range(4):
        H = [0.0] * 12
        for i in range(3):
            for j in range(3):
                num = cof[3 * i + j] - bxe[3 * i + j] if cand < 2 else cof[3 * i + j] + bxe[3 * i + j]
                H[4 * i + j] = _div(num, bb)
            H[4 * i + 3] = bh[i] if cand % 2 == 0 else -bh[i]
        out.append(H)
    return E, out


def fivept(tree, b1, b2, s1, s2, census=None, details=None):
    """b1, b2: [8, 3] (rows 0 .. 4 solve, rows 5 .. 7 choose); s1, s2: the sigmas of rows 5 .. 7.
    -> (H [12], valid, n_roots).  details: a dict that receives null_pivots, pivots, lin, P, roots, Es, sums"""
    b1 = [[float(v) for v in row] for row in np.asarray(b1, np.float64).reshape(8, 3)]
    b2 = [[float(v) for v in row] for row in np.asarray(b2, np.float64).reshape(8, 3)]
    zero = np.zeros(12)
    piv5, piv10 = [], []
    if details is not None:
        details.update(null_pivots=piv5, pivots=piv10)
    lin = null_space(b1, b2, piv5)
    if lin is None:
        _count(census, "null_pivot")
        return zero, 0, 0
    A = constraints(lin)
    if not eliminate(A, piv10):
        _count(census, "elim_pivot")
        return zero, 0, 0
    B, P = polynomial(A)
    roots = real_roots(P, census)
    if details is not None:
        details.update(lin=lin, P=P, roots=roots, Es=[], sums=[])
    if roots is None:
        _count(census, "bad_lead")
        return zero, 0, 0
    _count(census, "roots%d" % len(roots))
    if not roots:
        _count(census, "no_root")
        return zero, 0, 0
    corr = dict(kA=np.arange(3), b1=np.array(b1[5:8]), b2=np.array(b2[5:8]), s1=np.asarray(s1, np.float64).reshape(3),
                s2=np.asarray(s2, np.float64).reshape(3))
    best, best_H, sums = INF, None, []
    for z in roots:
        E, cands = candidates(lin, B, z, census)
        if details is not None:
            details["Es"].append(E)
        if not cands:
            continue
        d = R2.relative_distances(tree, np.array(cands), corr)
        for ci, H in enumerate(cands):
            with np.errstate(all="ignore"):
                total = float((d[ci, 0] + d[ci, 1]) + d[ci, 2])
            sums.append(total)
            if total < best:
                best, best_H = total, H
    if details is not None:
        details["sums"] = sums
    if best_H is None:
        _count(census, "no_finite_sum")
        return zero, 0, len(roots)
    if not all(_finite(v) for v in best_H):
        _count(census, "rel_nonfinite")
        return zero, 0, len(roots)
    if census is not None and sums.count(best) >= 2:
        census["tie"] += 1
    _count(census, "rel_valid")
    return np.array(best_H), 1, len(roots)


# ---- one (pair, camera) --------------------------------------------------------------------------------------------
def hypotheses(tree, corr, seed, pair_key, cam, n_hyp, census=None):
    """corr: ransac2d2d_ref.correspondences of the camera.  -> dict(rot_H [n_hyp, 9], rot_valid, rel_H [n_hyp, 12],
    rel_valid, rot_samples [n_hyp, 2], rel_samples [n_hyp, 8] (older keypoint indices, -1: not drawn), n_roots, n_corr)"""
    n = len(corr["kA"])
    out = dict(rot_H=np.zeros((n_hyp, 9)), rot_valid=np.zeros(n_hyp, np.uint8), rel_H=np.zeros((n_hyp, 12)),
               rel_valid=np.zeros(n_hyp, np.uint8), rot_samples=np.full((n_hyp, ROT_SAMPLES), -1, np.int32),
               rel_samples=np.full((n_hyp, REL_SAMPLES), -1, np.int32), n_roots=np.zeros(n_hyp, np.int32), n_corr=n)
    if n < MIN_CORR:
        _count(census, "below_10")
        return out
    if census is not None:
        census["nan_bearing"] += int(np.isnan(corr["b1"]).any(axis=1).sum() + np.isnan(corr["b2"]).any(axis=1).sum())
        census["fallback_bearing"] += int(np.all(corr["b1"] == (1.0, 0.0, 0.0), axis=1).sum())
    for h in range(n_hyp):
        pos = sample(seed, fold_key(pair_key, cam, 0), h, n, ROT_SAMPLES)
        out["rot_samples"][h] = corr["kA"][pos]
        out["rot_H"][h], out["rot_valid"][h] = twopt(corr["b1"][pos], corr["b2"][pos], census)
        pos = sample(seed, fold_key(pair_key, cam, 1), h, n, REL_SAMPLES)
        out["rel_samples"][h] = corr["kA"][pos]
        out["rel_H"][h], out["rel_valid"][h], out["n_roots"][h] = fivept(
            tree, corr["b1"][pos], corr["b2"][pos], corr["s1"][pos[5:]], corr["s2"][pos[5:]], census)
    return out
