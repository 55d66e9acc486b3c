"""Independent restatement of the gate chain in numpy.longdouble (x87 extended: 64-bit mantissa),
vectorised over pairs.  Written from the reference's sources, not from oracle/orc_match.c:

    triangulation::triangulateFast       okvis_frontend/src/stereo_triangulation.cpp:50-132
    Frontend::matchStereo, gated pair    okvis_frontend/src/Frontend.cpp:2027-2066
    Frontend::matchMotionStereo, pair    okvis_frontend/src/Frontend.cpp:1832-1887
    Transformation::inverse / operator*  okvis_kinematics/.../implementation/Transformation.hpp:207-209, 271-278

It does not reproduce an order of summation: at 11 more bits than binary64 the order is below what
the comparison asks.  Every comparison of the chain contributes a MARGIN, the distance of its left
side from its right side; a verdict is only claimed for pairs whose smallest margin exceeds the
caller's bound.  Margins are absolute (cosines, metres: quantities of order 1) except for the
determinant, which is compared with 1e-12 and so is measured relative to 1e-12.  Of a disjunction
(l0 < 0.01 || l1 < 0.01; "either cos 2.6 sigma test fails") the margin is that of its decisive
term: the largest excess when one holds, the smallest shortfall when none does.  A NaN operand makes
a comparison false whatever the precision: its margin is infinite.
"""
import numpy as np

LD = np.longdouble
INF = LD(np.inf)


def ld(a):
    return np.asarray(a, dtype=LD)


def dot(a, b):
    return (a * b).sum(axis=-1)


def normalized(v):
    with np.errstate(all="ignore"):
        return v / np.sqrt(dot(v, v))[..., None]


def _margin(x):
    """|x| with NaN -> inf"""
    x = np.abs(x)
    return np.where(np.isnan(x), INF, x)


def _either_less(a, b, bound):
    """(a < bound) | (b < bound) and the margin of the decisive term"""
    with np.errstate(all="ignore"):
        ta, tb = bound - a, bound - b           # > 0: the term holds
        hit = (a < bound) | (b < bound)
        worst = np.fmax(ta, tb)                 # fmax: a NaN term never holds and never decides
    return hit, _margin(worst)


def _midpoint_parallel(p1, e1, p2, e2, t12, c26):
    # stereo_triangulation.cpp:82-97 (= :101-116)
    tn = np.sqrt(dot(t12, t12))
    with np.errstate(all="ignore"):
        far = np.where(LD(0.01) < tn, tn, LD(0.01))  # std::max(0.01, norm): (a < b) ? b : a
    mid = p1 + LD(0.5) * t12 + (LD(40.0) * far)[..., None] * (e1 + e2)
    bad, m = _either_less(dot(e1, normalized(mid - p1)), dot(e2, normalized(mid - p2)), c26)
    return mid, ~bad, m


def triangulate_fast(p1, e1, p2, e2, sigma):
    """p1, e1, p2, e2: (n, 3); sigma: (n,).  Returns hp (n, 4), valid, parallel, margin."""
    p1, e1, p2, e2, sigma = ld(p1), ld(e1), ld(p2), ld(e2), ld(sigma)
    with np.errstate(all="ignore"):
        c26, c6 = np.cos(LD(2.6) * sigma), np.cos(LD(6.0) * sigma)
        t12 = p2 - p1
        b0, b1 = dot(t12, e1), dot(t12, e2)
        a00, a10 = dot(e1, e1), dot(e1, e2)
        a01, a11 = -a10, -dot(e2, e2)
        det = a00 * a11 - a01 * a10
        invertible = np.abs(det) > LD(1.0e-12)       # computeInverseWithCheck(.., 1.0e-12)
        m_det = _margin(np.abs(det) / LD(1.0e-12) - LD(1.0))
        l0 = (a11 * b0 - a01 * b1) / det              # A^-1 = [[a11, -a01], [-a10, a00]] / det
        l1 = (-a10 * b0 + a00 * b1) / det
        small, m_l = _either_less(l0, l1, LD(0.01))
        mid_p, valid_p, m_p = _midpoint_parallel(p1, e1, p2, e2, t12, c26)
        xm = l0[..., None] * e1 + p1
        xn = l1[..., None] * e2 + p2
        mid_t = (xm + xn) / LD(2.0)
        n1, n2 = normalized(mid_t - p1), normalized(mid_t - p2)
        bad_t, m_t = _either_less(dot(e1, n1), dot(e2, n2), c26)
        par_t = dot(n2, n1) > c6
        m_c6 = _margin(dot(n2, n1) - c6)
    fallback = ~invertible | small
    mid = np.where(fallback[..., None], mid_p, mid_t)
    hp = np.concatenate([mid, np.ones(mid.shape[:-1] + (1,), dtype=LD)], axis=-1)
    valid = np.where(fallback, valid_p, ~bad_t)
    parallel = fallback | par_t
    margin = np.where(invertible, np.minimum(m_det, m_l), m_det)
    margin = np.minimum(margin, np.where(fallback, m_p, np.minimum(m_t, m_c6)))
    return hp, valid, parallel, margin


def _inverse_apply(C, r, hp):
    """T^-1 * hp for T = (C, r): [C^T, -C^T r]"""
    C, r = ld(C).reshape(3, 3), ld(r)
    return np.concatenate([hp[..., :3] @ C - (r @ C) * hp[..., 3:4], hp[..., 3:4]], axis=-1)


def world_rays(T, bp):
    return normalized(ld(bp) @ ld(T[0]).reshape(3, 3).T)


def stereo_pairs(T0, T1, bp0, bp1, size0, size1, f0, f1):
    """The gated pair of matchStereo.  Returns hp_W, valid, parallel, margin."""
    e0, e1 = world_rays(T0, bp0), world_rays(T1, bp1)
    s0, s1 = ld(size0) / LD(f0), ld(size1) / LD(f1)
    sigma = np.where(s0 < s1, s1, s0) * LD(0.125)
    n = len(e0)
    hp, valid, parallel, margin = triangulate_fast(np.broadcast_to(ld(T0[1]), (n, 3)), e0,
                                                   np.broadcast_to(ld(T1[1]), (n, 3)), e1, sigma)
    with np.errstate(all="ignore"):
        z0 = _inverse_apply(T0[0], T0[1], hp)
        z1 = _inverse_apply(T1[0], T1[1], hp)
        d0, d1 = z0[:, 2] / z0[:, 3], z1[:, 2] / z1[:, 3]
        close, m_close = _either_less(d0, d1, LD(0.05))
        ee = dot(e0, e1)
        wide = ee < LD(0.8)
    gates = ~parallel
    valid = valid & ~(gates & (close | wide))
    margin = np.where(gates, np.minimum(margin, np.minimum(m_close, _margin(ee - LD(0.8)))), margin)
    return hp, valid, parallel, margin


def motion_pairs(T0, T1, bp0, bp1, size0, f0):
    """The gated pair of matchMotionStereo (sigma from keypoint 0 alone).  Returns hp_W, valid, parallel, margin."""
    e0, e1 = world_rays(T0, bp0), world_rays(T1, bp1)
    sigma = ld(size0) / LD(f0) * LD(0.125)
    n = len(e0)
    hp, valid, parallel, margin = triangulate_fast(np.broadcast_to(ld(T0[1]), (n, 3)), e0,
                                                   np.broadcast_to(ld(T1[1]), (n, 3)), e1, sigma)
    with np.errstate(all="ignore"):
        ee = dot(e0, e1)
        out = ee < LD(0.5)
        z0 = _inverse_apply(T0[0], T0[1], hp)
        z1 = _inverse_apply(T1[0], T1[1], hp)
        close, m_close = _either_less(z0[:, 2] / z0[:, 3], z1[:, 2] / z1[:, 3], LD(0.2))
        wide = ee < LD(0.8)
    m_ee = np.minimum(_margin(ee - LD(0.5)), _margin(ee - LD(0.8)))
    margin = np.where(out, _margin(ee - LD(0.5)), np.minimum(margin, m_ee))
    margin = np.where(~out & valid & ~parallel, np.minimum(margin, m_close), margin)
    valid = ~out & valid & ~wide & ~(~parallel & close)
    return hp, valid, parallel, margin
