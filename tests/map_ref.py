"""Independent restatement of matchToMap's landmark preparation in numpy.longdouble (x87 extended:
64-bit mantissa), vectorised over landmarks.  Written from the reference's sources, not from
oracle/orc_match.c or k_map.hip:

    Frontend::matchToMap, landmark loop     okvis_frontend/src/Frontend.cpp:1219-1359
    PinholeCamera::project(Homogeneous)     okvis_cv/.../implementation/PinholeCamera.hpp:255-290, 493-502
    CameraBase::isInImage                   okvis_cv/.../implementation/CameraBase.hpp:97-106
    RadialTangentialDistortion::distort     .../RadialTangentialDistortion.hpp:90-109
    EquidistantDistortion::distort          .../EquidistantDistortion.hpp:87-107
    RadialTangentialDistortion8::distort    .../RadialTangentialDistortion8.hpp:108-126
    Transformation::inverse / operator*     okvis_kinematics/.../implementation/Transformation.hpp:207-209, 271-278

As tests/gate_ref.py it reproduces no order of summation, and a vector of zero length normalises to
NaNs (x / 0), which is what the oracle and the kernels take the reference to do.  Every comparison
that can turn an output contributes a MARGIN, the distance of its left side from its right side
(pixels, cosines, ratios, scores: quantities of order 1; the two tests of z = hp_C[2] relative to the size
of hp_W and T_WC1, whose rounding z carries: a table scaled by 1e-300 keeps its margin); a
landmark's margin is the smallest one it met, and a verdict is only claimed above the caller's bound.
A comparison whose outcome cannot reach an output has none: the view-point and scale tests of an
exclusive call, "inside the image" for a point in front of the camera (OutsideImage and Successful
are treated alike), the sign of z for a projection outside the image.  A NaN operand makes a
comparison false at any precision: infinite margin.  Two conditions are not a comparison of the
source but bound its arithmetic: an acos argument within the margin of +-1 (acos has no derivative
there, and binary64 may find it above 1: a NaN score), and two slot scores that differ by less than
the margin without being equal (which of them is the worst slot).

longdouble also has a wider exponent than binary64.  The reference computes in binary64, where the
squared norm of a point at 1e300 m (hp[3] = 1e-300) is an infinity: _b64range keeps binary64's
RANGE (not its precision) on the products that can leave it.
"""
import numpy as np

LD = np.longdouble
INF = LD(np.inf)
_DBL_MAX = LD(np.finfo(np.float64).max)


def ld(a):
    return np.asarray(a, dtype=LD)


def _b64range(x):
    with np.errstate(all="ignore"):
        return np.where(np.abs(x) > _DBL_MAX, np.copysign(INF, x), x)


def dot(a, b):
    with np.errstate(all="ignore"):
        return _b64range((_b64range(a * b)).sum(axis=-1))


def norm(v):
    with np.errstate(all="ignore"):
        return np.sqrt(dot(v, v))


def normalized(v):
    with np.errstate(all="ignore"):
        return v / norm(v)[..., None]


def _margin(x):
    """|x| with NaN -> inf"""
    with np.errstate(all="ignore"):
        x = np.abs(x)
    return np.where(np.isnan(x), INF, x)


def _distort(cam, u0, u1):
    """(ok, x0, x1, margin of ok)"""
    d = [LD(v) for v in cam.d]
    none = np.full(u0.shape, INF, dtype=LD)
    with np.errstate(all="ignore"):
        if cam.dist_type == 0:
            return np.ones(u0.shape, bool), u0, u1, none
        if cam.dist_type == 1:
            k1, k2, p1, p2 = d
            mx, my, mxy = u0 * u0, u1 * u1, u0 * u1
            rho = mx + my
            rad = k1 * rho + k2 * rho * rho
            return (np.ones(u0.shape, bool), u0 + u0 * rad + LD(2) * p1 * mxy + p2 * (rho + LD(2) * mx),
                    u1 + u1 * rad + LD(2) * p2 * mxy + p1 * (rho + LD(2) * my), none)
        if cam.dist_type == 2:
            k1, k2, k3, k4 = d
            r = np.sqrt(u0 * u0 + u1 * u1)
            th = np.arctan(r)
            th2 = th * th
            th4 = th2 * th2
            thd = th * (LD(1) + k1 * th2 + k2 * th4 + k3 * th4 * th2 + k4 * th4 * th4)
            s = np.where(r > LD(1e-8), thd / r, LD(1))
            return np.ones(u0.shape, bool), s * u0, s * u1, _margin(r - LD(1e-8))
        k1, k2, p1, p2, k3, k4, k5, k6 = d
        mx, my, mxy = u0 * u0, u1 * u1, u0 * u1
        rho = mx + my
        ok = ~(rho > LD(9))
        rad = (LD(1) + ((k3 * rho + k2) * rho + k1) * rho) / (LD(1) + ((k6 * rho + k5) * rho + k4) * rho)
        return (ok, u0 * rad + LD(2) * p1 * mxy + p2 * (rho + LD(2) * mx),
                u1 * rad + LD(2) * p2 * mxy + p1 * (rho + LD(2) * my), _margin(rho - LD(9)))


def project(cam, head, zscale):
    """PinholeCamera::project for head (n, 3).  Returns (status, kp (n, 2), margin): status 0 Successful,
    1 OutsideImage, 3 Behind, 4 Invalid; margin of "status in {3, 4}", which is what the caller asks.
    zscale (n,): the size of the operands z was computed from; the two tests of z are measured against it."""
    z = head[:, 2]
    with np.errstate(all="ignore"):
        invalid = np.abs(z) < LD(1e-12)
        m = _margin((np.abs(z) - LD(1e-12)) / zscale)
        rz = LD(1) / z
        ok, x0, x1, m_ok = _distort(cam, head[:, 0] * rz, head[:, 1] * rz)
        px, py = LD(cam.fu) * x0 + LD(cam.cu), LD(cam.fv) * x1 + LD(cam.cv)
        inside = ~((px < 0) | (py < 0)) & ~((px >= LD(cam.w)) | (py >= LD(cam.h)))
        m_in = np.minimum(np.minimum(_margin(px), _margin(py)),
                          np.minimum(_margin(px - LD(cam.w)), _margin(py - LD(cam.h))))
        front = z > 0
    status = np.where(invalid | ~ok, 4, np.where(~inside, 1, np.where(front, 0, 3)))
    m = np.where(invalid, m, np.minimum(m, m_ok))
    live = ~invalid & ok
    m = np.where(live & ~front, np.minimum(m, m_in), m)     # behind: inside the image or not decides
    m = np.where(live & inside, np.minimum(m, _margin(z / zscale)), m)  # inside: the sign of z decides
    return status, np.stack([px, py], axis=-1), m


def prepare_landmarks(hp_W, quality, obs_begin, obs_pose, obs_bp, poses, T_WC1, cam, repr_thr, exclusive):
    """Frontend.cpp:1219-1359 for a landmark table (arguments as oracle_lib.prepare_landmarks).  Returns a dict
    with status, n_desc, obs_rows (n, 3), projection (n, 2), e_W and r_W (n, 2, 3) as longdouble, margin (n,)."""
    hp = ld(hp_W).reshape(-1, 4)
    n = len(hp)
    q = ld(quality)
    begin = np.asarray(obs_begin, dtype=np.int64)
    obs_pose = np.asarray(obs_pose, dtype=np.int64)
    bp = ld(obs_bp).reshape(-1, 3)
    PC = ld([np.asarray(p[0], dtype=np.float64).reshape(3, 3) for p in poses]).reshape(-1, 3, 3)
    Pr = ld([np.asarray(p[1], dtype=np.float64) for p in poses]).reshape(-1, 3)
    C1, r1 = ld(T_WC1[0]).reshape(3, 3), ld(T_WC1[1])
    thr = LD(repr_thr)
    focal = LD(cam.fu) + LD(cam.fv)          # the sum: Frontend.cpp:1215-1217
    cos10, cos06 = np.cos(LD(10) / focal), np.cos(LD(0.6))
    margin = np.full(n, INF, dtype=LD)
    with np.errstate(all="ignore"):
        p_W = _b64range(hp[:, :3] / hp[:, 3:4])
        r_W = p_W - r1
        e_W = normalized(r_W)
        rn = norm(r_W)
        r = np.where(LD(0.01) < rn, rn, LD(0.01))      # std::max(0.01, norm): (a < b) ? b : a
        hp_C = np.concatenate([hp[:, :3] @ C1 - (r1 @ C1) * hp[:, 3:4], hp[:, 3:4]], axis=1)
        head = np.where(hp_C[:, 3:4] < 0, -hp_C[:, :3], hp_C[:, :3])
        zscale = np.max(np.abs(hp), axis=1) * (LD(1) + np.max(np.abs(r1)))
        st, kp, m_st = project(cam, head, np.where(zscale > 0, zscale, LD(1)))
        alive = (st != 4) & (st != 3)
        margin = np.minimum(margin, m_st)
        maxU, maxV = LD(cam.w) + thr, LD(cam.h) + thr
        out = (kp[:, 0] < -thr) | (kp[:, 1] < -thr) | (kp[:, 0] > maxU) | (kp[:, 1] > maxV)
        m_box = np.minimum(np.minimum(_margin(kp[:, 0] + thr), _margin(kp[:, 1] + thr)),
                           np.minimum(_margin(kp[:, 0] - maxU), _margin(kp[:, 1] - maxV)))
        margin = np.where(alive, np.minimum(margin, m_box), margin)
        alive &= ~out
        margin = np.where(alive, np.minimum(margin, _margin(rn - LD(0.01))), margin)
    projection = np.where(alive[:, None], kp, LD(0))
    is3d = np.zeros(n, bool)
    o = np.zeros(n, dtype=np.int64)
    rows = np.full((n, 3), -1, dtype=np.int64)
    best = np.ones((n, 3), dtype=LD)
    ew = np.zeros((n, 3, 3), dtype=LD)
    rw = np.zeros((n, 3, 3), dtype=LD)
    n_obs = begin[1:] - begin[:-1]
    ar = np.arange(n)
    for k in range(int(n_obs.max()) if n else 0):
        act = alive & (k < n_obs)
        if not act.any():
            continue
        ob = np.where(act, begin[:-1] + k, 0)
        if len(obs_pose) == 0:
            break
        pi = obs_pose[ob]
        with np.errstate(all="ignore"):
            r_old = p_W - Pr[pi]
            f = LD(0.2) / focal / q
            cosA = dot(normalized(r_W), normalized(_b64range(r_W - _b64range(f[:, None] * r_old))))
            test = act & ~is3d
            margin = np.where(test, np.minimum(margin, _margin(cosA - cos10)), margin)
            is3d |= test & (cosA > cos10)
            cosVC = dot(e_W, normalized(r_old))
            if not exclusive:
                margin = np.where(act, np.minimum(margin, _margin(cosVC - cos06)), margin)
                act = act & ~(cosVC < cos06)
            scale = np.abs(r - norm(r_old)) / r
            if not exclusive:
                margin = np.where(act, np.minimum(margin, _margin(scale - LD(0.5))), margin)
                act = act & ~(scale > LD(0.5))
            margin = np.where(act, np.minimum(margin, _margin(LD(1) - np.abs(cosVC))), margin)
            score = LD(0.5) * (np.arccos(cosVC) / LD(0.6) + scale / LD(0.5))
            worst = np.zeros(n, dtype=LD)
            wi = np.zeros(n, dtype=np.int64)
            for s in range(3):
                gt = best[:, s] > worst
                wi = np.where(gt, s, wi)
                worst = np.where(gt, best[:, s], worst)
            # the worst slot is the largest score: its lead over the runner-up, unless they are equal
            srt = np.sort(best, axis=1)
            lead = srt[:, 2] - srt[:, 1]
            margin = np.where(act & (lead != 0), np.minimum(margin, _margin(lead)), margin)
            bw = best[ar, wi]
            margin = np.where(act & (score != bw), np.minimum(margin, _margin(score - bw)), margin)
            store = act & (score < bw)
            e_obs = np.einsum("nij,nj->ni", PC[pi], normalized(bp[ob]))
        sel = np.flatnonzero(store)
        rows[sel, o[sel]] = ob[sel]
        ew[sel, o[sel]] = e_obs[sel]
        rw[sel, o[sel]] = Pr[pi[sel]]
        o[sel] = np.maximum(o[sel], wi[sel])
        best[sel, wi[sel]] = score[sel]
    kept = alive & (o > 0)
    status = np.where(kept, np.where(is3d, 1, 2), 0).astype(np.int32)
    n_desc = np.where(kept, o, 0).astype(np.int32)
    obs_rows = np.where(kept[:, None], rows, -1).astype(np.int32)
    keep_row = kept[:, None] & (np.arange(2)[None, :] < o[:, None])
    e_out = np.where(keep_row[:, :, None], ew[:, :2], LD(0))
    r_out = np.where(keep_row[:, :, None], rw[:, :2], LD(0))
    return dict(status=status, n_desc=n_desc, obs_rows=obs_rows, projection=projection, e_W=e_out, r_W=r_out,
                margin=margin)
