"""Test-side restatement of the 8-coefficient radial-tangential camera (OKVFE_DIST_RADTAN8, the
OpenCV "rational" model of okvis::cameras::RadialTangentialDistortion8) on a pinhole camera.

The CPU oracle under oracle/ knows only the three older models, so this module is the reference for
the fourth.  Plain numpy FP64, vectorised over points, in the same operation order as the library
(one IEEE operation per numpy operation: no contraction), so results are bit-comparable with the
host tables and the device kernels:

  distort        value + 2x2 point Jacobian; fails for rho = |u|^2 > 9
  undistort      5 Gauss-Newton steps, success at chi2 < 1e-4, early stop at 1e-15; a step whose
                 distort fails ends the iteration with the result invalid
  backproject    PinholeCamera::backProject
  project        PinholeCamera::project with status (0 ok, 1 outside, 3 behind, 4 invalid) and the
                 2x3 Jacobian
  awareness_maps PinholeCamera::initialiseCameraAwarenessMaps (failed Jacobians = 0)
  overlap        NCameraSystem::computeOverlaps for one ordered camera pair

`cam` is any object with w, h, fu, fv, cu, cv and d = (k1, k2, p1, p2, k3, k4, k5, k6)
(okvis2_amd.synth.Camera with dist_type 3).
"""
from __future__ import annotations

import numpy as np


def _coeffs(cam):
    d = tuple(float(v) for v in cam.d)
    assert len(d) == 8, "RADTAN8 needs 8 coefficients"
    return d


def distort(cam, u0, u1, want_jac=True):
    """Returns (ok, x0, x1, J) with J = (J00, J01, J10, J11) arrays (None if not wanted)."""
    k1, k2, p1, p2, k3, k4, k5, k6 = _coeffs(cam)
    u0 = np.asarray(u0, dtype=np.float64)
    u1 = np.asarray(u1, dtype=np.float64)
    with np.errstate(all="ignore"):
        mx = u0 * u0
        my = u1 * u1
        mxy = u0 * u1
        rho = mx + my
        ok = ~(rho > 9.0)
        qn = k2 + k3 * rho
        pn = k1 + rho * qn
        num = rho * pn + 1.0
        qd = k5 + k6 * rho
        pd = k4 + rho * qd
        den = rho * pd + 1.0
        rad = num / den
        x0 = u0 * rad + 2.0 * p1 * mxy + p2 * (rho + 2.0 * mx)
        x1 = u1 * rad + 2.0 * p2 * mxy + p1 * (rho + 2.0 * my)
        if not want_jac:
            return ok, x0, x1, None
        den2 = den * den
        dn0 = rho * (u0 * qn * 2.0 + k3 * u0 * rho * 2.0) + u0 * pn * 2.0
        dn1 = rho * (u1 * qn * 2.0 + k3 * u1 * rho * 2.0) + u1 * pn * 2.0
        dd0 = rho * (u0 * qd * 2.0 + k6 * u0 * rho * 2.0) + u0 * pd * 2.0
        dd1 = rho * (u1 * qd * 2.0 + k6 * u1 * rho * 2.0) + u1 * pd * 2.0
        j00 = p1 * u1 * 2.0 + p2 * u0 * 6.0 + num / den + (u0 * dn0) / den - u0 * dd0 * num / den2
        j01 = p1 * u0 * 2.0 + p2 * u1 * 2.0 + (u0 * dn1) / den - u0 * dd1 * num / den2
        j10 = p1 * u0 * 2.0 + p2 * u1 * 2.0 + (u1 * dn0) / den - u1 * dd0 * num / den2
        j11 = p1 * u1 * 6.0 + p2 * u0 * 2.0 + num / den + (u1 * dn1) / den - u1 * dd1 * num / den2
    return ok, x0, x1, (j00, j01, j10, j11)


def undistort(cam, pd0, pd1):
    """Gauss-Newton: returns (ok, x0, x1)."""
    pd0 = np.array(pd0, dtype=np.float64, ndmin=1)
    pd1 = np.array(pd1, dtype=np.float64, ndmin=1)
    x0, x1 = pd0.copy(), pd1.copy()
    success = np.zeros(pd0.shape, dtype=bool)
    active = np.ones(pd0.shape, dtype=bool)
    with np.errstate(all="ignore"):
        for _ in range(5):
            ok, t0, t1, (Ea, Eb, Ec, Ed) = distort(cam, x0, x1)
            failed = active & ~ok
            success[failed] = False
            active &= ok
            e0 = pd0 - t0
            e1 = pd1 - t1
            a = Ea * Ea + Ec * Ec
            b = Ea * Eb + Ec * Ed
            c = Eb * Ea + Ed * Ec
            d = Eb * Eb + Ed * Ed
            det = a * d - b * c
            invdet = 1.0 / det
            i00, i01, i10, i11 = d * invdet, -b * invdet, -c * invdet, a * invdet
            b00 = i00 * Ea + i01 * Eb
            b01 = i00 * Ec + i01 * Ed
            b10 = i10 * Ea + i11 * Eb
            b11 = i10 * Ec + i11 * Ed
            n0 = x0 + (b00 * e0 + b01 * e1)
            n1 = x1 + (b10 * e0 + b11 * e1)
            x0 = np.where(active, n0, x0)
            x1 = np.where(active, n1, x1)
            chi2 = e0 * e0 + e1 * e1
            success |= active & (chi2 < 1e-4)
            done = active & (chi2 < 1e-15)
            success |= done
            active &= ~done
    return success, x0, x1


def backproject(cam, px, py):
    """Returns (ok, dirs[..., 3]) with dirs = (x, y, 1)."""
    one_over_fu, one_over_fv = 1.0 / cam.fu, 1.0 / cam.fv
    px = np.asarray(px, dtype=np.float64)
    py = np.asarray(py, dtype=np.float64)
    ok, x0, x1 = undistort(cam, (px - cam.cu) * one_over_fu, (py - cam.cv) * one_over_fv)
    return ok, np.stack([x0, x1, np.ones_like(x0)], axis=-1)


def project(cam, P):
    """P [..., 3] -> (status, pts [..., 2], J23 [..., 6])."""
    P = np.asarray(P, dtype=np.float64)
    p0, p1, p2 = P[..., 0], P[..., 1], P[..., 2]
    with np.errstate(all="ignore"):
        rz = 1.0 / p2
        rz2 = rz * rz
        ok, x0, x1, (Da, Db, Dc, Dd) = distort(cam, p0 * rz, p1 * rz)
        J = np.stack([cam.fu * Da * rz, cam.fu * Db * rz, -cam.fu * (p0 * Da + p1 * Db) * rz2,
                      cam.fv * Dc * rz, cam.fv * Dd * rz, -cam.fv * (p0 * Dc + p1 * Dd) * rz2], axis=-1)
        px = cam.fu * x0 + cam.cu
        py = cam.fv * x1 + cam.cv
        status = np.where(p2 > 0.0, 0, 3)
        status = np.where((px < 0.0) | (py < 0.0) | (px >= float(cam.w)) | (py >= float(cam.h)), 1, status)
        status = np.where(ok, status, 4)
        status = np.where(np.abs(p2) < 1.0e-12, 4, status)
    return status.astype(np.int32), np.stack([px, py], axis=-1), J


def awareness_maps(cam):
    """(rays [h, w, 3] float32, jac [h, w, 6] float32)."""
    v, u = np.mgrid[0:cam.h, 0:cam.w]
    ok, ray = backproject(cam, u.astype(np.float64), v.astype(np.float64))
    with np.errstate(all="ignore"):
        n = np.sqrt(ray[..., 0] * ray[..., 0] + ray[..., 1] * ray[..., 1] + ray[..., 2] * ray[..., 2])
        ray = np.where(ok[..., None], ray / n[..., None], 0.0)
    st, _, J = project(cam, ray)
    jac = np.where((st == 0)[..., None], J, 0.0)
    return ray.astype(np.float32), jac.astype(np.float32)


def backproject_keypoints(cam, kps):
    """Keypoint back-projections as the extractor reports them: (bp [n, 3], valid [n] uint8)."""
    ok, d = backproject(cam, kps["x"].astype(np.float64), kps["y"].astype(np.float64))
    return d.reshape(-1, 3), ok.reshape(-1).astype(np.uint8)


def overlap(cam, other, R, project_fn=None, backproject_fn=None):
    """NCameraSystem::computeOverlaps of `cam` seen by `other` (row-major R_other_cam): (any, mask)."""
    project_fn = project_fn or project
    backproject_fn = backproject_fn or backproject
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    v, u = np.mgrid[0:cam.h, 0:cam.w]
    _, ray = backproject_fn(cam, u.astype(np.float64), v.astype(np.float64))
    r0, r1, r2 = ray[..., 0], ray[..., 1], ray[..., 2]
    ro = np.stack([R[i, 0] * r0 + R[i, 1] * r1 + R[i, 2] * r2 for i in range(3)], axis=-1)
    st, pt, _ = project_fn(other, ro)
    with np.errstate(all="ignore"):
        _, ver = backproject_fn(other, pt[..., 0], pt[..., 1])
        na = np.sqrt(ro[..., 0] * ro[..., 0] + ro[..., 1] * ro[..., 1] + ro[..., 2] * ro[..., 2])
        nb = np.sqrt(ver[..., 0] * ver[..., 0] + ver[..., 1] * ver[..., 1] + ver[..., 2] * ver[..., 2])
        dot = ((ro[..., 0] / na) * (ver[..., 0] / nb) + (ro[..., 1] / na) * (ver[..., 1] / nb)
               + (ro[..., 2] / na) * (ver[..., 2] / nb))
        hit = (st == 0) & (np.abs(dot - 1.0) < 1.0e-10)
    return bool(hit.any()), hit.astype(np.uint8)
