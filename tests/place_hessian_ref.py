"""Reference of okvfe_place_hessian_blocks_device: a plain numpy restatement, from the reference's sources, of

  the terms               okvis_frontend/src/Frontend.cpp:433-518 (the inliers of the winner, adapter order) and :529-551
  one term                okvis_ceres/include/okvis/ceres/implementation/ReprojectionError.hpp:99-163, jacobians[0] only
  projectHomogeneous      okvis_cv/include/okvis/cameras/implementation/PinholeCamera.hpp:506-526 over project (:296-374):
                          the oracle's (oracle_lib.cam_project with its 2 x 3 Jacobian; the 8-coefficient model through
                          radtan8_ref.project)
  crossMx                 okvis_kinematics/include/okvis/kinematics/operators.hpp:60-73
  PoseManifold::plus      okvis_ceres/src/PoseLocalParameterization.cpp:49-64 with deltaQ (okvis_kinematics
                          implementation/Transformation.hpp:64-71), for the central differences of the host tests only

Every product, sum, quotient and square root is a separate numpy operation on float64 arrays: IEEE operations without
contraction, so the device must reproduce the results byte for byte.  The 3- and 4-term sums come in both orders
(ransac_ref.sum3 / sum4).  The matrix products are full: the zeros of T_CS, J, Jh and the square-root information are
multiplied and added.  PARITY UNPINNED: Eigen's Quaternion::normalize() and toRotationMatrix(), restated from the
published source (Eigen is not in the tree).

A census counts the branches taken.  Test infrastructure only."""
import numpy as np

import radtan8_ref
from ransac_ref import sum3, sum4

CENSUS = ("term", "w_negative", "behind", "outside_left", "outside_top", "outside_right", "outside_bottom",
          "distortion_failure", "singular_z", "bad_size", "landmark_in_two_cameras", "state_0", "state_1",
          "row_outside_set", "not_verified")


def new_census():
    return dict.fromkeys(CENSUS, 0)


def rotation(tree, q):
    """q = (x, y, z, w): q.normalize() then q.toRotationMatrix() (ReprojectionError.hpp:101-103, :115): Eigen divides by
    sqrt(z), z = squaredNorm(), iff z > 0; the matrix from tx = 2 x, twx = tx w, ... (Eigen/src/Geometry/Quaternion.h)"""
    with np.errstate(all="ignore"):
        x, y, z, w = (np.float64(v) for v in q)
        n2 = sum4(tree, x * x, y * y, z * z, w * w)
        if n2 > 0:
            n = np.sqrt(n2)
            x, y, z, w = x / n, y / n, z / n, w / n
        tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
        twx, twy, twz = tx * w, ty * w, tz * w
        txx, txy, txz = tx * x, ty * x, tz * x
        tyy, tyz, tzz = ty * y, tz * y, tz * z
        return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                         [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                         [txz - twy, tyz + twx, 1.0 - (txx + tyy)]], dtype=np.float64)


def inverse_transform(tree, pose):
    """pose = (t[3], qx, qy, qz, qw) -> the 4 x 4 matrix of its inverse (ReprojectionError.hpp:115-124)"""
    pose = np.asarray(pose, dtype=np.float64)
    C = rotation(tree, pose[3:7])
    T = np.zeros((4, 4))
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                T[i, j] = C[j, i]                                  # :116, :121
            T[i, 3] = sum3(tree, (-C[0, i]) * pose[0], (-C[1, i]) * pose[1], (-C[2, i]) * pose[2])  # :119, :124
    T[3, 3] = 1.0
    return T


def project(oracle, cam, heads):
    """PinholeCamera::project with the point Jacobian for every row of heads [n, 3]: (status [n], pt [n, 2], J23 [n, 6]);
    a singular depth (status 4 before anything is written) leaves NaN"""
    heads = np.asarray(heads, dtype=np.float64).reshape(-1, 3)
    n = len(heads)
    if cam.dist_type == 3:
        st, pt, J = radtan8_ref.project(cam, heads)
        st, pt, J = st.reshape(n).copy(), pt.reshape(n, 2).copy(), J.reshape(n, 6).copy()
    else:
        st, pt, J = np.zeros(n, np.int32), np.zeros((n, 2)), np.zeros((n, 6))
        for i in range(n):
            st[i], pt[i], J23 = oracle.cam_project(cam, heads[i], want_jac=True)
            J[i] = J23.reshape(-1)
    with np.errstate(all="ignore"):
        sing = np.abs(heads[:, 2]) < 1.0e-12                        # PinholeCamera.hpp:302-304
    pt[sing], J[sing] = np.nan, np.nan
    return st, pt, J


def terms(oracle, tree, cam, T_SW, t_WS, T_CS, hp_W, kps, census=None):
    """ReprojectionError.hpp:125-163 for n terms of one camera: hp_W [n, 4], kps [n] keypoint records.
    -> (residual [n, 2], J0_minimal [n, 12], singular [n] bool: the defined NaN rows)"""
    hp_W = np.asarray(hp_W, dtype=np.float64).reshape(-1, 4)
    n = len(hp_W)
    nan = np.float64(np.nan)
    with np.errstate(all="ignore"):
        hp_S = [sum4(tree, T_SW[i, 0] * hp_W[:, 0], T_SW[i, 1] * hp_W[:, 1], T_SW[i, 2] * hp_W[:, 2], T_SW[i, 3] * hp_W[:, 3])
                for i in range(4)]                                  # :125
        hp_C = [sum4(tree, T_CS[i, 0] * hp_S[0], T_CS[i, 1] * hp_S[1], T_CS[i, 2] * hp_S[2], T_CS[i, 3] * hp_S[3])
                for i in range(4)]                                  # :126
        neg = hp_C[3] < 0                                           # PinholeCamera.hpp:514
        head = np.stack([np.where(neg, -hp_C[i], hp_C[i]) for i in range(3)], axis=1)
        st, pt, J23 = project(oracle, cam, head)                    # the status is ignored (:133)
        zero = np.zeros(n)
        Jh = [[J23[:, 0], J23[:, 1], J23[:, 2], zero], [J23[:, 3], J23[:, 4], J23[:, 5], zero]]   # :523-524
        size = kps["size"].astype(np.float64)                       # Frontend.cpp:452-453
        s = np.sqrt(64.0 / (size * size))                           # Frontend.cpp:464, ReprojectionError.hpp:75-76
        S = [[s, zero], [zero, s]]
        Jw = [[S[i][0] * Jh[0][j] + S[i][1] * Jh[1][j] for j in range(4)] for i in range(2)]       # :134
        e = [kps["x"].astype(np.float64) - pt[:, 0], kps["y"].astype(np.float64) - pt[:, 1]]        # :139
        r = [S[i][0] * e[0] + S[i][1] * e[1] for i in range(2)]     # :142
        p = [hp_W[:, i] - t_WS[i] * hp_W[:, 3] for i in range(3)]   # :155
        X = [[zero, -p[2], p[1]], [p[2], zero, -p[0]], [-p[1], p[0], zero]]   # operators.hpp:60-73
        Jp = [[None] * 6 for _ in range(4)]
        for i in range(3):
            for j in range(3):
                Jp[i][j] = T_SW[i, j] * hp_W[:, 3]                  # :158
                Jp[i][3 + j] = sum3(tree, (-T_SW[i, 0]) * X[0][j], (-T_SW[i, 1]) * X[1][j], (-T_SW[i, 2]) * X[2][j])  # :159
        for j in range(6):
            Jp[3][j] = zero                                         # :157
        A = [[sum4(tree, Jw[i][0] * T_CS[0, j], Jw[i][1] * T_CS[1, j], Jw[i][2] * T_CS[2, j], Jw[i][3] * T_CS[3, j])
              for j in range(4)] for i in range(2)]                 # :163, the left product
        J0 = [sum4(tree, A[i][0] * Jp[0][j], A[i][1] * Jp[1][j], A[i][2] * Jp[2][j], A[i][3] * Jp[3][j])
              for i in range(2) for j in range(6)]
        singular_z = np.abs(head[:, 2]) < 1.0e-12
        bad_size = ~((size > 0.0) & (size < np.inf))
    singular = singular_z | bad_size                                # the defined deviation (okvfe.h)
    res = np.stack([np.broadcast_to(v, (n,)) for v in r], axis=1).copy() if n else np.zeros((0, 2))
    jac = np.stack([np.broadcast_to(v, (n,)) for v in J0], axis=1).copy() if n else np.zeros((0, 12))
    res[singular], jac[singular] = nan, nan
    if census is not None:
        census["term"] += n
        census["w_negative"] += int(neg.sum())
        census["singular_z"] += int(singular_z.sum())
        census["bad_size"] += int(bad_size.sum())
        live = ~singular_z
        census["behind"] += int((live & (st == 3)).sum())
        census["distortion_failure"] += int((live & (st == 4)).sum())
        out = live & (st == 1)
        with np.errstate(all="ignore"):
            census["outside_left"] += int((out & (pt[:, 0] < 0.0)).sum())
            census["outside_top"] += int((out & (pt[:, 1] < 0.0)).sum())
            census["outside_right"] += int((out & (pt[:, 0] >= float(cam.w))).sum())
            census["outside_bottom"] += int((out & (pt[:, 1] >= float(cam.h))).sum())
    return res, jac, singular


def term_rows(n_landmarks, n_kps, match_landmark, state, census=None):
    """the keypoints of one block that are terms, ascending: state == 2 and the row in [0, L)"""
    ml = np.asarray(match_landmark)[:n_kps]
    st = np.asarray(state)[:n_kps]
    inside = (ml >= 0) & (ml < n_landmarks)
    if census is not None:
        census["state_0"] += int((st == 0).sum())
        census["state_1"] += int((st == 1).sum())
        census["row_outside_set"] += int(((st == 2) & ~inside).sum())
    return np.flatnonzero((st == 2) & inside)


def evaluate(oracle, tree, hp, frames, match_landmark, state, cams, T_SC_params, pose, verified=True, census=None):
    """One multiframe.  frames: per camera dict(kps) (the gather block's rows below its count); match_landmark / state:
    per camera rows; T_SC_params: per camera (t[3], qx, qy, qz, qw); pose: T_Sold_Snew in the same layout.
    -> dict(H [6, 6], n_terms, n_singular, rows: per camera the term keypoints, residual: per camera [n_terms_c, 2],
    jacobian: per camera [n_terms_c, 12])"""
    hp = np.asarray(hp, dtype=np.float64).reshape(-1, 4)
    H = np.zeros((6, 6))
    out = dict(H=H, n_terms=0, n_singular=0, rows=[], residual=[], jacobian=[])
    if not verified:                                                # the reference has returned false (Frontend.cpp:389)
        if census is not None:
            census["not_verified"] += int(sum((np.asarray(s)[:len(f["kps"])] == 2).sum() for f, s in zip(frames, state)))
        for _ in frames:
            out["rows"].append(np.zeros(0, np.int64)), out["residual"].append(np.zeros((0, 2)))
            out["jacobian"].append(np.zeros((0, 12)))
        return out
    pose = np.asarray(pose, dtype=np.float64)
    T_SW = inverse_transform(tree, pose)                            # :120-124
    seen = []
    for c, fr in enumerate(frames):
        rows = term_rows(len(hp), len(fr["kps"]), match_landmark[c], state[c], census)
        lm = np.asarray(match_landmark[c])[rows]
        T_CS = inverse_transform(tree, T_SC_params[c])              # :115-119
        res, jac, sing = terms(oracle, tree, cams[c], T_SW, pose[:3], T_CS, hp[lm], fr["kps"][rows], census)
        with np.errstate(all="ignore"):
            for t in range(len(rows)):                              # Frontend.cpp:550, one term after the other
                J = jac[t].reshape(2, 6)
                H = H + (np.outer(J[0], J[0]) + np.outer(J[1], J[1]))
        out["rows"].append(rows), out["residual"].append(res), out["jacobian"].append(jac)
        out["n_terms"] += len(rows)
        out["n_singular"] += int(sing.sum())
        seen.append(lm)
    if census is not None:                                          # term rows whose landmark is a term of another camera too
        for a, lm in enumerate(seen):
            others = set().union(*[set(v.tolist()) for b, v in enumerate(seen) if b != a])
            census["landmark_in_two_cameras"] += int(sum(int(l) in others for l in lm))
    out["H"] = H
    return out


# ---- PoseManifold::plus, for central differences -------------------------------------------------------------------------
def _qmul(a, b):
    """Hamilton product of (x, y, z, w) quaternions"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def pose_plus(pose, delta):
    """PoseLocalParameterization.cpp:49-64: q' = (deltaQ(dalpha) q.normalized()).normalized(), t' = t + dt"""
    pose, delta = np.asarray(pose, dtype=np.float64), np.asarray(delta, dtype=np.float64)
    da = delta[3:]
    half = 0.5 * np.linalg.norm(da)
    sinc = np.sin(half) / half if half > 1.0e-12 else 1.0
    dq = np.append(sinc * 0.5 * da, np.cos(half))                   # Transformation.hpp:64-71
    q = pose[3:] / np.linalg.norm(pose[3:])
    q = _qmul(dq, q)
    return np.concatenate([pose[:3] + delta[:3], q / np.linalg.norm(q)])
