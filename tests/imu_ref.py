"""Reference of okvfe_imu_propagation and okvfe_imu_propagation_blocks_device: a plain numpy float64 restatement, from the
reference's sources, of

  ImuError::propagation       okvis_ceres/src/ImuError.cpp:557-779 (the loop :601-743, the epilogue :745-777)
  sinc, rightJacobian         okvis_kinematics implementation/Transformation.hpp:50-62 and :74-87 (ode::sinc is the same)
  Transformation              the same file: the constructor (:131-138), inverse (:207-210), set (:239-244), operator* (:261-264)
  crossMx                     okvis_kinematics operators.hpp:60-73
  Time - Time, toSec, <, ==   okvis_time implementation/Time.hpp:85-88, :120-131, Duration.hpp:57-62, Duration.cpp:55-73
  per camera                  ThreadedSlam.cpp:434-444 (T_WC = T_WS T_SC) and Frontend.cpp:246-251 (extractionDir)

Every product, sum, quotient and square root is a separate IEEE operation in the source's order, left to right, without
contraction.  3-term sums come in both orders of okvfe_set_fp64_reduction (ransac_ref.sum3), and so do the 4-term sums of
squaredNorm() (sum4); the quaternion product is Eigen's, each sum left to right (place_refine_ref.product).  The 15-term
sums of F_delta P_delta F_delta^T ((F P) first) and of T P_delta T^T run in ascending k from the first product, whatever
the switch says; the zeros are multiplied and added.  PARITY UNPINNED: Eigen's evaluation order of these expressions,
its products, normalized(), inverse() and toRotationMatrix() are restated from the published sources (Eigen is not in the
tree).

DEFINED DEVIATIONS (include/okvfe.h states them):
  * cos / sinc of theta_half and cos / sin of Phi in rightJacobian are cos_fixed, sinc_fixed and sin_fixed
    (elementary_ref), NaN beyond pi / 4; the NaN spreads, and n_out_of_range counts the intervals in which one of them was
    called outside its domain (a NaN argument included).  libm=True puts numpy's in their place, to record what they change.
  * the reference reads element it + 1 before it knows that it exists; here it is read only where it exists, and the
    iteration of the last element -- which no input with t_start < t_end reaches -- ends the loop.
  * t_end <= t_start: zero increments and i = 0 (what the reference's loop comes to apart from that read).
  * front().timeStamp > t_start (the reference's assertion) is status bit 1, an empty sample list status bit 2: nothing
    else is written for such a multiframe.
  * back().timeStamp < t_end: n_propagated = -1, pose and speed_and_bias are the inputs unchanged, F and P are untouched.

A timestamp is (uint32 sec, uint32 nsec).  A census counts the branches taken.  Test infrastructure only."""
import numpy as np

import elementary_ref as E
from place_refine_ref import normalized, product
from ransac_ref import sum3, sum4

CENSUS = ("skip_dt_nonpositive", "interp_end", "interp_start", "gyro_saturated", "gyro_unsaturated", "acc_saturated",
          "acc_unsaturated", "break_at_end", "return_minus_one", "t_end_le_t_start", "front_after_start", "empty",
          "sinc_quotient", "sinc_polynomial", "phi_small", "phi_large", "out_of_range", "interval", "last_element")
# Labels no scene reaches; tests/test_imu_ref.py asserts that they stay at zero:
#   last_element   with front <= t_start < t_end <= back the iteration before the last element's ends at t_end: its
#                  nexttime is back's timestamp, not later than t_end is not earlier either, so it breaks; it is not
#                  skipped, because `time` never passes t_end and equals it only after a break
UNREACHABLE = ("last_element",)

STATUS_FRONT_AFTER_START, STATUS_EMPTY = 1, 2
PARAM_NAMES = ("a_max", "g_max", "sigma_g_c", "sigma_a_c", "sigma_gw_c", "sigma_aw_c", "g")
C_6TH = np.float64(1.0) / np.float64(6.0)


def new_census():
    return dict.fromkeys(CENSUS, 0)


def _count(census, key, n=1):
    if census is not None:
        census[key] += n


# ---- okvis_time -------------------------------------------------------------------------------------------------------
def time_diff(a, b):
    """(a - b).toSec() of (sec, nsec) uint32 pairs: the Duration(int32, int32) constructor normalises"""
    i32 = lambda v: int(np.int32(np.uint32(v)))
    s, n = i32(a[0]) - i32(b[0]), i32(a[1]) - i32(b[1])
    while n > 1000000000:
        n -= 1000000000
        s += 1
    while n < 0:
        n += 1000000000
        s -= 1
    s = int(np.int64(s).astype(np.int32))
    with np.errstate(all="ignore"):
        return np.float64(s) + np.float64(1e-9) * np.float64(n)


def time_lt(a, b):
    return int(a[0]) < int(b[0]) or (int(a[0]) == int(b[0]) and int(a[1]) < int(b[1]))


def time_eq(a, b):
    return int(a[0]) == int(b[0]) and int(a[1]) == int(b[1])


# ---- Eigen ---------------------------------------------------------------------------------------------------------------
def to_rotation(q):
    """q.toRotationMatrix() of (x, y, z, w), not normalised first (Eigen/src/Geometry/Quaternion.h)"""
    x, y, z, w = (np.float64(v) for v in q)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]], dtype=np.float64)


def q_inverse(tree, q):
    """Eigen's inverse(): conjugate().coeffs() / squaredNorm() iff that is > 0, else zeros"""
    q = np.asarray(q, dtype=np.float64)
    n2 = sum4(tree, q[0] * q[0], q[1] * q[1], q[2] * q[2], q[3] * q[3])
    if n2 > 0:
        return np.array([-q[0], -q[1], -q[2], q[3]]) / n2
    return np.zeros(4)


def matvec(tree, M, v):
    return sum3(tree, M[:, 0] * v[0], M[:, 1] * v[1], M[:, 2] * v[2])


def matmul(tree, A, B):
    return sum3(tree, A[:, 0:1] * B[0:1, :], A[:, 1:2] * B[1:2, :], A[:, 2:3] * B[2:3, :])


def norm3(tree, v):
    return np.sqrt(sum3(tree, v[0] * v[0], v[1] * v[1], v[2] * v[2]))


def cross_mx(v):
    """operators.hpp:60-73"""
    z = np.float64(0.0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], dtype=np.float64)


def matmul15(A, B):
    """15-term sums in ascending k from the first product"""
    acc = A[:, 0:1] * B[0:1, :]
    for k in range(1, 15):
        acc = acc + A[:, k:k + 1] * B[k:k + 1, :]
    return acc


class _Fn:
    """the three elementary functions: the fixed sequences, or numpy's (libm=True)"""

    def __init__(self, libm):
        self.libm = libm

    def cos(self, x):
        return np.float64(np.cos(x)) if self.libm else np.float64(E.cos_fixed(x))

    def sin(self, x):
        return np.float64(np.sin(x)) if self.libm else np.float64(E.sin_fixed(x))

    def sinc(self, x):
        """-> (value, the quotient branch taken)"""
        if not self.libm:
            v, big = E.sinc_fixed(x)
            return np.float64(v), bool(big)
        if np.abs(x) > E.SINC_EDGE:
            return np.float64(np.sin(x)) / x, True
        return np.float64(E.sinc_fixed(x)[0]), False


def right_jacobian(tree, fn, phi_vec, census=None):
    """Transformation.hpp:74-87 -> (matrix, Phi outside the fixed functions' domain)"""
    Phi = norm3(tree, phi_vec)
    I = np.eye(3)
    Phi_x = cross_mx(phi_vec)
    Phi_x2 = matmul(tree, Phi_x, Phi_x)
    if Phi < 1.0e-4:
        _count(census, "phi_small")
        return I + (-0.5 * Phi_x + C_6TH * Phi_x2), False
    _count(census, "phi_large")
    Phi2 = Phi * Phi
    Phi3 = Phi2 * Phi
    a = (-(1.0 - fn.cos(Phi))) / Phi2
    b = (Phi - fn.sin(Phi)) / Phi3
    return I + (a * Phi_x + b * Phi_x2), not Phi <= E.PI_4


def propagation(tree, params, ts, gyro, acc, t_start, t_end, T_WS, speed_and_bias, want_jacobian=True,
                want_covariance=True, T_SC_params=(), libm=False, census=None):
    """One multiframe.  ts [n, 2] uint32 (sec, nsec), gyro / acc [n, 3], t_start / t_end (sec, nsec), T_WS 7 doubles in
    PoseParameterBlock layout (t[3], qx, qy, qz, qw), speed_and_bias 9, params: dict of PARAM_NAMES.
    -> dict(status, n_out_of_range, n_propagated, pose, speed_and_bias, jacobian, covariance, T_WC [n_cams, 7],
    gravity_C [n_cams, 3] float32); an entry is None where the call leaves the output untouched."""
    with np.errstate(all="ignore"):
        return _propagation(tree, params, np.asarray(ts).reshape(-1, 2), np.asarray(gyro, np.float64).reshape(-1, 3),
                            np.asarray(acc, np.float64).reshape(-1, 3), t_start, t_end, np.asarray(T_WS, np.float64),
                            np.asarray(speed_and_bias, np.float64), want_jacobian, want_covariance,
                            np.asarray(T_SC_params, np.float64).reshape(-1, 7), _Fn(libm), census)


def _propagation(tree, prm, ts, gyro, acc, t_start, t_end, T_WS, sb, want_jac, want_cov, T_SC, fn, census):
    P = {k: np.float64(prm[k]) for k in PARAM_NAMES}
    out = dict(status=0, n_out_of_range=0, n_propagated=None, pose=None, speed_and_bias=None, jacobian=None,
               covariance=None, T_WC=None, gravity_C=None)
    n = len(ts)
    if n == 0:
        _count(census, "empty")
        out["status"] = STATUS_EMPTY
        return out
    if time_lt(t_start, ts[0]):                                     # :570, the assertion
        _count(census, "front_after_start")
        out["status"] = STATUS_FRONT_AFTER_START
        return out
    if time_lt(ts[n - 1], t_end):                                   # :572
        _count(census, "return_minus_one")
        out.update(n_propagated=-1, pose=T_WS.copy(), speed_and_bias=sb.copy())
        _per_camera(tree, out, T_SC)
        return out
    r_0, q_WS_0 = T_WS[:3], T_WS[3:7]
    C_WS_0 = to_rotation(q_WS_0)
    Delta_q = np.array([0.0, 0.0, 0.0, 1.0])
    Z3, Zv = np.zeros((3, 3)), np.zeros(3)
    C_integral, C_doubleintegral, acc_integral, acc_doubleintegral = Z3, Z3, Zv, Zv
    cross, dalpha_db_g, dv_db_g, dp_db_g = Z3, Z3, Z3, Z3
    P_delta = np.zeros((15, 15))
    Delta_t = np.float64(0.0)
    has_started = False
    i = 0
    time = t_start
    n_oor = 0
    I3 = np.eye(3)
    loop = range(n)
    if not time_lt(t_start, t_end):
        _count(census, "t_end_le_t_start")
        loop = range(0)
    for it in loop:
        if it + 1 == n:
            _count(census, "last_element")
            break
        omega_S_0, acc_S_0 = gyro[it], acc[it]
        omega_S_1, acc_S_1 = gyro[it + 1], acc[it + 1]
        nexttime = ts[it + 1]
        dt = time_diff(nexttime, time)
        if time_lt(t_end, nexttime):                                # :618
            _count(census, "interp_end")
            interval = time_diff(nexttime, ts[it])
            nexttime = t_end
            dt = time_diff(nexttime, time)
            r = dt / interval
            omega_S_1 = (1.0 - r) * omega_S_0 + r * omega_S_1
            acc_S_1 = (1.0 - r) * acc_S_0 + r * acc_S_1
        if dt <= 0.0:
            _count(census, "skip_dt_nonpositive")
            continue
        Delta_t = Delta_t + dt
        if not has_started:                                         # :632
            _count(census, "interp_start")
            has_started = True
            r = dt / time_diff(nexttime, ts[it])
            omega_S_0 = r * omega_S_0 + (1.0 - r) * omega_S_1
            acc_S_0 = r * acc_S_0 + (1.0 - r) * acc_S_1
        _count(census, "interval")
        sigma_g_c, sigma_a_c = P["sigma_g_c"], P["sigma_a_c"]
        if bool(np.any(np.abs(omega_S_0) > P["g_max"]) or np.any(np.abs(omega_S_1) > P["g_max"])):
            sigma_g_c = sigma_g_c * 100.0
            _count(census, "gyro_saturated")
        else:
            _count(census, "gyro_unsaturated")
        if bool(np.any(np.abs(acc_S_0) > P["a_max"]) or np.any(np.abs(acc_S_1) > P["a_max"])):
            sigma_a_c = sigma_a_c * 100.0
            _count(census, "acc_saturated")
        else:
            _count(census, "acc_unsaturated")
        # orientation (:664-671)
        omega_S_true = 0.5 * (omega_S_0 + omega_S_1) - sb[3:6]
        theta_half = (norm3(tree, omega_S_true) * 0.5) * dt
        sinc_theta_half, big = fn.sinc(theta_half)
        _count(census, "sinc_quotient" if big else "sinc_polynomial")
        cos_theta_half = fn.cos(theta_half)
        oor = not theta_half <= E.PI_4
        dq = np.append(((sinc_theta_half * omega_S_true) * 0.5) * dt, cos_theta_half)
        Delta_q_1 = product(Delta_q, dq)
        # rotation matrix integrals (:673-680)
        C = to_rotation(Delta_q)
        C_1 = to_rotation(Delta_q_1)
        acc_S_true = 0.5 * (acc_S_0 + acc_S_1) - sb[6:9]
        CC = C + C_1
        C_integral_1 = C_integral + (0.5 * CC) * dt
        half_acc = matvec(tree, 0.5 * CC, acc_S_true) * dt
        acc_integral_1 = acc_integral + half_acc
        quarter_acc = (matvec(tree, 0.25 * CC, acc_S_true) * dt) * dt
        C_doubleintegral = C_doubleintegral + (C_integral * dt + ((0.25 * CC) * dt) * dt)
        acc_doubleintegral = acc_doubleintegral + (acc_integral * dt + quarter_acc)
        # Jacobian parts (:683-688)
        dalpha_db_g = dalpha_db_g + dt * C_1
        rj, oor_phi = right_jacobian(tree, fn, omega_S_true * dt, census)
        oor = oor or oor_phi
        cross_1 = matmul(tree, to_rotation(q_inverse(tree, dq)), cross) + rj * dt
        acc_S_x = cross_mx(acc_S_true)
        S = matmul(tree, matmul(tree, C, acc_S_x), cross) + matmul(tree, matmul(tree, C_1, acc_S_x), cross_1)
        dv_db_g_1 = dv_db_g + (0.5 * dt) * S
        dp_db_g = dp_db_g + (dt * dv_db_g + ((0.25 * dt) * dt) * S)
        if oor:
            n_oor += 1
            _count(census, "out_of_range")
        if want_cov:                                                # :691-728
            F_delta = np.eye(15)
            F_delta[0:3, 3:6] = -cross_mx(acc_integral * dt + quarter_acc)
            F_delta[0:3, 6:9] = I3 * dt
            F_delta[0:3, 9:12] = dt * dv_db_g + ((0.25 * dt) * dt) * S
            F_delta[0:3, 12:15] = (-C_integral) * dt + ((0.25 * CC) * dt) * dt
            F_delta[3:6, 9:12] = (-dt) * C_1
            F_delta[6:9, 3:6] = -cross_mx(half_acc)
            F_delta[6:9, 9:12] = (0.5 * dt) * S
            F_delta[6:9, 12:15] = (-0.5 * CC) * dt
            P_delta = matmul15(matmul15(F_delta, P_delta), F_delta.T)
            sigma2_dalpha = (dt * sigma_g_c) * sigma_g_c
            sigma2_v = (dt * sigma_a_c) * P["sigma_a_c"]
            sigma2_p = ((0.5 * dt) * dt) * sigma2_v
            sigma2_b_g = (dt * P["sigma_gw_c"]) * P["sigma_gw_c"]
            sigma2_b_a = (dt * P["sigma_aw_c"]) * P["sigma_aw_c"]
            for b, s2 in ((3, sigma2_dalpha), (6, sigma2_v), (0, sigma2_p), (9, sigma2_b_g), (12, sigma2_b_a)):
                for e in range(b, b + 3):
                    P_delta[e, e] = P_delta[e, e] + s2
        # memory shift (:731-741)
        Delta_q, C_integral, acc_integral, cross, dv_db_g = Delta_q_1, C_integral_1, acc_integral_1, cross_1, dv_db_g_1
        time = nexttime
        i += 1
        if time_eq(nexttime, t_end):
            _count(census, "break_at_end")
            break
    # the epilogue (:745-777)
    z = np.array([0.0, 0.0, 6371009.0])
    n2 = sum3(tree, z[0] * z[0], z[1] * z[1], z[2] * z[2])
    g_W = P["g"] * (z / np.sqrt(n2))
    r_new = ((r_0 + sb[0:3] * Delta_t) + matvec(tree, C_WS_0, acc_doubleintegral)) - ((0.5 * g_W) * Delta_t) * Delta_t
    q_new = normalized(tree, product(q_WS_0, Delta_q))
    sb_new = sb.copy()
    sb_new[0:3] = sb[0:3] + (matvec(tree, C_WS_0, acc_integral) - g_W * Delta_t)
    out.update(n_propagated=i, n_out_of_range=n_oor, pose=np.concatenate([r_new, q_new]), speed_and_bias=sb_new)
    if want_jac:
        F = np.eye(15)
        F[0:3, 3:6] = -cross_mx(matvec(tree, C_WS_0, acc_doubleintegral))
        F[0:3, 6:9] = I3 * Delta_t
        F[0:3, 9:12] = matmul(tree, C_WS_0, dp_db_g)
        F[0:3, 12:15] = matmul(tree, -C_WS_0, C_doubleintegral)
        F[3:6, 9:12] = matmul(tree, -C_WS_0, dalpha_db_g)
        F[6:9, 3:6] = -cross_mx(matvec(tree, C_WS_0, acc_integral))
        F[6:9, 9:12] = matmul(tree, C_WS_0, dv_db_g)
        F[6:9, 12:15] = matmul(tree, -C_WS_0, C_integral)
        out["jacobian"] = F
    if want_cov:
        T = np.eye(15)
        T[0:3, 0:3] = T[3:6, 3:6] = T[6:9, 6:9] = C_WS_0
        out["covariance"] = matmul15(matmul15(T, P_delta), T.T)
    _per_camera(tree, out, T_SC)
    return out


def _per_camera(tree, out, T_SC):
    out["T_WC"], out["gravity_C"] = per_camera(tree, out["pose"], T_SC)


def per_camera(tree, pose, T_SC):
    """T_WC = T_WS * T_SC (operator*, whose constructor normalises) and extractionDir = T_WC.inverse().C() * (0, 0, -1)
    as float32, from the pose the call returns -> (T_WC [n_cams, 7], gravity_C [n_cams, 3] float32)"""
    pose = np.asarray(pose, dtype=np.float64)
    T_SC = np.asarray(T_SC, dtype=np.float64).reshape(-1, 7)
    C_WS = to_rotation(pose[3:7])
    T_WC, grav = np.zeros((len(T_SC), 7)), np.zeros((len(T_SC), 3), np.float32)
    for c, sc in enumerate(T_SC):
        with np.errstate(all="ignore"):
            r = matvec(tree, C_WS, sc[0:3]) + pose[0:3]
            q = normalized(tree, product(pose[3:7], sc[3:7]))
            T_WC[c] = np.concatenate([r, q])
            C_inv = to_rotation(normalized(tree, q_inverse(tree, q)))
            grav[c] = matvec(tree, C_inv, np.array([0.0, 0.0, -1.0])).astype(np.float32)
    return T_WC, grav


# ---- the manifold of the state, for the central differences of tests/test_imu_ref.py --------------------------------------
def oplus(pose, delta):
    """PoseLocalParameterization::plus on (t, q): t + dt, deltaQ(dalpha) * q"""
    from place_hessian_ref import pose_plus
    return pose_plus(pose, delta)


def ominus(pose_a, pose_b):
    """the 6 minimal coordinates d with oplus(pose_b, d) = pose_a, to first order: (t_a - t_b, 2 vec(q_a q_b^-1))"""
    from place_hessian_ref import _qmul
    qa, qb = pose_a[3:7] / np.linalg.norm(pose_a[3:7]), pose_b[3:7] / np.linalg.norm(pose_b[3:7])
    dq = _qmul(qa, np.array([-qb[0], -qb[1], -qb[2], qb[3]]))
    if dq[3] < 0:
        dq = -dq
    return np.concatenate([pose_a[0:3] - pose_b[0:3], 2.0 * dq[0:3]])
