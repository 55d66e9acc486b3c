"""Scenes for okvfe_ransac2d2d_consensus_blocks_device (the consensus of Frontend::runRansac2d2d on device batches).

A scene is dict(name, cams, pairs, added, n_landmarks): `cams` fill the camera slots 0 .. n_cams - 1 of a context of
K = ransac_scenes.K keypoints; pair p holds per camera dict(fr0, fr1, rot_H, rot_valid, rel_H, rel_valid), fr0 the
older and fr1 the current block's rows below its count (kps, desc, bp, bpv, lm).  All pairs of a scene have the same
number of hypotheses.

  general_scene     rigs of 1, 2 and 5 cameras over the camera models (ransac_scenes' camera / rig / backproject): per rig
                    a pure rotation, a translation with parallax and a mix with 30 % wrong ids; 50 hypotheses per problem
  directed_scene    every census label of ransac2d2d_ref at least 16 times
  decision_scene    hand-set (n, rotation inliers, relative inliers) per camera, and the two-camera orderings
  knife_rotation / knife_relative   the threshold 9 bisected to adjacent values
  chunk_scene       chunk - 1, chunk, chunk + 1 and 2 chunk + 1 correspondences
  edge_scene        counts 0, 1 and K (every packed scene carries a valid id at or past the count)
  ring_scene / ring_restart_scene / full_table_scene / collision_scene   for contexts of 1100 keypoints and of the
                    call's limit: whole laps of the kernel's record ring (restarted per camera), its id table with one
                    empty slot, probe runs across the table's end, duplicate ids inside them

The hand-set scenes place bearings directly (a block's back-projections are data).  With the rotation hypothesis R and
the relative hypothesis [R | t], a correspondence is of one of four kinds:
  C  a point 1000 baselines away: an inlier of both;   B  a point 20 baselines away: parallax, an inlier of [R | t] only;
  A  a small parallax of the WRONG sign: within the rotation's threshold, triangulated behind the cameras;
  D  the current bearing turned 0.3 rad out of the epipolar plane: an outlier of both.
CPU only up to `prepare` / `launch`, which need torch and a GPU.  Test infrastructure only."""
import numpy as np

import ransac2d2d_ref as R2
import ransac_ref as R
import ransac_scenes as S
from gate_scenes import bisect_adjacent, rodrigues

K = S.K
SENTINEL, STATE_SENTINEL, DIST_SENTINEL = S.SENTINEL, S.STATE_SENTINEL, S.DIST_SENTINEL
N_LANDMARKS = 6000   # the size of the isLandmarkAdded table of the scenes that have one


def _kps(oracle, n, rng, size=12.0):
    kps = np.zeros(n, dtype=oracle.KEYPOINT_DTYPE)
    kps["x"], kps["y"] = rng.uniform(20, 700, n), rng.uniform(20, 400, n)
    kps["size"] = size
    return kps


def _frame(oracle, n, rng, bp=None, lm=None):
    return dict(kps=_kps(oracle, n, rng), desc=np.zeros((n, 48), np.uint8),
                bp=np.zeros((n, 3)) if bp is None else np.asarray(bp, dtype=np.float64).reshape(n, 3),
                bpv=np.ones(n, np.uint8), lm=np.full(n, -1, np.int32) if lm is None else np.asarray(lm, np.int32))


def empty_frame(oracle):
    return _frame(oracle, 0, np.random.default_rng(0))


def rot_matrix(Rm):
    return np.asarray(Rm, dtype=np.float64).reshape(9)


def rel_matrix(Rm, t):
    return np.concatenate([np.asarray(Rm, dtype=np.float64).reshape(3, 3), np.asarray(t, dtype=np.float64).reshape(3, 1)],
                          axis=1).reshape(12)


FAR_R = rodrigues((1.0, 0.3, -0.2), 2.0)
TRUE_R = rodrigues((0.2, 1.0, 0.1), 0.05)
TRUE_T = np.array([0.1, 0.01, -0.005])


def hand_camera(oracle, rng, nC, nA, nB, nD, free0=3, free1=4, Rm=TRUE_R, t=TRUE_T, id_base=0):
    """(fr0, fr1, kinds): nC + nA + nB + nD matched keypoints of the four kinds in shuffled rows of both blocks, plus
    free0 / free1 keypoints without an id; kinds[kA] names the kind of older row kA ('-' = free)"""
    n = nC + nA + nB + nD
    kinds = rng.permutation(np.array(list("C" * nC + "A" * nA + "B" * nB + "D" * nD)))
    b = np.linalg.norm(t)
    axis = t / b
    d = np.stack([rng.uniform(-0.4, 0.4, n), rng.uniform(-0.4, 0.4, n), np.ones(n)], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    depth = np.where(kinds == "C", 1000.0 * b * rng.uniform(1, 2, n), np.where(kinds == "A", 500.0 * b, 20.0 * b))
    P = d * depth[:, None]
    Q = np.where((kinds == "A")[:, None], P + t, P - t)
    turn = rodrigues(axis, 0.3)
    Q[kinds == "D"] = P[kinds == "D"] @ turn.T
    p2 = Q @ Rm                                   # R^T q, row-wise
    b1 = d * rng.uniform(0.5, 2.0, (n, 1))        # stored back-projections are not normalised
    b2 = p2 / np.linalg.norm(p2, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (n, 1))
    ids = id_base + 3 + 7 * np.arange(n)
    rows0, rows1 = rng.permutation(n + free0)[:n], rng.permutation(n + free1)[:n]
    fr0, fr1 = _frame(oracle, n + free0, rng), _frame(oracle, n + free1, rng)
    fr0["bp"][:] = rng.normal(size=(n + free0, 3))
    fr1["bp"][:] = rng.normal(size=(n + free1, 3))
    fr0["bp"][rows0], fr0["lm"][rows0] = b1, ids
    fr1["bp"][rows1], fr1["lm"][rows1] = b2, ids
    names = np.full(n + free0, "-")
    names[rows0] = kinds
    return fr0, fr1, names


def hand_counts(n, rot, rel):
    """(nC, nA, nB, nD) with rot = nC + nA inliers of R, rel = nC + nB inliers of [R | t] among n"""
    c = min(rot, rel)
    a, b = rot - c, rel - c
    assert n - c - a - b >= 0, (n, rot, rel)
    return c, a, b, n - c - a - b


def lists(kind):
    """(rot_H, rel_H) of two hypotheses"""
    true, far = (rot_matrix(TRUE_R), rel_matrix(TRUE_R, TRUE_T)), (rot_matrix(FAR_R), rel_matrix(FAR_R, TRUE_T))
    a, b = {"true first": (true, far), "twice": (true, true), "better later": (far, true), "far": (far, far)}[kind]
    return np.array([a[0], b[0]]), np.array([a[1], b[1]])


def cam_entry(fr0, fr1, rot_H, rel_H, rot_valid=None, rel_valid=None, **extra):
    return dict(fr0=fr0, fr1=fr1, rot_H=np.ascontiguousarray(rot_H, dtype=np.float64),
                rel_H=np.ascontiguousarray(rel_H, dtype=np.float64), rot_valid=rot_valid, rel_valid=rel_valid, **extra)


def empty_entry(oracle, nh, valid=None):
    return cam_entry(empty_frame(oracle), empty_frame(oracle), np.tile(rot_matrix(np.eye(3)), (nh, 1)),
                     np.tile(rel_matrix(np.eye(3), (1, 0, 0)), (nh, 1)), valid, valid)


def scene(name, cams, pairs, added=None):
    return dict(name=name, cams=cams, pairs=pairs, added=added, n_landmarks=0 if added is None else len(added))


def euroc_pair():
    return S.rig(("euroc", "euroc1"))[0]


# ---- the decision table ------------------------------------------------------------------------------------------
DECISION_CASES = ((9, 9, 9), (10, 10, 0), (11, 11, 0), (10, 8, 8), (15, 12, 12), (20, 16, 16), (20, 17, 18),
                  (20, 12, 17), (20, 12, 16), (20, 0, 0))
# (n, rot, rel) -> (branch, success bits, total_inliers, rotation_only)
DECISION_EXPECT = {(9, 9, 9): (0, 0, -1, 1), (10, 10, 0): (1, 0, -1, 1), (11, 11, 0): (1, 1, 11, 1),
                   (10, 8, 8): (2, 0, -1, 1), (15, 12, 12): (2, 0, -1, 1), (20, 16, 16): (2, 0, -1, 1),
                   (20, 17, 18): (1, 1, 17, 1), (20, 12, 17): (2, 2, 17, 0), (20, 12, 16): (2, 0, -1, 1),
                   (20, 0, 0): (2, 0, -1, 1)}
# two cameras: success then failure (the second camera still removes), failure then success (the first does not)
ORDER_CASES = (((20, 17, 18), (20, 12, 16)), ((20, 12, 16), (20, 12, 17)))
ORDER_EXPECT = (dict(removed=[1, 1], total=17 + 16, rotation_only=1, success=1),
                dict(removed=[0, 1], total=16 + 17, rotation_only=0, success=2))


def decision_scene(oracle, kind="true first", invalid=False, seed=21):
    """one pair per DECISION_CASES entry (camera 1 empty), then the ORDER_CASES pairs; the hypothesis lists of `kind`"""
    rng = np.random.default_rng(seed)
    rot_H, rel_H = lists(kind)
    valid = np.zeros(2, np.uint8) if invalid else None
    pairs = []
    for case in DECISION_CASES:
        fr0, fr1, names = hand_camera(oracle, rng, *hand_counts(*case))
        pairs.append([cam_entry(fr0, fr1, rot_H, rel_H, valid, valid, names=names), empty_entry(oracle, 2, valid)])
    for two in ORDER_CASES:
        pair = []
        for case in two:
            fr0, fr1, names = hand_camera(oracle, rng, *hand_counts(*case))
            pair.append(cam_entry(fr0, fr1, rot_H, rel_H, valid, valid, names=names))
        pairs.append(pair)
    return scene("decision-" + kind.replace(" ", "-") + ("-invalid" if invalid else ""), euroc_pair(), pairs)


# ---- the directed scene ------------------------------------------------------------------------------------------
DIRECTED_COPIES = 16


def _direct(oracle, rng, fr0, fr1, names):
    """the adapter's special rows on top of a hand camera with at least three D rows.  The rows that change are D rows
    (outliers before and after), so the inlier counts stay: one more outlier correspondence (a second older keypoint
    on a C landmark), one on a not-added id and one on an id outside the table dropped from the current block's map."""
    D = np.flatnonzero(names == "D")
    Cs = np.flatnonzero(names == "C")
    assert len(D) >= 3
    row1 = {int(l): k for k, l in enumerate(fr1["lm"]) if l >= 0}
    fr0["bpv"][D[0]] = 0                                   # bp_invalid_0
    fr1["bpv"][row1[int(fr0["lm"][D[1]])]] = 0             # bp_invalid_1
    kB = row1[int(fr0["lm"][D[2]])]                        # parallel bearings: b1 == b2 bitwise, [I | t] in the list
    fr1["bp"][kB] = fr0["bp"][D[2]]
    extra0 = _frame(oracle, 3, rng, bp=rng.normal(size=(3, 3)))
    extra0["lm"][:] = [fr0["lm"][Cs[0]] if len(Cs) else fr0["lm"][D[0]],  # two_older_on_one_landmark (shared_kB_mixed)
                       N_LANDMARKS - 5,                    # its id is not added
                       N_LANDMARKS + 9]                    # its id is outside the table
    extra1 = _frame(oracle, 3, rng, bp=rng.normal(size=(3, 3)))
    extra1["lm"][:] = [fr1["lm"][np.flatnonzero(fr1["lm"] >= 0)[0]],      # duplicate_id_in_current: the later k is ignored
                       N_LANDMARKS - 5, N_LANDMARKS + 9]
    cat = lambda a, b: {k: np.concatenate([a[k], b[k]]) for k in a}
    return cat(fr0, extra0), cat(fr1, extra1)


def directed_scene(oracle, seed=3):
    """DIRECTED_COPIES x three two-camera pairs:
      1: rotation taken through 0.8 with success | relative taken, fails itself, removes (sticky)
      2: rotation taken by ratio with success    | lists without an inlier: no winner, everything removed
      3: fewer than 10 correspondences: skipped  | relative taken with success"""
    rng = np.random.default_rng(seed)
    added = np.ones(N_LANDMARKS, np.uint8)
    added[N_LANDMARKS - 5] = 0
    true3 = (np.array([rot_matrix(TRUE_R), rot_matrix(np.eye(3)), rot_matrix(FAR_R)]),
             np.array([rel_matrix(TRUE_R, TRUE_T), rel_matrix(np.eye(3), TRUE_T), rel_matrix(FAR_R, TRUE_T)]))
    far3 = (np.array([rot_matrix(FAR_R)] * 3), np.array([rel_matrix(FAR_R, TRUE_T), rel_matrix(np.eye(3), TRUE_T),
                                                         rel_matrix(FAR_R, -TRUE_T)]))
    plan = ((((34, 1, 2, 3), true3), ((22, 0, 8, 10), true3)),
            (((10, 20, 0, 10), true3), ((0, 0, 0, 20), far3)),
            (((2, 0, 0, 3), true3), ((30, 0, 6, 4), true3)))
    pairs = []
    for copy in range(DIRECTED_COPIES):
        for pi, two in enumerate(plan):
            pair = []
            for ci, (counts, (rot_H, rel_H)) in enumerate(two):
                fr0, fr1, names = hand_camera(oracle, rng, *counts, id_base=100 * (copy % 7))
                fr0, fr1 = _direct(oracle, rng, fr0, fr1, names)
                pair.append(cam_entry(fr0, fr1, rot_H, rel_H))
            pairs.append(pair)
    return scene("directed", euroc_pair(), pairs, added)


# ---- knife edges -------------------------------------------------------------------------------------------------
def _probe_rows(fr0, fr1, names):
    kA = int(np.flatnonzero(names == "D")[0])
    kB = int(np.flatnonzero(fr1["lm"] == fr0["lm"][kA])[0])
    return kA, kB


def knife_rotation(oracle, tree, seed=12):
    """12 exact correspondences + two copies of a probe 5e-3 rad off, whose older keypoints have adjacent float32
    sizes between which the rotation-only distance goes from >= 9 to < 9; the relative list has no inlier"""
    rng = np.random.default_rng(seed)
    cams = euroc_pair()[:1]
    fr0, fr1, names = hand_camera(oracle, rng, 12, 0, 0, 2, free0=0, free1=0)
    rot_H, rel_H = rot_matrix(TRUE_R)[None], rel_matrix(FAR_R, TRUE_T)[None]
    probes = np.flatnonzero(names == "D")
    for kA in probes:
        kB = int(np.flatnonzero(fr1["lm"] == fr0["lm"][kA])[0])
        b1 = fr0["bp"][probes[0]] / np.linalg.norm(fr0["bp"][probes[0]])
        off = rodrigues(np.cross(b1, (0.0, 0.0, 1.0)) / np.linalg.norm(np.cross(b1, (0.0, 0.0, 1.0))), 5.0e-3)
        fr0["bp"][kA], fr1["bp"][kB] = b1, TRUE_R.T @ (off @ b1)

    def inlier(size):
        f = dict(fr0, kps=fr0["kps"].copy())
        f["kps"]["size"][probes[0]] = size
        corr = R2.correspondences(tree, f, fr1, cams[0].fu)
        return bool(R2.rotation_distances(tree, rot_H, corr)[0, list(corr["kA"]).index(probes[0])] < R2.THRESHOLD)

    assert inlier(np.float32(12.0)) and not inlier(np.float32(6.0))
    lo, hi = bisect_adjacent(inlier, np.float32(6.0), np.float32(12.0), dtype=np.float32)
    fr0["kps"]["size"][probes[0]], fr0["kps"]["size"][probes[1]] = lo, hi
    return scene("knife-rotation", cams, [[cam_entry(fr0, fr1, rot_H, rel_H, probes=probes)]])


def knife_relative(oracle, tree, seed=11):
    """12 exact correspondences with parallax + a probe 9e-3 rad out of its epipolar plane; two relative hypotheses,
    adjacent doubles apart in t[1], between which the probe's distance goes from < 9 to not; the rotation list has no
    inlier"""
    rng = np.random.default_rng(seed)
    cams = euroc_pair()[:1]
    fr0, fr1, names = hand_camera(oracle, rng, 0, 0, 12, 1, free0=0, free1=0)
    kA, kB = _probe_rows(fr0, fr1, names)
    b1 = fr0["bp"][kA] / np.linalg.norm(fr0["bp"][kA])
    P = b1 * 2.0
    q = rodrigues(TRUE_T / np.linalg.norm(TRUE_T), 9.0e-3) @ (P - TRUE_T)
    fr1["bp"][kB] = TRUE_R.T @ q
    rot_H = np.array([rot_matrix(FAR_R)] * 2)

    def hyp(ty):
        return rel_matrix(TRUE_R, np.array([TRUE_T[0], ty, TRUE_T[2]]))

    def inlier(ty):
        corr = R2.correspondences(tree, fr0, fr1, cams[0].fu)
        return bool(R2.relative_distances(tree, hyp(ty)[None], corr)[0, list(corr["kA"]).index(kA)] < R2.THRESHOLD)

    assert inlier(TRUE_T[1])
    far = next(ty for ty in (0.0105, 0.0095, 0.011, 0.009, 0.012, 0.008, 0.014, 0.006, 0.02, 0.001) if not inlier(ty))
    lo, hi = bisect_adjacent(inlier, TRUE_T[1], far)
    first, second = (lo, hi) if inlier(lo) else (hi, lo)
    return scene("knife-relative", cams, [[cam_entry(fr0, fr1, rot_H, np.array([hyp(first), hyp(second)]), probe=kA)]])


# ---- chunk and block edges ---------------------------------------------------------------------------------------
def chunk_scene(oracle, chunk, seed=31):
    """one camera; pairs with exactly chunk - 1, chunk, chunk + 1 and 2 chunk + 1 correspondences"""
    assert 2 * chunk + 1 <= K, "the contexts' K no longer spans two chunks: raise ransac_scenes.K"
    rng = np.random.default_rng(seed)
    rot_H, rel_H = lists("true first")
    pairs = []
    for total in (chunk - 1, chunk, chunk + 1, 2 * chunk + 1):
        nD = total // 8
        nB = total // 3
        fr0, fr1, _ = hand_camera(oracle, rng, total - nD - nB, 0, nB, nD, free0=min(9, K - total), free1=min(5, K - total))
        pairs.append([cam_entry(fr0, fr1, rot_H, rel_H)])
    return scene("chunks", euroc_pair()[:1], pairs)


def edge_scene(oracle, seed=41):
    """counts (older, current): (0, 40), (40, 0), (1, 1), (K, K)"""
    rng = np.random.default_rng(seed)
    rot_H, rel_H = lists("true first")
    fr0, fr1, _ = hand_camera(oracle, rng, 30, 0, 5, 2)
    one0, one1, _ = hand_camera(oracle, rng, 1, 0, 0, 0, free0=0, free1=0)
    full0, full1, _ = hand_camera(oracle, rng, K - 40, 0, 20, 20, free0=0, free1=0)
    e = empty_frame(oracle)
    pairs = [[cam_entry(e, fr1, rot_H, rel_H)], [cam_entry(fr0, e, rot_H, rel_H)], [cam_entry(one0, one1, rot_H, rel_H)],
             [cam_entry(full0, full1, rot_H, rel_H)]]
    return scene("edges", euroc_pair()[:1], pairs)


# ---- general scenes ----------------------------------------------------------------------------------------------
GENERAL_SPECS = S.GENERAL_SPECS
spec_id = S.spec_id
PAIR_KINDS = ("rotation", "translation", "mix")


def _relative(T0, T1):
    """(R12, t12): p_C0 = R12 p_C1 + t12"""
    C0, r0 = np.asarray(T0[0]).reshape(3, 3), np.asarray(T0[1])
    C1, r1 = np.asarray(T1[0]).reshape(3, 3), np.asarray(T1[1])
    return C0.T @ C1, C0.T @ (r1 - r0)


def _unit(t):
    n = np.linalg.norm(t)
    return t / n if n > 1.0e-12 else np.array([1.0, 0.0, 0.0])


def _hypotheses(R12, t12, n, rng, n_random=10):
    """the true model (a unit translation, as a five-point solver returns it), perturbed copies and random ones"""
    rot, rel = [rot_matrix(R12)], [rel_matrix(R12, _unit(t12))]
    while len(rot) < n:
        if len(rot) >= n - n_random:
            Rm = rodrigues(rng.normal(size=3), rng.uniform(0, np.pi))
            rot.append(rot_matrix(Rm)), rel.append(rel_matrix(Rm, _unit(rng.normal(size=3))))
        else:
            s = rng.random()
            Rm = R12 @ rodrigues(rng.normal(size=3), np.deg2rad(0.6) * s)
            rot.append(rot_matrix(Rm)), rel.append(rel_matrix(Rm, _unit(_unit(t12) + 0.1 * s * rng.normal(size=3))))
    order = rng.permutation(n)
    return np.array(rot)[order], np.array(rel)[order]


def _general_camera(oracle, cam, T0, T1, n0, rng, wrong, empty=False):
    if empty:
        return empty_frame(oracle), empty_frame(oracle)
    R12, t12 = _relative(T0, T1)
    kps0 = np.zeros(n0, dtype=oracle.KEYPOINT_DTYPE)
    kps0["x"], kps0["y"] = rng.uniform(20, cam.w - 20, n0), rng.uniform(20, cam.h - 20, n0)
    kps0["size"] = rng.choice(np.array([12.0, 18.0, 24.0], np.float32), n0, p=[0.8, 0.1, 0.1])
    bp0, bpv0 = S.backproject(oracle, cam, kps0)
    ids = rng.permutation(N_LANDMARKS - 100)[:n0].astype(np.int32)
    depth = rng.uniform(2.0, 8.0, n0)
    rows = []
    for k in range(n0):
        if not bpv0[k]:
            continue
        p0 = bp0[k] / np.linalg.norm(bp0[k]) * depth[k]
        st, px = R.project(oracle, cam, R12.T @ (p0 - t12))
        if st == 0:
            rows.append((px[0] + rng.normal(0, 0.3), px[1] + rng.normal(0, 0.3), ids[k]))
    rows = [rows[i] for i in rng.permutation(len(rows))][:K - 8]
    clutter = int(rng.integers(0, 8))
    n1 = len(rows) + clutter
    kps1 = np.zeros(n1, dtype=oracle.KEYPOINT_DTYPE)
    kps1["x"][:len(rows)], kps1["y"][:len(rows)] = [r[0] for r in rows], [r[1] for r in rows]
    kps1["x"][len(rows):], kps1["y"][len(rows):] = rng.uniform(20, cam.w - 20, clutter), rng.uniform(20, cam.h - 20, clutter)
    kps1["size"] = rng.choice(np.array([12.0, 18.0, 24.0], np.float32), n1, p=[0.8, 0.1, 0.1])
    lm1 = np.full(n1, -1, np.int32)
    lm1[:len(rows)] = [r[2] for r in rows]
    u = rng.random(n1)
    swap = (u < wrong) & (lm1 >= 0)
    lm1[swap] = rng.choice(ids, int(swap.sum()))          # another keypoint's id: a wrong match, at times a duplicate
    lm1[(u >= wrong) & (u < wrong + 0.05)] = -1
    bp1, bpv1 = S.backproject(oracle, cam, kps1)
    lm0 = ids.copy()
    lm0[rng.random(n0) < 0.05] = -1
    fr0 = dict(kps=kps0, desc=np.zeros((n0, 48), np.uint8), bp=bp0, bpv=bpv0, lm=lm0)
    fr1 = dict(kps=kps1, desc=np.zeros((n1, 48), np.uint8), bp=bp1, bpv=bpv1, lm=lm1)
    return fr0, fr1


def general_scene(oracle, spec, seed=3, n_hyp=50):
    """three pairs of a rig: a pure rotation of the sensor, a translation with parallax, the same with 30 % of the
    current ids swapped.  (seed: one for which the reference ends four pairs in each of the three outcomes)"""
    cams, T_SC = S.rig(spec)
    rng = np.random.default_rng([seed, len(cams), n_hyp, 2])
    T_WS0 = (rodrigues((0.3, 0.2, 1.0), 0.4), np.array([1.0, -2.0, 0.5]))
    moves = {"rotation": (rodrigues((0.1, 1.0, 0.2), 0.06), np.zeros(3)),
             "translation": (rodrigues((1.0, 0.2, 0.0), 0.02), np.array([0.25, 0.05, -0.1])),
             "mix": (rodrigues((0.0, 0.3, 1.0), 0.03), np.array([-0.2, 0.1, 0.05]))}
    pairs = []
    for pi, kind in enumerate(PAIR_KINDS):
        dR, dt = moves[kind]
        T_WS1 = (T_WS0[0] @ dR, T_WS0[1] + T_WS0[0] @ dt)
        pair = []
        for c, cam in enumerate(cams):
            T0 = S.compose((T_WS0[0].reshape(-1), T_WS0[1]), T_SC[c])
            T1 = S.compose((T_WS1[0].reshape(-1), T_WS1[1]), T_SC[c])
            n0 = K if (pi + c) % 3 == 0 else int(rng.integers(80, K))
            fr0, fr1 = _general_camera(oracle, cam, T0, T1, n0, rng, 0.3 if kind == "mix" else 0.04,
                                       empty=(pi == 1 and c == len(cams) - 1 and len(cams) > 1))
            rot_H, rel_H = _hypotheses(*_relative(T0, T1), n_hyp, rng)
            pair.append(cam_entry(fr0, fr1, rot_H, rel_H, (rng.random(n_hyp) >= 0.1).astype(np.uint8),
                                  (rng.random(n_hyp) >= 0.1).astype(np.uint8)))
        pairs.append(pair)
    return scene("general-" + spec_id(spec), cams, pairs)


def reference(tree, sc, remove_outliers=True, use_valid=True, census=None, threshold=R2.THRESHOLD):
    fus = [c.fu for c in sc["cams"]]
    out = []
    for pair in sc["pairs"]:
        cams = pair if use_valid else [dict(c, rot_valid=None, rel_valid=None) for c in pair]
        out.append(R2.run(tree, cams, fus, threshold, remove_outliers, sc["added"], census))
    return out


# ---- capacity: the ring's wrap, the full id table, probe runs across the table's end -----------------------------
# These scenes are built for a context of `Kc` keypoints (1100 or the call's limit), not for K, and take the kernel's
# constants from its test hooks: `ring` / `chunk` records, `slot(id)` the home slot of an id in a table of `n_slots`.
HASH_MULTIPLIER = 2654435761


def host_slot(ids, n_slots):
    """the kernel's home slot restated: ((id * 2654435761) mod 2^32) >> (32 - log2 n_slots), on an array of ids"""
    log2 = int(n_slots).bit_length() - 1
    assert 1 << log2 == n_slots
    return (((np.asarray(ids, dtype=np.int64) & 0xFFFFFFFF) * HASH_MULTIPLIER) % (1 << 32)) >> (32 - log2)


def _relabel(fr0, fr1, new_ids):
    """the matched ids 3 + 7 i of a hand camera become new_ids[i] in both blocks"""
    new_ids = np.asarray(new_ids, np.int32)
    for fr in (fr0, fr1):
        has = fr["lm"] >= 0
        fr["lm"][has] = new_ids[(fr["lm"][has] - 3) // 7]


def _mixed_camera(oracle, rng, total, Kc, free0=None, free1=5):
    """`total` correspondences of kinds C / B / D in the proportions of chunk_scene; the older block's free rows lie
    between the matched ones, so that its 256-keypoint tiles add uneven numbers of records"""
    nD, nB = total // 8, total // 3
    free0 = min(Kc - total, total // 2) if free0 is None else free0
    return hand_camera(oracle, rng, total - nD - nB, 0, nB, nD, free0=free0, free1=min(Kc - total, free1))


def ring_totals(ring, chunk, Kc):
    return (ring - 1, ring, ring + 1, 2 * ring + chunk - 1, Kc)


def ring_scene(oracle, ring, chunk, Kc, seed=61):
    """one camera; pairs with ring - 1, ring, ring + 1, 2 ring + chunk - 1 and Kc correspondences"""
    assert 2 * ring + chunk - 1 < Kc, "the context no longer spans two laps of the ring"
    rng = np.random.default_rng([seed, Kc])
    rot_H, rel_H = lists("true first")
    pairs = []
    for total in ring_totals(ring, chunk, Kc):
        fr0, fr1, _ = _mixed_camera(oracle, rng, total, Kc)
        pairs.append([cam_entry(fr0, fr1, rot_H, rel_H)])
    return scene("ring-%d" % Kc, euroc_pair()[:1], pairs)


def ring_restart_totals(ring, chunk):
    return ((ring + chunk + 5, chunk + 3), (chunk + 3, ring + chunk + 5), (ring + 7, ring + 7))


def ring_restart_scene(oracle, ring, chunk, Kc, seed=62):
    """two cameras: the first wraps the ring and the second does not, the other way round, and both wrap"""
    rng = np.random.default_rng([seed, Kc])
    rot_H, rel_H = lists("true first")
    pairs = []
    for totals in ring_restart_totals(ring, chunk):
        pair = []
        for total in totals:
            fr0, fr1, _ = _mixed_camera(oracle, rng, total, Kc)
            pair.append(cam_entry(fr0, fr1, rot_H, rel_H))
        pairs.append(pair)
    return scene("ring-restart-%d" % Kc, euroc_pair(), pairs)


FULL_TABLE_IDS = 20000   # the id space (and the size of the isLandmarkAdded table) of full_table_scene


def full_table_scene(oracle, Kc, with_added, n_present=2500, n_absent=1000, seed=63):
    """one camera, one pair: the current block holds Kc keypoints with Kc distinct ids (with_added: every one of them
    added), so that a table of Kc + 1 slots keeps ONE empty slot; the older block holds n_present of those ids,
    n_absent ids >= 0 that no current keypoint carries (their lookups end at the empty slot alone) and -1 in the rest"""
    rng = np.random.default_rng([seed, Kc])
    rot_H, rel_H = lists("true first")
    fr0, fr1, _ = _mixed_camera(oracle, rng, n_present, Kc, free0=Kc - n_present, free1=Kc - n_present)
    assert len(fr0["lm"]) == len(fr1["lm"]) == Kc
    ids = rng.permutation(FULL_TABLE_IDS)[:Kc + n_absent].astype(np.int32)
    _relabel(fr0, fr1, ids[:n_present])
    fr1["lm"][fr1["lm"] < 0] = ids[n_present:Kc]
    free = np.flatnonzero(fr0["lm"] < 0)
    fr0["lm"][free[:n_absent]] = ids[Kc:]
    added = np.ones(FULL_TABLE_IDS, np.uint8) if with_added else None
    sc = scene("full-table-%d-%s" % (Kc, "added" if with_added else "null"), euroc_pair()[:1],
               [[cam_entry(fr0, fr1, rot_H, rel_H)]], added)
    sc["absent"] = ids[Kc:]
    return sc


def id_table(lm1, added, slot, n_slots, last_wins=False):
    """the kernel's open-addressed table after the insertion of a current block's ids, keypoints ascending: per slot
    the keypoint it holds (-1: empty).  The SET of occupied slots of linear probing does not depend on the order of
    insertion, and a slot's id does not change once set, so the concurrent insertion on the device differs from this
    one only in which id sits in which slot of a run."""
    tab = np.full(n_slots, -1, np.int64)
    lm1 = np.asarray(lm1)
    for k, lm in enumerate(lm1.tolist()):
        if lm < 0 or (added is not None and (lm >= len(added) or not added[lm])):
            continue
        s = int(slot(lm))
        while tab[s] >= 0 and lm1[tab[s]] != lm:
            s = (s + 1) % n_slots
        if tab[s] < 0 or last_wins:
            tab[s] = k
    return tab


def table_lookup(tab, lm1, slot, lm, wrap=True):
    """the keypoint the table holds for id `lm` (-1: none) and the slots probed; wrap=False: a lookup that gives up at
    the table's end"""
    s, steps = int(slot(lm)), 1
    while tab[s] >= 0 and lm1[tab[s]] != lm:
        s, steps = s + 1, steps + 1
        if s == len(tab):
            if not wrap:
                return -1, steps
            s = 0
    return int(tab[s]), steps


COLLISION_CLUSTER, COLLISION_SECOND, COLLISION_BACKGROUND, COLLISION_DUPLICATES = 320, 100, 300, 40


def collision_scene(oracle, slot, n_slots, Kc, seed=64, id_limit=1 << 22):
    """one camera, one pair, added = None.  The current block's ids: COLLISION_CLUSTER distinct ids whose home is slot
    n_slots - 3 (their probe run crosses the table's end into slot 0), COLLISION_SECOND ids whose home is the slot
    where that run ends, COLLISION_BACKGROUND ids anywhere; COLLISION_DUPLICATES cluster ids sit on a second current
    keypoint of the same 256-keypoint tile and as many on one of another tile.  The older block looks up all of them,
    and absent ids whose home is the first cluster's home, the second's, or a slot inside the first's run.
    sc["clusters"] names the homes and the ids; sc["duplicates"] the (id, row, other row, same tile) placements."""
    rng = np.random.default_rng([seed, Kc])
    rot_H, rel_H = lists("true first")
    home_a = n_slots - 3
    pool = np.arange(id_limit, dtype=np.int64)
    home = host_slot(pool, n_slots)

    def supply(h, n):
        ids = rng.permutation(pool[home == h])[:n]
        assert len(ids) == n and all(int(slot(int(i))) == h for i in ids), "the restated hash is not the kernel's"
        return ids.astype(np.int32)

    a_all = supply(home_a, COLLISION_CLUSTER + 40)
    a_ids, a_absent = a_all[:COLLISION_CLUSTER], a_all[COLLISION_CLUSTER:]
    home_b = (home_a + COLLISION_CLUSTER) % n_slots         # the first empty slot behind the first cluster alone
    b_all = supply(home_b, COLLISION_SECOND + 20)
    b_ids, b_absent = b_all[:COLLISION_SECOND], b_all[COLLISION_SECOND:]
    inside_absent = supply(7, 20)                            # a home inside the first cluster's run, past the table's end
    taken = set(a_all.tolist()) | set(b_all.tolist()) | set(inside_absent.tolist())
    bg = np.array([i for i in rng.permutation(id_limit)[:2 * COLLISION_BACKGROUND].tolist() if i not in taken]
                  [:COLLISION_BACKGROUND], np.int32)
    ids = rng.permutation(np.concatenate([a_ids, b_ids, bg]))
    n = len(ids)
    n_dup, n_abs = 2 * COLLISION_DUPLICATES, len(a_absent) + len(b_absent) + len(inside_absent)
    assert n + n_dup + 20 <= Kc
    fr0, fr1, _ = _mixed_camera(oracle, rng, n, Kc, free0=n_abs + 30, free1=Kc - n)
    _relabel(fr0, fr1, ids)
    # the duplicates: a second current keypoint of a cluster id, in a free row of the same tile or of another one
    cluster = set(a_ids.tolist()) | set(b_ids.tolist())
    rows = [k for k in rng.permutation(len(fr1["lm"])).tolist() if int(fr1["lm"][k]) in cluster]
    free = set(np.flatnonzero(fr1["lm"] < 0).tolist())
    dups = []
    for same in (True, False):
        for _ in range(COLLISION_DUPLICATES):
            k = rows.pop()
            other = next(f for f in sorted(free, key=lambda f: (f * 7919) % 1009) if (f // 256 == k // 256) == same)
            free.remove(other)
            dups.append((int(fr1["lm"][k]), k, other, same))
    for lm, k, other, same in dups:
        fr1["lm"][other] = lm
        fr1["bp"][other] = rng.normal(size=3)
    absent = np.concatenate([a_absent, b_absent, inside_absent])
    free0 = np.flatnonzero(fr0["lm"] < 0)
    fr0["lm"][free0[:n_abs]] = absent
    sc = scene("collision-%d" % Kc, euroc_pair()[:1], [[cam_entry(fr0, fr1, rot_H, rel_H)]])
    sc["clusters"] = dict(home_a=home_a, a_ids=a_ids, home_b=home_b, b_ids=b_ids, absent=absent)
    sc["duplicates"] = dups
    return sc


# ---- GPU side ----------------------------------------------------------------------------------------------------
PER_CAM =("n_corr", "rot_best", "rot_inliers", "rel_best", "rel_inliers", "branch", "removed")
PER_PAIR = ("total_inliers", "rotation_only", "success")
U8 = ("branch", "removed", "rotation_only", "success")


def _past_count_id(fr_other):
    """a valid id for the rows at or past a block's count: one the other block carries, so that reading it would add a
    correspondence"""
    ids = np.asarray(fr_other["lm"])
    ids = ids[ids >= 0]
    return int(ids[0]) if len(ids) else 5


def pack(fe, sc):
    """(blocks0, lm0, blocks1, lm1): [n_pairs n_cams, ...] in pair-major order"""
    from okvis2_amd import multigpu
    Kc = fe.max_keypoints
    out = []
    for side, other in (("fr0", "fr1"), ("fr1", "fr0")):
        frames = [(c[side], c[other]) for pair in sc["pairs"] for c in pair]
        blocks = np.stack([multigpu.pack_block_host(Kc, f["kps"], f["desc"], f["bp"], f["bpv"]) for f, _ in frames])
        lm = np.zeros((len(frames), Kc), np.int32)
        for i, (f, o) in enumerate(frames):
            lm[i, :] = _past_count_id(o)
            lm[i, :len(f["lm"])] = f["lm"]
        out += [blocks, lm]
    return out


def prepare(fe, sc, optional=True, alias=False, merged=False):
    """the device tensors of a call (synchronises).  merged: both sides in ONE block array and ONE id array, the older
    multiframes first (blocks0_dev == blocks1_dev)"""
    import torch
    dev = S._dev
    P, n_cams, nh, Kc = len(sc["pairs"]), len(sc["cams"]), len(sc["pairs"][0][0]["rot_H"]), fe.max_keypoints
    b0, l0, b1, l1 = pack(fe, sc)
    if merged:
        blocks = dev(np.concatenate([b0, b1]))
        lm = dev(np.concatenate([l0, l1]))
        T = dict(blocks0=blocks, blocks1=blocks, lm0=lm, lm1=lm, n_mf0=2 * P, n_mf1=2 * P, mf1_base=P)
    else:
        T = dict(blocks0=dev(b0), blocks1=dev(b1), lm0=dev(l0), lm1=dev(l1), n_mf0=P, n_mf1=P, mf1_base=0)
    T["lm1_in"] = np.concatenate([l0, l1]) if merged else l1
    stack = lambda key: np.stack([np.stack([c[key] for c in pair]) for pair in sc["pairs"]])
    T["rot_H"], T["rel_H"] = dev(stack("rot_H")), dev(stack("rel_H"))
    has_valid = sc["pairs"][0][0]["rot_valid"] is not None
    T["rot_valid"] = dev(stack("rot_valid").astype(np.uint8)) if has_valid else None
    T["rel_valid"] = dev(stack("rel_valid").astype(np.uint8)) if has_valid else None
    T["added"] = None if sc["added"] is None else dev(sc["added"])
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
    for key in PER_CAM:
        T[key] = full((P, n_cams), STATE_SENTINEL if key in U8 else SENTINEL, torch.uint8 if key in U8 else torch.int32)
    for key in PER_PAIR:
        T[key] = full((P,), STATE_SENTINEL if key in U8 else SENTINEL, torch.uint8 if key in U8 else torch.int32)
    if optional:
        T.update(rot_hyp_inliers=full((P, n_cams, nh), SENTINEL, torch.int32),
                 rel_hyp_inliers=full((P, n_cams, nh), SENTINEL, torch.int32),
                 match1=full((P, n_cams, Kc), SENTINEL, torch.int32),
                 state=full((P, n_cams, Kc), STATE_SENTINEL, torch.uint8),
                 distance=full((P, n_cams, Kc), DIST_SENTINEL, torch.float64),
                 lm1_out=T["lm1"] if alias else full(tuple(T["lm1"].shape), SENTINEL, torch.int32))
    torch.cuda.synchronize()
    return T


def launch(fe, sc, T, remove_outliers=True, use_valid=True, stream=None, threshold=R2.THRESHOLD, first=0, count=None):
    """the call alone, on the pairs [first, first + count): nothing here waits for the device"""
    P, n_cams, nh, Kc = len(sc["pairs"]), len(sc["cams"]), len(sc["pairs"][0][0]["rot_H"]), fe.max_keypoints
    count = P - first if count is None else count

    def at(key, per):
        t = T.get(key)
        return None if t is None else t.data_ptr() + first * per * t.element_size()

    res = fe.make_ransac2d2d_result_device(
        *[at(k, n_cams) for k in PER_CAM], *[at(k, 1) for k in PER_PAIR], at("rot_hyp_inliers", n_cams * nh),
        at("rel_hyp_inliers", n_cams * nh), at("match1", n_cams * Kc), at("state", n_cams * Kc),
        at("distance", n_cams * Kc), None if T.get("lm1_out") is None else T["lm1_out"].data_ptr())
    mf0 = np.arange(first, first + count, dtype=np.int32)
    fe.ransac2d2d_consensus_blocks_device(
        T["blocks0"].data_ptr(), T["n_mf0"], T["blocks1"].data_ptr(), T["n_mf1"], mf0, mf0 + T["mf1_base"],
        list(range(n_cams)), T["lm0"].data_ptr(), T["lm1"].data_ptr(),
        None if T["added"] is None else T["added"].data_ptr(), sc["n_landmarks"], at("rot_H", n_cams * nh * 9),
        at("rot_valid", n_cams * nh) if use_valid else None, at("rel_H", n_cams * nh * 12),
        at("rel_valid", n_cams * nh) if use_valid else None, nh, res, threshold, remove_outliers, stream)


def check(sc, T, refs, what, alias=False, only=None):
    """every output of every pair against the reference, byte for byte; untouched rows keep their sentinels"""
    import torch
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in T.items() if isinstance(v, torch.Tensor)}
    n_cams, base = len(sc["cams"]), T["mf1_base"]
    for pi, (pair, ref) in enumerate(zip(sc["pairs"], refs)):
        if only is not None and pi not in only:
            continue
        w = what + (pi,)
        head = tuple(int(got[k][pi]) for k in PER_PAIR)
        assert head == (ref["total_inliers"], ref["rotation_only"], ref["success"]), (w, head, ref["total_inliers"],
                                                                                      ref["rotation_only"], ref["success"])
        for c, (cam, rc) in enumerate(zip(pair, ref["cams"])):
            per = tuple(int(got[k][pi, c]) for k in PER_CAM)
            assert per == tuple(rc[k] for k in PER_CAM), (w, c, per, [rc[k] for k in PER_CAM])
            if "state" not in got:
                continue
            for key in ("rot_hyp_inliers", "rel_hyp_inliers"):
                assert np.array_equal(got[key][pi, c], rc[key]), (w, c, key, got[key][pi, c], rc[key])
            n0, n1 = len(cam["fr0"]["kps"]), len(cam["fr1"]["kps"])
            assert np.array_equal(got["match1"][pi, c, :n0], rc["match1"]), (w, c, "match1")
            assert np.all(got["match1"][pi, c, n0:] == SENTINEL), (w, c, "match1 past the count")
            assert np.array_equal(got["state"][pi, c, :n0], rc["state"]), (w, c, "state", got["state"][pi, c, :n0], rc["state"])
            assert np.all(got["state"][pi, c, n0:] == STATE_SENTINEL), (w, c, "state past the count")
            ds, gd = rc["dist_set"], got["distance"][pi, c, :n0]
            assert np.array_equal(gd[ds].view(np.uint64), rc["distance"][ds].view(np.uint64)), (w, c, "distance", gd[ds][:4],
                                                                                              rc["distance"][ds][:4])
            assert np.all(gd[~ds] == DIST_SENTINEL) and np.all(got["distance"][pi, c, n0:] == DIST_SENTINEL), (w, c)
            b = (base + pi) * n_cams + c
            assert np.array_equal(got["lm1_out"][b, :n1], rc["landmark1_out"]), (w, c, "landmark1_out")
            past = T["lm1_in"][b, n1:] if alias else SENTINEL
            assert np.all(got["lm1_out"][b, n1:] == past), (w, c, "landmark1_out past the count")
    return got
