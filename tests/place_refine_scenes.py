"""Scenes for the refinement of verifyRecognisedPlace's pose (place_refine_ref.py), for small contexts (188 x 120, K = 320), on top of
place_hessian_scenes.py: every multiframe of a scene there gains a start (a list of hypotheses and the winner's index, or
an initial pose).  General scenes (rigs of 1, 2 and 5 cameras over the four camera models, batches of 1, 3 and 17; pixel
noise and wrong landmarks among the terms, so the Cauchy weights matter); noise-free scenes started at the truth; starts
far off, so that steps are rejected or ask for more than a quarter turn; term counts around the kernel's chunk; blocks of
0, 1 and K keypoints; a multiframe without a term; the directed scene with its singular terms and unverified
multiframes; rotations that reach each branch of the matrix-to-quaternion conversion.  CPU only.  Test infrastructure
only."""
import numpy as np

import place_hessian_ref as PH
import place_hessian_scenes as HS
import place_refine_ref as PR
import ransac_scenes as S

K = HS.K
N_HYP = 4
BAD_BEST = 16


def matrix12(pose):
    """a pose (t[3], qx, qy, qz, qw) as the row-major 3 x 4 a hypothesis is"""
    pose = np.asarray(pose, dtype=np.float64)
    return np.concatenate([PH.rotation(True, pose[3:7]), pose[:3].reshape(3, 1)], axis=1).reshape(-1)


def perturbed(pose, rng, angle, shift):
    C = PH.rotation(True, pose[3:7]) @ S.rodrigues(rng.normal(size=3), angle)
    return HS.pose7((C, pose[:3] + shift * rng.normal(size=3) / np.sqrt(3.0)))


def with_starts(sc, rng, starts, max_iterations=PR.MAX_ITERATIONS_DEFAULT, initial=False):
    """starts: one pose per multiframe.  The winner stands at a varying place in a list of N_HYP hypotheses, the others
    are random poses."""
    for i, (mf, start) in enumerate(zip(sc["mfs"], starts)):
        hyp = np.array([S.pose_matrix((S.rodrigues(rng.normal(size=3), rng.uniform(0, np.pi)), rng.uniform(-3, 3, 3)))
                        for _ in range(N_HYP)])
        mf["best"] = i % N_HYP
        hyp[mf["best"]] = matrix12(start)
        mf["hyp"] = hyp
        mf["initial"] = np.asarray(start, dtype=np.float64) if initial else None
    sc["max_iterations"] = max_iterations
    return sc


def general_scene(oracle, spec, n_mf=None, seed=0):
    """place_hessian_scenes.general_scene (noise of half a pixel, 15 % wrong landmarks, ragged blocks, a mix of verdicts),
    started at its poses: up to 0.01 rad and 2 cm off the truth"""
    sc = HS.general_scene(oracle, spec, n_mf=n_mf, seed=seed)
    return with_starts(sc, np.random.default_rng([seed, 5]), [mf["pose"] for mf in sc["mfs"]])


def _clean_scene(oracle, name, spec, n_mf, seed, noise, wrong, n_kps=(40, 90), positive_w=False):
    m = S.table()
    cams, T_SC = HS.rig(spec)
    rng = np.random.default_rng([seed, len(cams), n_mf])
    usable = S.usable_rows(m)
    if positive_w:                                                  # (the reference's Jacobian of a term with w < 0 has the wrong sign)
        usable = usable[m["hp"][usable, 3] > 0]
    mfs, truths = [], []
    for i in range(n_mf):
        T_WS = (m["T1"][0].reshape(3, 3) @ S.rodrigues((0, 1, 0), 0.02 * (i % 5)), m["T1"][1] + np.array([0.05 * (i % 7), 0.0, 0.0]))
        frames = [S.make_frame(oracle, cam, S.compose(T_WS, T_SC[c]), m["p"], usable, int(rng.integers(*n_kps)), rng,
                               wrong=wrong, none=0.05, noise=noise) for c, cam in enumerate(cams)]
        ml = [f["lm"] for f in frames]
        truths.append(HS.pose7(T_WS))
        mfs.append(HS._mf(frames, ml, [HS._states(rng, l, 0.9) for l in ml], truths[-1]))
    return HS.scene(name, cams, T_SC, m["hp"], mfs), truths, rng


def truth_scene(oracle, spec=("euroc", "euroc1"), n_mf=16, seed=7):
    """no noise beyond the float32 of a keypoint, no wrong landmark, started at the truth: the loop ends at once"""
    sc, truths, rng = _clean_scene(oracle, "truth-" + S.spec_id(spec), spec, n_mf, seed, 0.0, 0.0)
    return with_starts(sc, rng, truths)


def far_scene(oracle, spec=("euroc", "euroc1"), n_mf=16, seed=9, angle=0.5, shift=1.5, max_iterations=20):
    """noise and wrong landmarks, starts far off: steps are rejected, some ask for more than a quarter turn"""
    sc, truths, rng = _clean_scene(oracle, "far-" + S.spec_id(spec), spec, n_mf, seed, 0.5, 0.15)
    starts = [perturbed(t, rng, angle * (0.4 + 0.6 * (i % 4) / 3.0), shift * (0.3 + 0.7 * (i % 3) / 2.0))
              for i, t in enumerate(truths)]
    return with_starts(sc, rng, starts, max_iterations)


def wild_scene(oracle, spec=("euroc", "euroc1"), n_mf=16, seed=9, max_iterations=12):
    """two to three keypoints per camera and starts up to 3 rad and 6 m off: steps that ask for more than a quarter turn"""
    sc, truths, rng = _clean_scene(oracle, "wild-" + S.spec_id(spec), spec, n_mf, seed, 0.5, 0.15, n_kps=(2, 4))
    return with_starts(sc, rng, [perturbed(t, rng, 3.0, 6.0) for t in truths], max_iterations)


def wild_rt8_scene(oracle):
    """the same on one camera of the 8-coefficient model"""
    return wild_scene(oracle, spec=("radtan8",))


def no_term_scene(oracle, n_mf=24, seed=13):
    """verified multiframes without a term: every claimed keypoint an outlier of the consensus (status 3); the last
    eight are not verified and keep their inliers (status 0)"""
    sc, truths, rng = _clean_scene(oracle, "no-term", ("nodist",), n_mf, seed, 0.5, 0.0, n_kps=(5, 12))
    for mf in sc["mfs"][:-8]:
        mf["state"] = [np.where(s == 2, 1, s).astype(np.uint8) for s in mf["state"]]
    for i, mf in enumerate(sc["mfs"][-8:]):
        mf["verdict"] = i % 3
    return with_starts(sc, rng, truths)


def noisy_scene(oracle, spec=("euroc", "euroc1"), n_mf=16, seed=11):
    """noise and wrong landmarks, starts up to 3 degrees and 10 cm off: what the loop is for.  Landmarks with w > 0 only,
    so that every Jacobian is the derivative and the loop converges as ceres' would on a healthy map."""
    sc, truths, rng = _clean_scene(oracle, "noisy-" + S.spec_id(spec), spec, n_mf, seed, 0.5, 0.15, positive_w=True)
    starts = [perturbed(t, rng, np.deg2rad(3.0) * rng.random(), 0.1 * rng.random()) for t in truths]
    return with_starts(sc, rng, starts)


def term_count_scene(oracle, totals):
    sc = HS.term_count_scene(oracle, totals)
    return with_starts(sc, np.random.default_rng(33), [mf["pose"] for mf in sc["mfs"]], max_iterations=3)


def block_size_scene(oracle):
    """blocks of 0, 1 and K keypoints; the fourth multiframe has no term (status 3)"""
    sc = HS.block_size_scene(oracle)
    return with_starts(sc, np.random.default_rng(43), [mf["pose"] for mf in sc["mfs"]], max_iterations=3)


def directed_scene(oracle):
    """place_hessian_scenes.directed_scene: singular terms (status 4), two unverified multiframes (status 0); the last
    BAD_BEST multiframes name a winner outside the list (status 4)"""
    sc = HS.directed_scene(oracle)
    sc["mfs"] = sc["mfs"] + [dict(sc["mfs"][3]) for _ in range(BAD_BEST)]
    with_starts(sc, np.random.default_rng(53), [mf["pose"] for mf in sc["mfs"]], max_iterations=3)
    for i, mf in enumerate(sc["mfs"][-BAD_BEST:]):
        mf["best"] = N_HYP + i if i % 2 else -1 - i
    return sc


def conversion_scene(oracle, copies=16, seed=61):
    """a world turned so that the true rotation is (nearly) a half turn about x, y and z, and a small one: each branch of
    Eigen's Quaterniond(Matrix3d), `copies` times; started at the truth, one camera"""
    m = S.table()
    cams, T_SC = HS.rig(("nodist",))
    rng = np.random.default_rng(seed)
    usable = S.usable_rows(m)
    C, r = m["T1"][0].reshape(3, 3), np.asarray(m["T1"][1])
    frames = [S.make_frame(oracle, cams[0], S.compose((C, r), T_SC[0]), m["p"], usable, 24, rng, wrong=0.0, none=0.0)]
    ml = [frames[0]["lm"]]
    state = [np.full(24, 2, np.uint8)]
    hp, mfs, starts = [], [], []
    for axis in (None, 0, 1, 2):
        for k in range(copies):
            target = S.rodrigues(rng.normal(size=3), 0.2 * rng.random())
            if axis is not None:
                target = S.rodrigues(np.eye(3)[axis], np.pi - 0.05 * rng.random()) @ target
            R0 = target @ C.T                                       # the world turned by R0: the pose's rotation is `target`
            base = len(hp)
            hp += [np.append(R0 @ p[:3], p[3]) for p in m["hp"]]
            pose = HS.pose7((R0 @ C, R0 @ r))
            mfs.append(HS._mf(frames, [np.where(ml[0] >= 0, ml[0] + base, -1)], state, pose))
            starts.append(pose)
    sc = HS.scene("conversion", cams, T_SC, np.array(hp), mfs)
    return with_starts(sc, rng, starts, max_iterations=2)


def reference(oracle, tree, sc, use_verdict=True, use_initial=False, max_iterations=None, census=None):
    it = sc["max_iterations"] if max_iterations is None else max_iterations
    return [PR.refine(oracle, tree, sc["hp"], mf["frames"], mf["ml"], mf["state"], sc["cams"], sc["T_SC_params"],
                      mf["hyp"], mf["best"], mf["initial"] if use_initial else None, it,
                      mf["verdict"] == 3 or not use_verdict, census) for mf in sc["mfs"]]
