"""Scenes for okvfe_ransac3d2d_consensus_blocks_device and okvfe_remove_outliers_blocks_device, on the tables of
map_synth.make_map: rigs of 1, 2 and 5 cameras over all four camera models, frames whose keypoints sit at projections
of the landmarks with a share of wrong landmarks, hypotheses around the true T_WS and random ones; the directed cases,
knife edges, verdict edges and chunk edges of the consensus; the projection statuses and the max_error edge of
removeOutliers.  CPU only up to `prepare_consensus` / `prepare_remove` and the launches, which need torch and a GPU.
Test infrastructure only."""
import dataclasses
import functools

import numpy as np

import map_synth
import radtan8_ref
import ransac_ref as R
from gate_scenes import bisect_adjacent, rodrigues
from okvis2_amd import synth

K = 256            # keypoint capacity of the contexts the scenes are built for
SENTINEL = -7
STATE_SENTINEL = 0x77
DIST_SENTINEL = -12345.0
STATE_FLOOR = 16    # every general scene has at least this many inliers and outliers of a winner (the census floor)
PAST_COUNT_ROW = 5  # a valid table row in the landmark rows at or past a block's count: must be ignored


def camera(kind, w=None, h=None):
    cam = {"euroc": lambda: synth.euroc_config().cams[0], "euroc1": lambda: synth.euroc_config().cams[1],
           "equi": lambda: synth.hilti_config().cams[0],
           "nodist": lambda: dataclasses.replace(synth.d455_config().cams[0], dist_type=0),
           "radtan8": lambda: synth.radtan8_config().cams[0]}[kind]()
    return dataclasses.replace(cam, w=w or cam.w, h=h or cam.h)


def rig(kinds):
    """cameras and T_SC: camera c turned about y and moved along x, a little off for every camera"""
    if kinds == "hilti":
        cams = list(synth.hilti_config().cams)
    else:
        cams = [camera(k) for k in kinds]
    n = len(cams)
    T_SC = [(rodrigues((0.1, 1.0, 0.05 * c), 0.12 * (c - 0.5 * (n - 1))).reshape(-1),
             np.array([0.11 * c - 0.05, 0.01 * c, 0.02 * (c % 2)])) for c in range(n)]
    return cams, T_SC


def compose(T_WS, T_SC):
    """T_WS T_SC in plain numpy (what the caller's Transformation class would hand over)"""
    Cw, rw = np.asarray(T_WS[0], dtype=np.float64).reshape(3, 3), np.asarray(T_WS[1], dtype=np.float64)
    Cs, rs = np.asarray(T_SC[0], dtype=np.float64).reshape(3, 3), np.asarray(T_SC[1], dtype=np.float64)
    return (Cw @ Cs).reshape(-1), Cw @ rs + rw


@functools.lru_cache(maxsize=None)
def table(n_landmarks=400, seed=1):
    return map_synth.make_map(n_landmarks=n_landmarks, n_poses=12, seed=seed)


def backproject(oracle, cam, kps):
    if cam.dist_type == 3:
        return radtan8_ref.backproject_keypoints(cam, kps)
    return oracle.backproject_keypoints(cam, kps)


def make_frame(oracle, cam, T_WC, p_W, usable, n_kps, rng, wrong=0.3, none=0.1, noise=0.5):
    """n_kps keypoints: at the projections of landmarks while they last, the rest at random pixels; `wrong` of them
    carry another landmark, `none` of them none.  usable: the rows a keypoint may carry."""
    C, r = np.asarray(T_WC[0]).reshape(3, 3), np.asarray(T_WC[1])
    kps = np.zeros(n_kps, dtype=oracle.KEYPOINT_DTYPE)
    kps["size"] = 12.0
    lm = np.full(n_kps, -1, np.int32)
    k = 0
    for l in rng.permutation(usable):
        if k >= n_kps:
            break
        st, pt = R.project(oracle, cam, C.T @ (p_W[l] - r))
        if st != 0:
            continue
        kps[k]["x"], kps[k]["y"] = pt + rng.normal(0, noise, 2) if noise else pt
        lm[k] = l
        k += 1
    kps[k:]["x"] = rng.uniform(0, cam.w, n_kps - k)
    kps[k:]["y"] = rng.uniform(0, cam.h, n_kps - k)
    lm[k:] = rng.choice(usable, n_kps - k)
    u = rng.random(n_kps)
    swap = u < wrong
    lm[swap] = rng.choice(usable, int(swap.sum()))
    lm[(u >= wrong) & (u < wrong + none)] = -1
    kps["size"] = rng.choice(np.array([12.0, 18.0, 24.0], np.float32), n_kps, p=[0.8, 0.1, 0.1])
    bp, bpv = backproject(oracle, cam, kps)
    return dict(kps=kps, desc=rng.integers(0, 256, (n_kps, 48), dtype=np.uint8), bp=bp, bpv=bpv, lm=lm)


def pose_matrix(T):
    return np.concatenate([np.asarray(T[0], dtype=np.float64).reshape(3, 3),
                           np.asarray(T[1], dtype=np.float64).reshape(3, 1)], axis=1).reshape(-1)


def hypotheses(T_WS, n, rng, n_random=10):
    """the true pose, perturbed copies (up to 2 degrees / 5 cm) and random poses, as [n, 12]"""
    C, r = np.asarray(T_WS[0]).reshape(3, 3), np.asarray(T_WS[1])
    out = [pose_matrix(T_WS)]
    while len(out) < n:
        if len(out) >= n - n_random:
            out.append(pose_matrix((rodrigues(rng.normal(size=3), rng.uniform(0, np.pi)), rng.uniform(-3, 3, 3))))
        else:
            s = rng.random()
            out.append(pose_matrix((C @ rodrigues(rng.normal(size=3), np.deg2rad(2.0) * s),
                                    r + 0.05 * s * rng.normal(size=3) / np.sqrt(3.0))))
    order = rng.permutation(n)  # the true pose somewhere in the list
    return np.array(out)[order]


def usable_rows(m):
    n_obs = np.diff(m["obs_begin"])
    return np.flatnonzero((n_obs >= 1) & (np.abs(m["hp"][:, 3]) >= 1.0e-8))


def scene(name, cams, T_SC, hp, obs_begin, mfs):
    return dict(name=name, cams=cams, T_SC=T_SC, hp=np.ascontiguousarray(hp, dtype=np.float64),
                obs_begin=np.ascontiguousarray(obs_begin, dtype=np.int32), mfs=mfs)


GENERAL_SPECS = (("radtan8",), ("nodist",), ("euroc", "euroc1"), "hilti")


def spec_id(spec):
    return spec if isinstance(spec, str) else "+".join(spec)


def general_scene(oracle, spec, seed=0, n_mf=3, n_hyp=50):
    """n_mf multiframes of ragged blocks (one full, one empty somewhere) against one table"""
    m = table(800)
    cams, T_SC = rig(spec)
    rng = np.random.default_rng([seed, len(cams), n_hyp])
    usable = usable_rows(m)
    mfs = []
    for i in range(n_mf):
        T_WS = (m["T1"][0].reshape(3, 3) @ rodrigues((0, 1, 0), 0.02 * i), m["T1"][1] + np.array([0.05 * i, 0.0, 0.0]))
        frames = []
        for c, cam in enumerate(cams):
            n = K if (i + c) % 3 == 0 else int(rng.integers(40, K))
            if i == 1 and c == len(cams) - 1:
                n = 0
            frames.append(make_frame(oracle, cam, compose(T_WS, T_SC[c]), m["p"], usable, n, rng,
                                     wrong=(0.2, 0.24, 0.4)[i % 3] + rng.uniform(0.0, 0.02), none=0.05))
        valid = (rng.random(n_hyp) >= 0.1).astype(np.uint8)
        mfs.append(dict(frames=frames, H=hypotheses(T_WS, n_hyp, rng), valid=valid, T_WS=T_WS))
    return scene("general-" + spec_id(spec), cams, T_SC, m["hp"], m["obs_begin"], mfs)


W_CASES = (1.0e-8, np.nextafter(1.0e-8, 0.0), 0.0, -0.0, -1.0, -np.nextafter(1.0e-8, 0.0), np.nan)
DIRECTED_COPIES = 16


def directed_scene(oracle, seed=3):
    """2 cameras, one multiframe: per case DIRECTED_COPIES keypoints in every camera on top of a general frame -- the
    seven values of hp[3]; a landmark without observations; backproj_valid == 0; a zero back-projection; a landmark at
    the camera's centre under the first hypothesis, [I | 0] (NaN distance); one landmark on many keypoints; a row outside the
    table."""
    m = table()
    cams, T_SC = rig(("euroc", "euroc1"))
    rng = np.random.default_rng(seed)
    usable = usable_rows(m)
    T_WS = m["T1"]
    hp = m["hp"].copy()
    n_obs = np.diff(m["obs_begin"]).copy()
    extra_hp, extra_obs = [], []
    base = len(hp)

    def add(h4, obs):
        extra_hp.append(h4), extra_obs.append(obs)
        return base + len(extra_hp) - 1

    frames = []
    for c, cam in enumerate(cams):
        T_WC = compose(T_WS, T_SC[c])
        n_dir = DIRECTED_COPIES * (len(W_CASES) + 7)
        fr = make_frame(oracle, cam, T_WC, m["p"], usable, K, rng, wrong=0.25)
        k = K - n_dir
        for w in W_CASES:
            for _ in range(DIRECTED_COPIES):
                l = int(fr["lm"][k]) if fr["lm"][k] >= 0 else int(usable[0])
                p = m["p"][l]
                fr["lm"][k] = add(np.array([p[0] * w, p[1] * w, p[2] * w, w]) if w == w and w != 0 else
                                  np.array([p[0], p[1], p[2], w]), 2)
                k += 1
        for _ in range(DIRECTED_COPIES):  # no landmark
            fr["lm"][k] = -1
            k += 1
        for _ in range(DIRECTED_COPIES):  # no observation in the table
            fr["lm"][k] = add(np.array([*m["p"][int(usable[k % len(usable)])], 1.0]), 0)
            k += 1
        for _ in range(DIRECTED_COPIES):  # the back-projection failed
            fr["lm"][k] = int(usable[k % len(usable)])
            fr["bpv"][k] = 0
            k += 1
        for _ in range(DIRECTED_COPIES):  # a zero back-projection
            fr["lm"][k] = int(usable[k % len(usable)])
            fr["bp"][k] = 0.0
            fr["bpv"][k] = 1
            k += 1
        centre = add(np.array([*T_SC[c][1], 1.0]), 1)  # = r_SC: body - r_SC is exactly zero under [I | 0]
        dup = int(usable[7])
        for _ in range(DIRECTED_COPIES):  # the landmark in the camera's centre
            fr["lm"][k] = centre
            k += 1
        for _ in range(DIRECTED_COPIES):  # one landmark on many keypoints
            fr["lm"][k] = dup
            k += 1
        for _ in range(DIRECTED_COPIES):  # a row outside the table (filled in below)
            fr["lm"][k] = -2
            k += 1
        assert k == K
        frames.append(fr)
    hp = np.concatenate([hp, np.array(extra_hp)])
    obs_begin = np.concatenate([[0], np.cumsum(np.concatenate([n_obs, extra_obs]))]).astype(np.int32)
    for fr in frames:
        fr["lm"][fr["lm"] == -2] = len(hp) + 3
    H = hypotheses(T_WS, 12, rng, n_random=3)
    H = np.concatenate([pose_matrix((np.eye(3), np.zeros(3)))[None], H])  # hypothesis 0: [I | 0] (the NaN distances)
    return scene("directed", cams, T_SC, hp, obs_begin, [dict(frames=frames, H=H, valid=None, T_WS=T_WS)])


def _knife_base(oracle, seed):
    """one euroc camera, 12 exact correspondences + the probe (keypoint 0, 2 px off its projection)"""
    m = table()
    cams, T_SC = rig(("euroc",))
    rng = np.random.default_rng(seed)
    usable = usable_rows(m)
    T_WS = m["T1"]
    fr = make_frame(oracle, cams[0], compose(T_WS, T_SC[0]), m["p"], usable, 13, rng, wrong=0.0, none=0.0, noise=0.0)
    assert np.all(fr["lm"] >= 0)
    fr["kps"]["size"] = 12.0
    fr["kps"]["x"][0] += 2.0
    fr["bp"], fr["bpv"] = backproject(oracle, cams[0], fr["kps"])
    return m, cams, T_SC, T_WS, fr


def _probe_distance(tree, m, cams, T_SC, fr, H):
    corr = R.correspondences(tree, m["hp"], m["obs_begin"], [fr], [fr["lm"]], [cams[0].fu])
    return R.distances(tree, H, corr, T_SC)[:, 0]


def knife_translation(oracle, tree, seed=11):
    """two hypotheses, adjacent doubles apart in t[0], between which the probe's distance goes from < 16 to not"""
    m, cams, T_SC, T_WS, fr = _knife_base(oracle, seed)
    C, r = np.asarray(T_WS[0]).reshape(3, 3), np.asarray(T_WS[1])

    def hyp(dx):
        return pose_matrix((C, np.array([r[0] + dx, r[1], r[2]])))

    def inlier(dx):
        return bool(_probe_distance(tree, m, cams, T_SC, fr, hyp(dx)[None])[0] < R.THRESHOLD)

    # the probe is 2 px off; moving the pose along x either way brings it past the threshold
    far = next(d for d in (0.5, -0.5) if not inlier(d))
    sign = 1.0 if far > 0 else -1.0
    lo, hi = bisect_adjacent(lambda a: inlier(sign * a), 1.0e-9, abs(far))
    H = np.array([hyp(sign * lo), hyp(sign * hi)])
    d = _probe_distance(tree, m, cams, T_SC, fr, H)
    assert d[0] < R.THRESHOLD and not d[1] < R.THRESHOLD
    return scene("knife-translation", cams, T_SC, m["hp"], m["obs_begin"], [dict(frames=[fr], H=H, valid=None, T_WS=T_WS)])


def knife_size(oracle, tree, seed=12):
    """two copies of the probe whose float32 sizes are adjacent, between which the distance goes from < 16 to not"""
    m, cams, T_SC, T_WS, fr = _knife_base(oracle, seed)
    H = pose_matrix(T_WS)[None]

    def inlier(size):
        f = dict(fr, kps=fr["kps"].copy())
        f["kps"]["size"][0] = size
        return bool(_probe_distance(tree, m, cams, T_SC, f, H)[0] < R.THRESHOLD)

    assert inlier(np.float32(12.0)) and not inlier(np.float32(0.5))
    lo, hi = bisect_adjacent(inlier, np.float32(0.5), np.float32(12.0), dtype=np.float32)
    two = {k: np.concatenate([v[:1], v]) for k, v in fr.items()}
    two["kps"]["size"][0], two["kps"]["size"][1] = lo, hi
    corr = R.correspondences(tree, m["hp"], m["obs_begin"], [two], [two["lm"]], [cams[0].fu])
    d = R.distances(tree, H, corr, T_SC)[0]
    assert not d[0] < R.THRESHOLD and d[1] < R.THRESHOLD
    return scene("knife-size", cams, T_SC, m["hp"], m["obs_begin"], [dict(frames=[two], H=H, valid=None, T_WS=T_WS)])


VERDICT_CASES = ((9, 9), (10, 10), (12, 9), (10, 7), (20, 14), (30, 21), (20, 15))
VERDICT_EXPECT = {(9, 9): (-1, 0, 0), (10, 10): (0, 10, 1), (12, 9): (0, 9, 0), (10, 7): (0, 7, 0),
                  (20, 14): (0, 14, 0), (30, 21): (0, 21, 0), (20, 15): (0, 15, 1)}


def verdict_scene(oracle, H_of, valid=None, seed=21):
    """one multiframe per VERDICT_CASES entry (n correspondences, i of them inliers of the true pose: the landmarks of
    the others are copies moved a metre); H_of(T_WS, rng) -> the hypotheses of every multiframe"""
    m = table()
    cams, T_SC = rig(("euroc",))
    rng = np.random.default_rng(seed)
    usable = usable_rows(m)
    T_WS = m["T1"]
    moved = m["hp"].copy()
    moved[:, :3] += np.array([1.0, 0.5, 0.0]) * moved[:, 3:4]
    hp = np.concatenate([m["hp"], moved])
    n_obs = np.diff(m["obs_begin"])
    obs_begin = np.concatenate([[0], np.cumsum(np.concatenate([n_obs, n_obs]))]).astype(np.int32)
    mfs = []
    for n, i in VERDICT_CASES:
        fr = make_frame(oracle, cams[0], compose(T_WS, T_SC[0]), m["p"], usable, n, rng, wrong=0.0, none=0.0, noise=0.0)
        fr["lm"][i:] += len(m["hp"])
        extra = make_frame(oracle, cams[0], compose(T_WS, T_SC[0]), m["p"], usable, 5, rng, wrong=0.0, none=1.0)
        fr = {k: np.concatenate([fr[k], extra[k]]) for k in fr}  # (keypoints without a landmark behind them)
        mfs.append(dict(frames=[fr], H=H_of(T_WS, rng), valid=valid, T_WS=T_WS))
    return scene("verdict", cams, T_SC, hp, obs_begin, mfs)


def far_pose(T_WS, rng):
    return pose_matrix((rodrigues((1, 0, 0), 2.0), np.asarray(T_WS[1]) + np.array([30.0, -20.0, 10.0])))


def chunk_scene(oracle, chunk, seed=31):
    """3 cameras; multiframes with exactly chunk - 1, chunk, chunk + 1 and 2 chunk + 1 correspondences"""
    assert 2 * chunk + 1 <= 3 * K, "the contexts' K no longer spans two chunks: raise ransac_scenes.K"
    m = table()
    cams, T_SC = rig(("euroc", "euroc1", "euroc"))
    rng = np.random.default_rng(seed)
    usable = usable_rows(m)
    T_WS = m["T1"]
    mfs = []
    for total in (chunk - 1, chunk, chunk + 1, 2 * chunk + 1):
        left, frames = total, []
        for c, cam in enumerate(cams):
            n = min(K, left) if c < 2 else left
            left -= n
            fr = make_frame(oracle, cam, compose(T_WS, T_SC[c]), m["p"], usable, K if c < 2 else max(n, 3), rng,
                            wrong=0.3, none=0.0)
            fr["lm"][n:] = -1
            frames.append(fr)
        assert left == 0
        mfs.append(dict(frames=frames, H=hypotheses(T_WS, 8, rng, n_random=2), valid=None, T_WS=T_WS))
    return scene("chunks", cams, T_SC, m["hp"], m["obs_begin"], mfs)


LAP_K = 260   # the smallest multiple of 4 at which the five-camera rig holds 2 ring + chunk + 7 keypoints (ring = 2 * 256)


def lap_totals(ring, chunk):
    return (2 * ring - 1, 2 * ring, 2 * ring + 1, 2 * ring + chunk + 7)


def lap_scene(oracle, ring, chunk, Kc=LAP_K, seed=71):
    """the five-camera rig on contexts of Kc keypoints (K's 1280 slots do not hold the last total); multiframes with
    exactly 2 ring - 1, 2 ring, 2 ring + 1 and 2 ring + chunk + 7 correspondences: two whole laps of the kernel's ring
    and a partial chunk behind them.  Every block is full; the keypoints without a landmark lie between the others, so
    that the 256-slot tiles add uneven numbers of records.  The second multiframe has too many wrong landmarks to be
    accepted; the others are accepted and lose their outliers."""
    m = table()
    cams, T_SC = rig("hilti")
    assert lap_totals(ring, chunk)[-1] <= len(cams) * Kc, "the rig no longer holds two laps and a chunk: raise Kc"
    rng = np.random.default_rng([seed, Kc])
    usable = usable_rows(m)
    T_WS = m["T1"]
    mfs = []
    for mi, total in enumerate(lap_totals(ring, chunk)):
        share = np.full(len(cams), total // len(cams))
        share[:total % len(cams)] += 1
        shift = int(min(Kc - share.max(), share.min(), 40))   # (uneven blocks, the same total)
        share[0] += shift
        share[-1] -= shift
        frames = []
        for c, cam in enumerate(cams):
            fr = make_frame(oracle, cam, compose(T_WS, T_SC[c]), m["p"], usable, Kc, rng, wrong=0.3 if mi == 1 else 0.15, none=0.0)
            fr["lm"][rng.permutation(Kc)[:Kc - share[c]]] = -1
            frames.append(fr)
        mfs.append(dict(frames=frames, H=hypotheses(T_WS, 8, rng, n_random=2), valid=None, T_WS=T_WS))
    return scene("laps", cams, T_SC, m["hp"], m["obs_begin"], mfs)


def reference(tree, sc, remove_outliers=True, use_valid=True, census=None, threshold=R.THRESHOLD):
    fus =[c.fu for c in sc["cams"]]
    return [R.consensus(tree, sc["hp"], sc["obs_begin"], mf["frames"], [f["lm"] for f in mf["frames"]], fus, sc["T_SC"],
                        mf["H"], mf["valid"] if use_valid else None, threshold, remove_outliers, census)
            for mf in sc["mfs"]]


# ---- removeOutliers scenes -------------------------------------------------------------------------------------
REMOVE_KINDS = ("euroc", "equi", "nodist", "radtan8")


def remove_cameras():
    """the four models at one image size, as the slots of one context"""
    return [camera(k, 752, 480) for k in REMOVE_KINDS]


def remove_scene(oracle, seed=41, n_kps=200):
    """one frame per camera model (mixed slots in one call) + an empty one: keypoints at projections with 0 .. 8 px of
    noise, wrong landmarks (every projection status), landmarks with negative hp[3], NaN keypoints, rows outside"""
    m = table()
    cams = remove_cameras()
    rng = np.random.default_rng(seed)
    usable = usable_rows(m)
    frames, poses, cam_ids = [], [], []
    for c, cam in enumerate(cams):
        T_WC = compose(m["T1"], rig(("euroc",))[1][0])
        fr = make_frame(oracle, cam, T_WC, m["p"], usable, n_kps, rng, wrong=0.0, none=0.1, noise=0.0)
        off = rng.uniform(0, 8, n_kps) * np.exp(1j * rng.uniform(0, 2 * np.pi, n_kps))
        fr["kps"]["x"] += off.real.astype(np.float32)
        fr["kps"]["y"] += off.imag.astype(np.float32)
        some = rng.random(n_kps) < 0.45  # any landmark: outside on every side, behind
        fr["lm"][some] = rng.integers(0, len(m["hp"]), int(some.sum()))
        fr["lm"][5:12] = usable[5:12]
        fr["kps"]["x"][5:9] = np.nan
        fr["kps"]["y"][9:12] = np.nan
        fr["lm"][12:17] = len(m["hp"]) + 1
        frames.append(fr), poses.append(T_WC), cam_ids.append(c)
    frames.append({k: v[:0] for k, v in frames[0].items()}), poses.append(poses[0]), cam_ids.append(0)
    return dict(name="remove-general", cams=cams, hp=m["hp"], frames=frames, poses=poses, cam_ids=cam_ids)


def remove_status_scene(oracle, copies=16):
    """hand-placed landmarks for an identity pose: outside on each side, behind, |z| < 1e-12, the RADTAN8 distortion
    failure (rho > 9), hp_C[3] < 0 on a landmark that projects"""
    cams = remove_cameras()
    I = (np.eye(3).reshape(-1), np.zeros(3))
    pts = [(-3.0, 0.0, 1.0), (0.0, -3.0, 1.0), (3.0, 0.0, 1.0), (0.0, 3.0, 1.0), (0.1, 0.1, -2.0), (0.1, 0.1, 1.0e-13),
           (4.0, 4.0, 1.0), (0.05, 0.02, 1.0)]
    hp = np.array([[x, y, z, 1.0] for x, y, z in pts] + [[-0.05, -0.02, -1.0, -1.0]])
    frames, poses, cam_ids = [], [], []
    for c, cam in enumerate(cams):
        n = copies * len(hp)
        kps = np.zeros(n, dtype=oracle.KEYPOINT_DTYPE)
        kps["size"] = 12.0
        lm = np.repeat(np.arange(len(hp)), copies).astype(np.int32)
        for k in range(n):
            st, pt = R.project(oracle, cam, hp[lm[k], :3] / hp[lm[k], 3])
            kps["x"][k], kps["y"][k] = (pt[0] + 0.5 * (k % copies), pt[1]) if st == 0 else (100.0, 100.0)
        bp, bpv = backproject(oracle, cam, kps)
        frames.append(dict(kps=kps, desc=np.zeros((n, 48), np.uint8), bp=bp, bpv=bpv, lm=lm))
        poses.append(I), cam_ids.append(c)
    return dict(name="remove-status", cams=cams, hp=hp, frames=frames, poses=poses, cam_ids=cam_ids)


def remove_edge_scene(oracle, tree, kind="euroc"):
    """max_error bisected to adjacent doubles around one keypoint's error: (scene, max_error kept, max_error removed)"""
    cams = remove_cameras()
    c = REMOVE_KINDS.index(kind)
    I = (np.eye(3).reshape(-1), np.zeros(3))
    hp = np.array([[0.3, -0.2, 2.0, 1.0]])
    st, pt = R.project(oracle, cams[c], hp[0, :3])
    assert st == 0
    kps = np.zeros(3, dtype=oracle.KEYPOINT_DTYPE)
    kps["size"] = 12.0
    kps["x"], kps["y"] = pt[0] + 2.5, pt[1] - 3.0
    bp, bpv = backproject(oracle, cams[c], kps)
    fr = dict(kps=kps, desc=np.zeros((3, 48), np.uint8), bp=bp, bpv=bpv, lm=np.zeros(3, np.int32))

    def kept(max_error):
        return R.remove_outliers(oracle, tree, hp, kps, fr["lm"], cams[c], I, max_error)[1] == 3

    lo, hi = bisect_adjacent(kept, 3.0, 5.0)  # kept(hi), not kept(lo)
    assert kept(hi) and not kept(lo)
    return dict(name="remove-edge", cams=cams, hp=hp, frames=[fr], poses=[I], cam_ids=[c]), hi, lo


def remove_reference(oracle, tree, sc, max_error=R.MAX_ERROR, census=None):
    return [R.remove_outliers(oracle, tree, sc["hp"], fr["kps"], fr["lm"], sc["cams"][ci], T, max_error, census)
            for fr, T, ci in zip(sc["frames"], sc["poses"], sc["cam_ids"])]


# ---- GPU side --------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        a = np.zeros((1,) + a.shape[1:], dtype=a.dtype)
    return torch.from_numpy(a).cuda()


class DeviceTable:
    """hp_W and obs_begin in device memory and the okvfe_landmark_table_device over them"""

    def __init__(self, fe, hp, obs_begin=None):
        hp = np.ascontiguousarray(hp, dtype=np.float64).reshape(-1, 4)
        if obs_begin is None:
            obs_begin = np.arange(len(hp) + 1, dtype=np.int32)
        self.n_landmarks = len(hp)
        self.t = dict(hp=_dev(hp), obs_begin=_dev(np.ascontiguousarray(obs_begin, dtype=np.int32)))
        self.desc = fe.make_landmark_table_device(self.n_landmarks, int(obs_begin[-1]), 0, self.t["hp"].data_ptr(), 0,
                                                  self.t["obs_begin"].data_ptr(), 0, 0, 0, 0)


def pack_frames(fe, frames):
    """(blocks [n, block_bytes] u8, landmark rows [n, K] int32 with PAST_COUNT_ROW at or past the count)"""
    from okvis2_amd import multigpu
    Kc = fe.max_keypoints
    blocks = np.stack([multigpu.pack_block_host(Kc, f["kps"], f["desc"], f["bp"], f["bpv"]) for f in frames])
    lm = np.full((len(frames), Kc), PAST_COUNT_ROW, np.int32)
    for i, f in enumerate(frames):
        lm[i, :len(f["lm"])] = f["lm"]
    return blocks, lm


def prepare_consensus(fe, sc, optional=True, alias=False):
    """the device tensors of a consensus call (synchronises)"""
    import torch
    frames = [f for mf in sc["mfs"] for f in mf["frames"]]
    B, nh = len(sc["mfs"]), len(sc["mfs"][0]["H"])
    blocks, lm = pack_frames(fe, frames)
    valid = None if sc["mfs"][0]["valid"] is None else np.stack([mf["valid"] for mf in sc["mfs"]]).astype(np.uint8)
    T = dict(blocks=_dev(blocks), lm=_dev(lm), H=_dev(np.stack([mf["H"] for mf in sc["mfs"]])),
             valid=None if valid is None else _dev(valid))
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
    T.update(n_corr=full((B,), SENTINEL, torch.int32), best=full((B,), SENTINEL, torch.int32),
             n_inl=full((B,), SENTINEL, torch.int32), accepted=full((B,), STATE_SENTINEL, torch.uint8))
    if optional:
        T.update(hyp_inliers=full((B, nh), SENTINEL, torch.int32),
                 state=full(lm.shape, STATE_SENTINEL, torch.uint8), distance=full(lm.shape, DIST_SENTINEL, torch.float64),
                 lm_out=T["lm"] if alias else full(lm.shape, SENTINEL, torch.int32))
    T["lm_in"] = lm
    torch.cuda.synchronize()
    return T


def launch_consensus(fe, tab, sc, T, remove_outliers=True, use_valid=True, stream=None, threshold=R.THRESHOLD,
                     first=0, count=None):
    """the call alone, on the multiframes [first, first + count): nothing here waits for the device"""
    n_cams, Kc, nh = len(sc["cams"]), fe.max_keypoints, len(sc["mfs"][0]["H"])
    count = len(sc["mfs"]) - first if count is None else count
    row = first * n_cams

    def at(key, per):
        t = T.get(key)
        return None if t is None else t.data_ptr() + first * per * t.element_size()

    res = fe.make_ransac_result_device(at("n_corr", 1), at("best", 1), at("n_inl", 1), at("accepted", 1),
                                       at("hyp_inliers", nh), at("state", n_cams * Kc), at("distance", n_cams * Kc),
                                       at("lm_out", n_cams * Kc))
    fe.ransac3d2d_consensus_blocks_device(
        tab.desc, T["blocks"].data_ptr() + row * T["blocks"].shape[1], count, list(range(n_cams)), sc["T_SC"],
        at("lm", n_cams * Kc), at("H", nh * 12), at("valid", nh) if use_valid else None, nh, res, threshold,
        remove_outliers, stream)


def check_consensus(sc, T, refs, what, alias=False, only=None):
    """every output of every multiframe against the reference; rows at or past a block's count untouched"""
    import torch
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in T.items() if isinstance(v, torch.Tensor)}
    n_cams = len(sc["cams"])
    for mi, (mf, ref) in enumerate(zip(sc["mfs"], refs)):
        if only is not None and mi not in only:
            continue
        w = what + (mi,)
        head = (int(got["n_corr"][mi]), int(got["best"][mi]), int(got["n_inl"][mi]), int(got["accepted"][mi]))
        assert head == (ref["n_corr"], ref["best"], ref["n_inliers"], ref["accepted"]), (w, head, ref["n_corr"],
                                                                                         ref["best"], ref["n_inliers"])
        if "state" not in got:
            continue
        assert np.array_equal(got["hyp_inliers"][mi], ref["hyp_inliers"]), (w, got["hyp_inliers"][mi], ref["hyp_inliers"])
        for c in range(n_cams):
            b, n = mi * n_cams + c, len(mf["frames"][c]["kps"])
            assert np.array_equal(got["state"][b, :n], ref["state"][c]), (w, c, "state")
            assert np.all(got["state"][b, n:] == STATE_SENTINEL), (w, c, "state past the count")
            ds = ref["dist_set"][c]
            gd, rd = got["distance"][b, :n], ref["distance"][c]
            assert np.array_equal(gd[ds].view(np.uint64), rd[ds].view(np.uint64)), (w, c, "distance", gd[ds][:4], rd[ds][:4])
            assert np.all(gd[~ds] == DIST_SENTINEL) and np.all(got["distance"][b, n:] == DIST_SENTINEL), (w, c)
            assert np.array_equal(got["lm_out"][b, :n], ref["landmark_out"][c]), (w, c, "landmark_out")
            past = PAST_COUNT_ROW if alias else SENTINEL
            assert np.all(got["lm_out"][b, n:] == past), (w, c, "landmark_out past the count")
    return got


def prepare_remove(fe, sc, alias=False):
    import torch
    blocks, lm = pack_frames(fe, sc["frames"])
    T = dict(blocks=_dev(blocks), lm=_dev(lm))
    T["lm_out"] = T["lm"] if alias else torch.full(lm.shape, SENTINEL, dtype=torch.int32, device="cuda")
    T["kept"] = torch.full((len(sc["frames"]),), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return T


def launch_remove(fe, tab, sc, T, max_error=R.MAX_ERROR, stream=None):
    fe.remove_outliers_blocks_device(tab.desc, T["blocks"].data_ptr(), len(sc["frames"]), sc["cam_ids"], sc["poses"],
                                     T["lm"].data_ptr(), T["lm_out"].data_ptr(), T["kept"].data_ptr(), max_error, stream)


def check_remove(sc, T, refs, what, alias=False):
    import torch
    torch.cuda.synchronize()
    lm_out, kept = T["lm_out"].cpu().numpy(), T["kept"].cpu().numpy()
    for f, (fr, (rl, rk)) in enumerate(zip(sc["frames"], refs)):
        n = len(fr["kps"])
        assert np.array_equal(lm_out[f, :n], rl), (what, f, np.flatnonzero(lm_out[f, :n] != rl)[:8])
        assert np.all(lm_out[f, n:] == (PAST_COUNT_ROW if alias else SENTINEL)), (what, f, "past the count")
        assert int(kept[f]) == rk, (what, f, int(kept[f]), rk)


# ---- the whole chain: first pass -> consensus -> removeOutliers -> second pass -----------------------------------
def chain_scene(oracle, tree, exclusive, thr, n_hyp=8, seed=51, cams=None, T_SC=None, sizes=((150, 250),)):
    """Multiframes of len(cams) cameras (default: the EuRoC pair, T_SC[0] the identity) on a map_scenes table, and the
    references of every step.  sizes: per multiframe (keypoints on not-yet-3-D landmarks, clutter of which 4 / 5 sit
    on 3-D landmarks) of every block.  T_WS is the scene's pose; the pose `now` of removeOutliers and of the second
    pass is map_table_uninit_common.second_pose of every block's first-pass pose.  Per block, multiframe-major:
    frames, poses1, poses2, refs1, first, removed, second; per multiframe: cons; H [n_mf, n_hyp, 12]."""
    import map_scenes
    import map_table_common as M
    import map_table_uninit_common as U
    sc = map_scenes.general_scene("euroc", 0)
    cams = list(synth.euroc_config().cams) if cams is None else cams
    T_WS = (np.asarray(sc["T1"][0], dtype=np.float64).reshape(-1), np.asarray(sc["T1"][1], dtype=np.float64))
    if T_SC is None:
        T_SC = [(np.eye(3).reshape(-1), np.zeros(3)), (rodrigues((0, 1, 0), 0.01).reshape(-1), np.array([0.11, 0.0, 0.0]))]
    n_cams = len(cams)
    pose1 = [compose(T_WS, t) for t in T_SC]
    ref1 = [M.reference(oracle, sc, p, c, exclusive, thr) for p, c in zip(pose1, cams)]
    out = dict(sc=sc, cams=cams, T_SC=T_SC, frames=[], poses1=[], poses2=[], refs1=[], first=[], removed=[], second=[],
               cons=[], H=[])
    for mi, (n2, clutter) in enumerate(sizes):
        frames = [U.frame(oracle, sc, ref1[c], cams[c], n2, clutter, seed + 10 * mi + c, n3d=4 * clutter // 5)
                  for c in range(n_cams)]
        first = [M.reference_matches(oracle, sc, ref1[c], thr, (f["kps"], f["desc"], f["use"]))[0]
                 for c, f in enumerate(frames)]
        H = hypotheses(T_WS, n_hyp, np.random.default_rng([seed, mi]), n_random=2)
        blocks = [dict(kps=f["kps"], bp=f["bp"], bpv=f["bv"]) for f in frames]
        cons = R.consensus(tree, sc["hp"], sc["obs_begin"], blocks, first, [c.fu for c in cams], T_SC, H)
        for c, f in enumerate(frames):
            p2 = U.second_pose(pose1[c])
            rem = R.remove_outliers(oracle, tree, sc["hp"], f["kps"], cons["landmark_out"][c], cams[c], p2)
            out["frames"].append(f), out["poses1"].append(pose1[c]), out["poses2"].append(p2)
            out["refs1"].append(ref1[c]), out["first"].append(first[c]), out["removed"].append(rem)
            out["second"].append(U.reference(oracle, sc["obs_desc"], ref1[c], dict(f, previous=rem[0]), p2, cams[c],
                                             exclusive))
        out["cons"].append(cons), out["H"].append(H)
    out["H"] = np.array(out["H"])
    return out
