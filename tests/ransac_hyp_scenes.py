"""Scenes for okvfe_ransac3d2d_hypotheses_blocks_device / okvfe_place_hypotheses_blocks_device and their restatement
ransac_hyp_ref.py, in the format of ransac_scenes.scene (every multiframe may carry a sample `key`):

  truth_scene      noise-free multiframes on the tables of ransac_scenes: every keypoint sits at the projection of its
                   landmark and its back-projection is the landmark's exact direction in the camera frame, so that the
                   chosen hypothesis of every sample is the scene's T_WS up to the solver's own error.
                   MEASURED (tests/test_ransac_hyp_ref.py, the four rigs of ransac_scenes.GENERAL_SPECS, 50 hypotheses
                   per multiframe, both orders of the sums): the worst |H - T_WS| over the 12 entries of a valid,
                   not excluded sample is TRUTH_WORST; the bound TRUTH_BOUND is that value times 8 (slack for other
                   seeds).  Excluded (near-degenerate, counted, at most 2 %): a sample whose three solver points
                   span a triangle with sin(smallest angle) < TRUTH_MIN_SINE, or of which two bearings are closer
                   than TRUTH_MIN_SINE (sine of the angle between them).
  general scenes   ransac_scenes.general_scene as it is (0.5 px of noise, 20 .. 40 % wrong rows): the solution counts.
  directed_scene   one camera; per case multiframes of four (or three) hand-placed correspondences whose points are
                   table rows with w = 1 and whose bearings are the block's back-projections, both exact: A4 == 0, the
                   biquadratic branch, the doubling cap (q q overflows), collinear points, two samples on one landmark,
                   a NaN hp, the (1, 0, 0) fall-back, fewer than four correspondences, ties (sigma = inf: every
                   distance is 0) and the all-NaN choice (a fourth sample with a NaN hp).  Where a case needs its
                   samples in the order they lie in the list, the multiframe's key is one under which many of the 64
                   hypotheses draw (0, 1, 2, 3): ordered_keys() finds them with the restated hash.
Test infrastructure only."""
import functools

import numpy as np

import ransac_hyp_ref as RH
import ransac_ref as R
import ransac_scenes as S

K = S.K
N_HYP = 50
SEED = 0x0123456789ABCDEF
TRUTH_MIN_SINE = 0.02
TRUTH_WORST = 4.85e-9    # measured 4.841e-9 under both orders: see the module docstring and DESIGN.md
TRUTH_BOUND = 8 * TRUTH_WORST
CENSUS_FLOOR = 16
CENSUS_CASES = ("sol0", "sol1", "sol2", "sol3", "sol4", "biquadratic", "a4_zero", "doubling_cap", "nc_below_4",
                "collinear", "same_landmark", "nan_hp", "bearing_fallback", "tie", "all_nan_choice")


def exact_frame(oracle, cam, T_WC, p_W, usable, n_kps, rng):
    """n_kps keypoints at projections of distinct landmarks; bp = the landmark in the camera frame, exactly"""
    C, r = np.asarray(T_WC[0]).reshape(3, 3), np.asarray(T_WC[1])
    kps = np.zeros(n_kps, dtype=oracle.KEYPOINT_DTYPE)
    lm = np.full(n_kps, -1, np.int32)
    bp = np.zeros((n_kps, 3))
    k = 0
    for l in rng.permutation(usable):
        if k >= n_kps:
            break
        d = C.T @ (p_W[l] - r)
        st, pt = R.project(oracle, cam, d)
        if st != 0:
            continue
        kps[k]["x"], kps[k]["y"] = pt
        lm[k], bp[k] = l, d
        k += 1
    kps, lm, bp = kps[:k], lm[:k], bp[:k]
    kps["size"] = rng.choice(np.array([12.0, 18.0, 24.0], np.float32), k)
    return dict(kps=kps, desc=rng.integers(0, 256, (k, 48), dtype=np.uint8), bp=bp, bpv=np.ones(k, np.uint8), lm=lm)


def truth_scene(oracle, spec, seed=0, n_mf=3):
    m = S.table(800)
    cams, T_SC = S.rig(spec)
    rng = np.random.default_rng([seed, len(cams), 77])
    usable = S.usable_rows(m)
    mfs = []
    for i in range(n_mf):
        T_WS = (m["T1"][0].reshape(3, 3) @ S.rodrigues((0, 1, 0), 0.02 * i), m["T1"][1] + np.array([0.05 * i, 0.0, 0.0]))
        frames = [exact_frame(oracle, cam, S.compose(T_WS, T_SC[c]), m["p"], usable, int(rng.integers(30, 120)), rng)
                  for c, cam in enumerate(cams)]
        mfs.append(dict(frames=frames, T_WS=T_WS, H=np.zeros((N_HYP, 12)), valid=None))
    return S.scene("truth-" + S.spec_id(spec), cams, T_SC, m["hp"], m["obs_begin"], mfs)


def near_degenerate(P, f):
    """the exclusion rule of the ground-truth test, on the three solver samples"""
    def sine(a, b):
        return np.linalg.norm(np.cross(a, b)) / (np.linalg.norm(a) * np.linalg.norm(b))
    with np.errstate(all="ignore"):
        tri = min(sine(P[1] - P[0], P[2] - P[0]), sine(P[0] - P[1], P[2] - P[1]), sine(P[0] - P[2], P[1] - P[2]))
        ray = min(sine(f[0], f[1]), sine(f[0], f[2]), sine(f[1], f[2]))
    return not (tri >= TRUTH_MIN_SINE and ray >= TRUTH_MIN_SINE)


# ---- the directed scene --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ordered_keys(count=4, n_hyp=64, seed=SEED, n_keys=20000):
    """the `count` keys below n_keys under which most of n_hyp hypotheses draw the positions (0, 1, 2, 3) from a list
    of four: r(0, 4) == 0, r(1, 3) == 0 and r(2, 2) == 0"""
    key = np.arange(n_keys, dtype=np.uint64)[:, None]
    h = np.arange(n_hyp, dtype=np.uint64)[None, :]
    hit = np.ones((n_keys, n_hyp), bool)
    with np.errstate(over="ignore"):
        for j, rng in ((0, 4), (1, 3), (2, 2)):
            z = np.uint64(seed) + (key * np.uint64(512) + h * np.uint64(8) + np.uint64(j + 1)) * np.uint64(0x9E3779B97F4A7C15)
            z ^= z >> np.uint64(30)
            z *= np.uint64(0xBF58476D1CE4E5B9)
            z ^= z >> np.uint64(27)
            z *= np.uint64(0x94D049BB133111EB)
            z ^= z >> np.uint64(31)
            hit &= (((z >> np.uint64(32)) * np.uint64(rng)) >> np.uint64(32)) == 0
    best = np.argsort(-hit.sum(axis=1), kind="stable")[:count]
    return [(int(k), int(hit[k].sum())) for k in best]


DIRECTED = {
    # name: (four points, four back-projections, ordered).  Points and bearings are exact in binary where it matters.
    "a4_zero": ([(0, 0, 4), (1, 0, 4), (0, 1, 4), (1, 1, 4)],          # a right angle at P1 (k = 1), f2 . f3 = 0
                [(0.6, 0, 0.8), (1, 0, 0), (0, 1, 0), (0.5, 0.5, 1)], True),
    "doubling_cap": ([(0, 0, 4), (1, 0, 4), (0, 1, 4), (1, 1, 4)],     # the same with f2 . f3 = 1e-60: A4 = -4e-120
                     [(0.6, 0, 0.8), (1, 0, 0), (1e-60, 1, 0), (0.5, 0.5, 1)], True),
    "biquadratic": ([(2, 0, 0), (1.5, 2, 0), (0, 0, 3), (1, 1, 1)],    # f3 at right angles to f1 and f2: A3 = A1 = 0
                    [(1, 0, 0), (0.6, 0.8, 0), (0, 0, 1), (1, 1, 1)], True),
    "collinear": ([(0, 0, 4), (1, 0, 4), (2, 0, 4), (4, 0, 4)],        # every three of the four on a line
                  [(0, 0, 4), (1, 0, 4), (2, 0, 4), (4, 0, 4)], False),
    "nan_hp": ([(0, 0, 4), (1, 0, 5), (0, 1, 6), (np.nan, 1, 4.5)],    # as a solver sample: a NaN coefficient; as the
               [(0, 0, 4), (1, 0, 5), (0, 1, 6), (1, 1, 4.5)], False),  # fourth: every distance a NaN
}


def _mf_of(oracle, P, bp, hp_rows, base, sizes=12.0, bpv=None, key=None, lm=None):
    n = len(bp)
    kps = np.zeros(n, dtype=oracle.KEYPOINT_DTYPE)
    kps["x"], kps["y"] = 100.0 + 10.0 * np.arange(n), 100.0
    kps["size"] = sizes
    if lm is None:
        lm = base + len(hp_rows) + np.arange(n)
        hp_rows.extend([*p, 1.0] for p in P)
    fr = dict(kps=kps, desc=np.zeros((n, 48), np.uint8), bp=np.asarray(bp, dtype=np.float64).reshape(n, 3),
              bpv=np.ones(n, np.uint8) if bpv is None else np.asarray(bpv, np.uint8), lm=np.asarray(lm, np.int32))
    return dict(frames=[fr], T_WS=(np.eye(3).reshape(-1), np.zeros(3)), H=np.zeros((64, 12)), valid=None, key=key)


def directed_scene(oracle):
    """-> the scene (one camera, 64 hypotheses per multiframe, every multiframe with a key)"""
    m = S.table()
    cams, T_SC = S.rig(("euroc",))
    base = len(m["hp"])
    rows, mfs = [], []
    keys = ordered_keys()
    for name, (P, bp, ordered) in DIRECTED.items():
        for i, (key, _) in enumerate(keys):
            mfs.append(_mf_of(oracle, P, bp, rows, base, key=key if ordered else 1000 + i))
    good_P = [(0, 0, 4), (1, 0, 5), (0, 1, 6), (1, 1, 4.5)]
    # two samples on one landmark: four keypoints, two of them on the same row
    mf = _mf_of(oracle, good_P, good_P, rows, base, key=2000)
    mf["frames"][0]["lm"][3] = mf["frames"][0]["lm"][0]
    mfs.append(mf)
    # the (1, 0, 0) fall-back: the back-projection of one keypoint failed
    mfs.append(_mf_of(oracle, good_P, good_P, rows, base, bpv=[1, 0, 1, 1], key=2001))
    # fewer than four correspondences in the camera
    mfs.append(_mf_of(oracle, good_P[:3], good_P[:3], rows, base, key=2002))
    # ties: sigma = inf (a keypoint of infinite size), every finite distance becomes 0
    for i in range(2):
        mfs.append(_mf_of(oracle, good_P, good_P, rows, base, sizes=np.inf, key=2003 + i))
    hp = np.concatenate([m["hp"], np.array(rows, dtype=np.float64)])
    obs_begin = np.concatenate([m["obs_begin"], m["obs_begin"][-1] + 1 + np.arange(len(rows))]).astype(np.int32)
    return S.scene("directed-hyp", cams, T_SC, hp, obs_begin, mfs)


def census_scenes(oracle):
    """every scene of the census: (scene, n_hyp)"""
    out = [(S.general_scene(oracle, spec), N_HYP) for spec in S.GENERAL_SPECS]
    out += [(truth_scene(oracle, spec), N_HYP) for spec in S.GENERAL_SPECS]
    out.append((directed_scene(oracle), 64))
    return out


def keys_of(sc):
    return [mf.get("key", i) if mf.get("key") is not None else i for i, mf in enumerate(sc["mfs"])]


def reference(tree, sc, n_hyp, seed=SEED, keys=None, place=False, gates=None, census=None, landmarks=None):
    """per multiframe ransac_hyp_ref.hypotheses (with its correspondences under "corr")"""
    fus = [c.fu for c in sc["cams"]]
    keys = keys_of(sc) if keys is None else keys
    obs_begin = np.arange(len(sc["hp"]) + 1) if place else sc["obs_begin"]
    out = []
    for i, mf in enumerate(sc["mfs"]):
        rows = [f["lm"] for f in mf["frames"]] if landmarks is None else landmarks[i]
        corr = R.correspondences(tree, sc["hp"], obs_begin, mf["frames"], rows, fus)
        ref = RH.hypotheses(tree, corr, sc["T_SC"], K, seed, int(keys[i]), n_hyp, None if gates is None else gates[i],
                            census, mf["frames"])
        ref["corr"] = corr
        out.append(ref)
    return out


# ---- GPU side --------------------------------------------------------------------------------------------------
H_SENTINEL = S.DIST_SENTINEL
BYTE_SENTINEL = S.STATE_SENTINEL


def prepare(fe, sc, n_hyp, keys=None, gates=None, optional=True, landmarks=None):
    """the device tensors of a hypotheses call over a scene (synchronises).  keys: None = the scene's own (every
    multiframe's `key`, its index where it has none; no key array at all if no multiframe has one)"""
    import torch
    frames = [f for mf in sc["mfs"] for f in mf["frames"]]
    if landmarks is not None:
        frames = [dict(f, lm=rows) for f, rows in zip(frames, (r for mf in landmarks for r in mf))]
    B = len(sc["mfs"])
    blocks, lm = S.pack_frames(fe, frames)
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
    T = dict(blocks=S._dev(blocks), lm=S._dev(lm), hp=S._dev(sc["hp"]),
             H=full((B, n_hyp, 12), H_SENTINEL, torch.float64), valid=full((B, n_hyp), BYTE_SENTINEL, torch.uint8))
    if optional:
        T.update(n_corr=full((B,), S.SENTINEL, torch.int32), samples=full((B, n_hyp, 4), S.SENTINEL, torch.int32),
                 n_sol=full((B, n_hyp), S.SENTINEL, torch.int32))
    if keys is None and any(mf.get("key") is not None for mf in sc["mfs"]):
        keys = keys_of(sc)
    T["keys"] = None if keys is None else S._dev(np.asarray(keys, dtype=np.uint64).view(np.int64))
    T["gate"] = None if gates is None else S._dev(np.asarray(gates, dtype=np.uint8))
    T["set"] = fe.make_place_set_device(len(sc["hp"]), T["hp"].data_ptr())
    torch.cuda.synchronize()
    return T


def launch(fe, tab, sc, T, seed=SEED, stream=None, first=0, count=None, place=False):
    """the call alone, on the multiframes [first, first + count): nothing here waits for the device"""
    n_cams, Kc, nh = len(sc["cams"]), fe.max_keypoints, T["H"].shape[1]
    count = len(sc["mfs"]) - first if count is None else count

    def at(key, per):
        t = T.get(key)
        return None if t is None else t.data_ptr() + first * per * t.element_size()

    res = fe.make_ransac_hypotheses_device(at("H", nh * 12), at("valid", nh), at("n_corr", 1), at("samples", nh * 4),
                                           at("n_sol", nh))
    blocks = T["blocks"].data_ptr() + first * n_cams * T["blocks"].shape[1]
    if place:
        fe.place_hypotheses_blocks_device(T["set"], blocks, count, list(range(n_cams)), sc["T_SC"], at("lm", n_cams * Kc),
                                          at("gate", 1), at("keys", 1), seed, nh, res, stream)
    else:
        fe.ransac3d2d_hypotheses_blocks_device(tab.desc, blocks, count, list(range(n_cams)), sc["T_SC"],
                                               at("lm", n_cams * Kc), at("keys", 1), seed, nh, res, stream)


def same_f64(a, b):
    """byte for byte, a NaN standing for any NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


def download(T):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in T.items() if isinstance(v, torch.Tensor)}


def check(sc, T, refs, what, only=None):
    """every output of every multiframe against the reference; multiframes outside `only` untouched"""
    got = download(T)
    for mi, ref in enumerate(refs):
        w = what + (mi,)
        if only is not None and mi not in only:
            assert np.all(got["H"][mi] == H_SENTINEL) and np.all(got["valid"][mi] == BYTE_SENTINEL), (w, "touched")
            if "samples" in got:
                assert got["n_corr"][mi] == S.SENTINEL and np.all(got["samples"][mi] == S.SENTINEL), (w, "touched")
                assert np.all(got["n_sol"][mi] == S.SENTINEL), (w, "touched")
            continue
        bad = np.flatnonzero([not same_f64(g, r) for g, r in zip(got["H"][mi], ref["H"])])
        assert not len(bad), (w, "hypotheses", bad[:8], got["H"][mi][bad[:1]], ref["H"][bad[:1]])
        assert np.array_equal(got["valid"][mi], ref["valid"]), (w, "hyp_valid")
        if "samples" in got:
            assert int(got["n_corr"][mi]) == ref["n_corr"], (w, "n_correspondences", int(got["n_corr"][mi]), ref["n_corr"])
            assert np.array_equal(got["samples"][mi], ref["samples"]), (w, "samples")
            assert np.array_equal(got["n_sol"][mi], ref["n_solutions"]), (w, "n_solutions")
    return got


# ---- the two chains ------------------------------------------------------------------------------------------------
CHAIN_SIZES = ((150, 250), (120, 200), (90, 300))
# The second chain's refined pose against the scene's true pose, (r, q) entry by entry, over the verified multiframes
# of place_scenes.general_scene(("euroc", "euroc1"), n_mf=7) (keypoints with pixel noise, so this is the accuracy of the
# refinement on that noise, not of the solver): MEASURED on the chain of restatements 2.843e-3 under both orders; the
# bound is that value times 8, as in the ground-truth test.
REFINED_WORST = 2.85e-3
REFINED_BOUND = 8 * REFINED_WORST


def first_chain_reference(tree, ch, K, n_hyp=N_HYP, seed=SEED):
    """ransac_scenes.chain_scene -> per multiframe (the hypotheses of the first pass's rows, the consensus over them)"""
    sc, n_cams = ch["sc"], len(ch["cams"])
    fus = [c.fu for c in ch["cams"]]
    out = []
    for mi in range(len(ch["frames"]) // n_cams):
        fr = ch["frames"][mi * n_cams:(mi + 1) * n_cams]
        first = ch["first"][mi * n_cams:(mi + 1) * n_cams]
        blocks = [dict(kps=f["kps"], bp=f["bp"], bpv=f["bv"]) for f in fr]
        corr = R.correspondences(tree, sc["hp"], sc["obs_begin"], blocks, first, fus)
        hyp = RH.hypotheses(tree, corr, ch["T_SC"], K, seed, mi, n_hyp)
        cons = R.consensus(tree, sc["hp"], sc["obs_begin"], blocks, first, fus, ch["T_SC"], hyp["H"], hyp["valid"])
        out.append((hyp, cons))
    return out


def second_chain_reference(oracle, tree, sc, prm, K, max_iterations, n_hyp=N_HYP, seed=SEED):
    """place_scenes.general_scene -> per multiframe (claims, hypotheses, consensus, refinement): the chain of the
    restatements from the matcher's rows to the refined pose"""
    import place_ref as P
    import place_refine_ref as PR
    import place_scenes as PS
    fus = [c.fu for c in sc["cams"]]
    out = []
    for mi, mf in enumerate(sc["mfs"]):
        counts = [len(f["kps"]) for f in mf["frames"]]
        cl = P.claim_stage(sc["hp"], counts, mf["kmin"], mf["dmin"], PS.MATCH_THRESHOLD, sc["min_inliers"])
        corr = R.correspondences(tree, sc["hp"], np.arange(len(sc["hp"]) + 1), mf["frames"], cl["match_landmark"], fus)
        hyp = RH.hypotheses(tree, corr, sc["T_SC"], K, seed, mi, n_hyp, gate=cl["gate"])
        co = P.consensus(tree, sc["hp"], mf["frames"], cl["match_landmark"], fus, sc["T_SC"], hyp["H"], hyp["valid"],
                         cl["gate"], sc["min_inliers"])
        ref = PR.refine(oracle, tree, sc["hp"], mf["frames"], cl["match_landmark"], co["state"], sc["cams"], prm, hyp["H"],
                        co["best"], None, max_iterations, co["verdict"] == 3)
        out.append((cl, hyp, co, ref))
    return out
