"""Scenes and device plumbing for okvfe_ransac2d2d_hypotheses_blocks_device (the hypotheses of Frontend::runRansac2d2d
on device batches).  A scene is one of ransac2d2d_scenes (the hypothesis lists its pairs carry are not read here).

  solver_scene      eight noise-free bearing pairs of a general motion, with the true [R | t / |t|]
  count_scene       one camera; pairs with 0, 1, 9, 10, 11, 64, 65 and K correspondences, then ransac2d2d_scenes'
                    block edges (blocks of 0, 1 and K keypoints)
  directed_scene    one camera, twelve correspondences a pair, so that most samples meet the special rows: a pure
                    rotation, a planar scene, duplicate bearings, bearings on one great circle, a NaN back-projection,
                    failed back-projections (the adapter's (1, 0, 0)), a general pair for comparison, and bearings
                    that no motion relates (a sample whose polynomial has no real root)
  motion_scene      one camera: a general motion with 10 % wrong ids and a pure rotation (the chain's two outcomes)

The reference of hypothesis h does not depend on n_hyp: `reference` solves OKVFE_RANSAC_MAX_HYPOTHESES per (pair,
camera) once per (scene, order, seed, keys) and the tests slice it.  CPU only up to `prepare` / `launch`, which need
torch and a GPU.  Test infrastructure only."""
import numpy as np

import ransac2d2d_hyp_ref as H2
import ransac2d2d_ref as R2
import ransac2d2d_scenes as S2
import ransac_scenes as S
from gate_scenes import rodrigues

K = S2.K
MAX_HYP = 64          # OKVFE_RANSAC_MAX_HYPOTHESES
SEED = 0x2D2D5EED0BADC0DE
SENTINEL, STATE_SENTINEL, DIST_SENTINEL = S2.SENTINEL, S2.STATE_SENTINEL, S2.DIST_SENTINEL


# ---- the solver alone ----------------------------------------------------------------------------------------------
def solver_scene(seed, rotation_only=False, planar=False, n=8):
    """-> (R, t, b1 [n, 3], b2 [n, 3]) with p_older = R p_current + t, |t| = 1 (0 with rotation_only), exact bearings.
    planar: the first five points lie on one plane (two physical solutions), the others do not"""
    rng = np.random.default_rng([seed, 77])
    Rm = rodrigues(rng.normal(size=3), rng.uniform(0.02, 0.5))
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    if rotation_only:
        t = np.zeros(3)
    P1 = np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(3, 9, n)], axis=1)
    if planar:
        nrm = rng.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        nrm[2] = abs(nrm[2]) + 1.0
        d = P1 / np.linalg.norm(P1, axis=1, keepdims=True)
        P1[:5] = (d * (6.0 / (d @ nrm))[:, None])[:5]   # the five solved points on the plane nrm . p = 6, the rest off it
    P2 = (P1 - t) @ Rm                                # R^T (p1 - t), row-wise
    b1 = P1 / np.linalg.norm(P1, axis=1, keepdims=True)
    b2 = P2 / np.linalg.norm(P2, axis=1, keepdims=True)
    return Rm, t, b1, b2


def pose_error(Hm, Rm, t):
    """the worst entry of [R | t / |t|] against the hypothesis"""
    Hm = np.asarray(Hm).reshape(3, 4)
    return float(max(np.abs(Hm[:, :3] - Rm).max(), np.abs(Hm[:, 3] - t).max()))


# ---- scenes for the device call ------------------------------------------------------------------------------------
def _entry(fr0, fr1, **extra):
    rot_H, rel_H = S2.lists("true first")
    return S2.cam_entry(fr0, fr1, rot_H, rel_H, **extra)


COUNTS = (0, 1, 9, 10, 11, 64, 65, K)


def count_scene(oracle, seed=71):
    rng = np.random.default_rng(seed)
    pairs = []
    for n in COUNTS:
        nD = n // 8
        fr0, fr1, _ = S2.hand_camera(oracle, rng, 0, 0, n - nD, nD, free0=min(7, K - n), free1=min(5, K - n))
        pairs.append([_entry(fr0, fr1)])
    pairs += S2.edge_scene(oracle)["pairs"]
    return S2.scene("hyp-counts", S2.euroc_pair()[:1], pairs)


def _bearing_pair(oracle, rng, b1, b2, free0=2, free1=3):
    """blocks whose matched rows carry the given back-projections (scaled: a block's rows are not normalised)"""
    n = len(b1)
    ids = 11 + 5 * np.arange(n)
    rows0, rows1 = rng.permutation(n + free0)[:n], rng.permutation(n + free1)[:n]
    fr0, fr1 = S2._frame(oracle, n + free0, rng), S2._frame(oracle, n + free1, rng)
    fr0["bp"][:] = rng.normal(size=(n + free0, 3))
    fr1["bp"][:] = rng.normal(size=(n + free1, 3))
    fr0["bp"][rows0], fr0["lm"][rows0] = b1 * rng.uniform(0.5, 2.0, (n, 1)), ids
    fr1["bp"][rows1], fr1["lm"][rows1] = b2 * rng.uniform(0.5, 2.0, (n, 1)), ids
    return fr0, fr1, rows0, rows1


DIRECTED = ("general", "rotation", "planar", "duplicates", "great_circle", "nan", "fallback", "unrelated")
NO_ROOT_SEED = 254   # of the family of test_ransac2d2d_hyp_ref.test_a_polynomial_without_a_real_root


def no_root_bearings(n):
    """bearing pairs that no motion relates: the five solved pairs of NO_ROOT_SEED, whose degree-10 polynomial has no
    real root, each two or three times with a perturbation of 1e-4 (exact copies would fail a pivot).  A sample that
    draws one pair of each of the five clusters as its first five, about one in eleven, reaches that branch."""
    u = np.random.default_rng([NO_ROOT_SEED, 5])
    b1, b2 = u.normal(size=(8, 3)), u.normal(size=(8, 3))
    rep = np.arange(n) % 5
    jit = np.random.default_rng([NO_ROOT_SEED, 6]).normal(size=(2, n, 3)) * 1.0e-4
    b1, b2 = b1[rep] / np.linalg.norm(b1[rep], axis=1, keepdims=True) + jit[0], b2[rep] / np.linalg.norm(b2[rep], axis=1, keepdims=True) + jit[1]
    return b1 / np.linalg.norm(b1, axis=1, keepdims=True), b2 / np.linalg.norm(b2, axis=1, keepdims=True)


def directed_scene(oracle, seed=5, n=12):
    rng = np.random.default_rng(seed)
    pairs = []
    for kind in DIRECTED:
        Rm, t, b1, b2 = solver_scene(seed + len(pairs), rotation_only=kind == "rotation", planar=kind == "planar", n=n)
        if kind == "duplicates":
            b1[: n // 2], b2[: n // 2] = b1[0], b2[0]
        if kind == "great_circle":
            a = np.linspace(-0.5, 0.5, n)
            b1 = np.stack([np.sin(a), np.zeros(n), np.cos(a)], axis=1)
            b2 = b1 @ Rm
        if kind == "unrelated":
            b1, b2 = no_root_bearings(n)
        fr0, fr1, rows0, rows1 = _bearing_pair(oracle, rng, b1, b2)
        if kind == "nan":
            fr0["bp"][rows0[:2], 1] = np.nan
            fr1["bp"][rows1[2], 0] = np.nan
        if kind == "fallback":
            fr0["bpv"][rows0[:4]] = 0
            fr1["bpv"][rows1[4:6]] = 0
        pairs.append([_entry(fr0, fr1, truth=(Rm, t))])
    return S2.scene("hyp-directed", S2.euroc_pair()[:1], pairs)


def motion_scene(oracle, seed=9, n=120, wrong=0.10):
    """pair 0: a general motion, `wrong` of the current ids swapped among themselves; pair 1: a pure rotation"""
    rng = np.random.default_rng(seed)
    pairs = []
    for rotation_only in (False, True):
        Rm, t, b1, b2 = solver_scene(seed + len(pairs), rotation_only=rotation_only, n=n)
        if rotation_only:
            Rm = rodrigues((0.2, 1.0, 0.1), 0.08)
            b2 = b1 @ Rm
        else:
            t = 0.2 * t   # (the bearings do not depend on |t|; kept for the truth)
        fr0, fr1, rows0, rows1 = _bearing_pair(oracle, rng, b1, b2, free0=6, free1=9)
        if not rotation_only:
            bad = rng.permutation(n)[: int(round(wrong * n))]
            fr1["lm"][rows1[bad]] = fr1["lm"][rows1[np.roll(bad, 1)]]
        pairs.append([_entry(fr0, fr1, truth=(Rm, t))])
    return S2.scene("hyp-motion", S2.euroc_pair()[:1], pairs)


# ---- the reference -------------------------------------------------------------------------------------------------
_REFS = {}


def reference(tree, sc, keys=None, seed=SEED, census=None, tag=None):
    """per pair, per camera: ransac2d2d_hyp_ref.hypotheses with MAX_HYP hypotheses (cached per scene name / tag)"""
    keys = list(range(len(sc["pairs"]))) if keys is None else [int(k) for k in keys]
    ck = (sc["name"] if tag is None else tag, bool(tree), seed, tuple(keys))
    if ck in _REFS and census is None:
        return _REFS[ck]
    fus = [c.fu for c in sc["cams"]]
    out = []
    for pair, key in zip(sc["pairs"], keys):
        cams = []
        for c, cam in enumerate(pair):
            corr = R2.correspondences(tree, cam["fr0"], cam["fr1"], fus[c], sc["added"])
            cams.append(dict(H2.hypotheses(tree, corr, seed, key, c, MAX_HYP, census), corr=corr))
        out.append(cams)
    _REFS[ck] = out
    return out


def directed_reference(tree, sc):
    """(references, census per kind) of directed_scene, every pair solved under its own census and its own index as key"""
    refs, census = [], {}
    for i, kind in enumerate(DIRECTED):
        census[kind] = H2.new_census()
        refs += reference(tree, dict(sc, pairs=sc["pairs"][i:i + 1]), keys=[i], census=census[kind], tag=sc["name"] + "/" + kind)
    return refs, census


def assert_directed_branches(refs, census):
    """every directed pair reaches the branch it was built for (figures of the restatement, so a changed seed that loses
    a case fails here)"""
    by = {k: (refs[i][0], census[k]) for i, k in enumerate(DIRECTED)}
    failed = lambda c: c["null_pivot"] + c["elim_pivot"]
    r, c = by["general"]
    assert r["rel_valid"].all() and r["rot_valid"].all() and failed(c) == 0 and c["no_root"] == 0, c
    r, c = by["rotation"]
    assert c["bad_lead"] + c["elim_pivot"] > 0 and c["rel_valid"] > 0 and r["rot_valid"].all(), c
    r, c = by["planar"]
    assert r["rel_valid"].all() and r["n_roots"].min() >= 2, c
    r, c = by["duplicates"]
    assert failed(c) > 0 and c["rot_zero_cross"] + c["rot_nonfinite"] > 0, c
    r, c = by["great_circle"]
    assert not r["rel_valid"].any() and failed(c) == MAX_HYP, c
    r, c = by["nan"]
    assert c["nan_bearing"] > 0 and c["rel_valid"] < MAX_HYP // 4 and c["rot_valid"] < MAX_HYP, c
    r, c = by["fallback"]
    assert c["fallback_bearing"] > 0 and c["null_pivot"] > 0, c
    r, c = by["unrelated"]
    assert c["no_root"] >= 2 and int(((r["n_roots"] == 0) & (r["rel_valid"] == 0)).sum()) == c["no_root"] + failed(c) + c["bad_lead"], c


# ---- GPU side ------------------------------------------------------------------------------------------------------
OUT = dict(rot_H=(9, "f8"), rot_valid=(None, "u1"), rel_H=(12, "f8"), rel_valid=(None, "u1"), rot_samples=(2, "i4"),
           rel_samples=(8, "i4"), n_roots=(None, "i4"))
REF_KEY = dict(rot_H="rot_H", rot_valid="rot_valid", rel_H="rel_H", rel_valid="rel_valid", rot_samples="rot_samples",
               rel_samples="rel_samples", n_roots="n_roots")
OPTIONAL = ("n_corr", "rot_samples", "rel_samples", "n_roots")


def prepare(fe, sc, n_hyp, optional=True, keys=None, merged=False):
    """the device tensors of a call (synchronises)"""
    import torch
    dev = S._dev
    P, n_cams = len(sc["pairs"]), len(sc["cams"])
    b0, l0, b1, l1 = S2.pack(fe, sc)
    if merged:
        blocks, lm = dev(np.concatenate([b0, b1])), dev(np.concatenate([l0, l1]))
        T = dict(blocks0=blocks, blocks1=blocks, lm0=lm, lm1=lm, n_mf0=2 * P, n_mf1=2 * P, mf1_base=P)
    else:
        T = dict(blocks0=dev(b0), blocks1=dev(b1), lm0=dev(l0), lm1=dev(l1), n_mf0=P, n_mf1=P, mf1_base=0)
    T["added"] = None if sc["added"] is None else dev(sc["added"])
    T["keys"] = None if keys is None else torch.tensor(np.asarray(keys, np.uint64).view(np.int64), device="cuda")
    dt = {"f8": torch.float64, "u1": torch.uint8, "i4": torch.int32}
    fill = {"f8": DIST_SENTINEL, "u1": STATE_SENTINEL, "i4": SENTINEL}
    for key, (width, kind) in OUT.items():
        if key in OPTIONAL and not optional:
            continue
        shape = (P, n_cams, n_hyp) + (() if width is None else (width,))
        T[key] = torch.full(shape, fill[kind], dtype=dt[kind], device="cuda")
    if optional:
        T["n_corr"] = torch.full((P, n_cams), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return T


def launch(fe, sc, T, n_hyp, seed=SEED, stream=None, first=0, count=None):
    """the call alone, on the pairs [first, first + count): nothing here waits for the device"""
    P, n_cams = len(sc["pairs"]), len(sc["cams"])
    count = P - first if count is None else count

    def at(key, per):
        t = T.get(key)
        return None if t is None else t.data_ptr() + first * per * t.element_size()

    per = n_cams * n_hyp
    res = fe.make_ransac2d2d_hypotheses_device(at("rot_H", per * 9), at("rot_valid", per), at("rel_H", per * 12),
                                               at("rel_valid", per), at("n_corr", n_cams), at("rot_samples", per * 2),
                                               at("rel_samples", per * 8), at("n_roots", per))
    mf0 = np.arange(first, first + count, dtype=np.int32)
    fe.ransac2d2d_hypotheses_blocks_device(
        T["blocks0"].data_ptr(), T["n_mf0"], T["blocks1"].data_ptr(), T["n_mf1"], mf0, mf0 + T["mf1_base"],
        list(range(n_cams)), T["lm0"].data_ptr(), T["lm1"].data_ptr(),
        None if T["added"] is None else T["added"].data_ptr(), sc["n_landmarks"], at("keys", 1), seed, n_hyp, res, stream)


def download(T):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in T.items() if isinstance(v, torch.Tensor) and k in tuple(OUT) + ("n_corr",)}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def check(sc, T, refs, what, n_hyp, only=None):
    """every output of every pair against the reference, byte for byte"""
    got = download(T)
    for pi, ref in enumerate(refs):
        if only is not None and pi not in only:
            continue
        for c, rc in enumerate(ref):
            if "n_corr" in got:
                assert int(got["n_corr"][pi, c]) == rc["n_corr"], (what, pi, c, "n_corr", got["n_corr"][pi, c], rc["n_corr"])
            for key in OUT:
                if key not in got:
                    continue
                g, r = got[key][pi, c], rc[REF_KEY[key]][:n_hyp]
                if not np.array_equal(bits(g), bits(r)):
                    h = int(np.flatnonzero((bits(g) != bits(r)).reshape(n_hyp, -1).any(axis=1))[0])
                    raise AssertionError((what, pi, c, key, "hypothesis", h, g[h], r[h]))
    return got
