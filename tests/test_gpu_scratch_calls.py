"""GPU: the eleven entry points that take the caller's host arrays (okvfe_match_stereo, okvfe_match_motion_stereo_ext,
okvfe_match_to_map, okvfe_match_to_map_landmarks, okvfe_match_to_map_uninitialised, okvfe_verify_place_match,
okvfe_fbrisk_transform, okvfe_bow_query_l1, okvfe_hamming_candidates, okvfe_hamming_argmin, okvfe_keyframe_coverage)
share one scratch buffer and one pinned block per context, laid out anew by every call (ScratchLayout / ScratchCall,
okvfe_ctx.h).  Here ONE context runs all of them interleaved, small -> large -> small: the large calls (700 keypoints,
1800 landmarks) grow both blocks, the small ones (1 to 3 keypoints or landmarks) then run in an oversized buffer full of
stale bytes of another call's layout.  Then the empty shapes, each with the result the entry point defines for it.

Every result is compared exactly (doubles as bit patterns) with the CPU oracle -- keyframe_ref.py for the coverage --,
never with another run of the library."""
import os

import numpy as np
import pytest

import gpu_common as G
import keyframe_ref as KR
import map_synth
from okvis2_amd import synth

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
SIZES = {"small": dict(n_kps=3, n_lm=2, n_db=2), "large": dict(n_kps=700, n_lm=1800, n_db=300)}


def _observe(oracle, cam, X, T, rng, n):
    Cm = np.asarray(T[0]).reshape(3, 3)
    Xc = (X - np.asarray(T[1])) @ Cm
    kp = np.zeros(n, dtype=oracle.KEYPOINT_DTYPE)
    kp["size"] = 12.0
    for i in range(n):
        st, pt, _ = oracle.cam_project(cam, Xc[i])
        kp["x"][i], kp["y"][i] = pt if st == 0 else (5.0, 5.0)
    kp["x"] += rng.normal(0, 0.3, n).astype(np.float32)
    kp["y"] += rng.normal(0, 0.3, n).astype(np.float32)
    bp, bv = oracle.backproject_keypoints(cam, kp)
    return kp, bp, bv


def _build(oracle, cfg, voc, tree, n_kps, n_lm, n_db, seed):
    """the inputs of every entry point at one size, and what the oracle says of them"""
    cam, thr = cfg.cams[0], cfg.match_threshold
    rng = np.random.default_rng(seed)
    s = {"cam": cam}
    # two frames of one scene: the stereo and the motion matcher
    n = n_kps
    T0 = (np.eye(3).reshape(-1), np.zeros(3))
    th = 0.05
    Rz = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]])
    T1 = (Rz.reshape(-1), np.array([0.35, 0.04, 0.02]))
    X = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-0.8, 0.8, n), rng.uniform(2.5, 9, n)], 1)
    kp0, bp0, bv0 = _observe(oracle, cam, X, T0, rng, n)
    kp1, bp1, bv1 = _observe(oracle, cam, X, T1, rng, n)
    d0 = rng.integers(0, 256, (n, 48), dtype=np.uint8)
    d1 = d0 ^ (rng.random((n, 48)) < 0.03).astype(np.uint8) * rng.integers(0, 256, (n, 48), dtype=np.uint8)
    perm = rng.permutation(n)
    d1, kp1, bp1, bv1 = d1[perm], kp1[perm], bp1[perm], bv1[perm]
    skip0 = (rng.random(n) < 0.1).astype(np.uint8)
    matched1 = (rng.random(n) < 0.1).astype(np.uint8)
    f = 0.5 * (cam.fu + cam.fv)
    s["pair"] = (d0, kp0, bp0, bv0, d1, kp1, bp1, bv1)
    s["T"], s["f"], s["flags"] = (T0, T1), f, (skip0, matched1)
    s["stereo"] = oracle.match_stereo(d0, kp0, bp0, bv0, d1, kp1, bp1, bv1, T0, T1, f, f, thr)
    s["motion"] = [oracle.match_motion_stereo(d0, kp0, bp0, bv0, a, d1, kp1, bp1, bv1, b, T0, T1, cam, thr)
                   for a, b in ((skip0, matched1), (None, None))]
    # 3-D landmarks with a pool of descriptors: matchToMap, and the same pool for verifyRecognisedPlace
    counts = rng.integers(1, 4, n_lm)
    begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    pool = rng.integers(0, 256, (begin[-1], 48), dtype=np.uint8)
    proj = np.stack([rng.uniform(0, cfg.w, n_lm), rng.uniform(0, cfg.h, n_lm)], 1)
    for l in range(min(n, n_lm)):
        proj[l] = (kp0["x"][l] + rng.normal(0, 3), kp0["y"][l] + rng.normal(0, 3))
        pool[begin[l]] = d0[l] ^ ((rng.random(48) < 0.05) * rng.integers(0, 256, 48)).astype(np.uint8)
    use = (rng.random(n) > 0.15).astype(np.uint8)
    use[0] = 1
    s["map"] = (d0, kp0, use, proj, begin, pool)
    s["map_ref"] = oracle.match_to_map(d0, kp0, use, proj, begin, pool, 20.0, thr)
    s["place_ref"] = oracle.verify_place(pool, begin, d0, thr)
    # landmarks that are not 3-D yet: rays of earlier observations
    m = int(begin[-1])
    r0 = rng.normal(0, 0.3, (m, 3)) + np.array([-0.2, 0, 0])
    e0 = np.zeros((m, 3))
    for l in range(n_lm):
        for d in range(begin[l], begin[l + 1]):
            ray = X[l % n] - r0[d] + rng.normal(0, 0.002, 3)
            e0[d] = ray / np.linalg.norm(ray)
    previous = np.full(n, -1, dtype=np.int32)
    previous[::3] = np.arange(n)[::3] % n_lm
    s["uninit"] = (d0, bp0, use & bv0, previous, begin, pool, e0, r0, T0, f)
    s["uninit_ref"] = oracle.match_to_map_uninit(d0, bp0, use & bv0, previous, begin, pool, e0, r0, T0, f, thr)
    # the raw landmark table
    mp = map_synth.make_map(n_lm, voc=voc, seed=seed)
    kps, desc, fuse = map_synth.make_frame(mp, oracle, n_kps=n, seed=seed + 1)
    s["table"] = (mp, kps, desc, fuse)
    ref = oracle.prepare_landmarks(mp["hp"], mp["quality"], mp["obs_begin"], mp["obs_pose"], mp["obs_bp"], mp["poses"],
                                   mp["T1"], mp["cam"], 20.0, False)
    idx, tproj, tbegin, rows = map_synth.packed_set(ref, mp["obs_desc"], 1)
    rl, rd = oracle.match_to_map(desc, kps, fuse, tproj, tbegin, rows, 20.0, thr)
    s["table_ref"] = (ref, np.where(rl >= 0, idx[np.maximum(rl, 0)], -1) if len(idx) else rl, rd)
    # vocabulary descent and the L1 query
    cb, ci = oracle.voc_tree_arrays(tree["parent"])
    feats = np.concatenate([d0, voc])[:n]
    s["voc"] = (feats, tree["desc"], cb, ci, tree["word"])
    s["voc_ref"] = oracle.voc_transform(feats, tree["desc"], cb, ci, tree["word"])
    n_words = int(tree["word"].max()) + 1
    entries = []
    for _ in range(n_db + 1):
        ids = np.sort(rng.choice(n_words, int(rng.integers(1, min(200, n_words))), replace=False)).astype(np.int32)
        v = rng.random(len(ids)) + 0.01
        entries.append((ids, v / v.sum()))
    q = entries.pop()
    dbb = np.concatenate([[0], np.cumsum([len(e[0]) for e in entries])]).astype(np.int32)
    dbi = np.concatenate([e[0] for e in entries]).astype(np.int32)
    dbv = np.concatenate([e[1] for e in entries])
    s["bow"] = (dbb, dbi, dbv, q[0], q[1])
    s["bow_ref"] = oracle.bow_query_l1(dbb, dbi, dbv, q[0], q[1], n_words)
    # plain Hamming scans
    A, B = d0, np.concatenate([d1, voc])[:max(2 * n // 3, 1)]
    s["ham"] = (A, B)
    s["ham_ref"] = (oracle.hamming_candidates(A, B, 90), oracle.hamming_argmin(A, B, 90))
    # coverage masks
    ids = rng.integers(1, 1 << 62, n).astype(np.uint64)
    ids[rng.random(n) < 0.5] = 0
    ids[0] = 7
    id_set = np.concatenate([ids[::2], rng.integers(1, 1 << 62, 3 * n).astype(np.uint64)])
    s["cov"] = (kp0, ids, id_set)
    s["cov_ref"] = (KR.coverage(cfg.w, cfg.h, kp0, ids, None), KR.coverage(cfg.w, cfg.h, kp0, ids, id_set))
    return s


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_motion(got, ref):
    for fld in ("k1", "dist", "initialisable", "accepted"):
        assert np.array_equal(got[fld], ref[fld]), fld
    assert np.array_equal(_bits(got["hp_W"]), _bits(ref["hp_W"]))


def _calls(fe, s):
    """the eleven entry points on one scene, one closure each"""
    T0, T1 = s["T"]
    cam = s["cam"]

    def stereo():
        got = fe.match_stereo(*s["pair"], T0, T1, s["f"], s["f"])
        assert np.array_equal(got.view(np.uint8), s["stereo"].view(np.uint8))

    def motion():
        d0, kp0, bp0, bv0, d1, kp1, bp1, bv1 = s["pair"]
        for (a, b), ref in zip((s["flags"], (None, None)), s["motion"]):
            _same_motion(fe.match_motion_stereo(cam, d0, kp0, bp0, bv0, a, d1, kp1, bp1, bv1, b, T0, T1), ref)

    def to_map():
        gl, gd = fe.match_to_map(*s["map"], 20.0)
        assert np.array_equal(gl, s["map_ref"][0]) and np.array_equal(gd, s["map_ref"][1])

    def landmarks():
        mp, kps, desc, use = s["table"]
        ref, rl, rd = s["table_ref"]
        lm, bd, pool = fe.match_to_map_landmarks(0, mp["hp"], mp["quality"], mp["obs_begin"], mp["obs_pose"],
                                                 mp["obs_desc"], mp["obs_bp"], mp["poses"], mp["T1"], 20.0, False, desc,
                                                 kps, use)
        for k in ("status", "n_desc", "obs_rows"):
            assert np.array_equal(pool[k], ref[k]), k
        for k in ("projection", "e_W", "r_W"):
            assert np.array_equal(_bits(pool[k]), _bits(ref[k])), k
        assert np.array_equal(lm, rl) and np.array_equal(bd, rd)

    def uninit():
        got, ref = fe.match_to_map_uninitialised(*s["uninit"]), s["uninit_ref"]
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[3], ref[3])
        assert np.array_equal(_bits(got[2]), _bits(ref[2])) and got[4] == ref[4]

    def place():
        _, _, _, _, begin, pool = s["map"]
        gk, gd = fe.verify_place_match(pool, begin, s["map"][0])
        assert np.array_equal(gk, s["place_ref"][0]) and np.array_equal(gd, s["place_ref"][1])

    def descent():
        gw, gn = fe.fbrisk_transform(*s["voc"])
        assert np.array_equal(gw, s["voc_ref"][0]) and np.array_equal(gn, s["voc_ref"][1])

    def query():
        assert np.array_equal(_bits(fe.bow_query_l1(*s["bow"])), _bits(s["bow_ref"]))

    def candidates():
        got, n = fe.hamming_candidates(*s["ham"], 90)
        assert n == len(s["ham_ref"][0]) and np.array_equal(got, s["ham_ref"][0])

    def argmin():
        gj, gd = fe.hamming_argmin(*s["ham"], 90)
        assert np.array_equal(gj, s["ham_ref"][1][0]) and np.array_equal(gd, s["ham_ref"][1][1])

    def coverage():
        kps, ids, id_set = s["cov"]
        for got, want in zip((fe.keyframe_coverage(kps, ids), fe.keyframe_coverage(kps, ids, id_set)), s["cov_ref"]):
            assert {k: int(got[k]) for k in KR.COVERAGE_FIELDS} == want

    return [stereo, motion, to_map, landmarks, uninit, place, descent, query, candidates, argmin, coverage]


@pytest.fixture(scope="module")
def scenes(oracle):
    cfg = synth.euroc_config()
    assert cfg.max_kpts == SIZES["large"]["n_kps"]
    voc = np.fromfile(os.path.join(GOLD, "small_voc_desc.bin"), dtype=np.uint8).reshape(-1, 48)
    tree = np.load(os.path.join(GOLD, "small_voc_tree.npz"))
    return cfg, {name: _build(oracle, cfg, voc, tree, seed=31 + i, **size) for i, (name, size) in enumerate(SIZES.items())}


def test_the_references_discriminate(scenes):
    """(no GPU work: what the large scene's oracle results hold, so that an exact comparison means something)"""
    _, sc = scenes
    L = sc["large"]
    assert (L["stereo"]["k1"] >= 0).sum() > 100 and (L["motion"][0]["k1"] >= 0).sum() > 100
    assert (L["map_ref"][0] >= 0).sum() > 100 and (L["uninit_ref"][0] >= 0).sum() > 50
    assert (L["place_ref"][1] < 60).sum() > 300 and (L["table_ref"][1] >= 0).sum() > 50
    assert len(np.unique(L["voc_ref"][0])) > 100 and (L["bow_ref"] >= 0).sum() > 100
    assert len(L["ham_ref"][0]) > 100 and (L["ham_ref"][1][0] >= 0).sum() > 100
    assert 0 < L["cov_ref"][1]["n_matched"] < L["cov_ref"][0]["n_matched"]
    for name in ("stereo", "map_ref", "uninit_ref", "place_ref", "voc_ref", "bow_ref"):
        ref = sc["small"][name]
        assert len(ref if isinstance(ref, np.ndarray) else ref[0]) in (2, 3), name


def test_small_large_small_on_one_context(oracle, scenes):
    cfg, sc = scenes
    fe = G.make_frontend(cfg)
    fe.set_camera(0, cfg.cams[0])
    small, large = _calls(fe, sc["small"]), _calls(fe, sc["large"])
    for call in small:           # a fresh context: every call sizes the blocks for itself
        call()
    for call in large:           # both blocks grow, several times
        call()
    for call in reversed(small):  # oversized blocks, stale bytes of the large layouts, another order of entry points
        call()
    for a, b in zip(large, small):  # ... and strictly alternating
        a()
        b()


def test_empty_shapes_between_full_calls(oracle, scenes):
    """the shapes every entry point now skips in one way, each with the result it defines"""
    cfg, sc = scenes
    thr = cfg.match_threshold
    fe = G.make_frontend(cfg)
    fe.set_camera(0, cfg.cams[0])
    L = sc["large"]
    large = _calls(fe, L)
    for call in large:  # stale bytes everywhere first
        call()
    d0, kp0, bp0, bv0, d1, kp1, bp1, bv1 = L["pair"]
    T0, T1 = L["T"]
    cam = cfg.cams[0]
    n = len(kp0)
    # n1 = 0: nothing to match against; n0 = 0: nothing asked
    got = fe.match_stereo(d0, kp0, bp0, bv0, d1[:0], kp1[:0], bp1[:0], bv1[:0], T0, T1, L["f"], L["f"])
    want = oracle.match_stereo(d0, kp0, bp0, bv0, d1[:0], kp1[:0], bp1[:0], bv1[:0], T0, T1, L["f"], L["f"], thr)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)) and np.all(got["k1"] == -1)
    assert len(fe.match_stereo(d0[:0], kp0[:0], bp0[:0], bv0[:0], d1, kp1, bp1, bv1, T0, T1, L["f"], L["f"])) == 0
    # skip0 / matched1 = None with n1 = 0
    got = fe.match_motion_stereo(cam, d0, kp0, bp0, bv0, None, d1[:0], kp1[:0], bp1[:0], bv1[:0], None, T0, T1)
    _same_motion(got, oracle.match_motion_stereo(d0, kp0, bp0, bv0, None, d1[:0], kp1[:0], bp1[:0], bv1[:0], None, T0, T1,
                                                 cam, thr))
    assert np.all(got["k1"] == -1)
    large[0]()
    # n_landmarks = 0
    desc, kps, use, proj, begin, pool = L["map"]
    zero = np.zeros(1, np.int32)
    gl, gd = fe.match_to_map(desc, kps, use, proj[:0], zero, pool[:0], 20.0)
    assert np.all(gl == -1) and np.all(gd == thr) and len(gl) == n
    u = L["uninit"]
    e = fe.match_to_map_uninitialised(u[0], u[1], u[2], u[3], zero, pool[:0], u[6][:0], u[7][:0], u[8], u[9])
    assert np.all(e[0] == -1) and np.all(e[1] == thr) and not e[3].any() and e[4] == 0
    gk, gd = fe.verify_place_match(pool[:0], zero, desc)
    assert len(gk) == 0 and len(gd) == 0
    mp, tk, td, tu = L["table"]
    lm, bd, pl = fe.match_to_map_landmarks(0, mp["hp"][:0], mp["quality"][:0], zero, mp["obs_pose"][:0], mp["obs_desc"][:0],
                                           mp["obs_bp"][:0], mp["poses"], mp["T1"], 20.0, False, td, tk, tu)
    assert np.all(lm == -1) and np.all(bd == thr) and len(pl["status"]) == 0
    large[2]()
    # a landmark pool of zero rows: landmarks without a descriptor
    nl = len(begin) - 1
    none = np.zeros(nl + 1, np.int32)
    gl, gd = fe.match_to_map(desc, kps, use, proj, none, pool[:0], 20.0)
    rl, rd = oracle.match_to_map(desc, kps, use, proj, none, pool[:0], 20.0, thr)
    assert np.array_equal(gl, rl) and np.array_equal(gd, rd) and np.all(gl == -1)
    e = fe.match_to_map_uninitialised(u[0], u[1], u[2], u[3], none, pool[:0], u[6][:0], u[7][:0], u[8], u[9])
    r = oracle.match_to_map_uninit(u[0], u[1], u[2], u[3], none, pool[:0], u[6][:0], u[7][:0], u[8], u[9], thr)
    assert np.array_equal(e[0], r[0]) and np.array_equal(e[1], r[1]) and e[4] == r[4] == 0 and np.all(e[0] == -1)
    gk, gd = fe.verify_place_match(pool[:0], none, desc)  # Frontend.cpp:333-335
    assert np.array_equal(gk, np.zeros(nl, np.int32)) and np.array_equal(gd, np.full(nl, thr, np.uint32))
    # a table whose landmarks have no observation
    lm, bd, pl = fe.match_to_map_landmarks(0, mp["hp"], mp["quality"], np.zeros(len(mp["hp"]) + 1, np.int32),
                                           mp["obs_pose"][:0], mp["obs_desc"][:0], mp["obs_bp"][:0], mp["poses"], mp["T1"],
                                           20.0, False, td, tk, tu)
    ref = oracle.prepare_landmarks(mp["hp"], mp["quality"], np.zeros(len(mp["hp"]) + 1, np.int32), mp["obs_pose"][:0],
                                   mp["obs_bp"][:0], mp["poses"], mp["T1"], mp["cam"], 20.0, False)
    assert np.array_equal(pl["status"], ref["status"]) and np.array_equal(pl["n_desc"], ref["n_desc"])
    assert np.all(lm == -1) and np.all(bd == thr)
    large[5]()
    # nB = 0, nA = 0
    A, B = L["ham"]
    gj, gd = fe.hamming_argmin(A[:3], B[:0], 90)
    assert np.array_equal(gj, [-1, -1, -1]) and np.array_equal(gd, [90, 90, 90])
    assert fe.hamming_candidates(A, B[:0], 90)[1] == 0 and fe.hamming_candidates(A[:0], B, 90)[1] == 0
    assert len(fe.hamming_argmin(A[:0], B, 90)[0]) == 0
    large[9]()
    # an empty query, an empty database, entries without words, no descriptors to descend with
    dbb, dbi, dbv, qi, qv = L["bow"]
    assert np.all(fe.bow_query_l1(dbb, dbi, dbv, qi[:0], qv[:0]) == -1.0)
    assert len(fe.bow_query_l1(zero, dbi[:0], dbv[:0], qi, qv)) == 0
    assert np.all(fe.bow_query_l1(np.zeros(4, np.int32), dbi[:0], dbv[:0], qi, qv) == -1.0)
    feats, nd, cb, ci, nw = L["voc"]
    assert len(fe.fbrisk_transform(feats[:0], nd, cb, ci, nw)[0]) == 0
    large[7]()
    # n_id_set = 0: without a set (id_set = None) and with the empty set; no keypoints at all
    ck, cid, cset = L["cov"]
    got = fe.keyframe_coverage(ck, cid, None)
    assert {k: int(got[k]) for k in KR.COVERAGE_FIELDS} == L["cov_ref"][0]
    got = fe.keyframe_coverage(ck, cid, np.zeros(0, np.uint64))
    assert {k: int(got[k]) for k in KR.COVERAGE_FIELDS} == KR.coverage(cfg.w, cfg.h, ck, cid, np.zeros(0, np.uint64))
    assert got["n_matched"] == 0
    got = fe.keyframe_coverage(ck[:0], cid[:0], cset)
    assert {k: int(got[k]) for k in KR.COVERAGE_FIELDS} == KR.coverage(cfg.w, cfg.h, ck[:0], cid[:0], cset)
    for call in large:
        call()
