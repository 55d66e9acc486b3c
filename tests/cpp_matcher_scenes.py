"""Scenes for the tests of the C++ mirror's host-buffer matchers on a real context (tests/test_gpu_cpp_matchers.py):
the builders of test_gpu_matchers.py, shrunk, and the floors each scene has to meet.  The floors are conditions on the
scenes, asserted with the oracle alone (tests/test_host_marshalling.py); the GPU test imports the same constants.
CPU only."""
import functools
import os

import numpy as np

import gate_scenes
import map_synth
import oracle_lib as O
from okvis2_amd import synth

THRESHOLD = synth.euroc_config().match_threshold
MOTION_N = 130  # three 64-row blocks per side, the last one partial
MIN_MOTION_MATCHED = 64
MIN_MOTION_ACCEPTED = 64
MIN_FIRST_PASS_MATCHED = 100
MIN_PER_STATUS = 16
MIN_SECOND_PASS_HP_SET = 8
MIN_ROWS_DEPENDING_ON_BPV = 4
MIN_PLACE_BELOW_THRESHOLD = 20
MAP_MODES = ((False, 20.0), (True, 150.0))  # (exclusive, reprojection threshold) of test_match_to_map_from_raw_landmark_table

_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def voc_descriptors():
    return np.fromfile(os.path.join(_GOLD, "small_voc_desc.bin"), dtype=np.uint8).reshape(-1, 48)


def radtan8_camera():
    return synth.radtan8_config().cams[0]


@functools.lru_cache(maxsize=None)
def motion_scene(radtan8=False):
    """the `observe` construction of test_gpu_matchers.py::test_match_motion_stereo at MOTION_N keypoints per side;
    radtan8: through the 8-coefficient camera of gate_scenes.py (projection and back-projection of tests/radtan8_ref.py)"""
    cam = radtan8_camera() if radtan8 else synth.euroc_config().cams[0]
    rng = np.random.default_rng(3)
    n = MOTION_N
    T0 = (np.eye(3).reshape(-1), np.zeros(3))
    th = 0.05
    Rz = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]])
    T1 = (Rz.reshape(-1), np.array([0.35, 0.04, 0.02]))
    X = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-0.8, 0.8, n), rng.uniform(2.5, 9, n)], 1)

    def observe(T, noise):
        Cm = np.asarray(T[0]).reshape(3, 3)
        Xc = (X - np.asarray(T[1])) @ Cm  # C^T (X - r)
        kp = np.zeros(n, dtype=O.KEYPOINT_DTYPE)
        kp["size"] = 12.0
        for i in range(n):
            st, pt = gate_scenes._project(cam, Xc[i])
            kp["x"][i], kp["y"][i] = pt if st == 0 else (5.0, 5.0)
        kp["x"] += rng.normal(0, noise, n).astype(np.float32)
        kp["y"] += rng.normal(0, noise, n).astype(np.float32)
        bp, bv = gate_scenes._backproject_keypoints(cam, kp)
        return kp, np.ascontiguousarray(bp, dtype=np.float64), np.ascontiguousarray(bv, dtype=np.uint8)

    kp0, bp0, bv0 = observe(T0, 0.3)
    kp1, bp1, bv1 = observe(T1, 0.3)
    d0 = rng.integers(0, 256, (n, 48), dtype=np.uint8)
    d1 = d0 ^ (rng.random((n, 48)) < 0.03).astype(np.uint8) * rng.integers(0, 256, (n, 48), dtype=np.uint8)
    perm = rng.permutation(n)
    d1, kp1, bp1, bv1 = d1[perm], kp1[perm], bp1[perm], bv1[perm]
    skip0 = (rng.random(n) < 0.1).astype(np.uint8)
    matched1 = (rng.random(n) < 0.1).astype(np.uint8)
    bv0 = bv0.copy()
    bv0[::11] = 0
    return dict(cam=cam, T0=T0, T1=T1, f0=(kp0, d0, bp0, bv0), f1=(kp1, d1, bp1, bv1), skip0=skip0, matched1=matched1)


def motion_reference(sc, with_flags):
    (kp0, d0, bp0, bv0), (kp1, d1, bp1, bv1) = sc["f0"], sc["f1"]
    s0, m1 = (sc["skip0"], sc["matched1"]) if with_flags else (None, None)
    return O.match_motion_stereo(d0, kp0, bp0, bv0, s0, d1, kp1, bp1, bv1, m1, sc["T0"], sc["T1"], sc["cam"], THRESHOLD)


@functools.lru_cache(maxsize=None)
def map_scene():
    """map_synth.make_map(1500) and its frame of 700 keypoints; per mode of MAP_MODES the oracle's pooling and the packed
    3-D set; for the second pass the status-2 set of the first mode, backProjectionsValid cleared at every third
    keypoint, and a `previous` in which every fourth keypoint the free second pass matches carries that match and
    every fourth another landmark"""
    m = map_synth.make_map(1500, voc=voc_descriptors())
    kps, desc, use = map_synth.make_frame(m, O)
    bp, bv = O.backproject_keypoints(m["cam"], kps)
    bp, bpv = np.ascontiguousarray(bp, dtype=np.float64), np.ascontiguousarray(bv, dtype=np.uint8).copy()
    bpv[::3] = 0
    sc = dict(m=m, cam=m["cam"], kps=kps, desc=desc, use=use, bp=bp, bpv=bpv, first={})
    for exclusive, thr in MAP_MODES:
        ref = O.prepare_landmarks(m["hp"], m["quality"], m["obs_begin"], m["obs_pose"], m["obs_bp"], m["poses"], m["T1"],
                                  m["cam"], thr, exclusive)
        idx, proj, begin, rows = map_synth.packed_set(ref, m["obs_desc"], 1)
        sc["first"][exclusive] = dict(ref=ref, idx=idx, proj=np.ascontiguousarray(proj, dtype=np.float64), begin=begin, rows=rows)
    ref = sc["first"][False]["ref"]
    idx, _, begin, rows = map_synth.packed_set(ref, m["obs_desc"], 2)
    e0 = np.array([ref["e_W"][l, d] for l in idx for d in range(ref["n_desc"][l])], dtype=np.float64).reshape(-1, 3)
    r0 = np.array([ref["r_W"][l, d] for l in idx for d in range(ref["n_desc"][l])], dtype=np.float64).reshape(-1, 3)
    sc.update(idx2=idx, begin2=begin, rows2=rows, e0=e0, r0=r0, focal=0.5 * (m["cam"].fu + m["cam"].fv))
    nobody = np.full(len(kps), -1, np.int32)
    free = second_pass_reference(dict(sc, previous=nobody), False, False, True)
    previous = nobody.copy()
    hit = np.flatnonzero(free[0] >= 0)
    previous[hit[::4]] = free[0][hit[::4]]  # carries the landmark it will match
    previous[hit[1::4]] = (free[0][hit[1::4]] + 1) % len(idx)  # carries another one
    sc["previous"] = previous
    return sc


def second_pass_reference(sc, with_use, with_previous, with_bpv=True):
    """oracle.match_to_map_uninit on the status-2 set; with_bpv = False: what the wrapper computed before it applied the
    reference's back-projection test"""
    n = len(sc["kps"])
    use = sc["use"] if with_use else np.ones(n, np.uint8)
    if with_bpv:
        use = use & sc["bpv"]
    previous = sc["previous"] if with_previous else np.full(n, -1, np.int32)
    return O.match_to_map_uninit(sc["desc"], sc["bp"], use, previous, sc["begin2"], sc["rows2"], sc["e0"], sc["r0"],
                                 sc["m"]["T1"], sc["focal"], THRESHOLD)


@functools.lru_cache(maxsize=None)
def place_scene():
    """the landmark / frame construction of test_verify_place_batched_and_vocabulary_descent: 40 landmarks of 1 to 4
    descriptors, 130 frame descriptors.  The landmark rows are disturbed vocabulary rows drawn from the first 200, of
    which the frame holds the first 130."""
    d = voc_descriptors()
    rng = np.random.default_rng(11)
    frame = np.concatenate([d[:100], d[100:130] ^ (rng.random((30, 48)) < 0.02).astype(np.uint8)])
    sizes = rng.integers(1, 5, 40)
    begin = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    pool = d[rng.integers(0, 200, begin[-1])] ^ ((rng.random((begin[-1], 48)) < 0.03) *
                                                 rng.integers(1, 256, (begin[-1], 48))).astype(np.uint8)
    return dict(frame=np.ascontiguousarray(frame), begin=begin, pool=np.ascontiguousarray(pool))


def check_floors():
    """the conditions the scenes have to meet for the GPU comparison to mean something -> the measured figures"""
    fig = {}
    for with_flags in (True, False):
        ref = motion_reference(motion_scene(), with_flags)
        fig["motion matched", with_flags] = int((ref["k1"] >= 0).sum())
        fig["motion accepted", with_flags] = int(ref["accepted"].sum())
        assert fig["motion matched", with_flags] >= MIN_MOTION_MATCHED, fig
        assert fig["motion accepted", with_flags] >= MIN_MOTION_ACCEPTED, fig
    sc = map_scene()
    for exclusive, thr in MAP_MODES:
        f = sc["first"][exclusive]
        rl, _ = O.match_to_map(sc["desc"], sc["kps"], sc["use"], f["proj"], f["begin"], f["rows"], thr, THRESHOLD)
        fig["first pass matched", exclusive] = int((rl >= 0).sum())
        assert fig["first pass matched", exclusive] >= MIN_FIRST_PASS_MATCHED, fig
        for s in (0, 1, 2):
            fig["status", s, exclusive] = int((f["ref"]["status"] == s).sum())
            assert fig["status", s, exclusive] >= MIN_PER_STATUS, fig
    for with_use in (False, True):
        for with_previous in (False, True):
            a = second_pass_reference(sc, with_use, with_previous)
            b = second_pass_reference(sc, with_use, with_previous, with_bpv=False)
            fig["second pass hpSet", with_use, with_previous] = int(((a[0] >= 0) & (a[3] != 0)).sum())
            fig["rows depending on bpv", with_use, with_previous] = int(((a[0] != b[0]) | (a[1] != b[1]) | (a[3] != b[3])).sum())
            assert fig["second pass hpSet", with_use, with_previous] >= MIN_SECOND_PASS_HP_SET, fig
            assert fig["rows depending on bpv", with_use, with_previous] >= MIN_ROWS_DEPENDING_ON_BPV, fig
    assert second_pass_reference(sc, True, True)[4] >= 1, "no keypoint carries the landmark it matches"
    p = place_scene()
    _, rd = O.verify_place(p["pool"], p["begin"], p["frame"], THRESHOLD)
    fig["place below threshold"] = int((rd < THRESHOLD).sum())
    assert fig["place below threshold"] >= MIN_PLACE_BELOW_THRESHOLD, fig
    return fig
