"""GPU: every table of map_scenes.py -- every branch of the landmark preparation the oracle's census can
reach, its knife edges, and the chunk edges of the packing kernel -- through
okvfe_match_to_map_landmarks (prepare_landmarks_kernel, compact_landmarks_kernel, match_to_map_kernel),
in both modes (non-exclusive at threshold 20, exclusive at 150) and under both orders of the 3-term
FP64 sums.

status, n_desc and obs_rows are compared for equality, projection, e_W and r_W as uint64 patterns.
Where the oracle holds a NaN the device must hold a NaN at the same place and nothing more is asked of
that element: the sign and payload of a default NaN differ between x86 (0 / 0 gives the negative quiet
NaN) and the GPU (the positive one), and neither is the reference's to define.

The packed set never reaches the host, so the frame makes it observable (map_scenes.dictated_frame): one
keypoint per pooled row of every 3-D landmark, at that landmark's projection and with that row as its
descriptor.  Its match is dictated -- that landmark, at distance 0 -- and is compared both with the
dictated answer and with oracle.match_to_map on map_synth.packed_set of the oracle's pooling.

The 8-coefficient camera is not in the oracle: its scene is checked as test_gpu_radtan8.py checks the
random map -- the FoV verdict and the projection bits against tests/radtan8_ref.py (the current pose of
that scene is the identity, so hp_C = hp_W in every summation order), the pooling against the oracle on
the same pinhole without a distortion wherever both keep the landmark.
"""
import dataclasses

import numpy as np
import pytest

import gpu_common as G
import map_scenes as S
import map_synth
import radtan8_ref as R8
from okvis2_amd import capi, synth

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp64_order")]

THRESHOLD = synth.euroc_config().match_threshold
_FRONTENDS = {}


def _frontend(cam):
    key = (cam.w, cam.h, cam.fu, cam.fv, cam.cu, cam.cv, cam.dist_type, tuple(cam.d))
    if key not in _FRONTENDS:
        cfg = dataclasses.replace(synth.euroc_config(), w=cam.w, h=cam.h, cams=[cam])
        fe = G.make_frontend(cfg)
        fe.set_camera(0, cam)
        _FRONTENDS[key] = fe
    return _FRONTENDS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_frontends():
    yield
    while _FRONTENDS:
        _FRONTENDS.popitem()[1].close()


def _same_f64(got, ref, what):
    got, ref = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(ref, dtype=np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN places differ", np.argwhere(np.isnan(got) != nan)[:5])
    same = got.view(np.uint64) == ref.view(np.uint64)
    assert np.all(same | nan), (what, np.argwhere(~(same | nan))[:5])


def _call(fe, sc, thr, exclusive, desc, kps, use):
    return fe.match_to_map_landmarks(0, sc["hp"], sc["quality"], sc["obs_begin"], sc["obs_pose"], sc["obs_desc"],
                                     sc["obs_bp"], sc["poses"], sc["T1"], thr, exclusive, desc, kps, use)


def _check_matches(oracle, sc, pool, thr, desc, kps, use, want, lm, bd, what):
    """the device's matches against the oracle's matcher on the packed set of `pool`, and against the dictated answer"""
    idx, proj, begin, rows = map_synth.packed_set(pool, sc["obs_desc"], 1)
    rl, rd = oracle.match_to_map(desc, kps, use, proj, begin, rows, thr, THRESHOLD)
    rl = np.where(rl >= 0, idx[np.maximum(rl, 0)], -1) if len(idx) else rl
    assert np.array_equal(lm, rl), (what, np.flatnonzero(lm != rl)[:8])
    assert np.array_equal(bd, rd), (what, np.flatnonzero(bd != rd)[:8])
    told = want >= 0
    assert np.array_equal(lm[told], want[told]) and np.all(bd[told] == 0), (what, "dictated")


def _check(oracle, sc, exclusive, thr, clutter=0, empty_frames=False):
    """one table in one mode; returns (oracle pooling, device pooling)"""
    what = (sc["name"], "exclusive" if exclusive else "non-exclusive")
    fe = _frontend(sc["cam"])
    ref = S.run_oracle(oracle, sc, exclusive, thr)
    kps, desc, use, want = S.dictated_frame(oracle, sc, ref, clutter)
    lm, bd, pool = _call(fe, sc, thr, exclusive, desc, kps, use)
    for k in ("status", "n_desc", "obs_rows"):
        assert np.array_equal(pool[k], ref[k]), (what, k, np.argwhere(pool[k] != ref[k])[:8])
    for k in ("projection", "e_W", "r_W"):
        _same_f64(pool[k], ref[k], what + (k,))
    _check_matches(oracle, sc, ref, thr, desc, kps, use, want, lm, bd, what)
    if empty_frames:
        lm0, bd0, pool0 = _call(fe, sc, thr, exclusive, desc[:0], kps[:0], use[:0])
        assert len(lm0) == 0 and len(bd0) == 0
        assert np.array_equal(pool0["status"], ref["status"]) and np.array_equal(pool0["obs_rows"], ref["obs_rows"])
        lm0, bd0, _ = _call(fe, sc, thr, exclusive, desc, kps, np.zeros_like(use))
        assert np.all(lm0 == -1) and np.all(bd0 == THRESHOLD)
    return ref, pool


def _check_radtan8(oracle, sc, exclusive, thr, clutter):
    what = (sc["name"], "exclusive" if exclusive else "non-exclusive")
    cam = sc["cam"]
    fe = _frontend(cam)
    assert np.array_equal(sc["T1"][0], np.eye(3).reshape(-1)) and not np.any(sc["T1"][1])
    hp = sc["hp"]
    head = np.where(hp[:, 3:4] < 0, -hp[:, :3], hp[:, :3])
    st, proj, _ = R8.project(cam, head)
    inside = (st != 4) & (st != 3) & ~(proj[:, 0] < -thr) & ~(proj[:, 1] < -thr) & \
        ~(proj[:, 0] > cam.w + thr) & ~(proj[:, 1] > cam.h + thr)
    twin = S.run_oracle(oracle, sc, exclusive, thr)  # (on the pinhole without a distortion)
    # the frame is dictated by the DEVICE's pooling here; the matcher on its packed set is still the oracle's
    _, _, pool = _call(fe, sc, thr, exclusive, np.zeros((0, 48), np.uint8), np.zeros(0, oracle.KEYPOINT_DTYPE),
                       np.zeros(0, np.uint8))
    assert not pool["status"][~inside].any() and not pool["projection"][~inside].any(), what
    _same_f64(pool["projection"][inside], proj[inside], what + ("projection",))
    both = inside & (twin["projection"] != 0).any(axis=1)  # past the FoV check in both: the pooling is the same
    assert both.sum() > 300 and (st == 4).sum() - (np.abs(head[:, 2]) < 1e-12).sum() >= 16  # (distortion failures)
    for k in ("status", "n_desc", "obs_rows"):
        assert np.array_equal(pool[k][both], twin[k][both]), (what, k)
    for k in ("e_W", "r_W"):
        _same_f64(pool[k][both], twin[k][both], what + (k,))
    kps, desc, use, want = S.dictated_frame(oracle, sc, pool, clutter)
    lm, bd, pool2 = _call(fe, sc, thr, exclusive, desc, kps, use)
    assert np.array_equal(pool2["status"], pool["status"]) and np.array_equal(pool2["obs_rows"], pool["obs_rows"])
    _check_matches(oracle, sc, pool, thr, desc, kps, use, want, lm, bd, what)
    assert (want >= 0).sum() > 100


@pytest.mark.parametrize("spec", S.GENERAL_SPECS, ids=lambda s: f"{s[0]}-s{s[1]}")
def test_general_scene_both_modes(oracle, spec):
    sc = S.general_scene(*spec)
    for exclusive, thr in S.MODES:
        if sc["cam"].dist_type == 3:
            _check_radtan8(oracle, sc, exclusive, thr, clutter=200)
            continue
        ref, _ = _check(oracle, sc, exclusive, thr, clutter=200, empty_frames=True)
        assert (ref["status"] == 1).sum() > 100 and (ref["status"] == 2).sum() > 50 and (ref["status"] == 0).sum() > 100
        assert np.isnan(ref["e_W"]).any()  # (pooled views with a zero-length back-projection)


@pytest.mark.parametrize("edge,exclusive", [(e, x) for e in S.KNIFE_EDGES for x in S.knife_modes(e)],
                         ids=lambda v: str(v))
def test_knife_edge_pair(oracle, edge, exclusive):
    """both sides of the edge, bisected under the current summation order, side by side in one table"""
    sc, thr, (lo, hi), _ = S.knife_edge(oracle, edge, exclusive)
    ref, pool = _check(oracle, sc, exclusive, thr)
    if edge != "clamp":  # (clamp turns no output)
        assert ref["status"][0] != ref["status"][1] or ref["n_desc"][0] != ref["n_desc"][1] or \
            np.any(ref["obs_rows"][0] - sc["obs_begin"][0] != ref["obs_rows"][1] - sc["obs_begin"][1]), (edge, lo, hi)


def test_z_sign_rows_both_modes(oracle):
    sc = S.z_sign_table()
    for exclusive, thr in S.MODES:
        ref, _ = _check(oracle, sc, exclusive, thr)
        assert np.all(ref["status"][0::3] != 0) and np.all(ref["status"][1::3] == 0) and np.all(ref["status"][2::3] != 0)


@pytest.mark.parametrize("n", S.PACK_SIZES)
def test_packing_at_the_chunk_edges(oracle, n):
    for pattern in S.PACK_PATTERNS:
        sc = S.packing_scene(n, pattern)
        for exclusive, thr in S.MODES:
            ref, _ = _check(oracle, sc, exclusive, thr, empty_frames=pattern in ("mixed", "none"))
            three_d = np.flatnonzero(ref["status"] == 1)
            want = {"all": np.arange(n), "none": np.zeros(0, np.int64),
                    "first": np.arange(0, n, 1024), "alternating": np.arange(0, n, 2)}.get(pattern)
            if pattern == "last":
                want = np.unique(np.concatenate([np.arange(1023, n, 1024), [n - 1]]))
            if want is not None:
                assert np.array_equal(three_d, want), (n, pattern)
            else:
                assert n < 8 or set(ref["n_desc"][three_d]) == {1, 2}, (n, pattern)


def test_status_2_landmarks_feed_the_uninitialised_matcher(oracle):
    """the not-3-D-yet landmarks of a degenerate scene, NaN rays included, as okvfe_match_to_map_uninitialised's map"""
    sc = S.general_scene("euroc", 0)
    exclusive, thr = S.MODES[0]
    fe = _frontend(sc["cam"])
    ref = S.run_oracle(oracle, sc, exclusive, thr)
    kps, desc, use, _ = S.dictated_frame(oracle, sc, ref, clutter=100)
    _, _, pool = _call(fe, sc, thr, exclusive, desc, kps, use)
    idx, _, begin, rows = map_synth.packed_set(pool, sc["obs_desc"], 2)
    assert len(idx) > 50
    # keypoints on the status-2 landmarks' rows, so that the gate chain runs
    rng = np.random.default_rng(3)
    pick = rng.choice(len(rows), min(len(rows), 150), replace=False)
    owner = idx[np.searchsorted(begin, pick, side="right") - 1]
    n = len(pick)
    kp2 = np.zeros(n, dtype=oracle.KEYPOINT_DTYPE)
    kp2["x"], kp2["y"], kp2["size"] = pool["projection"][owner, 0], pool["projection"][owner, 1], 12.0
    d2 = rows[pick] ^ ((rng.random((n, 48)) < 0.03) * rng.integers(1, 256, (n, 48))).astype(np.uint8)
    e0 = np.concatenate([pool["e_W"][l, :pool["n_desc"][l]] for l in idx])
    r0 = np.concatenate([pool["r_W"][l, :pool["n_desc"][l]] for l in idx])
    bp, bv = oracle.backproject_keypoints(sc["cam"], kp2)
    prev = np.full(n, -1, dtype=np.int32)
    f = 0.5 * (sc["cam"].fu + sc["cam"].fv)
    got = fe.match_to_map_uninitialised(d2, bp, bv, prev, begin, rows, e0, r0, sc["T1"], f)
    want = oracle.match_to_map_uninit(d2, bp, bv, prev, begin, rows, e0, r0, sc["T1"], f, THRESHOLD)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[3], want[3])
    _same_f64(got[2], want[2], "hps_W")


def test_landmark_table_argument_rejection(oracle):
    """rejected on the host, before anything is launched: the outputs of an accepted call are not touched either"""
    sc = S.packing_scene(2, "all")
    fe = _frontend(sc["cam"])
    ref = S.run_oracle(oracle, sc, False, 20.0)
    kps, desc, use, _ = S.dictated_frame(oracle, sc, ref)

    def rejected(**kw):
        t = dict(sc, thr=20.0)
        t.update(kw)
        with pytest.raises(capi.OkvfeError) as e:
            fe.match_to_map_landmarks(0, t["hp"], t["quality"], t["obs_begin"], t["obs_pose"], t["obs_desc"], t["obs_bp"],
                                      t["poses"], t["T1"], t["thr"], False, desc, kps, use)
        assert e.value.status == capi.ERR_INVALID_ARGUMENT, kw
        return str(e.value)

    b = sc["obs_begin"]
    assert "monotone" in rejected(obs_begin=np.array([b[0], b[2], b[1]], np.int32))
    assert "monotone" in rejected(obs_begin=np.array([-1, b[1], b[2]], np.int32))
    assert "monotone" in rejected(obs_begin=np.array([b[0], b[1], b[2] + 1], np.int32))  # past n_observations
    for bad in (-1, len(sc["poses"])):
        op = sc["obs_pose"].copy()
        op[-1] = bad
        assert "pose index" in rejected(obs_pose=op)
    for thr in (-1.0, -0.0 - 1e-300, float("nan")):
        rejected(thr=thr)
    # and the same table is accepted as it stands, at a threshold of exactly zero too
    lm, bd, pool = _call(fe, sc, 0.0, False, desc, kps, use)
    assert np.array_equal(pool["status"], ref["status"])
