"""GPU: okvfe_match_to_map_table_blocks_device -- matchToMap from the raw landmark table for a batch of frames
against ONE device-resident table (prepare_landmarks_frames_kernel, pack_landmarks_frames_kernel,
match_to_map_table_kernel) -- and okvfe_landmark_table_check_device.  Every frame's result is what
okvfe_match_to_map_landmarks gives for that frame alone: checked against the per-frame reference of
test_gpu_map_census.py (map_table_common.reference / reference_matches) and against the B = 1 call itself, in both
modes (non-exclusive at threshold 20, exclusive at 150) and under both orders of the 3-term FP64 sums.

status, n_desc, obs_rows and the match rows are compared for equality, projection, e_W and r_W as uint64 patterns with
the NaN-place rule; rows at or past a frame's keypoint count keep the sentinel -7."""
import dataclasses

import numpy as np
import pytest

import gpu_common as G
import map_scenes as S
import map_synth
import map_table_common as M
import radtan8_ref as R8
from okvis2_amd import capi, synth

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp64_order")]
torch = pytest.importorskip("torch")

_FRONTENDS = {}


def _frontend(cams):
    """a context of the first camera's size whose slots hold `cams`"""
    key = tuple((c.w, c.h, c.fu, c.fv, c.cu, c.cv, c.dist_type, tuple(c.d)) for c in cams)
    if key not in _FRONTENDS:
        cfg = dataclasses.replace(synth.euroc_config(), w=cams[0].w, h=cams[0].h, cams=list(cams))
        fe = G.make_frontend(cfg)
        for i, c in enumerate(cams):
            fe.set_camera(i, c)
        _FRONTENDS[key] = fe
    return _FRONTENDS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_frontends():
    yield
    while _FRONTENDS:
        _FRONTENDS.popitem()[1].close()


def _b1(fe, sc, cam_id, pose, thr, exclusive, frame, use=None):
    kps, desc, u = frame
    return fe.match_to_map_landmarks(cam_id, sc["hp"], sc["quality"], sc["obs_begin"], sc["obs_pose"], sc["obs_desc"],
                                     sc["obs_bp"], sc["poses"], pose, thr, exclusive, desc, kps, u if use is None else use)


def _check_batch(oracle, fe, sc, frames, poses, cam_ids, cams, thr, exclusive, what, variants=((True, True),),
                 b1=True, stream=None):
    """the batch in every (use_dev, pool_out) variant against the reference and, once, against the B = 1 call.
    Returns the per-frame references."""
    tab = M.DeviceTable(fe, sc)
    fe.landmark_table_check_device(tab.desc)
    refs = {}
    for f in range(len(frames)):
        key = (poses[f][0].tobytes(), poses[f][1].tobytes(), cam_ids[f])
        if key not in refs:
            refs[key] = M.reference(oracle, sc, poses[f], cams[cam_ids[f]], exclusive, thr)
    ref_of = [refs[(poses[f][0].tobytes(), poses[f][1].tobytes(), cam_ids[f])] for f in range(len(frames))]
    for with_use, with_pool in variants:
        lm, bd, pool, _ = M.run_batch(fe, tab, frames, poses, cam_ids, thr, exclusive, with_use, with_pool, stream)
        for f, fr in enumerate(frames):
            w = what + (f, "use" if with_use else "no use")
            M.check_frame(oracle, sc, ref_of[f], thr, fr, lm[f], bd[f], w, with_use)
            if with_pool:
                M.check_pool({k: pool[k][f] for k in M.POOL_KEYS}, ref_of[f], w)
        if b1 and with_use and with_pool:
            for f, fr in enumerate(frames):
                l1, d1, p1 = _b1(fe, sc, cam_ids[f], poses[f], thr, exclusive, fr)
                n = len(fr[0])
                assert np.array_equal(lm[f, :n], l1) and np.array_equal(bd[f, :n], d1), (what, f, "B = 1 matches")
                for k in M.POOL_KEYS:  # the BYTES of the B = 1 call's pool
                    assert np.array_equal(pool[k][f].view(np.uint8), np.ascontiguousarray(p1[k]).view(np.uint8)), (what, f, k)
    return ref_of


def _scene_batch(oracle, sc, K, exclusive, thr):
    """the frames of a general scene: the dictated frame of T1 cut into frames of at most K, one frame of exactly K
    keypoints, clutter-only frames for the other poses, an empty frame"""
    P = M.scene_poses(sc)
    ref0 = M.reference(oracle, sc, P[0], sc["cam"], exclusive, thr)
    kps, desc, use, want = S.dictated_frame(oracle, sc, ref0, clutter=200)
    frames = M.cut((kps, desc, use), K)
    wants = [want[a:a + K] for a in range(0, len(kps), K)]
    poses = [P[0]] * len(frames)
    for n, p, seed in ((K, P[1], 1), (300, P[2], 2), (0, P[3], 3), (333, P[3], 4), (100, P[4], 5)):
        frames.append(M.clutter_frame(oracle, sc, n, seed))
        poses.append(p)
        wants.append(np.full(n, -1, np.int32))
    return frames, poses, wants


@pytest.mark.parametrize("spec", [s for s in S.GENERAL_SPECS if s[0] != "radtan8"], ids=lambda s: f"{s[0]}-s{s[1]}")
def test_general_scene_as_a_batch(oracle, spec):
    sc = S.general_scene(*spec)
    fe = _frontend([sc["cam"]])
    K = fe.max_keypoints
    empty_sets = 0
    for exclusive, thr in S.MODES:
        what = (sc["name"], "exclusive" if exclusive else "non-exclusive")
        frames, poses, wants = _scene_batch(oracle, sc, K, exclusive, thr)
        assert any(len(f[0]) == K for f in frames) and any(len(f[0]) == 0 for f in frames)
        refs = _check_batch(oracle, fe, sc, frames, poses, [0] * len(frames), [sc["cam"]], thr, exclusive, what,
                            variants=((True, True), (False, True), (True, False), (False, False)))
        # the dictated answers of the first pose's frames
        lm, bd, _, _ = M.run_batch(fe, M.DeviceTable(fe, sc), frames, poses, [0] * len(frames), thr, exclusive)
        told = 0
        for f, w in enumerate(wants):
            t = w >= 0
            assert np.array_equal(lm[f, :len(w)][t], w[t]) and np.all(bd[f, :len(w)][t] == 0), (what, f, "dictated")
            told += int(t.sum())
        assert told >= 100, (what, told)
        empty_sets += sum(1 for r in refs if not (r["status"] == 1).any())
    assert empty_sets >= 1, sc["name"]


def test_radtan8_scene_as_a_batch(oracle):
    """The 8-coefficient camera is not in the oracle: the frame at the scene's pose (the identity) as
    test_gpu_map_census._check_radtan8 checks it -- FoV verdict and projection bits against tests/radtan8_ref.py, the
    pooling against the oracle's pinhole twin where both keep the landmark, the matches against the oracle's matcher on
    the device's pooling -- and every frame of the batch against the B = 1 call."""
    sc = S.general_scene("radtan8", 0)
    cam = sc["cam"]
    fe = _frontend([cam])
    K = fe.max_keypoints
    P = M.scene_poses(sc)
    assert np.array_equal(P[0][0], np.eye(3).reshape(-1)) and not np.any(P[0][1])
    tab = M.DeviceTable(fe, sc)
    fe.landmark_table_check_device(tab.desc)
    hp = sc["hp"]
    head = np.where(hp[:, 3:4] < 0, -hp[:, :3], hp[:, :3])
    st, proj, _ = R8.project(cam, head)
    for exclusive, thr in S.MODES:
        what = (sc["name"], "exclusive" if exclusive else "non-exclusive")
        inside = (st != 4) & (st != 3) & ~(proj[:, 0] < -thr) & ~(proj[:, 1] < -thr) & \
            ~(proj[:, 0] > cam.w + thr) & ~(proj[:, 1] > cam.h + thr)
        twin = S.run_oracle(oracle, sc, exclusive, thr)
        empty = (np.zeros(0, oracle.KEYPOINT_DTYPE), np.zeros((0, 48), np.uint8), np.zeros(0, np.uint8))
        _, _, pool, _ = M.run_batch(fe, tab, [empty], [P[0]], [0], thr, exclusive)
        pool0 = {k: pool[k][0] for k in M.POOL_KEYS}
        assert not pool0["status"][~inside].any() and not pool0["projection"][~inside].any(), what
        M.same_f64(pool0["projection"][inside], proj[inside], what + ("projection",))
        both = inside & (twin["projection"] != 0).any(axis=1)
        assert both.sum() > 300
        for k in ("status", "n_desc", "obs_rows"):
            assert np.array_equal(pool0[k][both], twin[k][both]), (what, k)
        for k in ("e_W", "r_W"):
            M.same_f64(pool0[k][both], twin[k][both], what + (k,))
        kps, desc, use, want = S.dictated_frame(oracle, sc, pool0, clutter=200)
        frames = M.cut((kps, desc, use), K)
        poses = [P[0]] * len(frames)
        for n, p, seed in ((K, P[1], 1), (300, P[2], 2), (0, P[3], 3), (333, P[3], 4)):
            frames.append(M.clutter_frame(oracle, sc, n, seed))
            poses.append(p)
        lm, bd, pool, _ = M.run_batch(fe, tab, frames, poses, [0] * len(frames), thr, exclusive)
        got = np.concatenate([lm[f, :len(fr[0])] for f, fr in enumerate(frames[:len(frames) - 4])])
        told = want >= 0
        assert told.sum() > 100 and np.array_equal(got[told], want[told]), what
        for f, fr in enumerate(frames):
            n = len(fr[0])
            if f < len(frames) - 4:  # the oracle's matcher on the device's pooling
                M.check_frame(oracle, sc, pool0, thr, fr, lm[f], bd[f], what + (f,))
            l1, d1, p1 = _b1(fe, sc, 0, poses[f], thr, exclusive, fr)
            assert np.array_equal(lm[f, :n], l1) and np.array_equal(bd[f, :n], d1), (what, f)
            assert np.all(lm[f, n:] == M.SENTINEL) and np.all(bd[f, n:] == M.SENTINEL)
            for k in M.POOL_KEYS:
                assert np.array_equal(pool[k][f].view(np.uint8), np.ascontiguousarray(p1[k]).view(np.uint8)), (what, f, k)


def _among_three_others(oracle, sc, thr, exclusive, what):
    """the table's own frame as frame 2 of a batch of four"""
    fe = _frontend([sc["cam"]])
    K = fe.max_keypoints
    ref = M.reference(oracle, sc, sc["T1"], sc["cam"], exclusive, thr)
    kps, desc, use, want = S.dictated_frame(oracle, sc, ref)
    assert len(kps) <= K
    T1 = (np.asarray(sc["T1"][0], dtype=np.float64).reshape(-1), np.asarray(sc["T1"][1], dtype=np.float64))
    moved = (T1[0], T1[1] + np.array([0.01, 0.0, 0.0]))
    frames = [M.clutter_frame(oracle, sc, 64, 1), M.clutter_frame(oracle, sc, 65, 2), (kps, desc, use),
              M.clutter_frame(oracle, sc, 1, 3)]
    poses = [moved, T1, T1, moved]
    refs = _check_batch(oracle, fe, sc, frames, poses, [0] * 4, [sc["cam"]], thr, exclusive, what)
    return refs[2]


@pytest.mark.parametrize("edge,exclusive", [(e, x) for e in S.KNIFE_EDGES for x in S.knife_modes(e)],
                         ids=lambda v: str(v))
def test_knife_edge_pair_in_a_batch(oracle, edge, exclusive):
    sc, thr, (lo, hi), _ = S.knife_edge(oracle, edge, exclusive)
    ref = _among_three_others(oracle, sc, thr, exclusive, (sc["name"],))
    if edge != "clamp":
        assert ref["status"][0] != ref["status"][1] or ref["n_desc"][0] != ref["n_desc"][1] or \
            np.any(ref["obs_rows"][0] - sc["obs_begin"][0] != ref["obs_rows"][1] - sc["obs_begin"][1]), (edge, lo, hi)


def test_z_sign_rows_in_a_batch(oracle):
    sc = S.z_sign_table()
    for exclusive, thr in S.MODES:
        ref = _among_three_others(oracle, sc, thr, exclusive, (sc["name"], exclusive))
        assert np.all(ref["status"][0::3] != 0) and np.all(ref["status"][1::3] == 0) and np.all(ref["status"][2::3] != 0)


@pytest.mark.parametrize("n", tuple(sorted(set(S.PACK_SIZES) | {63, 64, 65, 128, 129})))
def test_packing_at_the_chunk_edges(oracle, n):
    """the edges of the 1024-row scan chunks of pack_landmarks_frames_kernel and of the matcher's 64-landmark chunks"""
    for pattern in S.PACK_PATTERNS:
        sc = S.packing_scene(n, pattern)
        fe = _frontend([sc["cam"]])
        K = fe.max_keypoints
        T1 = (np.asarray(sc["T1"][0], dtype=np.float64).reshape(-1), np.asarray(sc["T1"][1], dtype=np.float64))
        for exclusive, thr in S.MODES:
            what = (sc["name"], exclusive)
            ref = M.reference(oracle, sc, T1, sc["cam"], exclusive, thr)
            kps, desc, use, want = S.dictated_frame(oracle, sc, ref)
            frames = M.cut((kps, desc, use), K) + [M.clutter_frame(oracle, sc, 70, 1)]
            _check_batch(oracle, fe, sc, frames, [T1] * len(frames), [0] * len(frames), [sc["cam"]], thr, exclusive,
                         what, b1=n <= 129)
            lm, bd, _, _ = M.run_batch(fe, M.DeviceTable(fe, sc), frames, [T1] * len(frames), [0] * len(frames), thr,
                                       exclusive, with_pool=False)
            got = np.concatenate([lm[f, :len(fr[0])] for f, fr in enumerate(frames[:-1])])
            gd = np.concatenate([bd[f, :len(fr[0])] for f, fr in enumerate(frames[:-1])])
            told = want >= 0
            assert np.array_equal(got[told], want[told]) and np.all(gd[told] == 0), (what, "dictated")


def test_table_without_landmarks(oracle):
    """n_landmarks == 0: the rows below a block's count still receive -1 and match_threshold, written by a kernel"""
    sc = S.packing_scene(2, "all")
    empty = dict(sc, hp=sc["hp"][:0], quality=sc["quality"][:0], obs_begin=np.zeros(1, np.int32),
                 obs_pose=sc["obs_pose"][:0], obs_desc=sc["obs_desc"][:0], obs_bp=sc["obs_bp"][:0])
    fe = _frontend([sc["cam"]])
    K = fe.max_keypoints
    tab = M.DeviceTable(fe, empty)
    assert tab.n_landmarks == 0 and tab.n_observations == 0
    fe.landmark_table_check_device(tab.desc)
    frames = [M.clutter_frame(oracle, sc, n, 1) for n in (130, 0, K)]
    T1 = (np.asarray(sc["T1"][0], dtype=np.float64).reshape(-1), np.asarray(sc["T1"][1], dtype=np.float64))
    for with_pool in (True, False):
        lm, bd, _, _ = M.run_batch(fe, tab, frames, [T1] * 3, [0] * 3, 20.0, False, with_pool=with_pool)
        for f, fr in enumerate(frames):
            n = len(fr[0])
            assert np.all(lm[f, :n] == -1) and np.all(bd[f, :n] == M.THRESHOLD), f
            assert np.all(lm[f, n:] == M.SENTINEL) and np.all(bd[f, n:] == M.SENTINEL), f


def test_mixed_cameras_in_one_context(oracle):
    """slots 0..2 of a context of EuRoC size: the EuRoC camera, the same pinhole without a distortion, an equidistant
    camera of that size; cam_ids differ per frame"""
    sc = S.general_scene("euroc", 0)
    c0 = sc["cam"]
    cams = [c0, dataclasses.replace(c0, dist_type=0, d=(0.0, 0.0, 0.0, 0.0)),
            dataclasses.replace(c0, fu=351.31400364193297, fv=351.4911744656785, dist_type=2,
                                d=tuple(synth.hilti_config().cams[0].d))]
    fe = _frontend(cams)
    K = fe.max_keypoints
    P = M.scene_poses(sc)
    for exclusive, thr in S.MODES:
        frames, poses, cam_ids = [], [], []
        for i, (c, p) in enumerate(((2, P[0]), (0, P[0]), (1, P[0]), (1, P[3]), (2, P[1]), (0, P[3]))):
            ref = M.reference(oracle, sc, p, cams[c], exclusive, thr)
            kps, desc, use, _ = S.dictated_frame(oracle, sc, ref, clutter=50, seed=10 + i)
            frames.append((kps[:K], desc[:K], use[:K]))
            poses.append(p)
            cam_ids.append(c)
        refs = _check_batch(oracle, fe, sc, frames, poses, cam_ids, cams, thr, exclusive,
                            ("mixed", exclusive), variants=((True, True), (False, False)))
        # the camera model shows: the three slots disagree about the landmarks of one pose
        assert not np.array_equal(refs[0]["status"], refs[1]["status"]) or \
            not np.array_equal(refs[0]["projection"], refs[1]["projection"])
        assert not np.array_equal(refs[1]["projection"], refs[2]["projection"])


def test_radtan8_slot_among_others(oracle):
    """a small case in which one slot holds the 8-coefficient model, so that the kRT8 launch is taken: the frames on
    the other slot still equal the oracle, the frame on the 8-coefficient slot the B = 1 call"""
    cfg = synth.radtan8_config()
    c8 = cfg.cams[0]
    plain = dataclasses.replace(c8, dist_type=1, d=tuple(synth.euroc_config().cams[0].d))
    cams = [plain, c8]
    sc = dict(S.packing_scene(129, "mixed"), cam=plain)
    fe = _frontend(cams)
    T1 = (np.asarray(sc["T1"][0], dtype=np.float64).reshape(-1), np.asarray(sc["T1"][1], dtype=np.float64))
    tab = M.DeviceTable(fe, sc)
    for exclusive, thr in S.MODES:
        ref = M.reference(oracle, sc, T1, plain, exclusive, thr)
        fr = S.dictated_frame(oracle, sc, ref, clutter=20)[:3]
        frames, cam_ids = [fr, fr, M.clutter_frame(oracle, sc, 90, 1)], [0, 1, 0]
        lm, bd, pool, _ = M.run_batch(fe, tab, frames, [T1] * 3, cam_ids, thr, exclusive)
        for f in (0, 2):
            M.check_frame(oracle, sc, ref, thr, frames[f], lm[f], bd[f], ("rt8 mix", exclusive, f))
            M.check_pool({k: pool[k][f] for k in M.POOL_KEYS}, ref, ("rt8 mix", exclusive, f))
        l1, d1, p1 = _b1(fe, sc, 1, T1, thr, exclusive, fr)
        assert np.array_equal(lm[1, :len(l1)], l1) and np.array_equal(bd[1, :len(l1)], d1)
        for k in M.POOL_KEYS:
            assert np.array_equal(pool[k][1].view(np.uint8), np.ascontiguousarray(p1[k]).view(np.uint8)), k
        st8, proj8, _ = R8.project(c8, np.where(sc["hp"][:, 3:4] < 0, -sc["hp"][:, :3], sc["hp"][:, :3]) @
                                   T1[0].reshape(3, 3) - T1[1] @ T1[0].reshape(3, 3))
        assert (pool["projection"][1] != pool["projection"][0]).any()  # (the other model projects elsewhere)
        kept = (pool["projection"][1] != 0).any(axis=1)
        assert kept.sum() > 50 and np.allclose(pool["projection"][1][kept], proj8[kept], rtol=0, atol=1e-6)


def test_table_check_rejects_malformed_tables(oracle):
    """to the check only, never to the matcher; okvfe_last_error names the row"""
    sc = S.packing_scene(65, "mixed")
    fe = _frontend([sc["cam"]])
    a = M.table_arrays(sc)
    fe.landmark_table_check_device(M.DeviceTable(fe, sc).desc)
    b = a["obs_begin"]

    def rejected(**kw):
        with pytest.raises(capi.OkvfeError) as e:
            fe.landmark_table_check_device(M.DeviceTable(fe, sc, **kw).desc)
        assert e.value.status == capi.ERR_INVALID_ARGUMENT, kw
        return str(e.value)

    bad = b.copy()
    bad[40], bad[41] = b[41], b[40]  # rows 39 (end before begin is row 40's) -> first offender: row 40
    msg = rejected(obs_begin=bad)
    first = next(l for l in range(65) if bad[l + 1] < bad[l] or bad[l] < 0 or bad[l + 1] > len(a["obs_pose"]))
    assert "monotone" in msg and f"at {first}" in msg, msg
    bad = b.copy()
    bad[-1] = len(a["obs_pose"]) + 1  # past n_observations: the last row
    msg = rejected(obs_begin=bad)
    assert "monotone" in msg and "at 64" in msg, msg
    bad = b.copy()
    bad[0] = -1
    assert "at 0" in rejected(obs_begin=bad)
    for value in (-1, len(sc["poses"])):
        op = a["obs_pose"].copy()
        op[77] = value
        op[100] = value
        msg = rejected(obs_pose=op)
        assert "pose index" in msg and "observation 77" in msg, msg
    # host-side rejections: nothing is launched
    t = M.DeviceTable(fe, sc)
    d = t.desc
    for field in ("hp_W", "obs_begin", "obs_desc", "poses"):
        broken = capi.LandmarkTableDevice.from_buffer_copy(d)
        setattr(broken, field, None)
        with pytest.raises(capi.OkvfeError) as e:
            fe.landmark_table_check_device(broken)
        assert e.value.status == capi.ERR_INVALID_ARGUMENT, field
    broken = capi.LandmarkTableDevice.from_buffer_copy(d)
    broken.n_observations = -1
    with pytest.raises(capi.OkvfeError):
        fe.landmark_table_check_device(broken)


def test_argument_rejection_and_missing_intrinsics(oracle):
    sc = S.packing_scene(2, "all")
    cfg = dataclasses.replace(synth.euroc_config(), cams=[sc["cam"]])
    fe = G.make_frontend(cfg, num_cameras=2)
    try:
        fe.set_camera(0, sc["cam"])
        tab = M.DeviceTable(fe, sc)
        T1 = (np.asarray(sc["T1"][0], dtype=np.float64).reshape(-1), np.asarray(sc["T1"][1], dtype=np.float64))
        fr = M.clutter_frame(oracle, sc, 10, 1)
        with pytest.raises(capi.OkvfeError) as e:  # slot 1 has no intrinsics
            M.run_batch(fe, tab, [fr, fr], [T1, T1], [0, 1], 20.0, False)
        assert e.value.status == capi.ERR_NOT_READY and "slot 1" in str(e.value)
        for cam in (-1, 2):
            with pytest.raises(capi.OkvfeError) as e:
                M.run_batch(fe, tab, [fr], [T1], [cam], 20.0, False)
            assert e.value.status == capi.ERR_NOT_READY
        for thr in (-1.0, float("nan")):
            with pytest.raises(capi.OkvfeError) as e:
                M.run_batch(fe, tab, [fr], [T1], [0], thr, False)
            assert e.value.status == capi.ERR_INVALID_ARGUMENT
        buf = torch.zeros(fe.max_keypoints, dtype=torch.int32, device="cuda")
        blocks = torch.zeros(fe.gather_block_bytes(), dtype=torch.uint8, device="cuda")
        for kw in (dict(blocks=None), dict(lm=None), dict(bd=None)):
            a = dict(blocks=blocks.data_ptr(), lm=buf.data_ptr(), bd=buf.data_ptr())
            a.update(kw)
            with pytest.raises(capi.OkvfeError) as e:
                fe.match_to_map_table_blocks_device(tab.desc, a["blocks"], 1, [0], [T1], 20.0, False, None, None,
                                                    a["lm"], a["bd"])
            assert e.value.status == capi.ERR_INVALID_ARGUMENT, kw
        st = capi.lib().okvfe_match_to_map_table_blocks_device(fe._h, None, None, -1, None, None, capi.C.c_double(20.0), 0,
                                                               None, None, None, None, None)
        assert st == capi.ERR_INVALID_ARGUMENT
    finally:
        fe.close()


def _small_case(oracle, n, pattern, seed_frames):
    sc = S.packing_scene(n, pattern)
    T1 = (np.asarray(sc["T1"][0], dtype=np.float64).reshape(-1), np.asarray(sc["T1"][1], dtype=np.float64))
    moved = (T1[0], T1[1] + np.array([0.05, -0.02, 0.01]))
    ref = M.reference(oracle, sc, T1, sc["cam"], False, 20.0)
    fr = S.dictated_frame(oracle, sc, ref, clutter=30, seed=seed_frames)[:3]
    K = synth.euroc_config().max_kpts
    frames = [(fr[0][:K], fr[1][:K], fr[2][:K]), M.clutter_frame(oracle, sc, 200, seed_frames)]
    return sc, frames, [T1, moved]


def _sleep_cycles_for(ms):
    """torch.cuda._sleep cycles for about `ms` of device time, measured"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    probe = 2_000_000
    a.record()
    torch.cuda._sleep(probe)
    b.record()
    torch.cuda.synchronize()
    return int(probe * ms / max(a.elapsed_time(b), 1e-3))


def test_the_call_does_not_synchronise_the_host(oracle):
    """a device-side delay of about 50 ms is queued on the stream first: the call returns while the stream is busy"""
    sc, frames, poses = _small_case(oracle, 1025, "mixed", 1)
    fe = _frontend([sc["cam"]])
    tab = M.DeviceTable(fe, sc)
    st = torch.cuda.Stream()
    M.run_batch(fe, tab, frames, poses, [0, 0], 20.0, False, stream=st)  # (sizes the per-stream workspace and the ring)
    cycles = _sleep_cycles_for(50.0)
    T = M.prepare_batch(fe, tab, frames, True)
    with torch.cuda.stream(st):
        torch.cuda._sleep(cycles)
    M.launch_batch(fe, tab, T, poses, [0, 0], 20.0, False, stream=st)
    busy = not st.query()
    lm, bd, pool, _ = M.collect(T, tab.n_landmarks, st)
    assert busy, "the call returned only after the stream had drained"
    for f in range(2):
        ref = M.reference(oracle, sc, poses[f], sc["cam"], False, 20.0)
        M.check_frame(oracle, sc, ref, 20.0, frames[f], lm[f], bd[f], ("async", f))
        M.check_pool({k: pool[k][f] for k in M.POOL_KEYS}, ref, ("async", f))


def test_two_streams_in_flight(oracle):
    """two calls with different tables and batches queued on two streams before either is waited for"""
    cases = [_small_case(oracle, 2049, "mixed", 1), _small_case(oracle, 1023, "alternating", 2)]
    fe = _frontend([cases[0][0]["cam"]])
    tabs = [M.DeviceTable(fe, c[0]) for c in cases]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for i in range(2):  # (sizes the per-stream workspaces)
        M.run_batch(fe, tabs[i], cases[i][1], cases[i][2], [0, 0], 20.0, False, stream=streams[i])
    cycles = _sleep_cycles_for(5.0)
    pending = [M.prepare_batch(fe, tabs[i], cases[i][1], True) for i in range(2)]
    for i in range(2):
        with torch.cuda.stream(streams[i]):
            torch.cuda._sleep(cycles)  # (holds the stream so that both calls are queued before either runs)
        M.launch_batch(fe, tabs[i], pending[i], cases[i][2], [0, 0], 20.0, False, stream=streams[i])
    for i in range(2):
        sc, frames, poses = cases[i]
        lm, bd, pool, _ = M.collect(pending[i], tabs[i].n_landmarks, streams[i])
        for f in range(2):
            ref = M.reference(oracle, sc, poses[f], sc["cam"], False, 20.0)
            M.check_frame(oracle, sc, ref, 20.0, frames[f], lm[f], bd[f], ("streams", i, f))
            M.check_pool({k: pool[k][f] for k in M.POOL_KEYS}, ref, ("streams", i, f))


def test_sliced_batch_of_64_frames(oracle):
    """64 frames x 1500 landmarks with the workspace limit lowered (test hook) so that the call runs in slices of 5
    frames, the last one short; equal to the unsliced call and, on a sample of frames, to the reference"""
    m = dict(map_synth.make_map(1500, seed=21), name="map-1500")
    fe = _frontend([m["cam"]])
    K = fe.max_keypoints
    tab = M.DeviceTable(fe, m)
    fe.landmark_table_check_device(tab.desc)
    C1, r1 = m["T1"][0].reshape(3, 3), m["T1"][1]
    frames, poses = [], []
    for f in range(64):
        poses.append(((C1 @ map_synth.rot_y(0.004 * (f - 32))).reshape(-1), r1 + np.array([0.01 * f, 0.0, 0.002 * f])))
        kps, desc, use = map_synth.make_frame(dict(m, T1=poses[-1]), oracle, n_kps=(K, 0, 650, 333)[f % 4], seed=f)
        frames.append((kps, desc, use))
    per_frame = 1500 * 32 + K * 4 + 4
    try:
        fe._test_set_map_table_workspace_limit(5 * per_frame + 100)
        lm, bd, pool, _ = M.run_batch(fe, tab, frames, poses, [0] * 64, 20.0, False)
    finally:
        fe._test_set_map_table_workspace_limit(0)
    lm1, bd1, pool1, _ = M.run_batch(fe, tab, frames, poses, [0] * 64, 20.0, False)
    assert np.array_equal(lm, lm1) and np.array_equal(bd, bd1)
    for k in M.POOL_KEYS:
        assert np.array_equal(pool[k].view(np.uint8), pool1[k].view(np.uint8)), k
    hits = 0
    for f in (0, 4, 5, 6, 9, 10, 62, 63):  # both sides of the slice edges, the short last slice
        ref = M.reference(oracle, m, poses[f], m["cam"], False, 20.0)
        hits += int((M.check_frame(oracle, m, ref, 20.0, frames[f], lm[f], bd[f], ("sliced", f)) >= 0).sum())
        M.check_pool({k: pool[k][f] for k in M.POOL_KEYS}, ref, ("sliced", f))
    assert hits > 300


def test_ten_streams_recycle_the_table_workspace(oracle):
    """Both passes on ten streams of ONE context, twice over, with 1..3 frames per call: the context keeps eight
    per-stream workspaces, so later streams evict the oldest entries (the default stream's first), an evicted stream
    gets a fresh buffer in the second round and a kept one has to grow.  Every stream's rows equal the default-stream
    call's byte for byte; rows past n_frames keep their sentinels."""
    import map_table_uninit_common as U
    sc, _, poses = _small_case(oracle, 200, "mixed", 3)
    poses = [poses[0], poses[1], poses[0]]
    ref = M.reference(oracle, sc, poses[0], sc["cam"], False, 20.0)
    frames = [U.frame(oracle, sc, ref, sc["cam"], 24, 16, seed, n3d=8) for seed in (1, 2, 3)]
    cfg = dataclasses.replace(synth.euroc_config(), cams=[sc["cam"]])
    fe = G.make_frontend(cfg)
    keys = ("lm", "bd", "lm2", "bd2", "hp", "hs", "ctr") + tuple(M.POOL_KEYS)

    def queue(nf, stream):
        """both passes on the first nf frames of a three-frame batch -> (the tensors before the calls, the tensors)"""
        T = U.prepare(fe, tab.n_landmarks, frames)
        before = {k: T[k].cpu().numpy().copy() for k in keys}
        fe.match_to_map_table_blocks_device(tab.desc, T["blocks"].data_ptr(), nf, [0] * nf, poses[:nf], 20.0, False,
                                            T["use"].data_ptr(), U.pool_device(fe, T), T["lm"].data_ptr(),
                                            T["bd"].data_ptr(), stream)
        fe.match_to_map_table_uninitialised_blocks_device(
            tab.desc, U.pool_device(fe, T, projection=False), T["blocks"].data_ptr(), nf, [0] * nf,
            [U.second_pose(p) for p in poses[:nf]], False, T["use"].data_ptr(), T["prev"].data_ptr(), T["lm2"].data_ptr(),
            T["bd2"].data_ptr(), T["hp"].data_ptr(), T["hs"].data_ptr(), T["ctr"].data_ptr(), stream)
        return before, T

    try:
        fe.set_camera(0, sc["cam"])
        tab = M.DeviceTable(fe, sc)
        _, T = queue(3, None)
        torch.cuda.synchronize()
        want = {k: T[k].cpu().numpy() for k in keys}
        assert (want["lm"] >= 0).sum() >= 8 and (want["lm2"] >= 0).sum() >= 8, "the scene exercises neither pass"
        streams = [torch.cuda.Stream() for _ in range(10)]
        pending = []
        for rnd in range(2):
            for i, st in enumerate(streams):
                nf = 1 + (i + rnd) % 3
                pending.append((rnd, i, nf) + queue(nf, st))
        torch.cuda.synchronize()
        for rnd, i, nf, before, T in pending:
            for k in keys:
                got = T[k].cpu().numpy()
                assert got[:nf].tobytes() == want[k][:nf].tobytes(), (rnd, i, k, "rows of the call")
                assert got[nf:].tobytes() == before[k][nf:].tobytes(), (rnd, i, k, "rows past n_frames")
    finally:
        fe.close()
