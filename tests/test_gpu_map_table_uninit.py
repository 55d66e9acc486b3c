"""GPU: okvfe_match_to_map_table_uninitialised_blocks_device -- the second pass of matchToMap for a batch of frames,
every frame over the landmarks ITS first pass left with status 2 (pack_uninit_frames_kernel,
match_to_map_table_uninit_kernel).  The first pass is okvfe_match_to_map_table_blocks_device with a pool on the same
stream (general scenes, packing edges, mixed cameras, slicing) or a hand-built pool (the gate scenes).  Every frame is
checked against the per-frame reference of map_table_uninit_common.reference under both orders of the 3-term FP64 sums:
landmark, distance, hp_set and already_matched for equality, hps_W as uint64 patterns with the NaN-place rule; rows at
or past a frame's keypoint count keep their sentinels."""
import dataclasses

import numpy as np
import pytest

import gate_scenes
import gpu_common as G
import map_scenes as S
import map_synth
import map_table_common as M
import map_table_uninit_common as U
from okvis2_amd import capi, synth

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp64_order")]
torch = pytest.importorskip("torch")

_FRONTENDS = {}


def _frontend(cams, max_kpts=None):
    """a context of the first camera's size whose slots hold `cams`"""
    key = tuple((c.w, c.h, c.fu, c.fv, c.cu, c.cv, c.dist_type, tuple(c.d)) for c in cams) + (max_kpts,)
    if key not in _FRONTENDS:
        cfg = dataclasses.replace(synth.euroc_config(), w=cams[0].w, h=cams[0].h, cams=list(cams))
        if max_kpts:
            cfg = dataclasses.replace(cfg, max_kpts=max_kpts)
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


def _pose(sc):
    return np.asarray(sc["T1"][0], dtype=np.float64).reshape(-1), np.asarray(sc["T1"][1], dtype=np.float64)


def _full_frame(oracle, sc, ref, cam, K, seed, clutter=60, n3d=0):
    """exactly K keypoints if the status-2 rows allow it, the rest clutter (n3d of it on 3-D landmarks)"""
    rows = int(ref["n_desc"][ref["status"] == 2].sum())
    n = max(0, min(rows, K - min(clutter, K)))
    return U.frame(oracle, sc, ref, cam, n, K - n, seed, n3d)


def _two_passes(fe, tab, frames, poses1, poses2, cam_ids, thr, exclusive, stream=None):
    """first pass with a pool, then the second pass on the same stream, nothing waited for in between"""
    T = U.prepare(fe, tab.n_landmarks, frames)
    U.launch_first(fe, tab, T, poses1, cam_ids, thr, exclusive, stream=stream)
    U.launch_second(fe, tab, T, poses2, cam_ids, exclusive, stream=stream)
    return T, U.collect(T, stream)


def _check_all(oracle, sc, refs1, frames, poses2, cams, cam_ids, exclusive, got, what, **kw):
    hits = 0
    for f, fr in enumerate(frames):
        r = U.reference(oracle, sc["obs_desc"], refs1[f], fr, poses2[f], cams[cam_ids[f]], exclusive, **kw)
        U.check_frame(got, f, len(fr["desc"]), r, what + (f,))
        hits += int((r[0] >= 0).sum())
    return hits


def _scene_batch(oracle, sc, K, exclusive, thr):
    """frames of K, 0, 1, 63, 64 and 65 keypoints at the scene's pose with the second pose of
    map_table_uninit_common.second_pose; one frame whose second pose is the first, bit for bit; one whose second pose
    is an observing pose of the table (zero baseline for its observations: NaN epipolar normals).  Some clutter
    keypoints of every frame sit on 3-D landmarks, so that the first pass matches them."""
    P = M.scene_poses(sc)
    cam = sc["cam"]
    ref0 = M.reference(oracle, sc, P[0], cam, exclusive, thr)
    full = _full_frame(oracle, sc, ref0, cam, K, 1, n3d=40)
    other = _full_frame(oracle, sc, ref0, cam, K, 2, n3d=40)
    frames = [full] + [U.head(other, n) for n in (0, 1, 63, 64, 65)] + [_full_frame(oracle, sc, ref0, cam, 400, 3, n3d=20),
                                                                      _full_frame(oracle, sc, ref0, cam, 500, 4, n3d=20)]
    poses2 = [U.second_pose(P[0])] * 6 + [P[0], P[1]]
    return frames, [P[0]] * len(frames), poses2, [ref0] * len(frames)


@pytest.mark.parametrize("spec", [s for s in S.GENERAL_SPECS if s[0] != "radtan8"], ids=lambda s: f"{s[0]}-s{s[1]}")
def test_general_scene_as_a_batch(oracle, spec):
    sc = S.general_scene(*spec)
    cam = sc["cam"]
    fe = _frontend([cam])
    K = fe.max_keypoints
    tab = M.DeviceTable(fe, sc)
    for exclusive, thr in S.MODES:
        what = (sc["name"], "exclusive" if exclusive else "non-exclusive")
        frames, poses1, poses2, refs1 = _scene_batch(oracle, sc, K, exclusive, thr)
        assert [len(f["desc"]) for f in frames[:6]] == [K, 0, 1, 63, 64, 65]
        nf, ids = len(frames), [0] * len(frames)
        T, got = _two_passes(fe, tab, frames, poses1, poses2, ids, thr, exclusive)
        for f in range(nf):  # (the first pass left what the oracle's preparation leaves)
            M.check_pool({k: T[k][f].cpu().numpy()[:tab.n_landmarks] for k in M.POOL_KEYS}, refs1[f], what + (f, "pool"))
        hits = _check_all(oracle, sc, refs1, frames, poses2, [cam], ids, exclusive, got, what)
        assert hits >= 100, (what, hits)
        first_lm = got["lm"].copy()
        # the other variants of (use_dev, previous) on the same pool, and the exclusive second pass on it
        for with_use, with_prev, excl2 in ((False, True, exclusive), (True, False, exclusive), (False, False, exclusive),
                                           (True, True, True)):
            U.launch_second(fe, tab, T, poses2, ids, excl2, with_use=with_use, previous="prev" if with_prev else None)
            got = U.collect(T)
            _check_all(oracle, sc, refs1, frames, poses2, [cam], ids, excl2, got, what + (with_use, with_prev, excl2),
                       with_use=with_use, with_previous=with_prev)
        # the first pass's best_landmark_dev straight in as `previous`, exclusive = 0: exactly the matched keypoints
        # are skipped
        U.launch_second(fe, tab, T, poses2, ids, False, previous="lm")
        got = U.collect(T)
        skipped = 0
        for f, fr in enumerate(frames):
            n = len(fr["desc"])
            fr2 = dict(fr, previous=first_lm[f, :n])
            r = U.reference(oracle, sc["obs_desc"], refs1[f], fr2, poses2[f], cam, False)
            U.check_frame(got, f, n, r, what + (f, "previous = first pass"))
            matched = first_lm[f, :n] >= 0
            assert np.all(got["lm2"][f, :n][matched] == -1) and np.all(got["bd2"][f, :n][matched] == M.THRESHOLD)
            free = U.reference(oracle, sc["obs_desc"], refs1[f], fr, poses2[f], cam, False, with_previous=False)
            assert np.array_equal(got["lm2"][f, :n][~matched], free[0][~matched]), (what, f, "the others are not")
            skipped += int(matched.sum())
        assert skipped >= 30, (what, skipped)


def _gate_frontend(cam):
    return _frontend([cam], max_kpts=2048)


@pytest.mark.parametrize("spec", gate_scenes.UNINIT_SPECS, ids=gate_scenes.spec_id)
def test_gate_scene_through_a_hand_built_pool(oracle, spec):
    """every branch of the gate chain: the scenes of test_gpu_gate_census.py, their landmarks as a table and a pool
    (rows truncated to two, a seventh of the landmarks status 1 with their rows left in place, empty ones status 0),
    exclusive, two frames per call: the scene and its first half"""
    sc = gate_scenes.uninit_scene(spec[0], spec[1], spec[2], **spec[3])
    cam = sc["cam"]
    fe = _gate_frontend(cam)
    obs_desc, pool = U.gate_pool(sc)
    L = len(pool["status"])
    tab = U.DescTable(fe, obs_desc, L)
    n = len(sc["desc"])
    frames = [U.gate_frame(sc), U.gate_frame(sc, n // 2)]
    T = U.prepare(fe, L, frames, pool=[pool, pool])
    U.launch_second(fe, tab, T, [sc["T1"]] * 2, [0, 0], True)
    got = U.collect(T)
    for f, fr in enumerate(frames):
        r = U.reference(oracle, obs_desc, pool, fr, sc["T1"], cam, True)
        U.check_frame(got, f, len(fr["desc"]), r, (sc["name"], f))


PACK_SIZES = (1, 2, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025, 2049)


@pytest.mark.parametrize("n", PACK_SIZES)
def test_packing_at_the_chunk_edges(oracle, n):
    """the edges of the 1024-row scan chunks of pack_uninit_frames_kernel, of the eight ranges and of the matcher's
    chunks; the `all` pattern leaves an empty status-2 set"""
    hits = 0
    for pattern in ("none", "mixed", "alternating", "all"):
        sc = S.packing_scene(n, pattern)
        cam = sc["cam"]
        fe = _frontend([cam])
        K = fe.max_keypoints
        tab = M.DeviceTable(fe, sc)
        T1 = _pose(sc)
        for exclusive, thr in S.MODES:
            what = (sc["name"], exclusive)
            ref = M.reference(oracle, sc, T1, cam, exclusive, thr)
            if pattern == "all":
                assert not (ref["status"] == 2).any()
            big = _full_frame(oracle, sc, ref, cam, K, 1, clutter=30)
            frames = [big, U.head(_full_frame(oracle, sc, ref, cam, K, 2, clutter=30), 65)]
            poses2 = [U.second_pose(T1)] * 2
            _, got = _two_passes(fe, tab, frames, [T1] * 2, poses2, [0, 0], thr, exclusive)
            hits += _check_all(oracle, sc, [ref] * 2, frames, poses2, [cam], [0, 0], exclusive, got, what)
            if pattern == "all":
                for f, fr in enumerate(frames):
                    m = len(fr["desc"])
                    assert np.all(got["lm2"][f, :m] == -1) and np.all(got["bd2"][f, :m] == M.THRESHOLD)
                    assert not got["hs"][f, :m].any() and not got["hp"][f, :m].any() and got["ctr"][f] == 0
    assert hits > 0 or n < 7, n


def test_table_without_landmarks(oracle):
    """L == 0: the rows below a block's count still receive -1, match_threshold, a zero hp and hp_set 0, written by a
    kernel; every pool member may be NULL then"""
    sc = S.packing_scene(2, "all")
    cam = sc["cam"]
    fe = _frontend([cam])
    K = fe.max_keypoints
    empty = dict(sc, hp=sc["hp"][:0], quality=sc["quality"][:0], obs_begin=np.zeros(1, np.int32),
                 obs_pose=sc["obs_pose"][:0], obs_desc=sc["obs_desc"][:0], obs_bp=sc["obs_bp"][:0])
    tab = M.DeviceTable(fe, empty)
    assert tab.n_landmarks == 0
    ref = M.reference(oracle, sc, _pose(sc), cam, False, 20.0)
    frames = [U.frame(oracle, sc, ref, cam, 0, m, 1) for m in (130, 0, K)]
    T = U.prepare(fe, 0, frames)
    for null_pool in (False, True):
        for k in ("lm2", "bd2"):
            T[k].fill_(U.SENTINEL)
        T["hp"].fill_(float(U.SENTINEL))
        T["hs"].fill_(U.HS_FILL)
        T["ctr"].fill_(U.CTR_FILL)
        torch.cuda.synchronize()
        pool = fe.make_landmark_pool_device() if null_pool else U.pool_device(fe, T, projection=False)
        fe.match_to_map_table_uninitialised_blocks_device(
            tab.desc, pool, T["blocks"].data_ptr(), 3, [0] * 3, [_pose(sc)] * 3, True, T["use"].data_ptr(),
            T["prev"].data_ptr(), T["lm2"].data_ptr(), T["bd2"].data_ptr(), T["hp"].data_ptr(), T["hs"].data_ptr(),
            T["ctr"].data_ptr())
        got = U.collect(T)
        for f, fr in enumerate(frames):
            m = len(fr["desc"])
            none = (np.full(m, -1, np.int32), np.full(m, M.THRESHOLD, np.int32), np.zeros((m, 4)), np.zeros(m, np.uint8), 0)
            U.check_frame(got, f, m, none, ("L = 0", null_pool, f))


def test_mixed_cameras_in_one_context(oracle):
    """slots 0..2 of a context of EuRoC size: the EuRoC camera, the same pinhole without a distortion, an equidistant
    camera of another focal length; cam_ids differ per frame, and with them sigma = 1 / focal of the gate chain"""
    sc = S.general_scene("euroc", 0)
    c0 = sc["cam"]
    cams = [c0, dataclasses.replace(c0, dist_type=0, d=(0.0, 0.0, 0.0, 0.0)),
            dataclasses.replace(c0, fu=351.31400364193297, fv=351.4911744656785, dist_type=2,
                                d=tuple(synth.hilti_config().cams[0].d))]
    fe = _frontend(cams)
    K = fe.max_keypoints
    tab = M.DeviceTable(fe, sc)
    P = M.scene_poses(sc)
    for exclusive, thr in S.MODES:
        frames, poses1, poses2, cam_ids, refs1 = [], [], [], [], []
        for i, (c, p) in enumerate(((2, P[0]), (0, P[0]), (1, P[0]), (1, P[3]), (2, P[1]), (0, P[3]))):
            ref = M.reference(oracle, sc, p, cams[c], exclusive, thr)
            frames.append(_full_frame(oracle, sc, ref, cams[c], 300, 10 + i))
            poses1.append(p)
            poses2.append(U.second_pose(p))
            cam_ids.append(c)
            refs1.append(ref)
        _, got = _two_passes(fe, tab, frames, poses1, poses2, cam_ids, thr, exclusive)
        hits = _check_all(oracle, sc, refs1, frames, poses2, cams, cam_ids, exclusive, got, ("mixed", exclusive))
        assert hits > 100
        # the focal length shows: frame 0 under slot 0's constants is another answer
        a = U.reference(oracle, sc["obs_desc"], refs1[0], frames[0], poses2[0], cams[2], exclusive)
        b = U.reference(oracle, sc["obs_desc"], refs1[0], frames[0], poses2[0], cams[0], exclusive)
        assert not (np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3]) and
                    np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64)))


def _small_case(oracle, n, pattern, seed):
    sc = S.packing_scene(n, pattern)
    T1 = _pose(sc)
    moved = (T1[0], T1[1] + np.array([0.05, -0.02, 0.01]))
    refs = [M.reference(oracle, sc, p, sc["cam"], True, 150.0) for p in (T1, moved)]
    frames = [_full_frame(oracle, sc, refs[0], sc["cam"], 600, seed), _full_frame(oracle, sc, refs[1], sc["cam"], 200, seed)]
    return sc, frames, [T1, moved], [U.second_pose(T1), U.second_pose(moved)], refs


def test_argument_rejection_and_missing_intrinsics(oracle):
    sc, frames, poses1, poses2, refs = _small_case(oracle, 65, "mixed", 1)
    cfg = dataclasses.replace(synth.euroc_config(), cams=[sc["cam"]])
    fe = G.make_frontend(cfg, num_cameras=2)
    try:
        fe.set_camera(0, sc["cam"])
        tab = M.DeviceTable(fe, sc)
        T = U.prepare(fe, tab.n_landmarks, frames)
        U.launch_first(fe, tab, T, poses1, [0, 0], 150.0, True)
        torch.cuda.synchronize()
        with pytest.raises(capi.OkvfeError) as e:  # slot 1 has no intrinsics
            U.launch_second(fe, tab, T, poses2, [0, 1], True)
        assert e.value.status == capi.ERR_NOT_READY and "frame 1" in str(e.value) and "slot 1" in str(e.value)
        for cam in (-1, 2):
            with pytest.raises(capi.OkvfeError) as e:
                U.launch_second(fe, tab, T, poses2, [0, cam], True)
            assert e.value.status == capi.ERR_NOT_READY

        def call(**kw):
            a = dict(table=tab.desc, pool=U.pool_device(fe, T, projection=False), blocks=T["blocks"].data_ptr(),
                     lm=T["lm2"].data_ptr(), bd=T["bd2"].data_ptr(), hp=T["hp"].data_ptr(), hs=T["hs"].data_ptr(),
                     ctr=T["ctr"].data_ptr())
            a.update(kw)
            fe.match_to_map_table_uninitialised_blocks_device(a["table"], a["pool"], a["blocks"], 2, [0, 0], poses2, True,
                                                              None, None, a["lm"], a["bd"], a["hp"], a["hs"], a["ctr"])

        for kw in (dict(blocks=None), dict(lm=None), dict(bd=None), dict(hp=None), dict(hs=None), dict(ctr=None),
                   dict(pool=None)):
            with pytest.raises(capi.OkvfeError) as e:
                call(**kw)
            assert e.value.status == capi.ERR_INVALID_ARGUMENT, kw
        for member in ("status", "n_desc", "obs_rows", "e_W", "r_W"):  # required when L > 0
            broken = capi.LandmarkPoolDevice.from_buffer_copy(U.pool_device(fe, T))
            setattr(broken, member, None)
            with pytest.raises(capi.OkvfeError) as e:
                call(pool=broken)
            assert e.value.status == capi.ERR_INVALID_ARGUMENT, member
        no_desc = capi.LandmarkTableDevice.from_buffer_copy(tab.desc)
        no_desc.obs_desc = None
        with pytest.raises(capi.OkvfeError) as e:
            call(table=no_desc)
        assert e.value.status == capi.ERR_INVALID_ARGUMENT
        f = getattr(capi.lib(), "okvfe_match_to_map_table_uninitialised_blocks_device")
        assert f(fe._h, None, None, None, -1, None, None, 0, None, None, None, None, None, None, None, None) == \
            capi.ERR_INVALID_ARGUMENT
        # n_frames == 0 is fine and launches nothing: the outputs keep their sentinels
        fe.match_to_map_table_uninitialised_blocks_device(
            tab.desc, U.pool_device(fe, T), T["blocks"].data_ptr(), 0, [], [], True, None, None, T["lm2"].data_ptr(),
            T["bd2"].data_ptr(), T["hp"].data_ptr(), T["hs"].data_ptr(), T["ctr"].data_ptr())
        got = U.collect(T)
        assert np.all(got["lm2"] == U.SENTINEL) and np.all(got["ctr"] == U.CTR_FILL)
        call()  # (and the unbroken call passes)
        got = U.collect(T)
        for f_ in range(2):
            r = U.reference(oracle, sc["obs_desc"], refs[f_], frames[f_], poses2[f_], sc["cam"], True,
                            with_use=False, with_previous=False)
            U.check_frame(got, f_, len(frames[f_]["desc"]), r, ("after the rejections", f_))
    finally:
        fe.close()


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
    """a device-side delay of about 50 ms is queued on the stream first: both passes return while the stream is busy"""
    sc, frames, poses1, poses2, refs = _small_case(oracle, 1025, "mixed", 1)
    fe = _frontend([sc["cam"]])
    tab = M.DeviceTable(fe, sc)
    st = torch.cuda.Stream()
    _two_passes(fe, tab, frames, poses1, poses2, [0, 0], 150.0, True, stream=st)  # (sizes the workspace and the ring)
    cycles = _sleep_cycles_for(50.0)
    T = U.prepare(fe, tab.n_landmarks, frames)
    with torch.cuda.stream(st):
        torch.cuda._sleep(cycles)
    U.launch_first(fe, tab, T, poses1, [0, 0], 150.0, True, stream=st)
    U.launch_second(fe, tab, T, poses2, [0, 0], True, stream=st)
    busy = not st.query()
    got = U.collect(T, st)
    assert busy, "the calls returned only after the stream had drained"
    hits = _check_all(oracle, sc, refs, frames, poses2, [sc["cam"]], [0, 0], True, got, ("async",))
    assert hits > 50


def test_two_streams_in_flight(oracle):
    """two pairs of calls with different tables and batches queued on two streams before either is waited for"""
    cases = [_small_case(oracle, 2049, "mixed", 1), _small_case(oracle, 1023, "alternating", 2)]
    fe = _frontend([cases[0][0]["cam"]])
    tabs = [M.DeviceTable(fe, c[0]) for c in cases]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for i in range(2):  # (sizes the per-stream workspaces)
        _two_passes(fe, tabs[i], cases[i][1], cases[i][2], cases[i][3], [0, 0], 150.0, True, stream=streams[i])
    cycles = _sleep_cycles_for(5.0)
    pending = [U.prepare(fe, tabs[i].n_landmarks, cases[i][1]) for i in range(2)]
    for i in range(2):
        with torch.cuda.stream(streams[i]):
            torch.cuda._sleep(cycles)  # (holds the stream so that both pairs are queued before either runs)
        U.launch_first(fe, tabs[i], pending[i], cases[i][2], [0, 0], 150.0, True, stream=streams[i])
        U.launch_second(fe, tabs[i], pending[i], cases[i][3], [0, 0], True, stream=streams[i])
    for i in range(2):
        sc, frames, poses1, poses2, refs = cases[i]
        got = U.collect(pending[i], streams[i])
        assert _check_all(oracle, sc, refs, frames, poses2, [sc["cam"]], [0, 0], True, got, ("streams", i)) > 50


def test_sliced_batch_of_64_frames(oracle):
    """64 frames x 1500 landmarks with the workspace limit lowered (test hook) so that the second pass runs in slices of
    5 frames, the last one short; byte-equal to the unsliced call and, on frames either side of the slice edges, equal
    to the reference"""
    m = dict(map_synth.make_map(1500, seed=21), name="map-1500")
    cam = m["cam"]
    fe = _frontend([cam])
    K = fe.max_keypoints
    tab = M.DeviceTable(fe, m)
    C1, r1 = m["T1"][0].reshape(3, 3), m["T1"][1]
    checked = (0, 4, 5, 6, 9, 10, 62, 63)
    poses1 = [((C1 @ map_synth.rot_y(0.004 * (f - 32))).reshape(-1), r1 + np.array([0.01 * f, 0.0, 0.002 * f]))
              for f in range(64)]
    poses2 = [U.second_pose(p) for p in poses1]
    refs = {f: M.reference(oracle, m, poses1[f], cam, True, 150.0) for f in checked}
    frames = []
    for f in range(64):
        ref = refs[f] if f in refs else refs[min(checked, key=lambda c: abs(c - f))]
        frames.append(_full_frame(oracle, m, ref, cam, (K, 0, 650, 333)[f % 4], f))
    T = U.prepare(fe, tab.n_landmarks, frames)
    U.launch_first(fe, tab, T, poses1, [0] * 64, 150.0, True)
    per_frame = 1500 * 16 + 4
    try:
        fe._test_set_map_table_workspace_limit(5 * per_frame + 100)
        U.launch_second(fe, tab, T, poses2, [0] * 64, True)
    finally:
        fe._test_set_map_table_workspace_limit(0)
    sliced = U.collect(T)
    for k in ("lm2", "bd2"):
        T[k].fill_(U.SENTINEL)
    T["hp"].fill_(float(U.SENTINEL))
    T["hs"].fill_(U.HS_FILL)
    torch.cuda.synchronize()
    U.launch_second(fe, tab, T, poses2, [0] * 64, True)
    whole = U.collect(T)
    for k in ("lm2", "bd2", "hp", "hs", "ctr"):
        assert np.array_equal(sliced[k].view(np.uint8), whole[k].view(np.uint8)), k
    hits = 0
    for f in checked:
        r = U.reference(oracle, m["obs_desc"], refs[f], frames[f], poses2[f], cam, True)
        U.check_frame(sliced, f, len(frames[f]["desc"]), r, ("sliced", f))
        hits += int((r[0] >= 0).sum())
    assert hits > 100
