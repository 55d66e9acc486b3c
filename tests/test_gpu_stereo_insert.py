"""GPU: okvfe_stereo_insert_blocks_device (stereo_insert_kernel) against stereo_insert_ref.py, byte for byte: action, lm,
landmark_out and counts of every row of every scene of stereo_insert_scenes.py (whose census floor
test_stereo_insert_scenes_host.py holds), rows at or past a block's count keeping their sentinels.  Under both orders of
the FP64 sums; both block layouts; landmark_out in place and apart; without action / lm; without keyframe flags; a batch
cut into two calls; the edges of the kernel's two tables
(an overlay with one slot to spare, the largest capacity the LDS limit admits); the chain detection -> matcher per pair -> bookkeeping on a side stream with nothing waited for in
between, for a stereo pair and Hilti's five cameras; the C++ mirror through its CLI; the error paths, which launch
nothing."""
import ctypes
import dataclasses
import os
import struct
import subprocess

import numpy as np
import pytest

import gpu_common as G
import stereo_insert_ref as SR
import stereo_insert_scenes as S
from okvis2_amd import capi, multigpu, synth

pytestmark = [pytest.mark.gpu]
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE_NAMES = ("euroc-stereo", "stereo-counts", "hilti-3", "turned-3", "hilti-5", "turned-5", "chains-first-succeeds",
               "chains-first-fails", "chains-first-creates", "shared-bad-failed-edge", "across-pairs")
_FRONTENDS = {}


def _frontend(cams):
    """a W x H context with K = stereo_insert_scenes.K whose slots hold `cams`"""
    key = tuple((c.fu, c.fv, c.cu, c.cv, c.dist_type, tuple(c.d)) for c in cams)
    if key not in _FRONTENDS:
        fe = capi.Frontend(S.W, S.H, 10.0, 0, 50, S.K, match_threshold=60, num_cameras=len(cams))
        for i, c in enumerate(cams):
            fe.set_camera(i, c)
        _FRONTENDS[key] = fe
    return _FRONTENDS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_frontends():
    yield
    while _FRONTENDS:
        _FRONTENDS.popitem()[1].close()


def _tree(fp64_order):
    return fp64_order == "eigen_tree"


def _scene(oracle, tree, name):
    return {s["name"]: s for s in S.all_scenes(oracle, tree)}[name]


def _run(fe, sc, refs, what, **kw):
    T = S.prepare(fe, sc, **kw)
    S.launch(fe, sc, T)
    return S.check(sc, T, refs, what)


def test_scene_names_are_all_of_them(oracle):
    assert {s["name"] for s in S.all_scenes(oracle, True)} == set(SCENE_NAMES)


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_scene(oracle, fp64_order, name):
    tree = _tree(fp64_order)
    sc = _scene(oracle, tree, name)
    fe = _frontend(sc["cams"])
    refs, _ = S.reference(oracle, tree, name)
    what = (fp64_order,)
    got = _run(fe, sc, refs, what)
    assert int(got["counts"][:, 0].sum()) > 0
    _run(fe, sc, refs, what + ("camera-major, in place",), layout="camera-major", alias=True)
    _run(fe, sc, refs, what + ("in place",), alias=True)
    _run(fe, sc, refs, what + ("camera-major, without action / lm",), layout="camera-major", optional=False)
    refs_kf, _ = S.reference(oracle, tree, name, all_keyframes=True)
    _run(fe, sc, refs_kf, what + ("without keyframe flags",), keyframe_flags=False)
    # the batch cut into two calls, each addressing its part of the batch's arrays
    B = len(sc["mfs"])
    if B >= 2:
        for layout in ("multiframe-major", "camera-major"):
            T = S.prepare(fe, sc, layout=layout)
            S.launch_slice(fe, sc, T, B // 2, B - B // 2)
            part = {k: T[k].cpu().numpy().copy() for k in ("lm_out", "counts")}
            rows = B // 2 * (len(sc["cams"]) if layout == "multiframe-major" else 1)
            assert np.all(part["counts"][:B // 2] == S.SENTINEL), "the second half's call wrote the first half's counts"
            if layout == "multiframe-major":
                assert np.all(part["lm_out"][:rows] == S.SENTINEL)
            S.launch_slice(fe, sc, T, 0, B // 2)
            S.check(sc, T, refs, what + ("two calls", layout))


def _edge_frontend(n_cams, Kc):
    fe = capi.Frontend(S.W, S.H, 10.0, 0, 50, Kc, match_threshold=60, num_cameras=n_cams)
    for c in range(n_cams):
        fe.set_camera(c, S.camera("dyadic"))
    return fe


@pytest.mark.parametrize("which", ("overlay-one-slot-spare", "largest-capacity"))
def test_table_edges(oracle, fp64_order, which):
    """(a) three cameras of 341 keypoints: n_cams K = 1023 rows re-initialise a landmark into an overlay of 1024 slots;
    (b) two cameras of the largest capacity the LDS limit admits (one more is refused): 3250 overlay entries and 3250 keys
    per pair in tables of 4096 slots.  One dense multiframe of the scene generator each: every keypoint carries a row of
    its own and is matched, every match re-initialises (premises: test_capacity_scenes_host.py)."""
    tree = _tree(fp64_order)
    if which == "overlay-one-slot-spare":
        n_cams = 3
        Kc = next(k for k in range(S.K + 1, 4097) if n_cams * k == (1 << S.lds_bytes(n_cams, k)[1]) - 1)
        assert (Kc, S.lds_bytes(n_cams, Kc)[1]) == (341, 10)
    else:
        n_cams = 2
        Kc = S.largest_capacity(n_cams)
        assert S.lds_bytes(n_cams, Kc)[0] <= S.MAX_LDS < S.lds_bytes(n_cams, Kc + 1)[0]
        # the call's own answer one keypoint further: refused before anything is read or launched
        over = _edge_frontend(n_cams, Kc + 1)
        try:
            d = torch.zeros(64, dtype=torch.uint8, device="cuda")
            tab = over.make_landmark_table_device(0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
            res = over.make_stereo_insert_device(None, None, d.data_ptr(), d.data_ptr())
            with pytest.raises(capi.OkvfeError) as e:
                over.stereo_insert_blocks_device(tab, None, d.data_ptr(), n_cams, 1, 1, [(0, 1)], list(range(n_cams)),
                                                 [(S.I3, np.zeros(3))] * n_cams, d.data_ptr(), d.data_ptr(), None, res)
            assert e.value.status == capi.ERR_UNSUPPORTED and str(S.lds_bytes(n_cams, Kc + 1)[0]) in str(e.value), str(e.value)
        finally:
            over.close()
    sc = S.table_edge_scene(oracle, n_cams, Kc)
    refs, _ = S.reference_of(oracle, tree, sc)
    fe = _edge_frontend(n_cams, Kc)
    try:
        got = _run(fe, sc, refs, (fp64_order,))
        _, ov_log2, kh_log2 = S.lds_bytes(n_cams, Kc)
        print(sc["name"], fp64_order, "counts", got["counts"][0].tolist(), "| overlay load %d / %d" % (got["counts"][0, 2], 1 << ov_log2),
              "| key table load %d / %d per pair" % (2 * Kc, 1 << kh_log2))
        assert got["counts"][0].tolist() == [n_cams * Kc, 0, n_cams * Kc, 0]
        _run(fe, sc, refs, (fp64_order, "camera-major, in place"), layout="camera-major", alias=True)
    finally:
        fe.close()


def test_edge_verdicts_on_the_device(oracle, fp64_order):
    """exactly 4.0 px adds nothing; the bisected pair of adjacent doubles gets one verdict each"""
    tree = _tree(fp64_order)
    sc = _scene(oracle, tree, "shared-bad-failed-edge")
    refs, _ = S.reference(oracle, tree, sc["name"])
    got = _run(_frontend(sc["cams"]), sc, refs, (fp64_order, "edge"))
    mf = sc["mfs"][3]
    verdicts = [bool(got["action"][0, 3, k0] & SR.OBS0) for k0, _ in mf["expect_obs0"]]
    assert verdicts == [e for _, e in mf["expect_obs0"]] and verdicts[:4] == [False, False, True, True]
    assert verdicts[4] != verdicts[5]


# ---- from detection on ----------------------------------------------------------------------------------------------
def _chain(oracle, cfg, pairs, frames, poses, tree):
    """frames[m][c]: images; poses[c]: T_WC, the same for every multiframe.  Detection and description of every image,
    the gather blocks (camera-major), one matcher call per pair and the bookkeeping, all on one side stream with nothing
    waited for in between; then everything downloaded and the restatement run on the device's keypoints and rows."""
    n_cams, B = len(cfg.cams), len(frames)
    fe = G.make_frontend(cfg, max_batch=n_cams * B, num_cameras=n_cams)
    try:
        for c in range(n_cams):
            fe.set_camera(c, cfg.cams[c])
        Kc, bb = fe.max_keypoints, fe.gather_block_bytes()
        d_img = torch.from_numpy(np.stack([frames[m][c] for c in range(n_cams) for m in range(B)])).cuda()
        cam_ids = np.repeat(np.arange(n_cams, dtype=np.int32), B)
        grav = np.stack([synth.gravity_in_camera(poses[c][0]) for c in range(n_cams) for _ in range(B)]).astype(np.float32)
        d_blocks = torch.zeros(n_cams * B, bb, dtype=torch.uint8, device="cuda")
        d_matches = torch.zeros(len(pairs), B, Kc * capi.STEREO_MATCH_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_lm = torch.full((n_cams * B, Kc), -1, dtype=torch.int32, device="cuda")
        d_action = torch.full((len(pairs), B, Kc), S.ACTION_SENTINEL, dtype=torch.uint8, device="cuda")
        d_lm_row = torch.full((len(pairs), B, Kc), S.SENTINEL, dtype=torch.int32, device="cuda")
        d_counts = torch.full((B, 4), S.SENTINEL, dtype=torch.int32, device="cuda")
        focal = [0.5 * (c.fu + c.fv) for c in cfg.cams]
        tab = fe.make_landmark_table_device(0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
        res = fe.make_stereo_insert_device(d_action.data_ptr(), d_lm_row.data_ptr(), d_lm.data_ptr(), d_counts.data_ptr())
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        fe.detect_describe_batch_device(d_img.data_ptr(), n_cams * B, cam_ids, grav, st)
        fe.pack_gather_blocks_device(0, n_cams * B, d_blocks.data_ptr(), st)
        for p, (c0, c1) in enumerate(pairs):
            fe.match_stereo_blocks_batch_device(d_blocks.data_ptr() + c0 * B * bb, d_blocks.data_ptr() + c1 * B * bb, B,
                                                poses[c0], poses[c1], focal[c0], focal[c1], d_matches[p].data_ptr(), st)
        fe.stereo_insert_blocks_device(tab, None, d_blocks.data_ptr(), 1, B, B, pairs, list(range(n_cams)),
                                       [poses[c] for _ in range(B) for c in range(n_cams)], d_matches.data_ptr(),
                                       d_lm.data_ptr(), None, res, st)
        st.synchronize()
        blocks = d_blocks.cpu().numpy()
        rows = d_matches.cpu().numpy().reshape(len(pairs), B, -1).view(capi.STEREO_MATCH_DTYPE)
        action, lm_row, lm_out, counts = (t.cpu().numpy() for t in (d_action, d_lm_row, d_lm, d_counts))
    finally:
        fe.close()
    oracle.set_reduction(tree)
    census = SR.new_census()
    for m in range(B):
        kps = [multigpu.unpack_block_host(blocks[c * B + m], Kc)[0] for c in range(n_cams)]
        n = [len(k) for k in kps]
        ref = SR.stereo_insert(oracle, tree, np.zeros((0, 4)), np.zeros(0, np.uint8), cfg.cams, pairs, Kc, kps,
                               [np.full(n[c], -1, np.int32) for c in range(n_cams)], poses,
                               [rows[p, m, :n[c0]] for p, (c0, _) in enumerate(pairs)], True, census)
        assert counts[m].tolist() == ref["counts"].tolist(), (m, counts[m], ref["counts"])
        for c in range(n_cams):
            assert np.array_equal(lm_out[c * B + m, :n[c]], ref["ids"][c]), (m, c)
            assert np.all(lm_out[c * B + m, n[c]:] == -1)
        for p, (c0, _) in enumerate(pairs):
            assert np.array_equal(action[p, m, :n[c0]], ref["action"][p]), (m, p)
            assert np.array_equal(lm_row[p, m, :n[c0]], ref["lm"][p]), (m, p)
            assert np.all(action[p, m, n[c0]:] == S.ACTION_SENTINEL) and np.all(lm_row[p, m, n[c0]:] == S.SENTINEL)
    return census


def test_chain_from_detection_stereo(oracle, fp64_order):
    cfg = synth.euroc_config()
    frames = [synth.stereo_pair(cfg.w, cfg.h, 4200 + m)[:2] for m in range(2)]
    census = _chain(oracle, cfg, [(0, 1)], frames, list(synth.stereo_poses(cfg.baseline)), _tree(fp64_order))
    print(census)
    assert census["neither_keyframe"] > 50 and census["add0_accepted"] > 50 and census["add1_accepted"] > 50


def test_chain_from_detection_five_cameras(oracle, fp64_order):
    cfg = synth.hilti_config()
    pairs = synth.rig_overlap_pairs(cfg, capi.camera_overlap)
    assert 1 <= len(pairs) <= capi.STEREO_MAX_PAIRS
    rays = [capi.build_awareness_maps(c)[0] for c in cfg.cams]
    frames = [synth.render_rig(cfg, rays, 60)]
    census = _chain(oracle, cfg, pairs, frames, synth.rig_poses(cfg), _tree(fp64_order))
    print(census)
    assert census["neither_keyframe"] > 20 and census["read_id_earlier_pair"] > 0


# ---- the C++ mirror ---------------------------------------------------------------------------------------------------
def _cli(tmp_path, sc, mfs, mode, matches=None, keyframe=True, layout=(None, None)):
    """HipFrontend::matchStereoInsertBlocks (mode 0) / matchStereoRig (mode 1) through tests/cpp/stereo_insert_cli"""
    cli = os.path.join(ROOT, "tests", "cpp", "stereo_insert_cli")
    assert os.path.exists(cli), "run __graft_entry__.build() first"
    n_cams, B, n_pairs = len(sc["cams"]), len(mfs), len(sc["pairs"])
    sm, sc_ = (n_cams, 1) if layout[0] is None else layout
    bb = multigpu.block_layout(S.K)["total"]
    blocks = np.zeros((B * n_cams, bb), np.uint8)
    lm = np.full((B * n_cams, S.K), S.PAST_COUNT_ROW, np.int32)
    for m, mf in enumerate(mfs):
        for c in range(n_cams):
            blocks[m * sm + c * sc_] = mf["blocks"][c]
            lm[m * sm + c * sc_, :len(mf["ids"][c])] = mf["ids"][c]
    req, resp = tmp_path / "req.bin", tmp_path / "resp.bin"
    with open(req, "wb") as f:
        f.write(struct.pack("<12i", n_cams, S.W, S.H, S.K, 60, B, n_pairs, sm, sc_, len(sc["hp"]), mode, int(keyframe)))
        for cam in sc["cams"]:
            d = list(cam.d) + [0.0] * (8 - len(cam.d))
            f.write(struct.pack("<2i12d", cam.dist_type, 0, cam.fu, cam.fv, cam.cu, cam.cv, *d))
        f.write(np.asarray(sc["pairs"], np.int32).tobytes())
        f.write(np.ascontiguousarray(sc["hp"], np.float64).tobytes() + np.ascontiguousarray(sc["initialised"], np.uint8).tobytes())
        for mf in mfs:
            for c in range(n_cams):
                f.write(np.asarray(mf["T_WC"][c][0], np.float64).tobytes() + np.asarray(mf["T_WC"][c][1], np.float64).tobytes())
        f.write(struct.pack("<i", bb) + blocks.tobytes() + lm.tobytes())
        if keyframe:
            f.write(bytes(1 if mf["keyframe"] else 0 for mf in mfs))
        if mode == 0:
            f.write(matches.tobytes())
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "okvis2_amd") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = subprocess.run([cli, str(req), str(resp)], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    buf = open(resp, "rb").read()
    rows = n_pairs * B * S.K
    got = dict(action=np.frombuffer(buf, np.uint8, rows, 0).reshape(n_pairs, B, S.K),
               lm=np.frombuffer(buf, np.int32, rows, rows).reshape(n_pairs, B, S.K),
               lm_out=np.frombuffer(buf, np.int32, B * n_cams * S.K, 5 * rows).reshape(B * n_cams, S.K))
    off = 5 * rows + 4 * B * n_cams * S.K
    got["counts"] = np.frombuffer(buf, np.int32, B * 4, off).reshape(B, 4)
    off += 16 * B
    if mode != 0:
        got["matches"] = np.frombuffer(buf, capi.STEREO_MATCH_DTYPE, rows, off).reshape(n_pairs, B, S.K)
        off += rows * capi.STEREO_MATCH_DTYPE.itemsize
    assert struct.unpack_from("<i", buf, off)[0] == 1 and off + 4 == len(buf)  # a surplus pose made the call throw
    return got, (sm, sc_)


def _check_cli(sc, mfs, got, strides, refs, what):
    FILL32 = int(np.frombuffer(b"\xf9" * 4, np.int32)[0])
    for m, (mf, ref) in enumerate(zip(mfs, refs)):
        assert got["counts"][m].tolist() == ref["counts"].tolist(), (what, m, got["counts"][m], ref["counts"])
        for c in range(len(sc["cams"])):
            b, n = m * strides[0] + c * strides[1], len(mf["kps"][c])
            assert np.array_equal(got["lm_out"][b, :n], ref["ids"][c]) and np.all(got["lm_out"][b, n:] == FILL32), (what, m, c)
        for p, (c0, _) in enumerate(sc["pairs"]):
            n = len(mf["kps"][c0])
            assert np.array_equal(got["action"][p, m, :n], ref["action"][p]), (what, m, p)
            assert np.array_equal(got["lm"][p, m, :n], ref["lm"][p]), (what, m, p)
            assert np.all(got["action"][p, m, n:] == 0xF9) and np.all(got["lm"][p, m, n:] == FILL32), (what, m, p)


def _with_blocks(mfs, rng=None):
    """the multiframes with host-packed gather blocks; rng: random descriptors and real back-projections are not needed
    by the bookkeeping, zeros do"""
    out = []
    for mf in mfs:
        blocks = [multigpu.pack_block_host(S.K, k, np.zeros((len(k), 48), np.uint8), np.zeros((len(k), 3)),
                                           np.zeros(len(k), np.uint8)) for k in mf["kps"]]
        out.append(dict(mf, blocks=blocks))
    return out


def test_cpp_mirror_insert(oracle, tmp_path):
    """matchStereoInsertBlocks on the rows of two scenes (three cameras with a not-keyframe; the entangled chains)"""
    for name in ("hilti-3", "shared-bad-failed-edge"):
        sc = _scene(oracle, True, name)
        refs, _ = S.reference(oracle, True, name)
        mfs = _with_blocks(sc["mfs"])
        matches = np.zeros((len(sc["pairs"]), len(mfs), S.K), dtype=capi.STEREO_MATCH_DTYPE)
        matches["k1"] = 3
        for m, mf in enumerate(mfs):
            for p, (c0, _) in enumerate(sc["pairs"]):
                matches[p, m, :len(mf["kps"][c0])] = mf["matches"][p]
        got, strides = _cli(tmp_path, sc, mfs, 0, matches)
        _check_cli(sc, mfs, got, strides, refs, name)
    # camera-major, without keyframe flags
    sc = _scene(oracle, True, "hilti-3")
    refs, _ = S.reference(oracle, True, "hilti-3", all_keyframes=True)
    mfs = _with_blocks(sc["mfs"])
    matches = np.zeros((len(sc["pairs"]), len(mfs), S.K), dtype=capi.STEREO_MATCH_DTYPE)
    for m, mf in enumerate(mfs):
        for p, (c0, _) in enumerate(sc["pairs"]):
            matches[p, m, :len(mf["kps"][c0])] = mf["matches"][p]
    got, strides = _cli(tmp_path, sc, mfs, 0, matches, keyframe=False, layout=(1, len(mfs)))
    _check_cli(sc, mfs, got, strides, refs, "camera-major")


def test_cpp_mirror_rig(oracle, tmp_path):
    """matchStereoRig: the matcher per pair, then the bookkeeping.  Blocks with real descriptors and back-projections:
    keypoints of two cameras at the projections of one point cloud, equal descriptors where they see the same point.
    The rows the CLI returns are the restatement's input; they must hold matches."""
    rng = np.random.default_rng(5)
    cams = [S.camera("dyadic")] * 2
    T_WC = [(S.I3.copy(), np.zeros(3)), (S.I3.copy(), np.array([0.125, 0.0, 0.0]))]
    hp = np.concatenate([S.junk_points(rng, S.L)])
    mfs = []
    for m in range(2):
        n = 120 + 20 * m
        P = np.stack([rng.uniform(-1.0, 1.0, n), rng.uniform(-0.6, 0.6, n), rng.uniform(3.0, 6.0, n)], axis=1)
        desc = rng.integers(0, 256, (n, 48), dtype=np.uint8)
        kps, blocks = [], []
        for c in range(2):
            xy = np.stack([256.0 * (P[:, 0] - 0.125 * c) / P[:, 2] + 160.0, 256.0 * P[:, 1] / P[:, 2] + 120.0], axis=1)
            k = S.keypoints(oracle, xy)
            bp, bpv = oracle.backproject_keypoints(cams[c], k)
            kps.append(k), blocks.append(multigpu.pack_block_host(S.K, k, desc, bp, bpv))
        mfs.append(dict(kps=kps, blocks=blocks, ids=[np.full(n, -1, np.int32)] * 2, T_WC=T_WC, keyframe=True))
    sc = dict(name="rig", cams=cams, hp=hp, initialised=np.zeros(S.L, np.uint8), pairs=[(0, 1)])
    for layout in ((2, 1), (1, 2)):  # one matcher launch per multiframe / one for both
        got, strides = _cli(tmp_path, sc, mfs, 1, layout=layout)
        oracle.set_reduction(True)
        refs = [SR.stereo_insert(oracle, True, hp, sc["initialised"], cams, sc["pairs"], S.K, mf["kps"], mf["ids"], T_WC,
                                 [got["matches"][0, m, :len(mf["kps"][0])]], True) for m, mf in enumerate(mfs)]
        assert all(int(r["counts"][0]) > 60 and int(r["counts"][3]) > 60 for r in refs), [r["counts"] for r in refs]
        _check_cli(sc, mfs, got, strides, refs, layout)


# ---- error paths: nothing is launched ---------------------------------------------------------------------------------
def _raw_call(fe, **kw):
    fn = capi.lib().okvfe_stereo_insert_blocks_device
    p = lambda v: None if v is None else ctypes.c_void_p(int(v))
    st = fn(fe._h, kw["table"], p(kw["init"]), p(kw["blocks"]), kw["sm"], kw["sc"], kw["n"], kw["n_cams"],
            capi._p(kw["pairs"]), kw["n_pairs"], capi._p(kw["cams"]), kw["T"], p(kw["matches"]), p(kw["lm"]), p(kw.get("kf")),
            kw["res"], None)
    return st, capi.lib().okvfe_last_error(fe._h).decode()


def test_bad_arguments_are_rejected_before_any_launch():
    INVALID, UNSUPPORTED, NOT_READY = 1, 4, 7
    fe = capi.Frontend(S.W, S.H, 10.0, 0, 50, S.K, match_threshold=60, num_cameras=3)
    try:
        for c in range(2):  # slot 2 stays without intrinsics
            fe.set_camera(c, S.camera("dyadic"))
        bb = fe.gather_block_bytes()
        FILL = 0x5A
        d_any = torch.full((4 * bb + 4 * S.K * 64,), FILL, dtype=torch.uint8, device="cuda")
        ptr = d_any.data_ptr()
        P = (capi.Pose * 8)(*[capi.make_pose(S.I3, np.zeros(3)) for _ in range(8)])
        tab = capi.Frontend.make_landmark_table_device(10, 0, 0, ptr, 0, 0, 0, 0, 0, 0)
        tab0 = capi.Frontend.make_landmark_table_device(0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
        res = capi.StereoInsertDevice(ptr, ptr, ptr, ptr)
        i32 = lambda *v: np.array(v, np.int32)
        good = dict(table=ctypes.byref(tab), init=ptr, blocks=ptr, sm=2, sc=1, n=2, n_cams=2, pairs=i32(0, 1), n_pairs=1,
                    cams=i32(0, 1), T=P, matches=ptr, lm=ptr, kf=ptr, res=ctypes.byref(res))
        neg = capi.Frontend.make_landmark_table_device(-1, 0, 0, ptr, 0, 0, 0, 0, 0, 0)
        nohp = capi.Frontend.make_landmark_table_device(10, 0, 0, 0, 0, 0, 0, 0, 0, 0)
        cases = [
            (dict(table=None), INVALID, ()), (dict(table=ctypes.byref(neg)), INVALID, ()),
            (dict(table=ctypes.byref(nohp)), INVALID, ()), (dict(init=None), INVALID, ()),
            (dict(blocks=None), INVALID, ()), (dict(pairs=None), INVALID, ()), (dict(cams=None), INVALID, ()),
            (dict(T=None), INVALID, ()), (dict(matches=None), INVALID, ()), (dict(lm=None), INVALID, ()),
            (dict(res=None), INVALID, ()),
            (dict(res=ctypes.byref(capi.StereoInsertDevice(ptr, ptr, None, ptr))), INVALID, ()),
            (dict(res=ctypes.byref(capi.StereoInsertDevice(ptr, ptr, ptr, None))), INVALID, ()),
            (dict(n=-1), INVALID, ()), (dict(n_cams=0), INVALID, ()), (dict(n_pairs=0), INVALID, ()),
            (dict(n_pairs=capi.STEREO_MAX_PAIRS + 1, pairs=i32(*([0, 1] * 17))), INVALID, ()),
            (dict(sm=-2), INVALID, ()), (dict(sc=-1), INVALID, ()),
            (dict(pairs=i32(1, 1)), INVALID, ("pair 0", "(1, 1)")),
            (dict(pairs=i32(0, 1, 0, 2), n_pairs=2), INVALID, ("pair 1", "(0, 2)")),
            (dict(pairs=i32(-1, 1)), INVALID, ("pair 0",)),
            (dict(sm=1, sc=1), INVALID, ("block 1",)), (dict(sm=0, sc=1), INVALID, ("block 0",)),
            (dict(sm=2, sc=2), INVALID, ("block 2",)),
            (dict(n_cams=3, cams=i32(0, 1, 2), sm=3), NOT_READY, ("camera 2", "slot 2", "no intrinsics")),
            (dict(cams=i32(0, 5)), NOT_READY, ("camera 1", "slot 5")),
        ]
        for change, status, words in cases:
            st, msg = _raw_call(fe, **dict(good, **change))
            assert st == status, (list(change), st, msg)
            for w in words:
                assert w in msg, (w, msg)
        # n_multiframes == 0 is fine and launches nothing; so is a table without rows and without flags
        st, msg = _raw_call(fe, **dict(good, n=0))
        assert st == 0, msg
        st, msg = _raw_call(fe, **dict(good, n=0, table=ctypes.byref(tab0), init=None))
        assert st == 0, msg
        torch.cuda.synchronize()
        assert bool((d_any == FILL).all())
    finally:
        fe.close()
    # a rig whose ids and tables do not fit the work-group's LDS
    big = capi.Frontend(64, 64, 10.0, 0, 50, 2500, match_threshold=60, num_cameras=2)
    try:
        for c in range(2):
            big.set_camera(c, dataclasses.replace(S.camera("dyadic"), w=64, h=64))
        d = torch.zeros(64, dtype=torch.uint8, device="cuda")
        res = capi.StereoInsertDevice(None, None, d.data_ptr(), d.data_ptr())
        st, msg = _raw_call(big, **dict(good, table=ctypes.byref(tab0), init=None, blocks=d.data_ptr(), matches=d.data_ptr(),
                                        lm=d.data_ptr(), kf=None, res=ctypes.byref(res)))
        assert st == UNSUPPORTED and "115536" in msg and "65280" in msg and "LDS" in msg, (st, msg)
    finally:
        big.close()
