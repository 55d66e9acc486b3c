"""GPU: the host-buffer matchers of the C++ mirror (okvfe::HipFrontend::matchStereo, matchMotionStereo, matchToMap,
matchToMapPooled, matchToMapUninitialised, verifyRecognisedPlace) on a real context, through
tests/cpp/host_matchers_cli.cpp (built from okvfe_camera_ext cameras, FrameData filled from arrays), on the scenes of
tests/cpp_matcher_scenes.py.  Every returned container is compared byte for byte (doubles as uint64) with
 - the Python binding's call of the same C entry point on the same arrays, and
 - the CPU oracle wherever it carries the camera model (not RADTAN8, as in test_gpu_gate_census.py);
the second-pass rows of the wrapper also with okvfe_match_to_map_table_uninitialised_blocks_device (what
matchToMapUninitialisedBlocks calls) on the same frame packed as a gather block.  Each test is one run of the program."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cpp_matcher_scenes as S
import gpu_common as G
import map_table_common as M
import map_table_uninit_common as U
from okvis2_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.join(ROOT, "okvis2_amd")
STEREO, MOTION, MAP, POOLED, UNINIT, PLACE = range(6)
K = 700


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    exe = tmp_path_factory.mktemp("host_matchers") / "host_matchers_cli"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "host_matchers_cli.cpp"), "-L" + LIB_DIR, "-lokvfe",
                           "-Wl,-rpath," + LIB_DIR, "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


@pytest.fixture(scope="module")
def fe():
    f = G.make_frontend(synth.euroc_config())
    assert f.max_keypoints >= K
    yield f
    f.close()


# ---- the request ---------------------------------------------------------------------------------------
def _i(*v):
    return struct.pack("<%di" % len(v), *v)


def _d(*v):
    return struct.pack("<%dd" % len(v), *v)


def _pose(T):
    return np.concatenate([np.asarray(T[0], dtype=np.float64).reshape(-1), np.asarray(T[1], dtype=np.float64)]).tobytes()


def _frame(kps, desc, bp, bv):
    n = len(kps)
    assert kps.dtype.itemsize == 28 and len(desc) == n and len(bp) == n and len(bv) == n
    return (_i(n) + np.ascontiguousarray(kps).tobytes() + np.ascontiguousarray(desc, dtype=np.uint8).tobytes() +
            np.ascontiguousarray(bp, dtype=np.float64).tobytes() + np.ascontiguousarray(bv, dtype=np.uint8).tobytes())


def _vec(a, dtype):
    a = np.zeros(0, dtype) if a is None else np.ascontiguousarray(a, dtype=dtype).reshape(-1)
    return _i(len(a)) + a.tobytes()


def _head(fr, n):
    return tuple(a[:n] for a in fr)


def _run(cli, tmp_path, cams, ops):
    req, resp = tmp_path / "req.bin", tmp_path / "resp.bin"
    with open(req, "wb") as f:
        f.write(_i(len(cams)))
        for cam in cams:
            f.write(_i(cam.w, cam.h, cam.dist_type) + _d(cam.fu, cam.fv, cam.cu, cam.cv, *(list(cam.d) + [0.0] * 8)[:8]))
        f.write(_i(K, S.THRESHOLD, len(ops)) + b"".join(ops))
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = LIB_DIR + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = subprocess.run([cli, str(req), str(resp)], env=env, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    return Reader(open(resp, "rb").read())


class Reader:
    def __init__(self, raw):
        self.raw, self.at = raw, 0

    def take(self, dtype, n, shape=None):
        size = np.dtype(dtype).itemsize * n
        assert self.at + size <= len(self.raw), "the response is shorter than the request implies"
        a = np.frombuffer(self.raw, dtype=dtype, count=n, offset=self.at)
        self.at += size
        return a if shape is None else a.reshape(shape)

    def done(self):
        assert self.at == len(self.raw), "the response is longer than the request implies"


def _same_rows(got, want, what):
    """whole records, byte for byte"""
    assert got.dtype == want.dtype and len(got) == len(want), what
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), \
        (what, [f for f in got.dtype.names if not np.array_equal(got[f], want[f])])


def _motion_ops(sc, cam_index):
    f0, f1 = sc["f0"], sc["f1"]
    head = _i(MOTION, cam_index)
    tail = _pose(sc["T0"]) + _pose(sc["T1"])
    return [head + _frame(*f0) + _frame(*f1) + tail + _vec(sc["skip0"], np.uint8) + _vec(sc["matched1"], np.uint8),
            head + _frame(*f0) + _frame(*f1) + tail + _vec(None, np.uint8) + _vec(None, np.uint8),
            head + _frame(*f0) + _frame(*_head(f1, 0)) + tail + _vec(sc["skip0"], np.uint8) + _vec(None, np.uint8),
            head + _frame(*_head(f0, 0)) + _frame(*f1) + tail + _vec(None, np.uint8) + _vec(sc["matched1"], np.uint8)]


def _binding_motion(fe, sc, f0, f1, s0, m1):
    (kp0, d0, bp0, bv0), (kp1, d1, bp1, bv1) = f0, f1
    return fe.match_motion_stereo(sc["cam"], d0, kp0, bp0, bv0, s0, d1, kp1, bp1, bv1, m1, sc["T0"], sc["T1"])


def _check_motion(fe, sc, r, with_oracle):
    n = S.MOTION_N
    f0, f1 = sc["f0"], sc["f1"]
    for with_flags in (True, False):
        got = r.take(capi.MOTION_MATCH_DTYPE, n)
        s0, m1 = (sc["skip0"], sc["matched1"]) if with_flags else (None, None)
        _same_rows(got, _binding_motion(fe, sc, f0, f1, s0, m1), ("motion", with_flags, "binding"))
        if with_oracle:
            ref = S.motion_reference(sc, with_flags)
            for f in ("k1", "dist", "initialisable", "accepted"):
                assert np.array_equal(got[f], ref[f]), ("motion", with_flags, f)
            assert np.array_equal(got["hp_W"].view(np.uint64), ref["hp_W"].view(np.uint64)), ("motion", with_flags)
            assert (ref["k1"] >= 0).sum() >= S.MIN_MOTION_MATCHED and ref["accepted"].sum() >= S.MIN_MOTION_ACCEPTED
        else:
            assert (got["k1"] >= 0).sum() >= S.MIN_MOTION_MATCHED // 2  # (the scene is not degenerate through this camera)
    got = r.take(capi.MOTION_MATCH_DTYPE, n)  # empty current frame
    _same_rows(got, _binding_motion(fe, sc, f0, _head(f1, 0), sc["skip0"], None), ("motion", "empty current frame"))
    assert np.all(got["k1"] == -1)
    # (empty older frame: no rows)


def test_motion_stereo_and_stereo(oracle, cli, fe, tmp_path):
    """matchMotionStereo at 130 keypoints per side with both optional vectors, with none, with an empty current and an
    empty older frame; matchStereo on the same frames between the two cameras of the rig (context of im0, focal lengths
    of im0 and im1)"""
    sc = S.motion_scene()
    cam = sc["cam"]
    other = synth.euroc_config().cams[1]
    (kp0, d0, bp0, bv0), (kp1, d1, bp1, bv1) = sc["f0"], sc["f1"]
    stereo = _i(STEREO, 0, 1) + _frame(*sc["f0"]) + _frame(*sc["f1"]) + _pose(sc["T0"]) + _pose(sc["T1"])
    r = _run(cli, tmp_path, [cam, other], _motion_ops(sc, 0) + [stereo])
    _check_motion(fe, sc, r, True)
    got = r.take(capi.STEREO_MATCH_DTYPE, S.MOTION_N)
    r.done()
    fa, fb = 0.5 * (cam.fu + cam.fv), 0.5 * (other.fu + other.fv)
    assert fa != fb
    _same_rows(got, fe.match_stereo(d0, kp0, bp0, bv0, d1, kp1, bp1, bv1, sc["T0"], sc["T1"], fa, fb), "matchStereo, binding")
    ref = oracle.match_stereo(d0, kp0, bp0, bv0, d1, kp1, bp1, bv1, sc["T0"], sc["T1"], fa, fb, S.THRESHOLD)
    assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)) and (ref["k1"] >= 0).sum() >= 32


def test_motion_stereo_radtan8(oracle, cli, fe, tmp_path):
    """the motion scene through the RADTAN8 camera, as camera 1 of a rig whose camera 0 is the EuRoC one"""
    sc = S.motion_scene(radtan8=True)
    cam = sc["cam"]
    assert cam.dist_type == capi.DIST_RADTAN8
    r = _run(cli, tmp_path, [synth.euroc_config().cams[0], cam], _motion_ops(sc, 1))
    _check_motion(fe, sc, r, False)  # (the binding's call takes the camera as an argument, like the wrapper's)
    r.done()


def _table_bytes(m):
    a = M.table_arrays(m)
    return (_i(len(a["hp"]), len(a["obs_pose"]), len(a["poses"])) +
            b"".join(a[k].tobytes() for k in ("hp", "quality", "obs_begin", "obs_pose", "obs_desc", "obs_bp", "poses")))


def test_match_to_map_first_pass_and_pooled(oracle, cli, fe, tmp_path):
    """matchToMap from the raw table as the first call on its camera (it sets the camera itself), with poolOut and
    `use`; then with `use` empty; the packed 3-D set through matchToMapPooled; an empty frame through both"""
    sc = S.map_scene()
    m, kps, desc, use = sc["m"], sc["kps"], sc["desc"], sc["use"]
    n, nl = len(kps), len(m["hp"])
    fr = (kps, desc, sc["bp"], sc["bpv"])
    ops = []
    for exclusive, thr in S.MAP_MODES:
        f = sc["first"][exclusive]
        common = _table_bytes(m) + _pose(m["T1"]) + _d(thr) + _i(int(exclusive))
        ops += [_i(MAP, 0) + _frame(*fr) + common + _vec(use, np.uint8) + _i(1),
                _i(MAP, 0) + _frame(*fr) + common + _vec(None, np.uint8) + _i(0),
                _i(POOLED, 0) + _frame(*fr) + _vec(use, np.uint8) + _vec(f["proj"], np.float64) + _vec(f["begin"], np.int32) +
                _vec(f["rows"], np.uint8) + _d(thr),
                _i(MAP, 0) + _frame(*_head(fr, 0)) + common + _vec(None, np.uint8) + _i(0),
                _i(POOLED, 0) + _frame(*_head(fr, 0)) + _vec(None, np.uint8) + _vec(f["proj"], np.float64) +
                _vec(f["begin"], np.int32) + _vec(f["rows"], np.uint8) + _d(thr)]
    r = _run(cli, tmp_path, [m["cam"]], ops)
    fe.set_camera(0, m["cam"])
    args = (m["hp"], m["quality"], m["obs_begin"], m["obs_pose"], m["obs_desc"], m["obs_bp"], m["poses"], m["T1"])
    for exclusive, thr in S.MAP_MODES:
        f, what = sc["first"][exclusive], ("exclusive" if exclusive else "non-exclusive",)
        ref = f["ref"]
        lm, bd = r.take(np.int32, n), r.take(np.int32, n)
        pool = dict(status=r.take(np.int32, nl), n_desc=r.take(np.int32, nl), obs_rows=r.take(np.int32, nl * 3, (nl, 3)),
                    projection=r.take(np.float64, nl * 2, (nl, 2)), e_W=r.take(np.float64, nl * 6, (nl, 2, 3)),
                    r_W=r.take(np.float64, nl * 6, (nl, 2, 3)))
        blm, bbd, bpool = fe.match_to_map_landmarks(0, *args, thr, exclusive, desc, kps, use)
        assert np.array_equal(lm, blm) and np.array_equal(bd, bbd), what
        for k in ("status", "n_desc", "obs_rows"):
            assert np.array_equal(pool[k], bpool[k]) and np.array_equal(pool[k], ref[k]), what + (k,)
        for k in ("projection", "e_W", "r_W"):
            assert np.array_equal(pool[k].view(np.uint64), bpool[k].view(np.uint64)), what + (k, "binding")
            assert np.array_equal(pool[k].view(np.uint64), ref[k].view(np.uint64)), what + (k, "oracle")
        for s in (0, 1, 2):
            assert (ref["status"] == s).sum() >= S.MIN_PER_STATUS
        rl, rd = oracle.match_to_map(desc, kps, use, f["proj"], f["begin"], f["rows"], thr, S.THRESHOLD)
        assert np.array_equal(lm, np.where(rl >= 0, f["idx"][np.maximum(rl, 0)], -1)) and np.array_equal(bd, rd), what
        assert (rl >= 0).sum() >= S.MIN_FIRST_PASS_MATCHED
        # `use` empty = every keypoint
        lm, bd = r.take(np.int32, n), r.take(np.int32, n)
        every = np.ones(n, np.uint8)
        blm, bbd, _ = fe.match_to_map_landmarks(0, *args, thr, exclusive, desc, kps, every)
        al, ad = oracle.match_to_map(desc, kps, every, f["proj"], f["begin"], f["rows"], thr, S.THRESHOLD)
        assert np.array_equal(lm, blm) and np.array_equal(bd, bbd), what + ("use empty",)
        assert np.array_equal(lm, np.where(al >= 0, f["idx"][np.maximum(al, 0)], -1)) and np.array_equal(bd, ad), what
        assert not np.array_equal(al, rl)
        # the packed set
        lm, bd = r.take(np.int32, n), r.take(np.int32, n)
        blm, bbd = fe.match_to_map(desc, kps, use, f["proj"], f["begin"], f["rows"], thr)
        assert np.array_equal(lm, blm) and np.array_equal(bd, bbd), what + ("pooled", "binding")
        assert np.array_equal(lm, rl) and np.array_equal(bd, rd), what + ("pooled", "oracle")
        # an empty frame: no rows from either
    r.done()


def test_match_to_map_second_pass(oracle, cli, fe, tmp_path):
    """matchToMapUninitialised on the status-2 set of the first pass, backProjectionsValid cleared at every third
    keypoint: `use` and previousLandmark empty and given.  A keypoint takes part iff use AND backProjectionsValid."""
    sc = S.map_scene()
    m, kps, desc = sc["m"], sc["kps"], sc["desc"]
    n = len(kps)
    fr = (kps, desc, sc["bp"], sc["bpv"])
    variants = [(u, p) for u in (False, True) for p in (False, True)]
    tail = _vec(sc["begin2"], np.int32) + _vec(sc["rows2"], np.uint8) + _vec(sc["e0"], np.float64) + \
        _vec(sc["r0"], np.float64) + _pose(m["T1"])
    ops = [_i(UNINIT, 0) + _frame(*fr) + _vec(sc["use"] if u else None, np.uint8) +
           _vec(sc["previous"] if p else None, np.int32) + tail for u, p in variants]
    ops.append(_i(UNINIT, 0) + _frame(*_head(fr, 0)) + _vec(None, np.uint8) + _vec(None, np.int32) + tail)
    r = _run(cli, tmp_path, [m["cam"]], ops)
    got = {}
    for v in variants:
        got[v] = (r.take(np.int32, n), r.take(np.int32, n), r.take(np.float64, n * 4, (n, 4)), r.take(np.uint8, n),
                  int(r.take(np.int32, 1)[0]))
    assert int(r.take(np.int32, 1)[0]) == 0  # the empty frame: no rows, nothing already matched
    r.done()
    nobody = np.full(n, -1, np.int32)
    for (u, p), g in got.items():
        what = ("use given" if u else "use empty", "previous given" if p else "previous empty")
        use = (sc["use"] if u else np.ones(n, np.uint8)) & sc["bpv"]
        b = fe.match_to_map_uninitialised(desc, sc["bp"], use, sc["previous"] if p else nobody, sc["begin2"], sc["rows2"],
                                          sc["e0"], sc["r0"], m["T1"], sc["focal"])
        ref = S.second_pass_reference(sc, u, p)
        for name, other in (("binding", b), ("oracle", ref)):
            assert np.array_equal(g[0], other[0]), what + (name, "landmark", np.flatnonzero(g[0] != other[0])[:8])
            assert np.array_equal(g[1], other[1]), what + (name, "distance")
            assert np.array_equal(g[3], other[3]), what + (name, "hpSet")
            assert np.array_equal(g[2].view(np.uint64), np.ascontiguousarray(other[2]).view(np.uint64)), what + (name, "hp_W")
            assert g[4] == other[4], what + (name, "alreadyMatched")
        assert ((ref[0] >= 0) & (ref[3] != 0)).sum() >= S.MIN_SECOND_PASS_HP_SET
        old = S.second_pass_reference(sc, u, p, with_bpv=False)
        assert ((ref[0] != old[0]) | (ref[1] != old[1]) | (ref[3] != old[3])).sum() >= S.MIN_ROWS_DEPENDING_ON_BPV
    assert got[True, True][4] >= 1
    # the device-resident form on the same frame as a gather block: both passes, previous absent
    fe.set_camera(0, m["cam"])
    tab = M.DeviceTable(fe, m)
    for u in (False, True):
        frame = dict(kps=kps, desc=desc, bp=sc["bp"], bv=sc["bpv"], use=sc["use"], previous=nobody)
        T = U.prepare(fe, tab.n_landmarks, [frame])
        U.launch_first(fe, tab, T, [m["T1"]], [0], S.MAP_MODES[0][1], False, with_use=u)
        U.launch_second(fe, tab, T, [m["T1"]], [0], False, with_use=u, previous=None)
        blocks = U.collect(T)
        g = got[u, False]
        lm = np.where(g[0] >= 0, sc["idx2"][np.maximum(g[0], 0)], -1)  # (packed index -> table row)
        assert np.array_equal(blocks["lm2"][0, :n], lm) and np.array_equal(blocks["bd2"][0, :n], g[1]), ("blocks", u)
        assert np.array_equal(blocks["hs"][0, :n], g[3]) and int(blocks["ctr"][0]) == g[4], ("blocks", u)
        set_ = g[3] != 0
        assert np.array_equal(blocks["hp"][0, :n][set_].view(np.uint64), g[2][set_].view(np.uint64)), ("blocks", u, "hp_W")


def test_verify_recognised_place(oracle, cli, fe, tmp_path):
    """verifyRecognisedPlace: 40 landmarks of 1 to 4 descriptors against 130 frame descriptors; zero landmarks; an
    empty frame"""
    p = S.place_scene()
    nl, n = len(p["begin"]) - 1, len(p["frame"])
    kps = np.zeros(n, dtype=oracle.KEYPOINT_DTYPE)
    kps["size"] = 12.0
    fr = (kps, p["frame"], np.zeros((n, 3)), np.ones(n, np.uint8))
    ops = [_i(PLACE, 0) + _vec(p["pool"], np.uint8) + _vec(p["begin"], np.int32) + _frame(*fr),
           _i(PLACE, 0) + _vec(None, np.uint8) + _vec(np.zeros(1, np.int32), np.int32) + _frame(*fr),
           _i(PLACE, 0) + _vec(p["pool"], np.uint8) + _vec(p["begin"], np.int32) + _frame(*_head(fr, 0))]
    r = _run(cli, tmp_path, [synth.euroc_config().cams[0]], ops)
    k_min, d_min = r.take(np.int32, nl), r.take(np.uint32, nl)
    k_none, d_none = r.take(np.int32, nl), r.take(np.uint32, nl)  # (zero landmarks wrote nothing in between)
    r.done()
    bk, bd = fe.verify_place_match(p["pool"], p["begin"], p["frame"])
    rk, rd = oracle.verify_place(p["pool"], p["begin"], p["frame"], S.THRESHOLD)
    assert np.array_equal(k_min, bk) and np.array_equal(d_min, bd) and d_min.dtype == bd.dtype
    assert np.array_equal(k_min, rk) and np.array_equal(d_min, rd)
    assert (rd < S.THRESHOLD).sum() >= S.MIN_PLACE_BELOW_THRESHOLD
    ek, ed = fe.verify_place_match(p["pool"], p["begin"], p["frame"][:0])
    assert np.array_equal(k_none, ek) and np.array_equal(d_none, ed) and np.all(d_none == S.THRESHOLD)
