"""GPU: every scene of gate_scenes.py -- every branch of the FP64 gate chain the oracle's census can
reach, the knife edges of the gates, and the edges of the map matcher's float bounding-box
prefilter -- through every form of its matcher, byte for byte against the oracle, under both orders
of the 3-term FP64 sums.

 stereo   okvfe_match_stereo, okvfe_match_stereo_batch_device (the scene written into the context's
          own result arrays), okvfe_match_stereo_blocks_device, okvfe_match_stereo_blocks_batch_device
 motion   okvfe_match_motion_stereo (okvfe_match_motion_stereo_ext for the radtan8 scene),
          okvfe_match_motion_stereo_blocks_device
 map      okvfe_match_to_map, okvfe_match_to_map_landmarks, okvfe_match_to_map_blocks_device,
          okvfe_match_to_map_uninitialised, okvfe_match_to_map_uninitialised_blocks_device

FP64 outputs are compared as uint64.  Where the oracle's row is NaN the device's row must be NaN in
the same places (the payload of a NaN is not part of the contract); everything else is bytes.

What the module pins in match_to_map_kernel: it discards 64-landmark chunks by a float bounding box of the
wave's keypoints.  Reduced with fminf / fmaxf, which drop a NaN lane, and tested against a landmark's projection
coordinate by coordinate, that box loses every landmark outside the finite neighbours of a keypoint with a NaN
coordinate, and every projection with ONE NaN coordinate, where the reference's "!(dd > thr)" admits both
(test_match_to_map_prefilter_scene_both_forms[outliers-*, wildproj-*],
test_match_to_map_blocks_on_both_sides_of_the_region_order_limit).
"""
import ctypes
import functools
import math

import numpy as np
import pytest

import gate_scenes as S
from okvis2_amd import capi, multigpu

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp64_order")]
torch = pytest.importorskip("torch")

K = 2048  # row capacity of every context here: scenes stay <= 2048 keypoints


_FRONTENDS = {}


def _frontend(w, h, layers):
    """single-layer context (layers = 1: every keypoint of size 12) or a scale space of 4 layers, whose
    device forms read the size class of a keypoint from its octave; one per image size, shared by the module"""
    key = (w, h, layers)
    if key not in _FRONTENDS:
        if layers == 1:
            _FRONTENDS[key] = capi.Frontend(w, h, 38.0, 0, 150, K, match_threshold=S.THRESHOLD, max_batch=2)
        else:
            _FRONTENDS[key] = capi.Frontend(w, h, 38.0, 2, 150, K // 4, match_threshold=S.THRESHOLD, max_batch=2)
    return _FRONTENDS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_frontends():
    yield
    while _FRONTENDS:
        _FRONTENDS.popitem()[1].close()


def _fe(sc, device_form):
    cam = sc["cam"]
    fe = _frontend(cam.w, cam.h, 4 if (device_form and sc.get("mixed")) else 1)
    assert fe.max_keypoints == K
    return fe


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows(a):
    """a, or one zero row where a has none: a pooled set without descriptors still passes a pointer"""
    return a if len(a) else np.zeros((1,) + a.shape[1:], dtype=a.dtype)


@functools.lru_cache(maxsize=None)
def _hip():
    """the HIP runtime this process already runs on (the one libokvfe.so and torch share)"""
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    return ctypes.CDLL(path)


def _upload(dst, arr, capacity_bytes):
    a = np.ascontiguousarray(arr)
    assert a.nbytes <= capacity_bytes
    if a.nbytes:
        st = _hip().hipMemcpy(ctypes.c_void_p(dst), ctypes.c_void_p(a.ctypes.data), ctypes.c_size_t(a.nbytes),
                              ctypes.c_int(1))
        assert st == 0, st


def _same_f64(got, ref, what):
    got, ref = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(ref, dtype=np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN rows differ", np.argwhere(np.isnan(got) != nan)[:5])
    same = got.view(np.uint64) == ref.view(np.uint64)
    assert np.all(same | nan), (what, np.argwhere(~(same | nan))[:5])


def _same_stereo(got, ref, what):
    assert len(got) == len(ref), what
    for f in ("k1", "dist", "initialisable", "pad"):
        assert np.array_equal(got[f], ref[f]), (what, f, np.flatnonzero(got[f] != ref[f])[:8])
    _same_f64(got["hp_W"], ref["hp_W"], what)


def _same_motion(got, ref, what, sc=None):
    assert len(got) == len(ref), what
    for f in ("k1", "dist", "initialisable", "accepted"):
        if f == "accepted" and sc is not None and "oracle_cam" in sc:
            # the oracle does not carry the 8-coefficient model: the 4 px verdict against its restatement
            want = S.radtan8_accepted(sc, got)
            sure = want >= 0
            assert np.array_equal(got[f][sure], want[sure]), (what, f)
            assert (want == 1).sum() > 20 and sure.sum() >= len(want) - 2, what
            continue
        assert np.array_equal(got[f], ref[f]), (what, f, np.flatnonzero(got[f] != ref[f])[:8])
    _same_f64(got["hp_W"], ref["hp_W"], what)
    hit = ref["k1"] >= 0
    # the reference stores acos(cos_quality); the host adaptor takes the acos (libm, as the C++ host does)
    q = np.array([math.acos(c) if abs(c) <= 1.0 else math.nan for c in got["cos_quality"][hit]])
    _same_f64(q, ref["quality"][hit], what + " quality")


def _block(sc, side):
    return multigpu.pack_block_host(K, sc["kp" + side], sc["d" + side], sc["bp" + side], sc["bv" + side])


def _head(sc, n):
    """the scene with image 0 cut to its first n keypoints"""
    out = dict(sc)
    for k in ("d0", "kp0", "bp0", "bv0", "skip0"):
        out[k] = sc[k][:n]
    return out


def _check_stereo_all_forms(oracle, sc):
    ref = S.run_pair(oracle, sc, False)
    n0 = len(sc["kp0"])
    args = (sc["T0"], sc["T1"], sc["f0"], sc["f1"])
    # 1. host buffers
    fe = _fe(sc, False)
    got = fe.match_stereo(sc["d0"], sc["kp0"], sc["bp0"], sc["bv0"], sc["d1"], sc["kp1"], sc["bp1"], sc["bv1"], *args)
    _same_stereo(got, ref, sc["name"] + " host")
    if n0 == 0:
        return
    fe = _fe(sc, True)
    rec = capi.STEREO_MATCH_DTYPE.itemsize
    # 2. gather blocks, one pair
    b0, b1 = _dev(_block(sc, "0")), _dev(_block(sc, "1"))
    d_out = torch.zeros((K, rec), dtype=torch.uint8, device="cuda")
    fe.match_stereo_blocks_device(b0.data_ptr(), b1.data_ptr(), *args, d_out.data_ptr())
    torch.cuda.synchronize()
    _same_stereo(d_out.cpu().numpy().view(capi.STEREO_MATCH_DTYPE).reshape(-1)[:n0], ref, sc["name"] + " blocks")
    # 3. gather blocks, a batch of two frames: the scene, and the scene with half of image 0
    half = _head(sc, n0 // 2)
    bb0 = _dev(np.stack([_block(sc, "0"), _block(half, "0")]))
    bb1 = _dev(np.stack([_block(sc, "1"), _block(sc, "1")]))
    d_out2 = torch.zeros((2, K, rec), dtype=torch.uint8, device="cuda")
    fe.match_stereo_blocks_batch_device(bb0.data_ptr(), bb1.data_ptr(), 2, *args, d_out2.data_ptr())
    torch.cuda.synchronize()
    rows = d_out2.cpu().numpy().view(capi.STEREO_MATCH_DTYPE).reshape(2, K)
    _same_stereo(rows[0, :n0], ref, sc["name"] + " blocks batch 0")
    _same_stereo(rows[1, :n0 // 2], S.run_pair(oracle, half, False), sc["name"] + " blocks batch 1")
    # 4. the context's own result arrays (what detect + describe leaves behind), images 0 and 1
    out = fe.device_outputs()
    assert out.max_keypoints == K
    for img, side in ((0, "0"), (1, "1")):
        n = len(sc["kp" + side])
        _upload(out.keypoints + img * K * 28, sc["kp" + side], K * 28)
        _upload(out.descriptors + img * K * 48, sc["d" + side], K * 48)
        _upload(out.backproj + img * K * 24, sc["bp" + side], K * 24)
        _upload(out.backproj_valid + img * K, sc["bv" + side], K)
        _upload(out.counts + img * 4, np.array([n], dtype=np.int32), 4)
    sp = capi.StereoPair()
    sp.image0, sp.image1 = 0, 1
    sp.T_WC0, sp.T_WC1 = capi.make_pose(*sc["T0"]), capi.make_pose(*sc["T1"])
    sp.f0, sp.f1 = sc["f0"], sc["f1"]
    d_out3 = torch.zeros((1, K, rec), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fe.match_stereo_batch_device([sp], d_out3.data_ptr())
    torch.cuda.synchronize()
    _same_stereo(d_out3.cpu().numpy().view(capi.STEREO_MATCH_DTYPE).reshape(-1)[:n0], ref, sc["name"] + " batch")


def _check_motion_all_forms(oracle, sc):
    cam = sc["cam"]
    n0 = len(sc["kp0"])
    fe = _fe(sc, False)
    for s0, m1 in ((sc["skip0"], sc["matched1"]), (None, None)):
        flagged = dict(sc, skip0=s0, matched1=m1)
        ref = S.run_pair(oracle, flagged, True)
        got = fe.match_motion_stereo(cam, sc["d0"], sc["kp0"], sc["bp0"], sc["bv0"], s0, sc["d1"], sc["kp1"],
                                     sc["bp1"], sc["bv1"], m1, sc["T0"], sc["T1"])
        _same_motion(got, ref, sc["name"] + " host", sc)
    if n0 == 0:
        return
    fe = _fe(sc, True)
    fe.set_camera(0, cam)
    b0, b1 = _dev(_block(sc, "0")), _dev(_block(sc, "1"))
    pad = lambda a: _dev(np.concatenate([a, np.zeros(K - len(a), np.uint8)]))
    d_s0, d_m1 = pad(sc["skip0"]), pad(sc["matched1"])
    d_out = torch.zeros((K, capi.MOTION_MATCH_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    for s0, m1, ps0, pm1 in ((sc["skip0"], sc["matched1"], d_s0.data_ptr(), d_m1.data_ptr()), (None, None, None, None)):
        ref = S.run_pair(oracle, dict(sc, skip0=s0, matched1=m1), True)
        fe.match_motion_stereo_blocks_device(0, b0.data_ptr(), b1.data_ptr(), ps0, pm1, sc["T0"], sc["T1"],
                                             d_out.data_ptr())
        torch.cuda.synchronize()
        _same_motion(d_out.cpu().numpy().view(capi.MOTION_MATCH_DTYPE).reshape(-1)[:n0], ref, sc["name"] + " blocks",
                     sc)


@pytest.mark.parametrize("spec", S.PAIR_SPECS, ids=S.spec_id)
def test_stereo_scene_every_form(oracle, spec):
    _check_stereo_all_forms(oracle, S.pair_scene(spec[0], spec[1], spec[2], **spec[3]))


@pytest.mark.parametrize("spec", S.PAIR_SPECS, ids=S.spec_id)
def test_motion_stereo_scene_every_form(oracle, spec):
    _check_motion_all_forms(oracle, S.pair_scene(spec[0], spec[1], spec[2], **spec[3]))


@pytest.mark.parametrize("gate", S.KNIFE_GATES)
def test_knife_edge_both_sides(oracle, gate):
    """bisected here, after fp64_order has set the order: the edge moves with it"""
    scenes, motion, (lo, hi), calls = S.knife_edge(oracle, gate)
    print(f"\n{gate}: {lo!r} | {hi!r} after {calls} oracle calls")
    verdicts = []
    for sc in scenes:
        ref = S.run_pair(oracle, sc, motion)
        verdicts.append((int((ref["k1"] >= 0).sum()), int(ref["initialisable"].sum()),
                         int(ref["accepted"].sum()) if motion else 0))
        (_check_motion_all_forms if motion else _check_stereo_all_forms)(oracle, sc)
    # the two sides are two verdicts (px4 holds both sides in either batch: the halves swap)
    assert verdicts[0] != verdicts[1] or gate == "px4", verdicts
    if gate == "px4":
        a = S.run_pair(oracle, scenes[0], True)["accepted"]
        assert np.array_equal(a, 1 - S.run_pair(oracle, scenes[1], True)["accepted"]) and 0 < a.sum() < len(a)


def test_match_stereo_refuses_a_size_that_is_no_scale_space_size(oracle):
    sc = S.pair_scene("euroc", 20, 20, seed=9)
    fe = _fe(sc, False)
    kp1 = sc["kp1"].copy()
    kp1["size"][7] = 13.0
    with pytest.raises(capi.OkvfeError, match=r"keypoint 7: size 13\.0+ is not 12 \* scale\(octave 0\)") as e:
        fe.match_stereo(sc["d0"], sc["kp0"], sc["bp0"], sc["bv0"], sc["d1"], kp1, sc["bp1"], sc["bv1"], sc["T0"],
                        sc["T1"], sc["f0"], sc["f1"])
    assert e.value.status == capi.ERR_UNSUPPORTED


# ---- matchToMapUninitialised -------------------------------------------------------------------------
def _same_uninit(got, ref, what):
    assert np.array_equal(got[0], ref[0]), (what, "landmark", np.flatnonzero(got[0] != ref[0])[:8])
    assert np.array_equal(got[1], ref[1]), (what, "distance")
    assert np.array_equal(got[3], ref[3]), (what, "hp_set")
    _same_f64(got[2], ref[2], what)
    assert got[4] == ref[4], (what, "counter", got[4], ref[4])


@pytest.mark.parametrize("spec", S.UNINIT_SPECS, ids=S.spec_id)
def test_match_to_map_uninitialised_scene_both_forms(oracle, spec):
    sc = S.uninit_scene(spec[0], spec[1], spec[2], **spec[3])
    ref = S.run_uninit(oracle, sc)
    fe = _fe(sc, False)
    got = fe.match_to_map_uninitialised(sc["desc"], sc["bp"], sc["use"], sc["previous"], sc["desc_begin"], sc["pool"],
                                        sc["e0"], sc["r0"], sc["T1"], sc["focal"])
    _same_uninit(got, ref, sc["name"] + " host")
    # device form, two frames: the scene and its first half
    n = len(sc["desc"])
    frames = [n, n // 2]
    blocks = np.stack([multigpu.pack_block_host(K, sc["kps"][:m], sc["desc"][:m], sc["bp"][:m], sc["bv"][:m])
                       for m in frames])
    use = np.zeros((2, K), np.uint8)
    prev = np.full((2, K), -1, np.int32)
    for f, m in enumerate(frames):
        use[f, :m], prev[f, :m] = sc["use"][:m], sc["previous"][:m]
    n_lm = len(sc["desc_begin"]) - 1
    d_blocks, d_use, d_prev = _dev(blocks), _dev(use), _dev(prev)
    d_begin = _dev(sc["desc_begin"])
    d_pool, d_e0, d_r0 = _dev(_rows(sc["pool"])), _dev(_rows(sc["e0"])), _dev(_rows(sc["r0"]))
    md = fe.make_map_device(n_lm, d_begin.data_ptr(), d_pool.data_ptr(), None, d_e0.data_ptr(), d_r0.data_ptr())
    d_lm = torch.full((2, K), -7, dtype=torch.int32, device="cuda")
    d_bd = torch.full((2, K), -7, dtype=torch.int32, device="cuda")
    d_hp = torch.zeros((2, K, 4), dtype=torch.float64, device="cuda")
    d_hs = torch.full((2, K), 9, dtype=torch.uint8, device="cuda")
    d_ctr = torch.full((2,), 123, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    fe.match_to_map_uninitialised_blocks_device(d_blocks.data_ptr(), 2, d_use.data_ptr(), d_prev.data_ptr(), md,
                                                [sc["T1"], sc["T1"]], sc["focal"], d_lm.data_ptr(), d_bd.data_ptr(),
                                                d_hp.data_ptr(), d_hs.data_ptr(), d_ctr.data_ptr())
    torch.cuda.synchronize()
    lm, bd, hp, hs, ctr = (t.cpu().numpy() for t in (d_lm, d_bd, d_hp, d_hs, d_ctr))
    for f, m in enumerate(frames):
        r = oracle.match_to_map_uninit(sc["desc"][:m], sc["bp"][:m], sc["use"][:m], sc["previous"][:m],
                                       sc["desc_begin"], sc["pool"], sc["e0"], sc["r0"], sc["T1"], sc["focal"],
                                       S.THRESHOLD)
        _same_uninit((lm[f, :m], bd[f, :m], hp[f, :m], hs[f, :m], int(ctr[f])), r, f"{sc['name']} blocks frame {f}")
        assert np.all(lm[f, m:] == -7) and np.all(hs[f, m:] == 9)


# ---- matchToMap, 3-D landmarks ---------------------------------------------------------------------------
def _check_map_forms(oracle, fe, sc, cap):
    ref = S.run_map(oracle, sc)
    n = len(sc["kps"])
    if n <= cap:
        gl, gd = fe.match_to_map(sc["desc"], sc["kps"], sc["use"], sc["proj"], sc["desc_begin"], sc["pool"],
                                 sc["repr_thr"])
        bad = np.flatnonzero((gl != ref[0]) | (gd != ref[1]))
        assert len(bad) == 0, (sc["name"], "host", bad[:8], gl[bad[:8]], ref[0][bad[:8]], sc["kps"][bad[:8]])
    n_lm = len(sc["desc_begin"]) - 1
    frames = [n, n // 2]
    bp, bv = np.zeros((n, 3)), np.zeros(n, np.uint8)
    blocks = np.stack([multigpu.pack_block_host(cap, sc["kps"][:m], sc["desc"][:m], bp[:m], bv[:m]) for m in frames])
    use = np.zeros((2, cap), np.uint8)
    for f, m in enumerate(frames):
        use[f, :m] = sc["use"][:m]
    d_blocks, d_use = _dev(blocks), _dev(use)
    d_begin, d_pool = _dev(sc["desc_begin"]), _dev(_rows(sc["pool"]))
    d_proj = _dev(np.stack([_rows(sc["proj"]), _rows(sc["proj"])]))  # one projection set per frame
    md = fe.make_map_device(n_lm, d_begin.data_ptr(), d_pool.data_ptr(), d_proj.data_ptr())
    d_lm = torch.full((2, cap), -7, dtype=torch.int32, device="cuda")
    d_bd = torch.full((2, cap), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    fe.match_to_map_blocks_device(d_blocks.data_ptr(), 2, d_use.data_ptr(), md, sc["repr_thr"], d_lm.data_ptr(),
                                  d_bd.data_ptr())
    torch.cuda.synchronize()
    lm, bd = d_lm.cpu().numpy(), d_bd.cpu().numpy()
    for f, m in enumerate(frames):
        rl, rd = oracle.match_to_map(sc["desc"][:m], sc["kps"][:m], sc["use"][:m], sc["proj"], sc["desc_begin"],
                                     sc["pool"], sc["repr_thr"], S.THRESHOLD)
        bad = np.flatnonzero((lm[f, :m] != rl) | (bd[f, :m] != rd))
        assert len(bad) == 0, (sc["name"], "blocks frame", f, bad[:8], lm[f, bad[:8]], rl[bad[:8]], sc["kps"][bad[:8]])
        assert np.all(lm[f, m:] == -7) and np.all(bd[f, m:] == -7)


@pytest.mark.parametrize("spec", S.MAP_SPECS, ids=S.spec_id)
def test_match_to_map_prefilter_scene_both_forms(oracle, spec):
    sc = S.map_scene(spec[0], spec[1], spec[2], **spec[3])
    _check_map_forms(oracle, _frontend(752, 480, 1), sc, K)


@pytest.mark.parametrize("n_k", [4096, 4097])
def test_match_to_map_blocks_on_both_sides_of_the_region_order_limit(oracle, n_k):
    """4096 keypoints are ordered by image region before the waves are cut, 4097 keep the identity order:
    the same matches either way, NaN and out-of-range keypoints included"""
    cap = 4100  # (two layers of 2050 rows: one layer holds at most 4096)
    fe = capi.Frontend(752, 480, 38.0, 1, 150, cap // 2, match_threshold=S.THRESHOLD)
    assert fe.max_keypoints == cap
    for kind in ("outliers", "disjoint"):
        _check_map_forms(oracle, fe, S.map_scene(kind, n_k, 700, seed=11, repr_thr=20.0), cap)
    fe.close()


def test_match_to_map_landmarks_with_nan_and_out_of_range_keypoints(oracle):
    """okvfe_match_to_map_landmarks projects the landmarks itself: the keypoints carry the edge values"""
    import os
    import map_synth
    gold = os.path.join(os.path.dirname(__file__), "golden")
    voc = np.fromfile(os.path.join(gold, "small_voc_desc.bin"), dtype=np.uint8).reshape(-1, 48)
    m = map_synth.make_map(1500, voc=voc)
    fe = _frontend(752, 480, 1)
    fe.set_camera(0, m["cam"])
    kps, desc, use = map_synth.make_frame(m, oracle)
    kps = kps.copy()
    rng = np.random.default_rng(5)
    idx = rng.permutation(len(kps))
    kps["x"][idx[:20]] = np.nan
    kps["y"][idx[20:40]] = np.nan
    kps["x"][idx[40:50]] = -rng.uniform(1, 200, 10)
    kps["y"][idx[50:60]] = rng.uniform(65536, 1e5, 10)
    kps["x"][idx[60:63]] = (np.inf, -np.inf, 3.0e38)
    for thr in (20.0, 150.0):
        ref = oracle.prepare_landmarks(m["hp"], m["quality"], m["obs_begin"], m["obs_pose"], m["obs_bp"], m["poses"],
                                       m["T1"], m["cam"], thr, False)
        lm, bd, _ = fe.match_to_map_landmarks(0, m["hp"], m["quality"], m["obs_begin"], m["obs_pose"], m["obs_desc"],
                                              m["obs_bp"], m["poses"], m["T1"], thr, False, desc, kps, use)
        ids, proj, begin, rows = map_synth.packed_set(ref, m["obs_desc"], 1)
        rl, rd = oracle.match_to_map(desc, kps, use, proj, begin, rows, thr, S.THRESHOLD)
        rl = np.where(rl >= 0, ids[np.maximum(rl, 0)], -1)
        bad = np.flatnonzero((lm != rl) | (bd != rd))
        assert len(bad) == 0, (thr, bad[:8], lm[bad[:8]], rl[bad[:8]], kps[bad[:8]])
        nan = np.isnan(kps["x"]) | np.isnan(kps["y"])
        assert (rl[nan & (use != 0)] >= 0).sum() > 10  # a NaN keypoint is near every landmark
