"""GPU: the cross-layer stage of the scale-space detector (octaves > 0) on the scenes of tests/scale_space_scenes.py --
k_pyramid.hip (both samplers, scale_filter_kernel, merge_layers_kernel), k_brisk_refine.hip, the FAST 5-8 virtual layer and
the two layer schedules of capi_detect.cpp.  tests/test_scale_space_scenes_host.py asserts on the CPU what these scenes
reach (every layer of four octaves delivering keypoints, rejections by each neighbour, equal neighbours, clipped windows,
cuts between equal scores, layers delivering nothing, every outcome of the scale parabola, 24+ rungs of the scale ladder);
here every comparison is byte for byte against the oracle."""
import ctypes as C

import numpy as np
import pytest

import gpu_common as G
import scale_space_ref as R
import scale_space_scenes as S
from okvis2_amd import capi, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

STAGES = ("harris", "nms", "sort", "select", "describe", "compact")
_REF = {}


def _frontend(cfg, w, h, octaves, max_batch=1, **kw):
    radius, thr, st = S.CONFIGS[cfg]
    kw.setdefault("rotation_invariant", cfg != "brisk")
    kw.setdefault("max_candidates", 0)
    return capi.Frontend(w, h, radius, octaves, thr, S.MAX_KPTS, max_batch=max_batch, score_type=st, **kw)


def _mode(oracle, cfg):
    return oracle.MODE_UPRIGHT if cfg == "brisk" else oracle.MODE_GRADIENT


def _reference(oracle, cfg, name, img, octaves):
    """oracle keypoints + descriptors of a scene, computed once per session"""
    key = (cfg, name, octaves)
    if key not in _REF:
        radius, thr, st = S.CONFIGS[cfg]
        _REF[key] = oracle.detect_describe(img, radius, octaves, thr, S.MAX_KPTS, _mode(oracle, cfg), score_type=st)
    return _REF[key]


def _assert_rows(got, want):
    G.assert_keypoints_equal(got, want)
    assert np.array_equal(got["size"].view(np.uint32), want["size"].view(np.uint32))
    assert np.array_equal(got["response"].view(np.uint32), want["response"].view(np.uint32))


def _run_batch(fe, d_img, B, stream):
    fe.detect_describe_batch_device(d_img.data_ptr(), B, None, None, stream)
    stream.synchronize()
    fe.check_capacity(B)
    return [fe.download(i) for i in range(B)]


def _stream():
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    return st


@pytest.mark.parametrize("cfg", sorted(S.CONFIGS))
@pytest.mark.parametrize("size", S.sizes(), ids=lambda s: "%dx%d-octaves%d" % s)
def test_every_scene_single_and_in_a_batch(oracle, size, cfg):
    """every scene of one size through okvfe_detect (the B = 1 seam) and in batches of 5 that hold the flat and the
    "layers 0-1 only" image through the device-resident call"""
    w, h, octaves = size
    radius, thr, st = S.CONFIGS[cfg]
    fe = _frontend(cfg, w, h, octaves, max_batch=5)
    assert fe.max_keypoints == 2 * octaves * S.MAX_KPTS
    stream = _stream()
    for batch in S.batch_for(w, h, octaves):
        want = [_reference(oracle, cfg, n, img, octaves) for n, img in batch]
        for n, img in batch:
            _assert_rows(fe.detect(img), oracle.detect(img, radius, octaves, thr, S.MAX_KPTS, score_type=st))
        d_img = torch.from_numpy(np.stack([img for _, img in batch])).cuda()
        got = _run_batch(fe, d_img, 5, stream)
        for i in range(5):
            _assert_rows(got[i][0], want[i][0])
            assert np.array_equal(got[i][1], want[i][1]), batch[i][0]
        assert len(want[1][0]) == 0  # the flat image
        assert set(np.unique(want[3][0]["octave"])) <= {0, 1}  # layers 0-1 only
    fe.close()


@pytest.mark.parametrize("cfg", sorted(S.CONFIGS))
def test_four_octaves_on_both_schedules(oracle, cfg):
    """eight layers side by side on eight streams (25 events, MergeLayers' arrays of 8 full), the same grouped by stage on
    one stream (profiling on: one launch bracket per stage and call), and side by side again on the same context"""
    w, h, octaves = 400, 392, 4
    batch = S.batch_for(w, h, octaves)[0]
    want = [_reference(oracle, cfg, n, img, octaves) for n, img in batch]
    d_img = torch.from_numpy(np.stack([img for _, img in batch])).cuda()
    stream = _stream()
    fe = _frontend(cfg, w, h, octaves, max_batch=5)
    plain = _run_batch(fe, d_img, 5, stream)
    fe.profile_enable(True)
    calls = 2
    staged = [_run_batch(fe, d_img, 5, stream) for _ in range(calls)]
    p = fe.profile_read()
    fe.profile_enable(False)
    again = _run_batch(fe, d_img, 5, stream)
    for i in range(5):
        _assert_rows(plain[i][0], want[i][0])
        assert np.array_equal(plain[i][1], want[i][1])
    for got in staged + [again]:
        for (ka, da, _, _), (kb, db, _, _) in zip(got, plain):
            assert ka.tobytes() == kb.tobytes() and da.tobytes() == db.tobytes()
    assert {k: p[k][1] for k in STAGES} == {k: calls for k in STAGES}, p
    assert set(np.unique(want[0][0]["octave"])) == set(range(8))
    fe.close()


def _camera(w, h):
    return synth.Camera(w, h, 0.6 * w, 0.61 * w, 0.5 * w - 1.5, 0.5 * h + 2.25, 1, (-0.28, 0.07, 0.0002, 0.00002))


@pytest.mark.parametrize("scale_invariant", [False, True])
@pytest.mark.parametrize("mode", ["upright", "gradient", "aware"])
def test_brisk_scale_space_with_each_extractor(oracle, mode, scale_invariant):
    """the published pairing: the continuous sizes of brisk_refine_kernel through each extractor, with and without the
    64-step scale ladder"""
    img, octaves = S.scene("checker-400x392")
    h, w = img.shape
    radius, thr, st = S.CONFIGS["brisk"]
    fe = _frontend("brisk", w, h, octaves, rotation_invariant=(mode != "upright"), scale_invariant=scale_invariant)
    omode = {"upright": oracle.MODE_UPRIGHT, "gradient": oracle.MODE_GRADIENT, "aware": oracle.MODE_CAMERA_AWARE}[mode]
    rays = jac = None
    kw, gravity, fu = {}, (0.0, 1.0, 0.0), np.float32(1.0)
    if mode == "aware":
        cam = _camera(w, h)
        fe.set_camera(0, cam)
        rays, jac = oracle.awareness_maps(cam)
        gravity, fu = (0.2, 0.95, -0.1), np.float32(cam.fu)
        kw = dict(cam=0, gravity=gravity)
    rk, rd = oracle.detect_describe(img, radius, octaves, thr, S.MAX_KPTS, omode, rays, jac, fu, gravity,
                                    score_type=st, scale_invariant=scale_invariant)
    k, d, _, _ = fe.detect_describe(img, **kw)
    _assert_rows(k, rk)
    assert np.array_equal(d, rd)
    assert len({capi.scale_index(s) for s in k["size"]}) >= 24 and len(k) > 100
    assert all(capi.scale_index(s) == oracle.scale_index(s) for s in k["size"])
    fe.close()


def _rung_sizes():
    """for every rung s = 1 .. 63 the two adjacent float32 sizes with okvfe_scale_index s - 1 and s"""
    out = []
    for s in range(1, 64):
        lo, hi = np.float32(1.0), np.float32(400.0)
        assert capi.scale_index(lo) < s <= capi.scale_index(hi)
        while np.nextafter(lo, np.float32(np.inf)) < hi:
            mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
            if capi.scale_index(mid) >= s:
                hi = mid
            else:
                lo = mid
        assert capi.scale_index(lo) == s - 1 and capi.scale_index(hi) == s
        out.append((lo, hi))
    return out


@pytest.mark.parametrize("mode", ["upright", "gradient", "aware"])
def test_scale_ladder_rungs(oracle, mode):
    """The device picks the rung from a float threshold table, the oracle from log(): both sides of all 63 rung
    boundaries, on keypoints in the middle of an image large enough for the largest pattern (border 324 px)."""
    w, h = 720, 700
    img = synth.noise_image(w, h, 77)
    rungs = _rung_sizes()
    assert all(oracle.scale_index(a) == s and oracle.scale_index(b) == s + 1 for s, (a, b) in enumerate(rungs))
    kps = np.zeros(2 * len(rungs), dtype=capi.KEYPOINT_DTYPE)
    kps["size"] = np.array(rungs, dtype=np.float32).reshape(-1)
    kps["x"] = 356.0 + 0.5 * (np.arange(len(kps)) // 2 % 16)  # (the two sides of a rung share their position)
    kps["y"] = 346.0 + 0.5 * (np.arange(len(kps)) // 32)
    kps["angle"], kps["response"], kps["class_id"] = -1.0, 50.0, -1
    fe = capi.Frontend(w, h, 30.0, 0, 100, 200, rotation_invariant=(mode != "upright"), scale_invariant=True)
    omode = {"upright": oracle.MODE_UPRIGHT, "gradient": oracle.MODE_GRADIENT, "aware": oracle.MODE_CAMERA_AWARE}[mode]
    rays = jac = None
    kw, gravity, fu = {}, (0.0, 1.0, 0.0), np.float32(1.0)
    if mode == "aware":
        cam = _camera(w, h)
        fe.set_camera(0, cam)
        rays, jac = oracle.awareness_maps(cam)
        fu = np.float32(cam.fu)
        kw = dict(cam=0, gravity=gravity)
    rk, rd = oracle.describe(img, kps, omode, rays, jac, fu, gravity, scale_invariant=True)
    assert len(rk) == len(kps)  # no keypoint is near the rim
    differ = int(sum(not np.array_equal(rd[2 * i], rd[2 * i + 1]) for i in range(len(rungs))))
    # neighbouring rungs scale the pattern by 2^(lb(30)/64) = 5.5 %: on noise that flips bits on every rung
    assert differ >= 60, differ
    gk, gd, _, _ = fe.compute(img, kps, **kw)
    G.assert_keypoints_equal(gk, rk)
    assert np.array_equal(gd, rd)
    fe.close()


def _device_ints(ptr, n):
    host = np.empty(n, dtype=np.int32)
    assert capi.lib().okvfe_copy_to_host(C.c_void_p(host.ctypes.data), C.c_void_p(ptr), C.c_size_t(host.nbytes),
                                         None) == capi.OK
    return host


def _layer_maxima(oracle, cfg, img, octaves):
    radius, thr, st = S.CONFIGS[cfg]
    return [len(m) for m in R.Prepared(img, 2 * octaves, thr, st).maxima]


@pytest.mark.parametrize("which", ["layer0", "upper"])
@pytest.mark.parametrize("cfg", sorted(S.CONFIGS))
def test_overflow_in_one_layer_empties_the_image(oracle, cfg, which):
    """include/okvfe.h, okvfe_check_capacity: an image whose candidate list overflowed keeps NO keypoints.  In a scale space
    the list of ONE layer overflows: the image must still come out empty (not with the other layers' keypoints), for a
    device-resident consumer (detect_counts, counts, the gather block) as for the host."""
    w, h, octaves = 400, 392, 4
    radius, thr, st = S.CONFIGS[cfg]
    victim = S.scene("checker-400x392")[0] if which == "layer0" else S.squares_over_blobs(w, h)
    others = [("squares-400x392", S.scene("squares-400x392")[0]), ("squares-30-180", S.squares(w, h, lo=30, hi=180))]
    n_victim = _layer_maxima(oracle, cfg, victim, octaves)
    # (twice: the fused score + NMS kernel lists both pixels of a tied pair before one of them is removed)
    n_others = 2 * max(max(_layer_maxima(oracle, cfg, img, octaves)) for _, img in others)
    if which == "layer0":  # layer 0 overflows, layer 2 does not
        cap, quiet = (n_victim[2] + 1) & ~1, 2
        assert n_victim[0] > cap >= n_victim[2]
    else:                  # an upper layer overflows, layer 0 does not
        cap, quiet = (max(n_others, 2 * n_victim[0], 64) + 1) & ~1, 0
        assert max(n_victim[1:]) > cap >= 2 * n_victim[0]
    # the layer that does not overflow has keypoints to deliver: an empty image is not what the layers give by themselves
    assert R.detect(victim, radius, octaves, thr, S.MAX_KPTS, st)[1]["per_layer_kept"][quiet] >= 5
    assert cap >= n_others and cap >= 64
    fe = _frontend(cfg, w, h, octaves, max_batch=3, max_candidates=cap)
    d_img = torch.from_numpy(np.stack([others[0][1], victim, others[1][1]])).cuda()
    stream = _stream()
    fe.detect_describe_batch_device(d_img.data_ptr(), 3, None, None, stream)
    stream.synchronize()
    with pytest.raises(capi.OkvfeError) as e:
        fe.check_capacity(3)
    assert e.value.status == capi.ERR_CAPACITY and "image 1" in str(e.value)
    want = [_reference(oracle, cfg, n, img, octaves) for n, img in others]
    for i, (rk, rd) in zip((0, 2), want):
        k, d, _, _ = fe.download(i)
        _assert_rows(k, rk)
        assert np.array_equal(d, rd)
    with pytest.raises(capi.OkvfeError) as e:
        fe.download(1)
    assert e.value.status == capi.ERR_CAPACITY
    out = fe.device_outputs()
    det, cnt = _device_ints(out.detect_counts, 3), _device_ints(out.counts, 3)
    print(cfg, which, "capacity", cap, "maxima per layer", n_victim, "detect_counts", det, "counts", cnt)
    assert det[1] == 0 and cnt[1] == 0, (det, cnt)
    assert [det[0], det[2]] == [len(oracle.detect(img, radius, octaves, thr, S.MAX_KPTS, score_type=st)) for _, img in others]
    assert cnt[0] == len(want[0][0]) and cnt[2] == len(want[1][0])
    nb = fe.gather_block_bytes()
    blocks = torch.zeros((3, nb), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fe.pack_gather_blocks_device(0, 3, blocks.data_ptr(), stream)
    stream.synchronize()
    host_counts = blocks[:, :4].cpu().numpy().copy().view(np.int32)[:, 0]
    assert host_counts[1] == 0 and host_counts[0] == len(want[0][0]) and host_counts[2] == len(want[1][0])
    fe.close()
