"""The loads of the selection tail (refine_emit, k_select.hip: one 12-byte run per window row from a clamped base, ray
and Jacobian as three loads) and the records it leaves for every descriptor route, against the CPU oracle,
byte for byte: `detect`, camera-aware `detect_describe` (keypoints as u32 patterns, descriptors, and the valid bytes
through the compaction: the kept set) and `download` of device batches.  Scenes and what each is for:
tests/select_tail_loads_cases.py; that they are not vacuous: tests/test_select_tail_loads_cases.py (no GPU)."""
import numpy as np
import pytest

from okvis2_amd import capi, synth

import describe_scenes as S
import gpu_common as G
import select_tail_loads_cases as C

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _batch(fe, imgs, aware=True, cam_ids=None):
    """detect_describe_batch_device on a tensor that holds exactly `imgs` -> per-image download()"""
    n = len(imgs)
    d_img = torch.from_numpy(np.array(imgs, dtype=np.uint8, order="C")).cuda()
    assert d_img.numel() == imgs.size
    grav = np.tile(np.array(C.GRAV, dtype=np.float32), (n, 1)) if aware else None
    ids = (np.zeros(n, np.int32) if cam_ids is None else cam_ids) if aware else None
    fe.detect_describe_batch_device(d_img.data_ptr(), n, ids, grav, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    fe.check_capacity(n)
    return [fe.download(i) for i in range(n)]


def _aware_ref(oracle, img, radius, thr, kpts, rays, jac, cam):
    return oracle.detect_describe(img, radius, 0, thr, kpts, oracle.MODE_CAMERA_AWARE, rays, jac, np.float32(cam.fu), C.GRAV)


def _assert_result(got, rk, rd, oracle=None, cam=None):
    k, d, bp, bv = got
    G.assert_keypoints_equal(k, rk)
    assert np.array_equal(d, rd)
    if cam is not None:
        rbp, rv = oracle.backproject_keypoints(cam, rk)
        assert np.array_equal(bv, rv) and np.array_equal(bp.view(np.uint64), rbp.view(np.uint64))


@pytest.mark.parametrize("w", [64, 76])
def test_window_rim_first_and_last_image_of_a_batch(oracle, w):
    """keypoints within two pixels of all four rims, in the first and the last image of a tensor that holds nothing
    else: the clamped 12-byte runs stay inside it and rebuild the same pixels"""
    h = C.RIM_H
    cam = C.rim_camera(w)
    rays, jac = oracle.awareness_maps(cam)
    imgs = C.rim_batch(w)
    fe = capi.Frontend(w, h, C.RIM_RADIUS, 0, C.RIM_THRESHOLD, C.RIM_KPTS, max_batch=3)
    fe.set_camera(0, cam)
    got = _batch(fe, imgs)
    for i in range(3):
        rk, rd = _aware_ref(oracle, imgs[i], C.RIM_RADIUS, C.RIM_THRESHOLD, C.RIM_KPTS, rays, jac, cam)
        _assert_result(got[i], rk, rd, oracle, cam)
        det = oracle.detect(imgs[i], C.RIM_RADIUS, 0, C.RIM_THRESHOLD, C.RIM_KPTS)
        G.assert_keypoints_equal(fe.detect(imgs[i]), det)
        _assert_result(fe.detect_describe(imgs[i], cam=0, gravity=C.GRAV), rk, rd)


@pytest.mark.parametrize("box_scale", [1.0, C.WIDE_BOX_SCALE])
def test_centre_sample_both_box_widths(oracle, monkeypatch, box_scale):
    """EuRoC camera, built-in pattern: the centre point's box lies in the 7 x 7 window of most keypoints; with boxes
    widened by 1.73 it never does and every extra sample comes from the image"""
    cfg, img = C.centre_scene()
    cam = cfg.cams[0]
    rays, jac = oracle.awareness_maps(cam)
    if box_scale != 1.0:
        q = S.pattern("box%s" % box_scale)
        monkeypatch.setattr(oracle, "pattern", lambda: q)
    fe = G.make_frontend(cfg, box_scale=box_scale)
    fe.set_camera(0, cam)
    rk, rd = _aware_ref(oracle, img, cfg.uniformity_radius, cfg.abs_threshold, cfg.max_kpts, rays, jac, cam)
    assert len(rk) > 100
    _assert_result(fe.detect_describe(img, cam=0, gravity=C.GRAV), rk, rd, oracle, cam)
    _assert_result(_batch(fe, img[None])[0], rk, rd, oracle, cam)
    G.assert_keypoints_equal(fe.detect(img), oracle.detect(img, cfg.uniformity_radius, 0, cfg.abs_threshold, cfg.max_kpts))


def test_keypoints_the_ray_test_drops(oracle):
    """a camera whose rays are zero on the right part of the image: dropped keypoints next to kept ones, the kept set
    (the valid bytes, through the compaction) equal to the oracle's"""
    img = C.drop_scene()
    cam = C.drop_camera()
    rays, jac = C.drop_maps(oracle)
    fe = capi.Frontend(C.DROP_W, C.DROP_H, C.RIM_RADIUS, 0, C.RIM_THRESHOLD, C.RIM_KPTS)
    fe.set_camera(0, cam)
    fe.set_camera_maps(0, rays, jac, cam.fu)
    rk, rd = _aware_ref(oracle, img, C.RIM_RADIUS, C.RIM_THRESHOLD, C.RIM_KPTS, rays, jac, cam)
    det = oracle.detect(img, C.RIM_RADIUS, 0, C.RIM_THRESHOLD, C.RIM_KPTS)
    assert 0 < len(rk) < len(det)
    _assert_result(fe.detect_describe(img, cam=0, gravity=C.GRAV), rk, rd, oracle, cam)
    _assert_result(_batch(fe, img[None])[0], rk, rd, oracle, cam)
    G.assert_keypoints_equal(fe.detect(img), det)


def test_camera_aware_batch_with_a_flat_image(oracle):
    """camera-aware batch of three, image 1 flat: the fused set-up's records, slots and valid bytes reach the compaction"""
    cfg, imgs = C.flat_middle_batch()
    cam = cfg.cams[0]
    rays, jac = oracle.awareness_maps(cam)
    fe = G.make_frontend(cfg, max_batch=3)
    fe.set_camera(0, cam)
    got = _batch(fe, imgs)
    for i in range(3):
        rk, rd = _aware_ref(oracle, imgs[i], cfg.uniformity_radius, cfg.abs_threshold, cfg.max_kpts, rays, jac, cam)
        _assert_result(got[i], rk, rd, oracle, cam)
        assert (len(rk) == 0) == (i == 1) and (i == 1 or len(rk) > 50)


@pytest.mark.parametrize("mode", ["upright", "gradient"])
def test_upright_and_gradient_batches(oracle, mode):
    """the same images without a camera: describe_rot_kernel rewrites the angle in the tail's copy of the record"""
    cfg, imgs = C.flat_middle_batch()
    fe = G.make_frontend(cfg, max_batch=3, rotation_invariant=(mode != "upright"))
    omode = oracle.MODE_GRADIENT if mode == "gradient" else oracle.MODE_UPRIGHT
    got = _batch(fe, imgs, aware=False)
    for i in range(3):
        rk, rd = oracle.detect_describe(imgs[i], cfg.uniformity_radius, 0, cfg.abs_threshold, cfg.max_kpts, omode)
        _assert_result(got[i], rk, rd)
        assert (len(rk) == 0) == (i == 1)


def test_detect_then_compute(oracle):
    """description as a call of its own (describe_setup_kernel shares the set-up code and its map loads), between two
    fused calls on the same context"""
    cfg, imgs = C.flat_middle_batch()
    img = imgs[0]
    cam = cfg.cams[0]
    rays, jac = oracle.awareness_maps(cam)
    fe = G.make_frontend(cfg)
    fe.set_camera(0, cam)
    rk, rd = _aware_ref(oracle, img, cfg.uniformity_radius, cfg.abs_threshold, cfg.max_kpts, rays, jac, cam)
    _assert_result(fe.detect_describe(img, cam=0, gravity=C.GRAV), rk, rd, oracle, cam)
    det = fe.detect(imgs[2])
    G.assert_keypoints_equal(det, oracle.detect(imgs[2], cfg.uniformity_radius, 0, cfg.abs_threshold, cfg.max_kpts))
    ck, cd = oracle.describe(imgs[2], det, oracle.MODE_CAMERA_AWARE, rays, jac, np.float32(cam.fu), C.GRAV)
    _assert_result(fe.compute(imgs[2], det, cam=0, gravity=C.GRAV), ck, cd, oracle, cam)
    _assert_result(fe.detect_describe(img, cam=0, gravity=C.GRAV), rk, rd, oracle, cam)


def test_two_internal_lanes(oracle):
    """okvfe_set_internal_lanes(ctx, 2): the tail on lane views of the buffers; 128 small images, three scenes in turn"""
    w, h, n = C.DROP_W, C.DROP_H, C.LANES_IMAGES
    cam = C.drop_camera()
    rays, jac = oracle.awareness_maps(cam)
    base = C.drop_scene()
    three = np.stack([base, base[:, ::-1], base[::-1]])
    imgs = np.ascontiguousarray(three[np.arange(n) % 3])
    fe = capi.Frontend(w, h, C.RIM_RADIUS, 0, C.RIM_THRESHOLD, C.RIM_KPTS, max_batch=n)
    fe.set_camera(0, cam)
    fe.set_internal_lanes(2)
    got = _batch(fe, imgs)
    refs = [_aware_ref(oracle, three[i], C.RIM_RADIUS, C.RIM_THRESHOLD, C.RIM_KPTS, rays, jac, cam) for i in range(3)]
    assert all(len(r[0]) >= 10 for r in refs)
    for i in range(n):
        _assert_result(got[i], *refs[i % 3])
    fe.set_internal_lanes(1)  # the same context unsplit
    got = _batch(fe, imgs[:3])
    for i in range(3):
        _assert_result(got[i], *refs[i], oracle, cam)


def test_select_list_kernel(oracle):
    """640 x 480 at radius 10: the fine grid goes to select_list_kernel, which shares the tail.  (The pre-sorted form of
    the array-bin kernel is behind a lab knob the product library does not read.)"""
    cfg = synth.mono640_config()
    cam = cfg.cams[0]
    rays, jac = oracle.awareness_maps(cam)
    img = synth.corners_image(cfg.w, cfg.h, 65)
    fe = G.make_frontend(cfg)
    fe.set_camera(0, cam)
    rk, rd = _aware_ref(oracle, img, cfg.uniformity_radius, cfg.abs_threshold, cfg.max_kpts, rays, jac, cam)
    assert len(rk) > 300
    _assert_result(fe.detect_describe(img, cam=0, gravity=C.GRAV), rk, rd, oracle, cam)
    _assert_result(_batch(fe, img[None])[0], rk, rd, oracle, cam)
    G.assert_keypoints_equal(fe.detect(img), oracle.detect(img, cfg.uniformity_radius, 0, cfg.abs_threshold, cfg.max_kpts))
