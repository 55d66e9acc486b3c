"""GPU: final slots assigned in the selection tail (k_select.hip, DescribeSetup::kps_out) on the batched camera-aware
route of a fused call -- validity decided completely in the tail, survivors counted per pass of 256 and written straight
to the output buffers, describe_aware_kernel in place, a back-projection kernel instead of the compaction pass -- against
the CPU oracle, byte for byte: keypoints, descriptors, rays, their validity, counts and detect_counts.  Scenes and what
each is for: tests/final_slots_cases.py; that they are not vacuous: tests/test_final_slots_cases_host.py (no GPU).
Every fused result is also compared with the unfused route (detect, then compute) on the same context."""
import ctypes as Ct
import os

import numpy as np
import pytest

from okvis2_amd import capi

import describe_scenes as S
import final_slots_cases as C
import gpu_common as G
import radtan8_ref as R8

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(params=C.PATTERNS)
def pat(request, oracle, monkeypatch):
    """both widths of the extra boxes: the built-in pattern and box_scale 1.73 (oracle and library alike)"""
    p = S.pattern(request.param)
    monkeypatch.setattr(oracle, "pattern", lambda: p)
    return request.param, S.BOX_SCALES.get(request.param, 1.0)


def _serves(w, h, radius, max_kpts):
    """select_lazy_kernel serves the configuration (launch_select's own plan, exported by the lab build): its tail is the
    one that assigns final slots"""
    lab = Ct.CDLL(os.path.join(ROOT, "okvis2_amd", "libokvfe_lab.so"))
    out = (Ct.c_int32 * 3)()
    lab.okvfe_lab_select_plan(int(w), int(h), Ct.c_float(radius), int(max_kpts), int(max_kpts), out)
    return bool(out[0])


def _frontend(M, box_scale=1.0, radius=C.RADIUS, thr=C.THR, max_kpts=C.MAX_KPTS, max_batch=1, radtan8=False):
    assert _serves(C.W, C.H, radius, max_kpts)
    fe = capi.Frontend(C.W, C.H, radius, 0, thr, max_kpts, max_batch=max_batch, box_scale=box_scale)
    cam = C.camera(radtan8=radtan8)
    fe.set_camera(0, cam)
    rays, jac, fu = C.maps(M)
    fe.set_camera_maps(0, rays, jac, fu)
    return fe, cam


def _counts(fe, n, which):
    host = np.zeros(n, dtype=np.int32)
    st = capi.lib().okvfe_copy_to_host(Ct.c_void_p(host.ctypes.data), Ct.c_void_p(getattr(fe.device_outputs(), which)),
                                       Ct.c_size_t(host.nbytes), None)
    assert st == 0
    return host


def _reference(oracle, img, M, cam, radius=C.RADIUS, thr=C.THR, max_kpts=C.MAX_KPTS):
    """(detected count, keypoints, descriptors, rays, validity) by the oracle"""
    det, k, d = C.reference(oracle, img, M, radius, thr, max_kpts)
    bp, bv = (R8 if cam.dist_type == capi.DIST_RADTAN8 else oracle).backproject_keypoints(cam, k)
    return len(det), k, d, bp, bv


def _assert_equal(got, ref, what=None):
    k, d, bp, bv = got
    _, rk, rd, rbp, rbv = ref
    assert len(k) == len(rk), (what, len(k), len(rk))
    G.assert_keypoints_equal(k, rk)
    assert np.array_equal(d, rd), what
    assert np.array_equal(bv, rbv), what
    assert np.array_equal(bp.view(np.uint64), rbp.view(np.uint64)), what


def _batch(fe, imgs):
    """one fused call on a tensor that holds exactly `imgs` -> per image download(), counts, detect_counts"""
    n = len(imgs)
    d_img = torch.from_numpy(np.array(imgs, dtype=np.uint8, order="C")).cuda()
    grav = np.tile(np.array(C.GRAV, dtype=np.float32), (n, 1))
    fe.detect_describe_batch_device(d_img.data_ptr(), n, np.zeros(n, np.int32), grav, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    fe.check_capacity(n)
    return [fe.download(i) for i in range(n)], _counts(fe, n, "counts"), _counts(fe, n, "detect_counts")


def _check_batch(fe, imgs, refs):
    got, counts, detected = _batch(fe, imgs)
    for i, ref in enumerate(refs):
        _assert_equal(got[i], ref, i)
        assert counts[i] == len(ref[1]) and detected[i] == ref[0], (i, counts[i], detected[i], ref[0])


def _unfused(fe, img):
    det = fe.detect(img)
    return len(det), fe.compute(img, det, cam=0, gravity=C.GRAV)


def test_rim_and_band_scenes(oracle, pat):
    """keypoints on the border line of all four rims; keypoints a sample box drops behind the border test and keypoints
    the exact test keeps behind the quick one (M row norms 1.22): one image per call and a batch of both"""
    key, box_scale = pat
    for M, img in ((None, C.rim_scene(key)), (C.BAND_M, C.band_scene())):
        fe, cam = _frontend(M, box_scale)
        ref = _reference(oracle, img, M, cam)
        assert 0 < len(ref[1]) < ref[0]
        _assert_equal(fe.detect_describe(img, cam=0, gravity=C.GRAV), ref)
        assert _counts(fe, 1, "counts")[0] == len(ref[1]) and _counts(fe, 1, "detect_counts")[0] == ref[0]
        n_det, unfused = _unfused(fe, img)  # fused against unfused: the same bytes
        assert n_det == ref[0]
        _assert_equal(unfused, ref)
        _assert_equal(fe.detect_describe(img, cam=0, gravity=C.GRAV), ref)


def test_images_that_keep_nothing_inside_a_batch_of_three(oracle, pat):
    """an image without keypoints, and an image whose keypoints are all dropped, each between two ordinary images"""
    key, box_scale = pat
    fe, cam = _frontend(None, box_scale, max_batch=3)
    rim, band = C.rim_scene(key), C.band_scene()
    for middle in (C.flat_scene(), C.all_dropped_scene(key)):
        imgs = [rim, middle, band]
        refs = [_reference(oracle, im, None, cam) for im in imgs]
        assert len(refs[1][1]) == 0 and len(refs[0][1]) > 10 and len(refs[2][1]) > 10
        _check_batch(fe, imgs, refs)
    assert _reference(oracle, C.all_dropped_scene(key), None, cam)[0] > 100


@pytest.mark.parametrize("kept", C.PASS_COUNTS)
def test_kept_counts_around_the_pass_length(oracle, kept):
    """255, 256, 257 and 513 kept keypoints (the cap decides), about half of them dropped by the extractor: the running
    base of the final slots crosses one and two passes"""
    fe, cam = _frontend(None, radius=C.PASS_RADIUS, thr=C.PASS_THR, max_kpts=kept, max_batch=2)
    img = C.pass_scene()
    ref = _reference(oracle, img, None, cam, C.PASS_RADIUS, C.PASS_THR, kept)
    assert ref[0] == kept and 0 < len(ref[1]) < kept
    _check_batch(fe, [img, img[::-1].copy()], [ref, _reference(oracle, img[::-1].copy(), None, cam, C.PASS_RADIUS, C.PASS_THR, kept)])
    _assert_equal(_unfused(fe, img)[1], ref)


def test_radtan8_camera_slot(oracle):
    """the back-projection kernel's RADTAN8 instantiation"""
    fe, cam = _frontend(C.BAND_M, radtan8=True, max_batch=2)
    assert cam.dist_type == capi.DIST_RADTAN8
    imgs = [C.band_scene(), C.rim_scene("default")]
    refs = [_reference(oracle, im, C.BAND_M, cam) for im in imgs]
    assert all(r[4].any() for r in refs)
    _check_batch(fe, imgs, refs)
    _assert_equal(_unfused(fe, imgs[0])[1], refs[0])


@pytest.mark.parametrize("n", [16, 128])
def test_two_internal_lanes(oracle, n):
    """okvfe_set_internal_lanes(ctx, 2): 16 images (below 64 per lane the library runs the call unsplit) and 128 images
    (two lane views of the output buffers), three scenes in turn"""
    fe, cam = _frontend(C.BAND_M, max_batch=n)
    fe.set_internal_lanes(2)
    three = [C.band_scene(), C.rim_scene("default"), C.all_dropped_scene("default")]
    refs = [_reference(oracle, im, C.BAND_M, cam) for im in three]
    _check_batch(fe, [three[i % 3] for i in range(n)], [refs[i % 3] for i in range(n)])
    fe.set_internal_lanes(1)
    _check_batch(fe, three, refs)


@pytest.mark.parametrize("order", ["fused_first", "compute_first"])
def test_call_ordering(oracle, order):
    """a fused call, a detect-only call and compute on one context, in both orders: the final-slot route and the
    *_tmp + compaction route share the output buffers and leave nothing behind for each other"""
    fe, cam = _frontend(C.BAND_M)
    a, b = C.band_scene(), C.rim_scene("default")
    ref_a, ref_b = _reference(oracle, a, C.BAND_M, cam), _reference(oracle, b, C.BAND_M, cam)

    def fused():
        _assert_equal(fe.detect_describe(a, cam=0, gravity=C.GRAV), ref_a)
        assert _counts(fe, 1, "counts")[0] == len(ref_a[1]) and _counts(fe, 1, "detect_counts")[0] == ref_a[0]

    def detect_then_compute():
        n_det, got = _unfused(fe, b)
        assert n_det == ref_b[0]
        _assert_equal(got, ref_b)

    for step in ((fused, detect_then_compute, fused) if order == "fused_first" else (detect_then_compute, fused, detect_then_compute)):
        step()
