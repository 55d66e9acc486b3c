"""GPU: what one call decides does not reach the next.  The descriptor kernel of a call follows from its batch (are all
images camera-aware? none?), and a detect-only call (okvfe_detect_batch_device) never looks at a batch at all: on one
context, a call with every image camera-aware followed by detect + describe without gravity -- and the reverse order --
gives what fresh contexts give."""
import numpy as np
import pytest

import gpu_common as G
from okvis2_amd import synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _frontend(cfg):
    fe = G.make_frontend(cfg, max_batch=2)
    for ci, cam in enumerate(cfg.cams):
        fe.set_camera(ci, cam)
    return fe


def _results(fe):
    return [fe.download(i) for i in range(2)]


def _assert_same(a, b):
    for x, y in zip(a, b):
        assert len(x[0]) == len(y[0]) and len(x[0]) > 50
        for u, v in zip(x, y):  # keypoints, descriptors, back-projections, their validity
            assert u.tobytes() == v.tobytes()


def test_detect_only_call_after_an_all_aware_call_and_the_reverse(oracle):
    cfg = synth.euroc_config()
    L, R, _ = synth.stereo_pair(cfg.w, cfg.h, 77)
    d_img = torch.from_numpy(np.stack([L, R])).cuda()
    ptr = d_img.data_ptr()
    cam_ids = np.array([0, 1], dtype=np.int32)
    grav = np.tile(np.array([0.0, 1.0, 0.0], dtype=np.float32), (2, 1))
    s = torch.cuda.current_stream().cuda_stream

    def aware(fe):
        fe.detect_describe_batch_device(ptr, 2, cam_ids, grav, s)
        torch.cuda.synchronize()
        return _results(fe)

    def split_plain(fe):
        fe.detect_batch_device(ptr, 2, s)
        fe.describe_batch_device(ptr, 2, None, None, s)
        torch.cuda.synchronize()
        return _results(fe)

    want_aware, want_plain = aware(_frontend(cfg)), split_plain(_frontend(cfg))
    # the two calls do differ (camera-aware descriptors against the default mode), and the fresh ones equal the oracle
    assert any(a[1].tobytes() != p[1].tobytes() for a, p in zip(want_aware, want_plain))
    for ci, img in enumerate((L, R)):
        cam = cfg.cams[ci]
        rays, jac = oracle.awareness_maps(cam)
        k, d = oracle.detect_describe(img, cfg.uniformity_radius, 0, cfg.abs_threshold, cfg.max_kpts,
                                      oracle.MODE_CAMERA_AWARE, rays, jac, np.float32(cam.fu), (0.0, 1.0, 0.0))
        G.assert_keypoints_equal(want_aware[ci][0], k)
        assert np.array_equal(want_aware[ci][1], d)

    fe = _frontend(cfg)
    _assert_same(aware(fe), want_aware)
    _assert_same(split_plain(fe), want_plain)   # detect-only right behind the all-aware call
    _assert_same(aware(fe), want_aware)

    fe = _frontend(cfg)                         # the reverse order
    _assert_same(split_plain(fe), want_plain)
    _assert_same(aware(fe), want_aware)
    _assert_same(split_plain(fe), want_plain)
