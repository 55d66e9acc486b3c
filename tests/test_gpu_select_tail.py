"""The tail of the selection kernels (K4: sub-pixel refinement, emission, the extractor's per-keypoint set-up) against
the CPU oracle, byte for byte, through libokvfe.so: keypoints (float fields as u32), the keypoints the extractor drops
(the valid bytes: both sides compact them away) and descriptors.  One to three small images per call; the cases sit on
the boundaries of the tail's work distribution (caps around 8, 64 and 256 keypoints), on empty images inside a batch, on
the image rim, on refined positions that round onto another pixel of the camera maps, on both extra-box widths, on the
score-map form of the nine scores, on select_list_kernel and on the extractor modes without extra samples."""
import functools

import numpy as np
import pytest

from okvis2_amd import capi, synth

import describe_scenes as S
import gpu_common as G

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GRAV = (0.05, 0.99, -0.1)


@functools.lru_cache(maxsize=None)
def _maps(name):
    import oracle_lib as O
    cam = {"euroc": synth.euroc_config, "mono640": synth.mono640_config}[name]().cams[0]
    return O.awareness_maps(cam)


@functools.lru_cache(maxsize=None)
def _checker(w, h, seed):
    """exact two-level cells: far more maxima than any cap used here"""
    img = synth.corners_image(w, h, seed, cell=12, levels=(0, 255), noise=0, jitter=0)
    img.setflags(write=False)
    return img


def _aware_ref(oracle, cfg, img, max_kpts, rays, jac, cam, grav=GRAV, radius=None):
    return oracle.detect_describe(img, cfg.uniformity_radius if radius is None else radius, 0, cfg.abs_threshold,
                                  max_kpts, oracle.MODE_CAMERA_AWARE, rays, jac, np.float32(cam.fu), grav)


@pytest.mark.parametrize("cap", [1, 7, 8, 9, 63, 64, 65, 255, 256, 257])
def test_cap_on_pass_and_group_boundaries(oracle, cap):
    """kept == cap: the last group of lanes and the last pass of the tail are partly filled"""
    cfg = synth.euroc_config()
    cam = cfg.cams[0]
    img = _checker(cfg.w, cfg.h, 77)
    rays, jac = _maps("euroc")
    assert len(oracle.detect(img, cfg.uniformity_radius, 0, cfg.abs_threshold, cap)) == cap  # supply exceeds the cap
    fe = G.make_frontend(cfg, max_keypoints=cap)
    fe.set_camera(0, cam)
    rk, rd = _aware_ref(oracle, cfg, img, cap, rays, jac, cam)
    k, d, _, _ = fe.detect_describe(img, cam=0, gravity=GRAV)
    G.assert_keypoints_equal(k, rk)
    assert np.array_equal(d, rd)
    G.assert_keypoints_equal(fe.detect(img), oracle.detect(img, cfg.uniformity_radius, 0, cfg.abs_threshold, cap))


def test_empty_image_between_textured_ones(oracle):
    """a flat image (no candidates, no keypoints) in the middle of a batch leaves its neighbours alone"""
    cfg = synth.euroc_config()
    cam = cfg.cams[0]
    rays, jac = _maps("euroc")
    imgs = np.stack([synth.corners_image(cfg.w, cfg.h, 41), np.full((cfg.h, cfg.w), 128, np.uint8),
                     synth.corners_image(cfg.w, cfg.h, 42)])
    fe = G.make_frontend(cfg, max_batch=3)
    fe.set_camera(0, cam)
    d_img = torch.from_numpy(imgs).cuda()
    grav = np.tile(np.array(GRAV, dtype=np.float32), (3, 1))
    fe.detect_describe_batch_device(d_img.data_ptr(), 3, np.zeros(3, np.int32), grav, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for i in range(3):
        rk, rd = _aware_ref(oracle, cfg, imgs[i], cfg.max_kpts, rays, jac, cam)
        k, d, _, _ = fe.download(i)
        G.assert_keypoints_equal(k, rk)
        assert np.array_equal(d, rd)
        assert (len(rk) == 0) == (i == 1) and (i == 1 or len(rk) > 50)


RIM_RADIUS, RIM_THRESHOLD, RIM_KPTS = 4.0, 20, 400


def _rim_case(w):
    h = 96
    cam = synth.Camera(w, h, 80.0, 81.0, w / 2 - 0.7, h / 2 + 0.4, 1, (-0.05, 0.004, 0.0002, -0.0001))
    seed = 1
    return cam, synth.corners_image(w, h, seed, cell=7, jitter=2)


@pytest.mark.parametrize("w", [128, 132])
def test_image_rim(oracle, w):
    """corners next to all four borders: the clamped rows and the missing dwords of the 7 x 7 windows, the border rule and
    the boxes of the extra samples that leave the image"""
    cam, img = _rim_case(w)
    h = img.shape[0]
    rays, jac = oracle.awareness_maps(cam)
    det = oracle.detect(img, RIM_RADIUS, 0, RIM_THRESHOLD, RIM_KPTS)
    # not vacuous: kept keypoints within 4 pixels of every border, and keypoints the extractor drops
    assert (det["x"] <= 4).any() and (det["x"] >= w - 5).any() and (det["y"] <= 4).any() and (det["y"] >= h - 5).any()
    rk, rd = oracle.detect_describe(img, RIM_RADIUS, 0, RIM_THRESHOLD, RIM_KPTS, oracle.MODE_CAMERA_AWARE, rays, jac,
                                    np.float32(cam.fu), GRAV)
    assert 0 < len(rk) < len(det)
    fe = capi.Frontend(w, h, RIM_RADIUS, 0, RIM_THRESHOLD, RIM_KPTS)
    fe.set_camera(0, cam)
    G.assert_keypoints_equal(fe.detect(img), det)
    k, d, _, _ = fe.detect_describe(img, cam=0, gravity=GRAV)
    G.assert_keypoints_equal(k, rk)
    assert np.array_equal(d, rd)


@pytest.mark.parametrize("box_scale", [1.0, 1.73])
def test_map_lookup_and_both_extra_box_widths(oracle, monkeypatch, box_scale):
    """ray and Jacobian are read at the pixel the REFINED position rounds to; box_scale 1.73: the wide extra boxes"""
    cfg = synth.euroc_config()
    cam = cfg.cams[0]
    rays, jac = _maps("euroc")
    img = synth.corners_image(cfg.w, cfg.h, 61)
    det, score = oracle.detect(img, cfg.uniformity_radius, 0, cfg.abs_threshold, cfg.max_kpts, want_score=True)
    # the integer maximum (u, v) a keypoint was refined from: the pixel within one of it that carries its score
    moved_x = moved_y = 0
    for p in det:
        found = [(u, v) for v in range(int(p["y"]) - 1, int(p["y"]) + 3) for u in range(int(p["x"]) - 1, int(p["x"]) + 3)
                 if 0 <= u < cfg.w and 0 <= v < cfg.h and abs(p["x"] - u) <= 1 and abs(p["y"] - v) <= 1 and
                 np.float32(score[v, u]) == p["response"]]
        if len(found) == 1:
            moved_x += int(p["x"] + np.float32(0.5)) != found[0][0]
            moved_y += int(p["y"] + np.float32(0.5)) != found[0][1]
    assert moved_x > 0 and moved_y > 0  # not vacuous
    if box_scale != 1.0:
        q = S.pattern("box%s" % box_scale)
        monkeypatch.setattr(oracle, "pattern", lambda: q)
    fe = G.make_frontend(cfg, box_scale=box_scale)
    fe.set_camera(0, cam)
    for grav in (GRAV, (-1.0, 0.05, 0.1)):
        rk, rd = _aware_ref(oracle, cfg, img, cfg.max_kpts, rays, jac, cam, grav)
        k, d, _, _ = fe.detect_describe(img, cam=0, gravity=grav)
        G.assert_keypoints_equal(k, rk)
        assert np.array_equal(d, rd) and len(rk) > 100


def test_scores_from_the_score_map(oracle):
    """set_keep_score_map(True): the nine scores of the fit are read from the map, not recomputed from the pixels"""
    cfg = synth.euroc_config()
    cam = cfg.cams[0]
    rays, jac = _maps("euroc")
    img = synth.corners_image(cfg.w, cfg.h, 62)
    fe = G.make_frontend(cfg)
    fe.set_camera(0, cam)
    fe.set_keep_score_map(True)
    rk, rd = _aware_ref(oracle, cfg, img, cfg.max_kpts, rays, jac, cam)
    k, d, _, _ = fe.detect_describe(img, cam=0, gravity=GRAV)
    G.assert_keypoints_equal(k, rk)
    assert np.array_equal(d, rd) and len(rk) > 100
    G.assert_keypoints_equal(fe.detect(img), oracle.detect(img, cfg.uniformity_radius, 0, cfg.abs_threshold, cfg.max_kpts))


def test_list_kernel(oracle):
    """mono 640 x 480 at radius 10: the fine grid goes to select_list_kernel, which shares the tail"""
    cfg = synth.mono640_config()
    cam = cfg.cams[0]
    rays, jac = _maps("mono640")
    img = synth.corners_image(cfg.w, cfg.h, 63)
    fe = G.make_frontend(cfg)
    fe.set_camera(0, cam)
    rk, rd = _aware_ref(oracle, cfg, img, cfg.max_kpts, rays, jac, cam)
    k, d, _, _ = fe.detect_describe(img, cam=0, gravity=GRAV)
    G.assert_keypoints_equal(k, rk)
    assert np.array_equal(d, rd) and len(rk) > 300


@pytest.mark.parametrize("mode,scale_invariant", [("upright", False), ("gradient", False), ("gradient", True)])
def test_modes_without_extra_samples(oracle, mode, scale_invariant):
    """upright / gradient extraction (identity M, no extra samples) and the scale ladder's border table"""
    cfg = synth.euroc_config()
    img = synth.corners_image(cfg.w, cfg.h, 64)
    fe = G.make_frontend(cfg, rotation_invariant=(mode != "upright"), scale_invariant=scale_invariant)
    omode = oracle.MODE_GRADIENT if mode == "gradient" else oracle.MODE_UPRIGHT
    rk, rd = oracle.detect_describe(img, cfg.uniformity_radius, 0, cfg.abs_threshold, cfg.max_kpts, omode,
                                    scale_invariant=scale_invariant)
    k, d, _, bpv = fe.detect_describe(img)
    G.assert_keypoints_equal(k, rk)
    assert np.array_equal(d, rd) and len(rk) > 100
