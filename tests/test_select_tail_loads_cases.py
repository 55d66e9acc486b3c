"""The scenes of tests/test_gpu_select_tail_loads.py are not vacuous: what each is there for, asserted from the CPU
oracle's keypoints alone (no GPU)."""
import numpy as np
import pytest

import select_tail_loads_cases as C


def _rim_det(oracle, img):
    return oracle.detect(img, C.RIM_RADIUS, 0, C.RIM_THRESHOLD, C.RIM_KPTS)


@pytest.mark.parametrize("w", [64, 76])
def test_rim_scenes_reach_all_four_rims(oracle, w):
    h = C.RIM_H
    s = C.rim_scenes(w)
    mx, my = _rim_det(oracle, s["mx"]), _rim_det(oracle, s["my"])
    left, _, _, bottom = C.rim_counts(mx, w, h)
    _, right, top, _ = C.rim_counts(my, w, h)
    assert min(left, right, top, bottom) >= 2, (left, right, top, bottom)
    # the left-rim scene opens the batch, a bottom-rim scene closes it: a read before or behind the tensor would be theirs
    batch = C.rim_batch(w)
    assert C.RIM_ORDER[0] == "mx" and np.array_equal(batch[0], s["mx"])
    assert C.rim_counts(_rim_det(oracle, batch[0]), w, h)[0] >= 2
    assert C.rim_counts(_rim_det(oracle, batch[-1]), w, h)[3] >= 2
    # refinements of exactly +-1 (or 0) reach the window's edge
    assert C.integer_coordinates(mx) >= 3 and C.integer_coordinates(my) >= 3


def test_centre_sample_scene_takes_both_paths(oracle):
    cfg, img = C.centre_scene()
    det, score = oracle.detect(img, cfg.uniformity_radius, 0, cfg.abs_threshold, cfg.max_kpts, want_score=True)
    p = oracle.pattern()
    assert p.n_points > 64 and p.px[0] == 0.0 and p.py[0] == 0.0  # the first extra sample is the centre point
    inside, outside, unknown = C.centre_census(det, score, cfg.w, cfg.h, p.sigma_half[0])
    assert inside >= 50, (inside, outside, unknown)
    # widened boxes: no box of the centre point fits the 5 x 5 form, so none may come from the window
    wide = np.float32(p.sigma_half[0]) * np.float32(C.WIDE_BOX_SCALE)
    assert wide >= 2.0
    assert C.centre_census(det, score, cfg.w, cfg.h, wide)[0] == 0


def test_centre_predicate_on_hand_made_positions():
    s, w, h = 1.6042560338974, 752, 480
    assert C.centre_box_in_window(100.0, 100.0, 100, 100, s, w, h)
    assert C.centre_box_in_window(101.0, 99.0, 100, 100, s, w, h)      # refined by exactly +1 / -1: the window's edge
    assert not C.centre_box_in_window(102.0, 100.0, 100, 100, s, w, h)  # (cannot happen: the fit is clamped to +-1)
    assert not C.centre_box_in_window(1.0, 100.0, 1, 100, s, w, h)      # the box leaves the image
    assert not C.centre_box_in_window(float("nan"), 100.0, 100, 100, s, w, h)
    assert not C.centre_box_in_window(100.0, 100.0, 100, 100, 2.8, w, h)  # a 7-pixel box


def test_zero_ray_scene_drops_some_and_keeps_some(oracle):
    img = C.drop_scene()
    cam = C.drop_camera()
    rays, jac = C.drop_maps(oracle)
    det = oracle.detect(img, C.RIM_RADIUS, 0, C.RIM_THRESHOLD, C.RIM_KPTS)
    rk, _ = oracle.detect_describe(img, C.RIM_RADIUS, 0, C.RIM_THRESHOLD, C.RIM_KPTS, oracle.MODE_CAMERA_AWARE, rays, jac,
                                   np.float32(cam.fu), C.GRAV)
    inner = det[(det["x"] > 20) & (det["x"] < C.DROP_W - 20) & (det["y"] > 20) & (det["y"] < C.DROP_H - 20)]
    lost = int((inner["x"] >= C.DROP_FROM_X + 1).sum())
    assert lost >= 5 and len(rk) >= 10
    assert (rk["x"] < C.DROP_FROM_X + 1).all()  # nothing on a zero ray survives
    assert len(rk) <= len(det) - lost


def test_flat_middle_image_has_no_keypoints(oracle):
    cfg, imgs = C.flat_middle_batch()
    assert len(oracle.detect(imgs[1], cfg.uniformity_radius, 0, cfg.abs_threshold, cfg.max_kpts)) == 0
