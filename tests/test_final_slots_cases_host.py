"""CPU: the scenes of tests/final_slots_cases.py are not vacuous -- by the oracle alone, each puts keypoints on both sides
of the decisions the selection tail now takes on the batched camera-aware route."""
import numpy as np
import pytest

import describe_scenes as S
import final_slots_cases as C


@pytest.fixture(params=C.PATTERNS)
def pat(request, oracle, monkeypatch):
    p = S.pattern(request.param)
    monkeypatch.setattr(oracle, "pattern", lambda: p)
    return request.param, p


def test_rim_scene_has_both_sides_of_the_border_line_on_every_rim(oracle, pat):
    key, p = pat
    det, kept, _ = C.reference(oracle, C.rim_scene(key), None)
    b = int(p.border)
    kept_xy = {(float(k["x"]), float(k["y"])) for k in kept}
    near = lambda v, line: abs(float(v) - line) <= 2.6
    for name, coord, line in (("left", "x", b), ("right", "x", C.W - b), ("top", "y", b), ("bottom", "y", C.H - b)):
        at = [q for q in det if near(q[coord], line)]
        on = [(float(q["x"]), float(q["y"])) in kept_xy for q in at]
        assert any(on) and not all(on), (key, name, len(at))
    c = C.census(p, det, kept, None)
    assert c["border"] >= 12 and c["kept_quick"] + c["kept_exact"] >= 12 and c["box"] == 0, c


def test_band_scene_drops_by_a_sample_box_and_keeps_past_the_quick_test(oracle, pat):
    key, p = pat
    det, kept, _ = C.reference(oracle, C.band_scene(), C.BAND_M)
    c = C.census(p, det, kept, C.BAND_M)
    # passes the border test, dropped by a sample box; fails the quick test, survives the exact one
    assert c["box"] >= 1 and c["kept_exact"] >= 1 and c["kept_quick"] >= 50 and c["border"] >= 50, (key, c)
    assert len(det) > 2 * 256  # three passes of the tail
    n = np.sqrt(np.float32(C.BAND_M[0]) ** 2 + np.float32(C.BAND_M[1]) ** 2)
    assert n > 1.2  # row norms of M above 1
    _, jac, _ = C.maps(C.BAND_M)
    assert S.predicted_route("aware_batched", jac, C.W, C.H, key) == "kAwareBatched"


def test_images_that_keep_nothing(oracle, pat):
    key, _ = pat
    det, kept, _ = C.reference(oracle, C.all_dropped_scene(key), None)
    assert len(det) > 100 and len(kept) == 0
    det, kept, _ = C.reference(oracle, C.flat_scene(), None)
    assert len(det) == 0 and len(kept) == 0


def test_kept_counts_around_the_pass_length(oracle):
    img = C.pass_scene()
    for n in C.PASS_COUNTS:
        det, kept, _ = C.reference(oracle, img, None, C.PASS_RADIUS, C.PASS_THR, n)
        assert len(det) == n and 0.3 * n < len(kept) < 0.7 * n  # the cap decides; survivors and drops interleave
