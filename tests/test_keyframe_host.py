"""CPU: the host side of the keyframe decision (okvfe_keyframe_decision / capi.keyframe_decision) against the numpy
restatement of Frontend::doWeNeedANewKeyframe in keyframe_ref.py, and the restatement against itself: the known
stencils of OpenCV's filled midpoint circle, the subset identity (matches is a subset of detections) and the dilation
identity (a mask is the set of distinct centres dilated by one stencil) that the kernel's design rests on.

PARITY UNPINNED: cv::circle and the point rounding are restated from OpenCV's published source (OpenCV is neither in
the reference tree nor installed); the stencils below are known answers of that restatement, not of a cv build."""
import ctypes as C
import struct

import numpy as np
import pytest

import keyframe_ref as R
from okvis2_amd import capi


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _rec(n_keypoints=0, n_matched=0, detections=0, matches=0, intersection=0, union=0):
    return {"n_keypoints": n_keypoints, "n_matched": n_matched, "detections_area": detections,
            "matches_area": matches, "intersection_area": intersection, "union_area": union}


def _arr(records):
    a = np.zeros(len(records), dtype=capi.COVERAGE_DTYPE)
    for i, r in enumerate(records):
        for f in R.COVERAGE_FIELDS:
            a[f][i] = r[f]
    return a


def _check(current, others, threshold=0.55):
    want_need, want_overlap = R.decision(current, others, np.float32(threshold))
    oth = None if not others else np.stack([_arr(o) for o in others])
    need, overlap = capi.keyframe_decision(_arr(current), oth, threshold)
    assert need == want_need, (current, others, overlap, want_overlap)
    assert _bits(overlap) == _bits(want_overlap), (current, others, overlap, want_overlap)
    return need, overlap


# ---- the restatement's disc ---------------------------------------------------------------------------------------
STENCILS = {4: ([4, 3, 3, 2, 0], 49), 9: ([9, 8, 8, 8, 8, 7, 6, 5, 4, 0], 253), 3: ([3, 2, 2, 0], 29),
            5: ([5, 4, 4, 4, 3, 0], 81), 0: ([0], 1)}


@pytest.mark.parametrize("r", sorted(STENCILS))
def test_stencil_known_answers(r):
    hw, pixels = STENCILS[r]
    assert R.stencil(r) == hw
    assert sum(2 * h + 1 for h in hw) * 2 - (2 * hw[0] + 1) == pixels
    m = np.zeros((2 * r + 5, 2 * r + 7), np.uint8)  # a disc well inside a mask, painted span by span
    R.circle(m, r + 3, r + 2, r)
    assert int(np.count_nonzero(m)) == pixels
    for j in range(-r - 2, r + 3):
        row = np.flatnonzero(m[r + 2 + j])
        if abs(j) > r:
            assert row.size == 0
        else:
            assert row[0] == r + 3 - hw[abs(j)] and row[-1] == r + 3 + hw[abs(j)] and row.size == 2 * hw[abs(j)] + 1


def test_radius_and_centre_rounding():
    assert [R.radius_for(w, h) for w, h in ((752, 480), (640, 480), (720, 540), (1024, 1024))] == [4, 4, 4, 9]
    assert [R.centre(x) for x in (5, 15, 25, 35)] == [0, 2, 2, 4]  # cvRound: half to even
    assert R.centre(751.5) == 75 and R.centre(479.5) == 48  # one pixel outside a 48 x 75 mask
    assert R.centre(0.0) == 0


def _random_frame(rng, w, h, n, frac):
    kps = np.zeros(n, dtype=capi.KEYPOINT_DTYPE)
    kps["x"] = rng.uniform(0, w - 0.5, n)
    kps["y"] = rng.uniform(0, h - 0.5, n)
    ids = np.where(rng.random(n) < frac, rng.integers(1, 1 << 40, n), 0).astype(np.uint64)
    return kps, ids


@pytest.mark.parametrize("w,h", [(752, 480), (1024, 1024), (720, 540)])
def test_subset_and_dilation_identities(w, h):
    rng = np.random.default_rng(w)
    rows, cols = R.mask_shape(w, h)
    r = R.radius_for(w, h)
    hw = R.stencil(r)
    for n, frac in ((1, 1.0), (20, 0.4), (226, 0.4), (700, 0.0), (700, 1.0)):
        kps, ids = _random_frame(rng, w, h, n, frac)
        kps["x"][: n // 4] = np.floor(kps["x"][: n // 4] / 10) * 10 + 5  # half-way centres, many duplicates
        kps["x"][-1], kps["y"][-1] = w - 0.5, h - 0.5
        id_set = None if frac == 1.0 else np.concatenate([ids[::2], np.zeros(2, np.uint64), ids[:3]])
        det, mat, _ = R.masks(w, h, kps, ids, id_set)
        c = R.coverage(w, h, kps, ids, id_set)
        assert not np.any(mat & ~det)  # matches is a subset of detections
        assert c["intersection_area"] == c["matches_area"] and c["union_area"] == c["detections_area"]
        in_set = None if id_set is None else set(int(v) for v in id_set)
        for mask, keep in ((det, np.ones(n, bool)),
                           (mat, np.array([int(i) != 0 and (in_set is None or int(i) in in_set) for i in ids]))):
            centres = {(R.centre(kps["x"][k]), R.centre(kps["y"][k])) for k in range(n) if keep[k]}
            dil = np.zeros_like(mask)
            for cx, cy in centres:
                for j in range(-r, r + 1):
                    y, x0, x1 = cy + j, max(cx - hw[abs(j)], 0), min(cx + hw[abs(j)], cols - 1)
                    if 0 <= y < rows and x0 <= x1:
                        dil[y, x0:x1 + 1] = 255
            assert np.array_equal(dil, mask)


def test_issue_saturation_figures():
    """dense frames saturate the 48 x 75 mask: the sparse cases are the ones that discriminate"""
    rng = np.random.default_rng(5)
    areas = {}
    for n in (20, 226, 700):
        kps, ids = _random_frame(rng, 752, 480, n, 0.4)
        areas[n] = R.coverage(752, 480, kps, ids)["detections_area"]
    assert areas[700] > 3550 and areas[20] < 20 * 49 + 1 and areas[20] < areas[226] < areas[700] <= 3600


# ---- the decision -------------------------------------------------------------------------------------------------
def test_decision_seeded_sweep():
    rng = np.random.default_rng(1058)
    verdicts = set()
    for trial in range(400):
        n_cam = int(rng.integers(1, 4))
        n_oth = int(rng.integers(0, 5))

        def rec():
            u = int(rng.integers(0, 3600)) if rng.random() > 0.15 else 0
            i = int(rng.integers(0, u + 1))
            return _rec(int(rng.integers(0, 30)), 0, u, i, i, u)
        current = [rec() for _ in range(n_cam)]
        others = [[rec() for _ in range(n_cam)] for _ in range(n_oth)]
        if trial % 7 == 0:  # whole multiframes without a painted pixel: 0 / 0
            current = [_rec(int(rng.integers(0, 30))) for _ in range(n_cam)]
        if trial % 5 == 0 and others:
            others[0] = [_rec() for _ in range(n_cam)]
        need, overlap = _check(current, others)
        verdicts.add(need)
        assert not np.isnan(overlap)
    assert verdicts == {True, False}


def test_decision_edge_cases():
    full = _rec(100, 90, 1000, 900, 900, 1000)
    # no other frames: overlapOthers = 0 -> a keyframe is needed, whatever the current frame's own overlap
    assert _check([full, full], []) == (True, 0.0)
    # the current multiframe paints nothing (NaN overlap): std::min(overlapOthers, NaN) is overlapOthers
    need, overlap = _check([_rec(20), _rec(20)], [[full, full]])
    assert overlap == 0.9 and not need
    # another multiframe paints nothing: std::max(a, NaN) is a
    assert _check([full], [[_rec()], [_rec(5, 1, 10, 4, 4, 10)]]) == (True, 0.4)
    assert _check([full], [[_rec()]]) == (True, 0.0)
    # counts are summed over the cameras before the division, not averaged
    a, b = _rec(50, 0, 0, 0, 10, 100), _rec(50, 0, 0, 0, 290, 300)
    assert _check([a, b], [[b, a]])[1] == 300 / 400
    # fewer than 7 keypoints per camera: never a keyframe; exactly 7 per camera: decided by the overlap
    low = _rec(1, 0, 100, 0, 0, 100)
    for n_cam in (1, 2, 3):
        cur = [dict(low) for _ in range(n_cam)]
        cur[0]["n_keypoints"] = 7 * n_cam - 1 - (n_cam - 1)
        assert sum(c["n_keypoints"] for c in cur) == 7 * n_cam - 1
        assert _check(cur, [cur])[0] is False
        cur[0]["n_keypoints"] += 1
        assert _check(cur, [cur])[0] is True


def test_decision_threshold_boundary():
    """float(overlap) lands exactly on 0.55f from below and from above (not > 0.55f: keyframe), then one float up"""
    thr = np.float32(0.55)
    for i, u, want in ((11, 20, True), (55_000_003, 100_000_000, True), (55_000_006, 100_000_000, False),
                       (54_999_999, 100_000_000, True)):
        ratio = np.float64(i) / np.float64(u)
        if (i, u) == (11, 20):
            assert ratio < np.float64(thr) and np.float32(ratio) == thr
        if i == 55_000_003:
            assert ratio > np.float64(thr) and np.float32(ratio) == thr
        if i == 55_000_006:
            assert np.float32(ratio) > thr
        r = _rec(50, 0, u, i, i, u)
        assert _check([r], [[r]])[0] is want


def test_decision_argument_validation():
    good = _arr([_rec(10, 0, 5, 5, 5, 5)])
    with pytest.raises(capi.OkvfeError) as e:
        capi.keyframe_decision(np.zeros(0, capi.COVERAGE_DTYPE))
    assert e.value.status == capi.ERR_INVALID_ARGUMENT
    for field in ("n_keypoints", "intersection_area", "union_area"):
        bad = good.copy()
        bad[field][0] = -1
        with pytest.raises(capi.OkvfeError):
            capi.keyframe_decision(bad)
        with pytest.raises(capi.OkvfeError):
            capi.keyframe_decision(good, bad.reshape(1, 1))
    with pytest.raises(ValueError):
        capi.keyframe_decision(_arr([_rec(), _rec()]), _arr([_rec(), _rec(), _rec()]))
    lib = capi.lib()
    need, overlap = C.c_int32(), C.c_double()
    p = good.ctypes.data_as(C.c_void_p)
    thr = C.c_float(0.55)
    assert lib.okvfe_keyframe_decision(p, 1, None, 0, thr, C.byref(need), None) == capi.OK  # overlap may be NULL
    assert lib.okvfe_keyframe_decision(p, 1, None, 0, thr, None, C.byref(overlap)) == capi.ERR_INVALID_ARGUMENT
    assert lib.okvfe_keyframe_decision(p, 1, None, 1, thr, C.byref(need), None) == capi.ERR_INVALID_ARGUMENT
    assert lib.okvfe_keyframe_decision(p, 1, p, -1, thr, C.byref(need), None) == capi.ERR_INVALID_ARGUMENT
    assert lib.okvfe_keyframe_decision(None, 1, None, 0, thr, C.byref(need), None) == capi.ERR_INVALID_ARGUMENT
    assert lib.okvfe_keyframe_decision(p, 0, None, 0, thr, C.byref(need), None) == capi.ERR_INVALID_ARGUMENT


def test_binding_surface():
    assert capi.COVERAGE_DTYPE.itemsize == 24 and capi.COVERAGE_DTYPE.names == R.COVERAGE_FIELDS
    for name in ("okvfe_keyframe_coverage_blocks_device", "okvfe_keyframe_coverage", "okvfe_keyframe_decision"):
        assert name in capi.EXPORTS
        getattr(capi.lib(), name)
    assert capi.ABI_VERSION == 8 == capi.lib().okvfe_abi_version()
    assert callable(capi.Frontend.keyframe_coverage_blocks_device) and callable(capi.Frontend.keyframe_coverage)
