"""CPU: the host arithmetic behind ViSlamBackend::overlapFraction, the order of the motion-stereo sweep and
ViSlamBackend::trackingQuality (okvfe_overlap_fraction, okvfe_motion_frame_order, okvfe_tracking_quality) against the
restatement in overlap_ref.py, bit for bit (u64 patterns of the doubles); the floors the GPU scenes must meet; and the
binding surface.

PARITY UNPINNED for cv::circle and the point rounding, as in keyframe_ref.py."""
import math
import os
import re
import struct

import numpy as np
import pytest

import keyframe_ref as R
import overlap_ref as OR
import overlap_scenes as S
from okvis2_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def _counts(n_matched=(0, 0), intersection=(0, 0), union=(0, 0), n_keypoints=(0, 0)):
    return {"n_keypoints": list(n_keypoints), "n_matched": list(n_matched), "intersection_area": list(intersection),
            "union_area": list(union)}


def _carr(records):
    a = np.zeros(len(records), dtype=capi.OVERLAP_COUNTS_DTYPE)
    for i, r in enumerate(records):
        for f in OR.COUNT_FIELDS:
            a[f][i] = r[f]
    return a


# ---- okvfe_overlap_fraction ---------------------------------------------------------------------------------------
def test_overlap_fraction_seeded_sweep_bit_for_bit():
    rng = np.random.default_rng(2410)
    recs = []
    for _ in range(2000):
        union = rng.integers(0, 5000, 2)
        inter = [int(rng.integers(0, u + 1)) for u in union]
        mode = rng.random()
        for f in ((0, 1) if mode < 0.1 else (int(rng.integers(0, 2)),) if mode < 0.3 else ()):
            union[f] = 0  # x / 0: inf, or NaN where the intersection is 0 as well
            if rng.random() < 0.5:
                inter[f] = 0
        nm = (0, 0) if rng.random() < 0.15 else tuple(int(v) for v in rng.integers(1, 700, 2))
        recs.append(_counts(nm, inter, [int(u) for u in union], (700, 700)))
    got = capi.overlap_fraction(_carr(recs))
    want = [OR.overlap_from_counts(r) for r in recs]
    assert [_bits(g) for g in got] == [_bits(w) for w in want]
    assert any(math.isnan(w) for w in want) and any(math.isinf(w) for w in want) and any(0 < w < 1 for w in want)


def test_overlap_fraction_nan_and_empty():
    nan0 = _counts((1, 1), (0, 5), (0, 10))   # o[0] = 0 / 0: std::min(NaN, x) = NaN
    nan1 = _counts((1, 1), (5, 0), (10, 0))   # o[1] = 0 / 0: o[1] < o[0] is false, o[0] comes back
    both = _counts((2, 3), (0, 0), (0, 0))
    empty = _counts((0, 0), (0, 0), (40, 50), (9, 9))
    got = capi.overlap_fraction(_carr([nan0, nan1, both, empty]))
    assert math.isnan(got[0]) and got[1] == 0.5 and math.isnan(got[2]) and _bits(got[3]) == _bits(0.0)
    for g, r in zip(got, (nan0, nan1, both, empty)):
        assert _bits(g) == _bits(OR.overlap_from_counts(r))
    assert len(capi.overlap_fraction(np.zeros(0, dtype=capi.OVERLAP_COUNTS_DTYPE))) == 0


@pytest.mark.parametrize("bad", [
    _counts((0, 1), (0, 1), (1, 1)), _counts((3, 0), (1, 0), (1, 1)),   # exactly one side without a matched keypoint
    _counts((1, 1), (-1, 0), (1, 1)), _counts((1, 1), (0, 0), (1, -2)), _counts((-1, -1)),
    _counts((1, 1), (1, 1), (1, 1), (-5, 0))])
def test_overlap_fraction_refuses_inconsistent_and_negative_records(bad):
    good = _counts((1, 1), (1, 1), (2, 2))
    with pytest.raises(capi.OkvfeError) as e:
        capi.overlap_fraction(_carr([good, bad]))
    assert e.value.status == capi.ERR_INVALID_ARGUMENT


# ---- okvfe_motion_frame_order -------------------------------------------------------------------------------------
def _order(overlaps, ids, previous=-1):
    got = capi.motion_frame_order(overlaps, ids, previous).tolist()
    assert got == OR.motion_frame_order(overlaps, ids, previous), (overlaps, ids, previous)
    return got


def test_frame_order_seeded_sweep():
    rng = np.random.default_rng(1751)
    for _ in range(300):
        n = int(rng.integers(0, 25))
        ov = rng.choice([0.0, 1e-8, 1e-9, 0.25, 0.5, 1.0], n) if rng.random() < 0.5 else rng.random(n)
        ids = rng.choice(np.arange(1, 1000, dtype=np.uint64), n, replace=False)
        previous = int(rng.integers(-1, n)) if n else -1
        _order(ov, ids, previous)


def test_frame_order_cut_ties_and_previous():
    edge = np.nextafter(1e-8, 1.0)
    assert _order([1e-8, edge, 0.5], [1, 2, 3]) == [2, 1]              # <= 1.0e-8 ends the list, the next double does not
    assert _order([0.5, 0.5, 0.5], [7, 9, 8]) == [1, 2, 0]              # tied overlaps: the larger id first
    assert _order([1.0, 0.0, 0.3], [5, 6, 4], previous=1) == [1, 0, 2]  # previous at 1.0 ties a self-identical frame: id decides
    assert _order([1.0, 0.0, 0.3], [6, 5, 4], previous=1) == [0, 1, 2]
    assert _order([1e-8, 0.0, 1e-9], [1, 2, 3]) == []                   # everything below the cut
    assert _order([0.0, 0.0], [1, 2], previous=0) == [0]
    assert _order([float("nan"), 0.2], [1, 2], previous=0) == [0, 1]    # previous: its overlap is not looked at
    assert _order([], []) == []
    assert _order([0.3], [2 ** 63 + 5]) == [0]


def test_frame_order_refuses_duplicates_and_nan():
    with pytest.raises(capi.OkvfeError) as e:
        capi.motion_frame_order([0.5, 0.4, 0.3], [4, 9, 4])
    assert e.value.status == capi.ERR_INVALID_ARGUMENT
    with pytest.raises(capi.OkvfeError) as e:  # std::sort on a NaN is undefined: refused, the entry named
        capi.motion_frame_order([0.5, 0.4, float("nan"), float("nan")], [1, 2, 3, 4], previous=0)
    assert e.value.status == capi.ERR_INVALID_ARGUMENT and "entry 2" in str(e.value)
    with pytest.raises(capi.OkvfeError):
        capi.motion_frame_order([0.5], [1], previous=1)
    with pytest.raises(capi.OkvfeError):
        capi.motion_frame_order([0.5], [1], previous=-2)


# ---- okvfe_tracking_quality ---------------------------------------------------------------------------------------
def _cov(n_matched, matches_area):
    a = np.zeros(1, dtype=capi.COVERAGE_DTYPE)
    a["n_matched"], a["matches_area"] = n_matched, matches_area
    return a[0]


def _quality(records, w=752, h=480, kptrad=S.KPTRAD):
    got = capi.tracking_quality(np.array(records, dtype=capi.COVERAGE_DTYPE), w, h, kptrad)
    want = OR.tracking_quality_from_records(records, w, h, kptrad)
    assert _bits(got) == _bits(want), (records, got, want)
    return got


def test_tracking_quality_known_answers():
    assert OR.point_area(752, 480, S.KPTRAD) == 65  # int(4.56^2 pi), while the painted disc of radius 4 has 49 pixels
    assert R.radius_for(752, 480, S.KPTRAD) == 4 and sum(2 * h + 1 for h in R.stencil(4)) * 2 - 9 == 49
    assert _quality([_cov(4, 500), _cov(3, 700)]) == 0.0                      # 7 matched points
    assert _quality([_cov(4, 500), _cov(4, 700)]) == (435 + 635) / (2 * (3600 - 65))  # 8
    assert _quality([_cov(8, 64), _cov(0, 0)]) == 0.0                         # below pointArea: max(0, .)
    assert _quality([_cov(8, 65), _cov(0, 0)]) == 0.0                         # at
    assert _quality([_cov(8, 66), _cov(0, 0)]) == 1 / 7070                    # above
    assert _quality([_cov(9, 3600)]) == 1.0


def test_tracking_quality_seeded_sweep_and_refusals():
    rng = np.random.default_rng(157)
    for _ in range(300):
        w, h = int(rng.integers(10, 2000)), int(rng.integers(10, 2000))
        kptrad = float(rng.choice([0.0, 0.09, S.KPTRAD, 0.125, 0.5, 1.0]))
        recs = [_cov(int(rng.integers(0, 9)), int(rng.integers(0, (w // 10) * (h // 10) + 1)))
                for _ in range(int(rng.integers(1, 6)))]
        _quality(recs, w, h, kptrad)  # a point larger than the image: a zero or negative union, as in the reference
    for kw in (dict(w=0), dict(h=-1), dict(kptrad=float("nan")), dict(kptrad=-0.1)):
        with pytest.raises(capi.OkvfeError):
            capi.tracking_quality(np.array([_cov(9, 100)]), kw.get("w", 752), kw.get("h", 480), kw.get("kptrad", 0.09))
    for bad in (_cov(-1, 100), _cov(9, -1)):
        with pytest.raises(capi.OkvfeError):
            capi.tracking_quality(np.array([_cov(9, 100), bad]), 752, 480, 0.09)
    with pytest.raises(capi.OkvfeError):
        capi.tracking_quality(np.zeros(0, dtype=capi.COVERAGE_DTYPE), 752, 480, 0.09)


def test_tracking_quality_of_painted_frames():
    """the records a coverage call without a set returns, here from keyframe_ref, give what the literal transcription
    of :157-196 gives on the same frame"""
    rng = np.random.default_rng(196)
    w, h = 752, 480
    for n in (6, 12, 60):
        frame, seen, recs = [], [], []
        for _ in range(2):
            kps = np.zeros(n, dtype=capi.KEYPOINT_DTYPE)
            kps["x"], kps["y"] = rng.uniform(0, w - 0.5, n), rng.uniform(0, h - 0.5, n)
            ids = np.where(rng.random(n) < 0.8, rng.integers(1, 99, n), 0).astype(np.uint64)
            elsewhere = rng.random(n) < 0.7
            frame.append((kps, ids))
            seen.append(elsewhere)
            recs.append(R.coverage(w, h, kps, np.where(elsewhere, ids, 0), None, S.KPTRAD))
        want = OR.tracking_quality(w, h, frame, seen, S.KPTRAD)
        got = capi.tracking_quality(np.array([tuple(r[f] for f in R.COVERAGE_FIELDS) for r in recs],
                                             dtype=capi.COVERAGE_DTYPE), w, h, S.KPTRAD)
        assert _bits(got) == _bits(want), n
    assert want > 0.0


# ---- the scenes of the GPU tests ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.CONFIGS))
def test_scene_floors_and_host_functions_on_the_restated_counts(name):
    cfg, K, mfs, ref = S.reference(name)
    assert R.radius_for(cfg.w, cfg.h, S.KPTRAD) == S.CONFIGS[name][1]
    S.check_floors(name)
    if name == "hilti":
        assert len(cfg.cams) * K > 2048
    pairs = sorted(ref)
    got = capi.overlap_fraction(S.counts_array(ref, pairs))
    assert [_bits(g) for g in got] == [_bits(ref[p]["overlap"]) for p in pairs]
    # the shortcut the kernel takes -- matched iff the id is among the other multiframe's ids -- against the real
    # set intersection of the restatement
    for (a, b) in pairs:
        other = [set(int(v) for _, ids in mfs[m] for v in ids) - {0} for m in (b, a)]
        nm = [sum(1 for _, ids in mfs[m] for v in ids if int(v) in other[f]) for f, m in enumerate((a, b))]
        assert nm == ref[(a, b)]["n_matched"], (a, b)


# ---- binding surface ----------------------------------------------------------------------------------------------
def test_binding_surface():
    assert capi.OVERLAP_COUNTS_DTYPE.itemsize == 32
    assert [capi.OVERLAP_COUNTS_DTYPE.fields[f][1] for f in OR.COUNT_FIELDS] == [0, 8, 16, 24]
    for name in ("okvfe_overlap_pairs_blocks_device", "okvfe_overlap_fraction", "okvfe_motion_frame_order",
                 "okvfe_tracking_quality"):
        assert name in capi.EXPORTS and hasattr(capi.lib(), name), name
    assert hasattr(capi.Frontend, "overlap_pairs_blocks_device")
    makefile = open(os.path.join(ROOT, "okvis2_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bcapi_overlap\.cpp\b", makefile, flags=re.M)
    assert capi.ABI_VERSION == 8 and capi.lib().okvfe_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "okvfe.h")).read()
    assert "#define OKVFE_ABI_VERSION 8" in header
