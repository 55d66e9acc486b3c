"""numpy restatement of Frontend::doWeNeedANewKeyframe (okvis_frontend/src/Frontend.cpp:1058-1167) for the tests.

Written from the cited lines, deliberately the slow way: real u8 masks, one cv::circle per keypoint, explicit
`&` / `|` / count -- NOT the dilation-of-centres shortcut and not the bit rows the kernel uses.

PARITY UNPINNED for the part that is not in the reference tree: cv::circle and the Point2f -> Point conversion are
restated from OpenCV's published source (imgproc/src/drawing.cpp, Circle(); core/types.hpp, Point_<float> * double
and the rounding Point_<int> conversion, cvRound = round half to even).  No OpenCV is available to compare with.
"""
import numpy as np

KPTRAD = 0.09  # Frontend.cpp:104
OVERLAP_THRESHOLD = np.float32(0.55)  # keyframeInsertionOverlapThreshold_, Frontend.cpp:145

COVERAGE_FIELDS = ("n_keypoints", "n_matched", "detections_area", "matches_area", "intersection_area", "union_area")


def mask_shape(w, h):
    return h // 10, w // 10  # :1075-1076 (rows, cols)


def radius_for(w, h, kptrad=KPTRAD):
    rows, cols = mask_shape(w, h)
    return int(float(min(rows, cols)) * kptrad)  # :1083, int(radius) at :1087


def centre(v):
    """One coordinate of cv::Point(keypoint.pt * 0.1): float(double(v) * 0.1), then cvRound (half to even)."""
    return int(np.rint(np.float32(np.float64(np.float32(v)) * 0.1)))


def circle_spans(r):
    """The (row offset, half-width) spans OpenCV's filled integer midpoint circle emits, in emission order."""
    spans = []
    err, dx, dy, plus, minus = 0, r, 0, 1, 2 * r - 1
    while dx >= dy:
        spans.append((dy, dx))   # rows cy +- dy: [cx - dx, cx + dx]
        spans.append((dx, dy))   # rows cy +- dx: [cx - dy, cx + dy]
        dy += 1
        err += plus
        plus += 2
        if err > 0:
            err -= minus
            dx -= 1
            minus -= 2
    return spans


def stencil(r):
    """Half-width per row offset |j| = 0..r: the widest of the spans that land on that row."""
    hw = [0] * (r + 1)
    for j, half in circle_spans(r):
        hw[j] = max(hw[j], half)
    return hw


def circle(mask, cx, cy, r):
    """cv::circle(mask, (cx, cy), r, 255, cv::FILLED): every emitted span, clipped to the mask."""
    rows, cols = mask.shape
    for j, half in circle_spans(r):
        x0, x1 = max(cx - half, 0), min(cx + half, cols - 1)
        if x0 > x1:
            continue
        for y in (cy - j, cy + j):
            if 0 <= y < rows:
                mask[y, x0:x1 + 1] = 255


def masks(w, h, keypoints, landmark_ids, id_set=None, kptrad=KPTRAD):
    """(detections, matches) of one camera image, u8.  id_set None: :1089; else :1138."""
    rows, cols = mask_shape(w, h)
    r = radius_for(w, h, kptrad)
    detections = np.zeros((rows, cols), np.uint8)
    matches = np.zeros((rows, cols), np.uint8)
    s = None if id_set is None else set(int(v) for v in id_set)
    n_matched = 0
    for k in range(len(keypoints)):
        cx, cy = centre(keypoints["x"][k]), centre(keypoints["y"][k])
        circle(detections, cx, cy, r)
        lm = int(landmark_ids[k])
        if lm != 0 and (s is None or lm in s):
            circle(matches, cx, cy, r)
            n_matched += 1
    return detections, matches, n_matched


def coverage(w, h, keypoints, landmark_ids, id_set=None, kptrad=KPTRAD):
    """The six counts of one image as a dict (field names of okvfe_coverage)."""
    detections, matches, n_matched = masks(w, h, keypoints, landmark_ids, id_set, kptrad)
    return {"n_keypoints": len(keypoints), "n_matched": n_matched,
            "detections_area": int(np.count_nonzero(detections)), "matches_area": int(np.count_nonzero(matches)),
            "intersection_area": int(np.count_nonzero(matches & detections)),
            "union_area": int(np.count_nonzero(matches | detections))}


def _div(a, b):
    """double(a) / double(b) with IEEE results for b == 0 (Python raises instead)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def _std_max(a, b):
    return b if a < b else a  # std::max(a, b): a unless a < b


def _std_min(a, b):
    return b if b < a else a  # std::min(a, b): a unless b < a


def decision(current, others, threshold=OVERLAP_THRESHOLD):
    """:1103, :1116-1166.  current: records (dicts) of the current multiframe's cameras; others: list of such
    lists.  Returns (need_keyframe, overlap) with overlap the value after :1154."""
    intersection = sum(c["intersection_area"] for c in current)
    union = sum(c["union_area"] for c in current)
    num_keypoints = sum(c["n_keypoints"] for c in current)
    overlap = _div(intersection, union)
    overlap_others = 0.0
    for frame in others:
        i = sum(c["intersection_area"] for c in frame)
        u = sum(c["union_area"] for c in frame)
        overlap_others = _std_max(overlap_others, _div(i, u))
    overlap = _std_min(overlap_others, overlap)
    if num_keypoints < 7 * len(current):
        return False, overlap
    if np.float32(overlap) > np.float32(threshold):
        return False, overlap
    return True, overlap
