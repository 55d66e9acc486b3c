"""numpy restatement of ViSlamBackend::overlapFraction (okvis_ceres/src/ViSlamBackend.cpp:2341-2427),
ViSlamBackend::trackingQuality (:157-196) and the ordering in front of the motion-stereo sweep
(okvis_frontend/src/Frontend.cpp:1742-1767) for the tests.

A literal transcription, the slow way: real u8 masks painted with keyframe_ref's circle, Python sets of landmark ids
per multiframe, a real set intersection, `matches.count(id)` as a membership test in THAT intersection, and a sort of
(overlap, id) tuples.  It does NOT use the "id is among the other side's ids" shortcut of the kernel: the tests are
what justify that shortcut.

A multiframe is a list with one (keypoints, landmark_ids) per camera: a KEYPOINT_DTYPE array and a u64 array of the
same length.  PARITY UNPINNED for cv::circle and the point rounding, as in keyframe_ref.py."""
import math

import numpy as np

import keyframe_ref as R

UNIFORMITY_RADIUS = 38.0  # okvis2 configuration files (detection: uniformity_radius)

COUNT_FIELDS = ("n_keypoints", "n_matched", "intersection_area", "union_area")


def backend_kptrad(uniformity_radius=UNIFORMITY_RADIUS):
    return 0.09 * uniformity_radius / 36.0  # ViSlamBackend.hpp:209


def _paint(mask, kp_x, kp_y, r):
    # cv::circle(mask, keypoint.pt * 0.1, int(radius), 255, cv::FILLED).  A non-finite coordinate saturates in the
    # conversion to int (INT_MIN) and the disc is clipped away entirely: nothing is painted
    if not (np.isfinite(kp_x) and np.isfinite(kp_y)):
        return
    R.circle(mask, R.centre(kp_x), R.centre(kp_y), r)


def set_intersection(a, b):
    """std::set_intersection of two ascending ranges."""
    out, i, j = [], 0, 0
    while i < len(a) and j < len(b):
        if a[i] < b[j]:
            i += 1
        elif b[j] < a[i]:
            j += 1
        else:
            out.append(a[i])
            i += 1
            j += 1
    return out


def overlap_masks(w, h, frame_a, frame_b, kptrad):
    """:2349-2408.  Returns (landmarks, matches, detectionsImg, matchesImg, n_matched): detectionsImg[f][im] and
    matchesImg[f][im] are u8 masks, n_matched[f][im] the number of circles painted into matchesImg[f][im]."""
    assert len(frame_a) == len(frame_b), "must be same number of frames"  # :2344
    frames = (frame_a, frame_b)
    num_frames = len(frame_a)
    landmarks = (set(), set())
    detections_img = ([None] * num_frames, [None] * num_frames)
    matches_img = ([None] * num_frames, [None] * num_frames)
    n_matched = ([0] * num_frames, [0] * num_frames)
    rows, cols = R.mask_shape(w, h)                       # :2361-2362
    radius = float(min(rows, cols)) * kptrad              # :2363
    # paint detection images and remember matched points
    for f in range(2):
        for im in range(num_frames):
            detections_img[f][im] = np.zeros((rows, cols), np.uint8)
            matches_img[f][im] = np.zeros((rows, cols), np.uint8)
            kps, ids = frames[f][im]
            for k in range(len(kps)):
                _paint(detections_img[f][im], kps["x"][k], kps["y"][k], int(radius))  # :2370
                lm_id = int(ids[k])
                if lm_id != 0:
                    landmarks[f].add(lm_id)               # :2374
    # find matches: std::set_intersection of the two ordered sets
    matches = set(set_intersection(sorted(landmarks[0]), sorted(landmarks[1])))  # :2381-2384
    # without matches there will be no overlap
    if len(matches) == 0:
        return landmarks, matches, detections_img, matches_img, n_matched
    # draw match images
    for f in range(2):
        for im in range(num_frames):
            kps, ids = frames[f][im]
            for k in range(len(kps)):
                if int(ids[k]) in matches:                # :2402 matches.count(...)
                    _paint(matches_img[f][im], kps["x"][k], kps["y"][k], int(radius))
                    n_matched[f][im] += 1
    return landmarks, matches, detections_img, matches_img, n_matched


def overlap_counts(w, h, frame_a, frame_b, kptrad):
    """The integer counts of one ordered pair, as a dict of [side A, side B] lists (fields of okvfe_overlap_counts),
    plus "per_image": per side and camera the six fields of okvfe_coverage, and "overlap": the double the function
    returns (:2386-2389, :2410-2426), from the same masks."""
    frames = (frame_a, frame_b)
    _, matches, det, mat, nm = overlap_masks(w, h, frame_a, frame_b, kptrad)
    out = {name: [0, 0] for name in COUNT_FIELDS}
    out["overlap"] = _iou(matches, det, mat)
    per_image = ([], [])
    for f in range(2):
        for im in range(len(frame_a)):
            c = {"n_keypoints": len(frames[f][im][0]), "n_matched": nm[f][im],
                 "detections_area": int(np.count_nonzero(det[f][im])), "matches_area": int(np.count_nonzero(mat[f][im])),
                 "intersection_area": int(np.count_nonzero(mat[f][im] & det[f][im])),   # :2418, :2420
                 "union_area": int(np.count_nonzero(mat[f][im] | det[f][im]))}          # :2419, :2421
            per_image[f].append(c)
            for name in COUNT_FIELDS:
                out[name][f] += c[name]
    out["per_image"] = per_image
    return out


def overlap_fraction(w, h, frame_a, frame_b, kptrad):
    """:2341-2427, the returned double."""
    _, matches, det, mat, _ = overlap_masks(w, h, frame_a, frame_b, kptrad)
    return _iou(matches, det, mat)


def _iou(matches, det, mat):
    if len(matches) == 0:
        return 0.0                                        # :2387-2389
    overlap = [0.0, 0.0]
    for f in range(2):
        intersection_count = 0
        union_count = 0
        for im in range(len(det[f])):
            intersection_count += int(np.count_nonzero(mat[f][im] & det[f][im]))
            union_count += int(np.count_nonzero(mat[f][im] | det[f][im]))
        overlap[f] = R._div(intersection_count, union_count)  # :2423
    return R._std_min(overlap[0], overlap[1])             # :2426


def overlap_from_counts(c):
    """:2386-2389, :2410-2426 from a counts dict (what okvfe_overlap_fraction restates)."""
    if c["n_matched"][0] == 0 and c["n_matched"][1] == 0:
        return 0.0
    o = [R._div(c["intersection_area"][f], c["union_area"][f]) for f in range(2)]
    return R._std_min(o[0], o[1])


def motion_frame_order(overlaps, frame_ids, previous):
    """Frontend.cpp:1751-1767.  overlaps[i]: overlapFraction(previous frame, frame i); previous: index or -1.  Returns
    the indices of matchFrameIds in order.  (No NaN: std::sort is undefined there.)"""
    pairs = []
    index_of = {}
    for i, fid in enumerate(frame_ids):
        index_of[int(fid)] = i
        if i == previous:
            pairs.append((1.0, int(fid)))                 # :1753-1755
            continue
        pairs.append((float(overlaps[i]), int(fid)))      # :1759
    assert len(index_of) == len(pairs), "allFrames is a set"
    assert not any(math.isnan(p[0]) for p in pairs)
    pairs.sort()                                          # :1761
    match_frame_ids = []
    for i in range(len(pairs)):
        if pairs[len(pairs) - i - 1][0] <= 1.0e-8:        # :1765
            break
        match_frame_ids.append(pairs[len(pairs) - i - 1][1])
    return [index_of[fid] for fid in match_frame_ids]


def point_area(w, h, kptrad):
    rows, cols = R.mask_shape(w, h)
    radius = float(min(rows, cols)) * kptrad              # :171, a double
    return int(radius * radius * math.pi)                 # :191


def tracking_quality_from_records(records, w, h, kptrad):
    """:190-195 from per-image records with n_matched and matches_area."""
    rows, cols = R.mask_shape(w, h)
    pa = point_area(w, h, kptrad)
    intersection_count = 0
    union_count = 0
    matched_points = 0
    for c in records:
        matched_points += int(c["n_matched"])
        intersection_count += max(0, int(c["matches_area"]) - pa)
        union_count += rows * cols - pa
    return 0.0 if matched_points < 8 else R._div(intersection_count, union_count)


def tracking_quality(w, h, frame, observed_elsewhere, kptrad):
    """:157-196.  frame: one (keypoints, landmark_ids) per camera; observed_elsewhere: per camera one bool per
    keypoint, the outcome of :178-187 (landmark exists and has an observation in another frame)."""
    rows, cols = R.mask_shape(w, h)
    radius = float(min(rows, cols)) * kptrad
    intersection_count = 0
    union_count = 0
    matched_points = 0
    for im in range(len(frame)):
        matches_img = np.zeros((rows, cols), np.uint8)
        kps, ids = frame[im]
        for k in range(len(kps)):
            if int(ids[k]) != 0 and observed_elsewhere[im][k]:
                matched_points += 1
                _paint(matches_img, kps["x"][k], kps["y"][k], int(radius))
        pa = int(radius * radius * math.pi)
        intersection_count += max(0, int(np.count_nonzero(matches_img)) - pa)
        union_count += rows * cols - pa
    return 0.0 if matched_points < 8 else R._div(intersection_count, union_count)
