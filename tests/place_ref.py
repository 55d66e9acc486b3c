"""Reference of okvfe_place_landmark_set, okvfe_place_claims_blocks_device and okvfe_place_consensus_blocks_device: a
literal transcription, in the reference's loop order and with Python dicts standing for its std::maps, of

  the landmark set        okvis_frontend/src/Frontend.cpp:289-327
  the claims              okvis_frontend/src/Frontend.cpp:330-355 (after the descriptor loops: k_min / dist_min are inputs)
  the gates               okvis_frontend/src/Frontend.cpp:359, 380
  the adapter             okvis_frontend/src/LoopclosureNoncentralAbsoluteAdapter.cpp:69-154
  the verdict             okvis_frontend/src/Frontend.cpp:389, the inlier flags :393-397

The arithmetic of a correspondence (point, bearing, sigma), the distances and the winner rule are ransac_ref's: the
loop-closure adapter computes what FrameNoncentralAbsoluteAdapter computes, without the test on the observations, and
FrameAbsolutePoseSacProblem accepts both adapters.  A census counts what the transcription meets.  Test infrastructure
only."""
import numpy as np

import ransac_ref as R

THRESHOLD = 16.0     # Frontend.cpp:382
ITERATIONS = 50      # Frontend.cpp:383
MIN_POINTS = 8       # Frontend.cpp:359
MIN_CORR = 7         # Frontend.cpp:380
MIN_RATIO = 0.7      # Frontend.cpp:389

SET_CENSUS = ("id_zero", "not_initialised", "norm_zero", "norm_tiny", "norm_below_edge", "norm_at_edge", "norm_nan",
              "two_cameras", "twice_one_camera", "first_filtered_later_kept", "different_hp_first_wins", "kept")
CLAIM_CENSUS = ("no_hit", "hit_one_camera", "hit_several_cameras", "collision_2", "collision_3", "collision_all",
                "loser_counted", "empty_block", "k_min_outside", "w_below_1e-8", "w_nan", "w_negative", "claimed")


def new_census(keys):
    return dict.fromkeys(keys, 0)


def _count(census, key, n=1):
    if census is not None:
        census[key] += n


def norm4(tree, x):
    """Eigen's Vector4d::norm(): the square root of the four-term sum of squares, in either order"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.sqrt(R.sum4(tree, x[0] * x[0], x[1] * x[1], x[2] * x[2], x[3] * x[3]))


def landmark_set(tree, old, census=None):
    """old: per camera dict(ids [n] u64, hp [n, 4], init [n] u8, desc [n, 48]).
    -> dict(ids [L] u64, hp [L, 4], desc_begin [L + 1] i32, pool [rows, 48]) in ascending id."""
    descriptors, landmarks = {}, {}
    filtered, cams_of, first_cam_count = set(), {}, {}
    for im, fr in enumerate(old):                                  # :289
        for k_old in range(len(fr["ids"])):                        # :290
            lm_id = int(fr["ids"][k_old])
            if lm_id == 0:                                         # :292
                _count(census, "id_zero")
                continue
            landmark = np.asarray(fr["hp"][k_old], dtype=np.float64)
            if not fr["init"][k_old]:                              # :300
                _count(census, "not_initialised")
                filtered.add(lm_id)
                continue
            n = norm4(tree, landmark)
            if n < 1.0e-12:                                        # :302
                _count(census, "norm_zero" if n == 0 else "norm_tiny" if n < 5.0e-13 else "norm_below_edge")
                filtered.add(lm_id)
                continue
            if np.isnan(n):
                _count(census, "norm_nan")
            elif n < 2.0e-12:
                _count(census, "norm_at_edge")
            _count(census, "kept")
            if lm_id in descriptors:                               # :319
                descriptors[lm_id].append(fr["desc"][k_old])       # :321
                if census is not None:
                    if im not in cams_of[lm_id]:
                        census["two_cameras"] += 1
                    else:
                        census["twice_one_camera"] += 1
                    if not np.array_equal(landmarks[lm_id].view(np.uint64), landmark.view(np.uint64)):
                        census["different_hp_first_wins"] += 1
                cams_of[lm_id].add(im)
            else:
                descriptors[lm_id] = [fr["desc"][k_old]]           # :323
                landmarks[lm_id] = landmark.copy()                 # :324
                cams_of[lm_id] = {im}
                if lm_id in filtered:
                    _count(census, "first_filtered_later_kept")
    ids = sorted(landmarks)                                        # the std::map's order (:330)
    desc_begin = np.zeros(len(ids) + 1, np.int32)
    pool = []
    for l, lm_id in enumerate(ids):
        pool.extend(descriptors[lm_id])
        desc_begin[l + 1] = len(pool)
    return dict(ids=np.array(ids, dtype=np.uint64), hp=np.array([landmarks[i] for i in ids], dtype=np.float64).reshape(-1, 4),
                desc_begin=desc_begin, pool=np.array(pool, dtype=np.uint8).reshape(-1, 48))


def claims(hp, counts, k_min, dist_min, threshold, census=None):
    """One multiframe.  hp [L, 4]; counts: keypoints per camera; k_min / dist_min: per camera [L], what the descriptor
    loops of :337-346 leave per landmark row.  -> (ctr, points {row: hp}, matches {(im, k): row})"""
    ctr, points, matches = 0, {}, {}
    claimed_by = {}
    for row in range(len(hp)):                                     # :330, rows = ascending landmark ids
        hits = 0
        for im in range(len(counts)):                              # :331
            if counts[im] == 0:                                    # :332
                _count(census, "empty_block")
                continue
            dist, k = int(dist_min[im][row]), int(k_min[im][row])
            if dist < threshold:                                   # :347
                if not 0 <= k < counts[im]:                        # (the matcher cannot produce one: ignored)
                    _count(census, "k_min_outside")
                    continue
                ctr += 1                                           # :348
                points[row] = hp[row]                              # :349
                matches[(im, k)] = row                             # :350: the last writer keeps the keypoint
                claimed_by.setdefault((im, k), []).append(row)
                hits += 1
        _count(census, "no_hit" if hits == 0 else "hit_one_camera" if hits == 1 else "hit_several_cameras")
    if census is not None:
        for rows in claimed_by.values():
            if len(rows) == 2:
                census["collision_2"] += 1
            elif len(rows) == 3:
                census["collision_3"] += 1
            elif len(rows) == len(hp) and len(rows) > 3:
                census["collision_all"] += 1
            census["loser_counted"] += len(rows) - 1
    return ctr, points, matches


def adapter(points, matches, counts, census=None):
    """LoopclosureNoncentralAbsoluteAdapter's constructor.  -> per camera int array [count]: the row of the landmark whose
    correspondence keypoint k becomes, -1 = none; in its order (camera-major, keypoints ascending)"""
    out = []
    for im in range(len(counts)):                                  # :76
        rows = np.full(counts[im], -1, np.int32)
        for k in range(counts[im]):                                # :112
            if (im, k) not in matches:                             # :114
                continue
            row = matches[(im, k)]
            hp = points[row]                                       # :123
            _count(census, "claimed")
            if np.abs(hp[3]) < 1.0e-8:                             # :126
                _count(census, "w_below_1e-8")
                continue
            if np.isnan(hp[3]):
                _count(census, "w_nan")
            elif hp[3] < 0:
                _count(census, "w_negative")
            rows[k] = row
        out.append(rows)
    return out


def gate(ctr, n_points, n_corr, min_inliers):
    if ctr < min_inliers or n_points < MIN_POINTS:                 # :359
        return 0
    if n_corr < MIN_CORR:                                          # :380
        return 1
    return 2


def claim_stage(hp, counts, k_min, dist_min, threshold, min_inliers, census=None):
    """what okvfe_place_claims_blocks_device writes for one multiframe"""
    hp = np.asarray(hp, dtype=np.float64).reshape(-1, 4)
    ctr, points, matches = claims(hp, counts, k_min, dist_min, threshold, census)
    match_landmark = [np.full(n, -1, np.int32) for n in counts]
    for (im, k), row in matches.items():
        match_landmark[im][k] = row
    corr_rows = adapter(points, matches, counts, census)           # (the count is written whatever the gate says)
    n_corr = sum(int((r >= 0).sum()) for r in corr_rows)
    return dict(n_matches=ctr, n_points=len(points), n_corr=n_corr, gate=gate(ctr, len(points), n_corr, min_inliers),
                match_landmark=match_landmark)


def consensus(tree, hp, frames, match_landmark, fus, T_SC, H, valid=None, gate_in=None, min_inliers=10,
              threshold=THRESHOLD):
    """what okvfe_place_consensus_blocks_device writes for one multiframe.  frames: per camera dict(kps, bp, bpv);
    match_landmark: per camera rows [count] (-1 = none); gate_in: the caller's gate or None."""
    hp = np.asarray(hp, dtype=np.float64).reshape(-1, 4)
    H = np.asarray(H, dtype=np.float64).reshape(-1, 12)
    nh = len(H)
    valid = np.ones(nh, dtype=bool) if valid is None else np.asarray(valid) != 0
    # the adapter over the `matches` map these rows stand for
    counts = [len(f["kps"]) for f in frames]
    matches = {(im, k): int(r) for im, rows in enumerate(match_landmark) for k, r in enumerate(rows[:counts[im]])
               if 0 <= r < len(hp)}
    points = {r: hp[r] for r in matches.values()}
    rows = adapter(points, matches, counts)
    corr = R.correspondences(tree, hp, np.arange(len(hp) + 1), frames, rows, fus)
    assert [np.flatnonzero(r >= 0).tolist() for r in rows] == [corr["row"][corr["cam"] == c].tolist() for c in range(len(frames))]
    n = len(corr["cam"])
    out = dict(n_corr=n, best=-1, n_inliers=0, accepted=0, hyp_inliers=np.full(nh, -1, np.int32), corr=corr)
    inl = None
    if gate_in is not None and gate_in == 0:                       # :359
        out["verdict"] = 0
    elif n < MIN_CORR:                                             # :380
        out["verdict"] = 1
    else:
        dist = R.distances(tree, H, corr, T_SC)
        with np.errstate(all="ignore"):
            inl = dist < threshold
        counts_h = inl.sum(axis=1)
        # ransac_ref's winner rule (its own floor of ten correspondences is not this call's)
        best, most, _ = R.verdict(counts_h, valid, max(n, R.MIN_CORR))
        ratio = np.float64(most) / np.float64(n)
        out.update(best=best, n_inliers=most, hyp_inliers=np.where(valid, counts_h, -1).astype(np.int32), dist=dist)
        out["verdict"] = 2 if most < min_inliers or ratio < MIN_RATIO else 3   # :389
    out["accepted"] = int(out["verdict"] == 3)
    out.update(state=[], distance=[], dist_set=[], landmark_out=[])
    for c, fr in enumerate(frames):
        cnt = counts[c]
        st, dd, ds = np.zeros(cnt, np.uint8), np.zeros(cnt, np.float64), np.zeros(cnt, bool)
        lo = np.asarray(match_landmark[c][:cnt], dtype=np.int32).copy()
        sel = corr["cam"] == c
        k = corr["row"][sel]
        st[k] = 1
        if out["best"] >= 0:
            st[k] = np.where(inl[out["best"]][sel], 2, 1)          # :393-397
            dd[k] = out["dist"][out["best"]][sel]
            ds[k] = True
        if out["accepted"]:
            lo[st == 1] = -1
        out["state"].append(st), out["distance"].append(dd), out["dist_set"].append(ds), out["landmark_out"].append(lo)
    return out


def verify(tree, hp, frames, k_min, dist_min, match_threshold, fus, T_SC, H, valid=None, min_inliers=10,
           threshold=THRESHOLD, census=None):
    """:330-397 for one multiframe, as the reference runs it: (claim_stage's dict, consensus' dict with the claims' gate)"""
    counts = [len(f["kps"]) for f in frames]
    cl = claim_stage(hp, counts, k_min, dist_min, match_threshold, min_inliers, census)
    co = consensus(tree, hp, frames, cl["match_landmark"], fus, T_SC, H, valid, cl["gate"], min_inliers, threshold)
    assert co["n_corr"] == cl["n_corr"] and (co["verdict"] >= 2) == (cl["gate"] == 2)
    return cl, co
