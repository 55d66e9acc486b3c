"""Reference of okvfe_ransac3d2d_consensus_blocks_device and okvfe_remove_outliers_blocks_device: a plain numpy
restatement, from the reference's sources, of

  the correspondences     okvis_frontend/src/FrameNoncentralAbsoluteAdapter.cpp:101-145
  the distance            okvis_frontend/include/opengv/sac_problems/absolute_pose/FrameAbsolutePoseSacProblem.hpp:140-165
  the verdict             okvis_frontend/src/Frontend.cpp:2226, 2242-2261 (the winner: opengv's Ransac::computeModel as
                          published -- a model replaces the best one only on strictly more inliers, from zero)
  removeOutliers          okvis_frontend/src/Frontend.cpp:2152-2205

Every product, sum, quotient and square root is a separate numpy operation on float64 arrays: IEEE operations without
contraction, so the device must reproduce the results byte for byte.  The 3- and 4-term sums come in both orders
(`tree`: Eigen's x0 + (x1 + x2) and (x0 + x1) + (x2 + x3); else left to right).  The same functions run on
numpy.longdouble arrays: the margin of every (hypothesis, correspondence) verdict.  The camera projection of
removeOutliers is the oracle's (oracle_lib.cam_project; the 8-coefficient model through radtan8_ref.project).

A census counts the branches taken.  Test infrastructure only."""
import numpy as np

import radtan8_ref

SQRT2 = np.array([0x3FF6A09E667F3BCD], dtype=np.uint64).view(np.float64)[0]  # std::sqrt(2) in double
THRESHOLD = 16.0   # Frontend.cpp:2235
MIN_CORR = 10      # Frontend.cpp:2226, 2243
MAX_ERROR = 4.0    # Frontend.cpp:2185

CENSUS = ("no_landmark", "outside_table", "no_observation", "w_below_1e-8", "w_nan", "w_negative", "bp_invalid",
          "bp_zero", "correspondence", "duplicate_landmark", "nan_distance")


def sum3(tree, a, b, c):
    return a + (b + c) if tree else (a + b) + c


def sum4(tree, a, b, c, d):
    return (a + b) + (c + d) if tree else ((a + b) + c) + d


def new_census():
    return dict.fromkeys(CENSUS, 0)


def correspondences(tree, hp_W, obs_begin, frames, landmarks, fus, census=None):
    """frames: per camera dict(kps, bp, bpv) (the gather block's rows below its count); landmarks: per camera int
    array of table rows (-1 = none).  -> dict(cam, row, lm, p [n, 3], b [n, 3], sigma [n]) in the adapter's order."""
    hp_W = np.asarray(hp_W, dtype=np.float64).reshape(-1, 4)
    nl = len(hp_W)
    cam, row, lm = [], [], []
    for c, (fr, rows) in enumerate(zip(frames, landmarks)):
        rows = np.asarray(rows)
        for k in range(len(fr["kps"])):
            l = int(rows[k])
            if l < 0:                                              # :105
                _count(census, "no_landmark")
                continue
            if l >= nl:
                _count(census, "outside_table")
                continue
            if int(obs_begin[l + 1]) - int(obs_begin[l]) < 1:      # :109, without this frame's own observation
                _count(census, "no_observation")
                continue
            w = hp_W[l, 3]
            if np.abs(w) < 1.0e-8:                                 # :116
                _count(census, "w_below_1e-8")
                continue
            if np.isnan(w):
                _count(census, "w_nan")
            elif w < 0:
                _count(census, "w_negative")
            cam.append(c), row.append(k), lm.append(l)
    cam, row, lm = (np.array(v, dtype=np.int64) for v in (cam, row, lm))
    n = len(cam)
    p = np.zeros((n, 3))
    b = np.zeros((n, 3))
    sigma = np.zeros(n)
    with np.errstate(all="ignore"):
        for c, fr in enumerate(frames):
            sel = cam == c
            k = row[sel]
            if not len(k):
                continue
            hp = hp_W[lm[sel]]
            p[sel] = hp[:, :3] / hp[:, 3:4]                        # :120
            s = (0.8 * fr["kps"]["size"][k].astype(np.float64)) / 12.0   # :128
            v = np.asarray(fr["bp"], dtype=np.float64).reshape(-1, 3)[k].copy()
            bad = np.asarray(fr["bpv"])[k] == 0
            v[bad] = (1.0, 0.0, 0.0)                               # :129-132
            fu = np.float64(fus[c])
            sigma[sel] = ((SQRT2 * s) * s) / (fu * fu)             # :135
            z = sum3(tree, v[:, 0] * v[:, 0], v[:, 1] * v[:, 1], v[:, 2] * v[:, 2])   # :137, Eigen's normalize()
            pos = z > 0
            nrm = np.sqrt(z)
            v[pos] = v[pos] / nrm[pos, None]
            b[sel] = v
            if census is not None:
                census["bp_invalid"] += int(bad.sum())
                census["bp_zero"] += int((~pos).sum())
    if census is not None:
        census["correspondence"] += n
        census["duplicate_landmark"] += n - len(set(zip(cam.tolist(), lm.tolist()))) if n else 0
    return dict(cam=cam, row=row, lm=lm, p=p, b=b, sigma=sigma)


def _count(census, key):
    if census is not None:
        census[key] += 1


def distances(tree, H, corr, T_SC, dtype=np.float64):
    """H: [n_hyp, 12] row-major 3 x 4 [R | t]; T_SC: per camera (C, r).  -> [n_hyp, n_corr] in `dtype`."""
    H = np.asarray(H, dtype=np.float64).reshape(-1, 3, 4).astype(dtype)
    nh, n = len(H), len(corr["cam"])
    out = np.zeros((nh, n), dtype=dtype)
    if n == 0:
        return out
    p = corr["p"].astype(dtype)
    b = corr["b"].astype(dtype)
    sigma = corr["sigma"].astype(dtype)
    Csc = np.array([np.asarray(T[0], dtype=np.float64).reshape(3, 3) for T in T_SC]).astype(dtype)[corr["cam"]]
    rsc = np.array([np.asarray(T[1], dtype=np.float64) for T in T_SC]).astype(dtype)[corr["cam"]]
    one = dtype(1.0)
    with np.errstate(all="ignore"):
        for h in range(nh):
            R, t = H[h, :, :3], H[h, :, 3]
            Ri = R.T                                                                       # :142
            ti = [sum3(tree, (-Ri[i, 0]) * t[0], (-Ri[i, 1]) * t[1], (-Ri[i, 2]) * t[2]) for i in range(3)]   # :143
            d = []
            for i in range(3):
                body = sum4(tree, Ri[i, 0] * p[:, 0], Ri[i, 1] * p[:, 1], Ri[i, 2] * p[:, 2], ti[i] * one)  # :155
                d.append(body - rsc[:, i])                                                 # :158
            rep = [sum3(tree, Csc[:, 0, i] * d[0], Csc[:, 1, i] * d[1], Csc[:, 2, i] * d[2]) for i in range(3)]
            nrm = np.sqrt(sum3(tree, rep[0] * rep[0], rep[1] * rep[1], rep[2] * rep[2]))   # :159
            e = [rep[i] / nrm - b[:, i] for i in range(3)]                                 # :162
            out[h] = sum3(tree, e[0] * e[0], e[1] * e[1], e[2] * e[2]) / sigma             # :164-165
    return out


def verdict(counts, valid, n_corr):
    """-> (best_hypothesis, n_inliers, accepted)"""
    if n_corr < MIN_CORR:                                          # Frontend.cpp:2226
        return -1, 0, 0
    best, most = -1, 0
    for h, (c, v) in enumerate(zip(counts, valid)):
        if v and c > most:
            best, most = h, int(c)
    acc = most >= MIN_CORR and np.float64(most) / np.float64(n_corr) > 0.7   # Frontend.cpp:2243
    return best, most, int(acc)


def consensus(tree, hp_W, obs_begin, frames, landmarks, fus, T_SC, H, valid=None, threshold=THRESHOLD,
              remove_outliers=True, census=None):
    """One multiframe.  -> dict: n_corr, best, n_inliers, accepted, hyp_inliers [n_hyp]; per camera: state [count] u8,
    distance [count] (NaN-free only where dist_set), dist_set [count] bool, landmark_out [count]; dist [n_hyp, n_corr]."""
    H = np.asarray(H, dtype=np.float64).reshape(-1, 12)
    nh = len(H)
    valid = np.ones(nh, dtype=bool) if valid is None else np.asarray(valid) != 0
    corr = correspondences(tree, hp_W, obs_begin, frames, landmarks, fus, census)
    n = len(corr["cam"])
    dist = distances(tree, H, corr, T_SC)
    with np.errstate(all="ignore"):
        inl = dist < threshold                                     # a NaN is an outlier
    scored = n >= MIN_CORR
    counts = inl.sum(axis=1)
    best, most, acc = verdict(counts, valid, n)
    hyp_inliers = np.where(valid & scored, counts, -1).astype(np.int32)
    if census is not None and n:
        census["nan_distance"] += int(np.isnan(dist[0]).sum())
    out = dict(n_corr=n, best=best, n_inliers=most, accepted=acc, hyp_inliers=hyp_inliers, corr=corr, dist=dist,
               state=[], distance=[], dist_set=[], landmark_out=[])
    for c, (fr, rows) in enumerate(zip(frames, landmarks)):
        cnt = len(fr["kps"])
        st = np.zeros(cnt, np.uint8)
        dd = np.zeros(cnt, np.float64)
        ds = np.zeros(cnt, bool)
        lo = np.asarray(rows[:cnt], dtype=np.int32).copy()
        sel = corr["cam"] == c
        k = corr["row"][sel]
        st[k] = 1
        if best >= 0:
            st[k] = np.where(inl[best][sel], 2, 1)
            dd[k] = dist[best][sel]
            ds[k] = True
        if acc and remove_outliers:
            lo[st == 1] = -1                                       # Frontend.cpp:2245-2260
        out["state"].append(st), out["distance"].append(dd), out["dist_set"].append(ds), out["landmark_out"].append(lo)
    return out


def margins(tree, H, corr, T_SC, threshold=THRESHOLD):
    """(verdicts in float64, verdicts in longdouble, relative margin of the longdouble distance to the threshold)"""
    d64 = distances(tree, H, corr, T_SC)
    dld = distances(tree, H, corr, T_SC, dtype=np.longdouble)
    with np.errstate(all="ignore"):
        margin = np.abs(dld - np.longdouble(threshold)) / np.longdouble(threshold)
        return d64 < threshold, dld < np.longdouble(threshold), margin


# ---- removeOutliers --------------------------------------------------------------------------------------------
REMOVE_CENSUS = ("no_landmark", "outside_table", "w_negative", "successful", "outside_left", "outside_top",
                 "outside_right", "outside_bottom", "behind", "invalid_z", "invalid_distortion", "too_far", "kept",
                 "nan_norm")


def project(oracle, cam, head):
    """(status, pixel): 0 Successful, 1 OutsideImage, 3 Behind, 4 Invalid"""
    if cam.dist_type == 3:
        st, pt, _ = radtan8_ref.project(cam, np.asarray(head, dtype=np.float64))
        return int(st), np.asarray(pt, dtype=np.float64)
    st, pt, _ = oracle.cam_project(cam, head)
    return int(st), pt


def pose_inverse_times(tree, T, hp):
    """hp_C = T^-1 hp in the expression order of the first pass (k_map.hip, pose_inverse_times)"""
    C, r = np.asarray(T[0], dtype=np.float64).reshape(-1), np.asarray(T[1], dtype=np.float64)
    hp = np.asarray(hp, dtype=np.float64)
    out = np.zeros(4)
    with np.errstate(all="ignore"):
        for i in range(3):
            cr = sum3(tree, C[i] * r[0], C[3 + i] * r[1], C[6 + i] * r[2])
            hh = sum3(tree, C[i] * hp[0], C[3 + i] * hp[1], C[6 + i] * hp[2])
            out[i] = hh + (-cr) * hp[3]
    out[3] = hp[3]
    return out


def remove_outliers(oracle, tree, hp_W, kps, landmark, cam, T_WC, max_error=MAX_ERROR, census=None):
    """One frame.  -> (landmark_out [count] int32, kept)"""
    hp_W = np.asarray(hp_W, dtype=np.float64).reshape(-1, 4)
    out = np.asarray(landmark[:len(kps)], dtype=np.int32).copy()
    kept = 0
    for k in range(len(kps)):
        l = int(out[k])
        if l < 0:                                                  # :2171
            _count(census, "no_landmark")
            continue
        if l >= len(hp_W):                                         # :2177
            _count(census, "outside_table")
            continue
        hp_C = pose_inverse_times(tree, T_WC, hp_W[l])             # :2180
        if hp_C[3] < 0:                                            # projectHomogeneous
            _count(census, "w_negative")
            head = -hp_C[:3]
        else:
            head = hp_C[:3]
        st, proj = project(oracle, cam, head)
        remove = True
        if st == 0:                                                # :2183
            _count(census, "successful")
            with np.errstate(all="ignore"):
                dx = proj[0] - np.float64(kps["x"][k])
                dy = proj[1] - np.float64(kps["y"][k])
                nrm = np.sqrt(dx * dx + dy * dy)
                remove = bool(nrm > max_error)                     # :2185
            if np.isnan(nrm):
                _count(census, "nan_norm")
            if remove:
                _count(census, "too_far")
        elif census is not None:
            if st == 3:
                census["behind"] += 1
            elif st == 4:
                census["invalid_z" if abs(head[2]) < 1.0e-12 else "invalid_distortion"] += 1
            else:
                side = ("outside_left" if proj[0] < 0 else "outside_top" if proj[1] < 0 else
                        "outside_right" if proj[0] >= cam.w else "outside_bottom")
                census[side] += 1
        if remove:
            out[k] = -1
        else:
            kept += 1
            _count(census, "kept")
    return out, kept
