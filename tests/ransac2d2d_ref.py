"""Reference of okvfe_ransac2d2d_consensus_blocks_device: a plain numpy restatement, from the reference's sources, of

  the correspondences     okvis_frontend/src/FrameRelativeAdapter.cpp:137-194 (a dict for the std::map)
  the rotation distance   okvis_frontend/include/opengv/sac_problems/relative_pose/FrameRotationOnlySacProblem.hpp:126-144
  the relative distance   .../FrameRelativePoseSacProblem.hpp:130-160, with opengv::triangulation::triangulate2 and
                          Eigen's 2 x 2 inverse as published (neither is in the reference tree)
  the winners             opengv's Ransac::computeModel as published: strictly more inliers, from zero
  the decision            okvis_frontend/src/Frontend.cpp:2293-2392 (numpy.float32 for the two ratios)

Every product, sum, quotient and square root is a separate numpy operation on float64 arrays: IEEE operations without
contraction, so the device must reproduce the results byte for byte.  The 3- and 4-term sums come in both orders
(`tree`: Eigen's x0 + (x1 + x2) and (x0 + x1) + (x2 + x3); else left to right).  The same functions run on
numpy.longdouble arrays: the margin of every (hypothesis, correspondence) verdict.

A census counts the branches taken.  Test infrastructure only."""
import numpy as np

from ransac_ref import SQRT2, sum3, sum4

THRESHOLD = 9.0    # Frontend.cpp:2312, 2329
MIN_CORR = 10      # Frontend.cpp:2300

CENSUS = ("no_id_1", "not_added", "outside_added_table", "duplicate_id_in_current", "no_id_0", "id_not_in_map",
          "two_older_on_one_landmark", "bp_invalid_0", "bp_invalid_1", "parallel_bearings", "nan_distance",
          "branch_skipped", "branch_rotation_by_ratio", "branch_rotation_by_0.8", "branch_relative",
          "sticky_removal", "no_winner", "removed_row", "shared_kB_mixed")


def new_census():
    return dict.fromkeys(CENSUS, 0)


def _count(census, key, n=1):
    if census is not None:
        census[key] += int(n)


def _normalized(tree, v):
    """Eigen's normalize(): z = squaredNorm, divided by sqrt(z) iff z > 0"""
    v = np.array(v, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        z = sum3(tree, v[:, 0] * v[:, 0], v[:, 1] * v[:, 1], v[:, 2] * v[:, 2])
        pos = z > 0
        n = np.sqrt(z)
        v[pos] = v[pos] / n[pos, None]
    return v


def correspondences(tree, fr0, fr1, fu, added=None, census=None):
    """fr0 / fr1: the older / current block's rows below its count, dict(kps, bp, bpv, lm); added: bytes per landmark id
    or None.  -> dict(kA, kB, b1 [n, 3], b2 [n, 3], s1 [n], s2 [n]) in the adapter's order."""
    id_map = {}
    for k, lm in enumerate(np.asarray(fr1["lm"]).tolist()):                # :139
        if lm < 0:                                                         # :143
            _count(census, "no_id_1")
            continue
        if added is not None:                                              # :147
            if lm >= len(added):
                _count(census, "outside_added_table")
                continue
            if not added[lm]:
                _count(census, "not_added")
                continue
        if lm in id_map:                                                   # :151: insert does not overwrite
            _count(census, "duplicate_id_in_current")
            continue
        id_map[lm] = k
    kA, kB = [], []
    for k, lm in enumerate(np.asarray(fr0["lm"]).tolist()):                # :154
        if lm < 0:                                                         # :157
            _count(census, "no_id_0")
            continue
        if lm not in id_map:                                               # :160
            _count(census, "id_not_in_map")
            continue
        kA.append(k), kB.append(id_map[lm])
    kA, kB = np.array(kA, dtype=np.int64), np.array(kB, dtype=np.int64)
    n = len(kA)
    _count(census, "two_older_on_one_landmark", n - len(set(kB.tolist())))
    fu = np.float64(fu)
    sa = (0.8 * fr0["kps"]["size"][kA].astype(np.float64)) / 12.0          # :175
    sb = (0.8 * fr1["kps"]["size"][kB].astype(np.float64)) / 12.0          # :186
    s1 = ((SQRT2 * sa) * sa) / (fu * fu)                                   # :176
    s2 = ((SQRT2 * sb) * sb) / (fu * fu)                                   # :187
    bad0 = np.asarray(fr0["bpv"])[kA] == 0
    bad1 = np.asarray(fr1["bpv"])[kB] == 0
    v = np.asarray(fr0["bp"], dtype=np.float64).reshape(-1, 3)[kA].copy()
    v[bad0 | bad1] = (1.0, 0.0, 0.0)                                       # :179, and :190 writes bearingVectors1_
    b1 = _normalized(tree, v)                                              # :182
    b2 = _normalized(tree, np.asarray(fr1["bp"], dtype=np.float64).reshape(-1, 3)[kB])   # :193, the stored value
    _count(census, "bp_invalid_0", bad0.sum())
    _count(census, "bp_invalid_1", bad1.sum())
    return dict(kA=kA, kB=kB, b1=b1, b2=b2, s1=s1, s2=s2)


def _score(tree, e1, e2, s1, s2, dtype):
    q1 = sum3(tree, e1[0] * e1[0], e1[1] * e1[1], e1[2] * e1[2])
    q2 = sum3(tree, e2[0] * e2[0], e2[1] * e2[1], e2[2] * e2[2])
    return (q1 * dtype(0.5)) / s1 + (q2 * dtype(0.5)) / s2


def rotation_distances(tree, Ms, corr, dtype=np.float64):
    """Ms: [n_hyp, 9] row-major rotations.  -> [n_hyp, n_corr] in `dtype`"""
    Ms = np.asarray(Ms, dtype=np.float64).reshape(-1, 3, 3).astype(dtype)
    n = len(corr["kA"])
    out = np.zeros((len(Ms), n), dtype=dtype)
    if n == 0:
        return out
    b1, b2 = corr["b1"].astype(dtype).T, corr["b2"].astype(dtype).T
    s1, s2 = corr["s1"].astype(dtype), corr["s2"].astype(dtype)
    with np.errstate(all="ignore"):
        for h, M in enumerate(Ms):
            f2u = [sum3(tree, M[i, 0] * b2[0], M[i, 1] * b2[1], M[i, 2] * b2[2]) for i in range(3)]   # :131
            f1u = [sum3(tree, M[0, i] * b1[0], M[1, i] * b1[1], M[2, i] * b1[2]) for i in range(3)]   # :134
            e1 = [f2u[i] - b1[i] for i in range(3)]                                                   # :136
            e2 = [f1u[i] - b2[i] for i in range(3)]                                                   # :137
            out[h] = _score(tree, e1, e2, s1, s2, dtype)                                              # :140-143
    return out


def relative_distances(tree, Hs, corr, dtype=np.float64, census=None):
    """Hs: [n_hyp, 12] row-major [R12 | t12].  -> [n_hyp, n_corr] in `dtype`"""
    Hs = np.asarray(Hs, dtype=np.float64).reshape(-1, 3, 4).astype(dtype)
    n = len(corr["kA"])
    out = np.zeros((len(Hs), n), dtype=dtype)
    if n == 0:
        return out
    b1, b2 = corr["b1"].astype(dtype).T, corr["b2"].astype(dtype).T
    s1, s2 = corr["s1"].astype(dtype), corr["s2"].astype(dtype)
    one, two = dtype(1.0), dtype(2.0)
    dot = lambda a, b: sum3(tree, a[0] * b[0], a[1] * b[1], a[2] * b[2])
    with np.errstate(all="ignore"):
        for h, H in enumerate(Hs):
            R, t = H[:, :3], H[:, 3]
            ti = [sum3(tree, (-R[0, i]) * t[0], (-R[1, i]) * t[1], (-R[2, i]) * t[2]) for i in range(3)]   # :137
            # triangulate2
            f2u = [sum3(tree, R[i, 0] * b2[0], R[i, 1] * b2[1], R[i, 2] * b2[2]) for i in range(3)]
            c0, c1 = dot(t, b1), dot(t, f2u)
            A00, A10 = dot(b1, b1), dot(b1, f2u)
            A01, A11 = -A10, -dot(f2u, f2u)
            det = A00 * A11 - A10 * A01
            invdet = one / det
            I00, I10, I01, I11 = A11 * invdet, (-A10) * invdet, (-A01) * invdet, A00 * invdet
            l0, l1 = I00 * c0 + I01 * c1, I10 * c0 + I11 * c1
            p = [(l0 * b1[i] + (t[i] + l1 * f2u[i])) / two for i in range(3)]
            rep2 = [sum4(tree, R[0, i] * p[0], R[1, i] * p[1], R[2, i] * p[2], ti[i] * one) for i in range(3)]   # :146
            n1, n2 = np.sqrt(dot(p, p)), np.sqrt(dot(rep2, rep2))                                           # :147-148
            e1 = [p[i] / n1 - b1[i] for i in range(3)]                                                      # :153
            e2 = [rep2[i] / n2 - b2[i] for i in range(3)]                                                   # :154
            out[h] = _score(tree, e1, e2, s1, s2, dtype)                                                    # :157-160
            _count(census, "parallel_bearings", (det == 0).sum())
    return out


def winner(counts, valid):
    best, most = -1, 0
    for h, (c, v) in enumerate(zip(counts, valid)):
        if v and c > most:
            best, most = h, int(c)
    return best, most


def _valid(valid, nh):
    return np.ones(nh, dtype=bool) if valid is None else np.asarray(valid) != 0


def run(tree, cameras, fus, threshold=THRESHOLD, remove_outliers=True, added=None, census=None):
    """One pair.  cameras: per camera dict(fr0, fr1, rot_H [nh, 9], rot_valid, rel_H [nh, 12], rel_valid).  -> dict:
    total_inliers, rotation_only, success; cams: per camera dict(n_corr, rot_best, rot_inliers, rel_best, rel_inliers,
    branch, removed, rot_hyp_inliers, rel_hyp_inliers, match1 [count0], state [count0], distance [count0], dist_set,
    landmark1_out [count1], corr, rot_dist, rel_dist)."""
    total, rotation_only, success = 0, 0, 0
    out = []
    for cam, fu in zip(cameras, fus):                                      # :2293
        fr0, fr1 = cam["fr0"], cam["fr1"]
        corr = correspondences(tree, fr0, fr1, fu, added, census)
        n = len(corr["kA"])
        nh = len(cam["rot_H"])
        vr, vl = _valid(cam.get("rot_valid"), nh), _valid(cam.get("rel_valid"), nh)
        dr = rotation_distances(tree, cam["rot_H"], corr)
        dl = relative_distances(tree, cam["rel_H"], corr, census=census)
        with np.errstate(all="ignore"):
            ir, il = dr < threshold, dl < threshold                        # a NaN is an outlier
        _count(census, "nan_distance", np.isnan(dr).sum() + np.isnan(dl).sum())
        scored = n >= MIN_CORR                                             # :2300
        rot_best, rot_most, rel_best, rel_most = -1, 0, -1, 0
        branch, removed, taken, inl = 0, 0, -1, np.zeros(n, dtype=bool)
        dist = None
        if scored:
            rot_best, rot_most = winner(ir.sum(axis=1), vr)
            rel_best, rel_most = winner(il.sum(axis=1), vl)
            rot_ratio = np.float32(rot_most) / np.float32(n)               # :2320
            rel_ratio = np.float32(rel_most) / np.float32(n)               # :2337
            if rot_ratio > rel_ratio or rot_ratio > np.float32(0.8):       # :2341
                _count(census, "branch_rotation_by_ratio" if rot_ratio > rel_ratio else "branch_rotation_by_0.8")
                branch = 1
                if rot_most > 10:
                    success |= 1
                rotation_only = 1
                total += rot_most
                taken = rot_best
                if taken >= 0:
                    inl, dist = ir[taken], dr[taken]
            else:
                _count(census, "branch_relative")
                branch = 2
                if rel_most > 10 and rel_ratio > np.float32(0.8):          # :2351
                    success |= 2
                total += rel_most
                taken = rel_best
                if taken >= 0:
                    inl, dist = il[taken], dl[taken]
            removed = int(success != 0)                                    # :2361
            if taken < 0:
                _count(census, "no_winner")
            if removed and not ((branch == 1 and rot_most > 10) or (branch == 2 and rel_most > 10 and rel_ratio > np.float32(0.8))):
                _count(census, "sticky_removal")
        else:
            _count(census, "branch_skipped")
        c0, c1 = len(fr0["kps"]), len(fr1["kps"])
        match1 = np.full(c0, -1, np.int32)
        state = np.zeros(c0, np.uint8)
        dd = np.zeros(c0, np.float64)
        ds = np.zeros(c0, bool)
        match1[corr["kA"]] = corr["kB"]
        state[corr["kA"]] = np.where(inl, 2, 1)
        if dist is not None:
            dd[corr["kA"]] = dist
            ds[corr["kA"]] = True
        lo = np.asarray(fr1["lm"][:c1], dtype=np.int32).copy()
        if removed and remove_outliers:                                    # :2365-2375
            bad = set(corr["kB"][~inl].tolist())
            lo[sorted(bad)] = -1
            _count(census, "removed_row", len(bad))
            _count(census, "shared_kB_mixed", len(bad & set(corr["kB"][inl].tolist())))
        out.append(dict(n_corr=n, rot_best=rot_best, rot_inliers=rot_most, rel_best=rel_best, rel_inliers=rel_most,
                        branch=branch, removed=removed,
                        rot_hyp_inliers=np.where(vr & scored, ir.sum(axis=1), -1).astype(np.int32),
                        rel_hyp_inliers=np.where(vl & scored, il.sum(axis=1), -1).astype(np.int32),
                        match1=match1, state=state, distance=dd, dist_set=ds, landmark1_out=lo, corr=corr,
                        rot_dist=dr, rel_dist=dl))
    ok = success != 0                                                      # :2387-2392
    return dict(total_inliers=total if ok else -1, rotation_only=rotation_only if ok else 1, success=success, cams=out)


def margins(tree, rot_H, rel_H, corr, threshold=THRESHOLD):
    """(verdicts in float64, verdicts in longdouble, relative margin of the longdouble distance to the threshold), the
    rotation-only hypotheses stacked on the relative ones"""
    d64 = np.concatenate([rotation_distances(tree, rot_H, corr), relative_distances(tree, rel_H, corr)])
    dld = np.concatenate([rotation_distances(tree, rot_H, corr, dtype=np.longdouble),
                          relative_distances(tree, rel_H, corr, dtype=np.longdouble)])
    with np.errstate(all="ignore"):
        margin = np.abs(dld - np.longdouble(threshold)) / np.longdouble(threshold)
        return d64 < threshold, dld < np.longdouble(threshold), margin
