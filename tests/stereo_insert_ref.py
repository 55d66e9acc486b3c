"""The landmark bookkeeping of Frontend::matchStereo (okvis_frontend/src/Frontend.cpp:2076-2141) restated line by line
for one multiframe, as the reference runs it: camera pairs in list order, k0 ascending, every row seeing what the rows
before it wrote.  Landmarks live in a dict (id -> [point, initialised, re-set in this call]), the ids in one list per
camera.  The projection chain is ransac_ref.py's (pose_inverse_times, project).  This is what
okvfe_stereo_insert_blocks_device is compared with, byte for byte; it also counts which branches a scene reaches."""
import numpy as np

import ransac_ref as R

REINIT, CREATE, OBS0, OBS1 = 1, 2, 4, 8
MAX_DISTANCE = 4.0  # :2122, :2135

CENSUS = ("both_reinit", "both_initialised", "both_not_initialisable", "only_id1", "only_id0", "neither_keyframe",
          "neither_not_keyframe", "add0_accepted", "add0_status", "add0_distance", "add0_nan", "add1_accepted",
          "add1_status", "add1_distance", "add1_nan", "read_id_same_pair", "read_id_earlier_pair", "read_point_reset",
          "read_point_created")


def new_census():
    return {k: 0 for k in CENSUS}


def _count(census, key):
    if census is not None:
        census[key] += 1


def stereo_insert(oracle, tree, hp_W, initialised, cams, pairs, K, kps, ids_in, T_WC, matches, keyframe=True,
                  census=None):
    """One multiframe.  hp_W [L, 4], initialised [L]: the table.  cams / kps / ids_in / T_WC: per camera of the rig the
    synth.Camera, the keypoints, the landmark ids they carry (table rows, -1 none; anything outside [-1, L) is read as
    none) and the pose (C, r).  pairs: (c0, c1) in the reference's order; matches[p]: the stereo matcher's rows of pair p
    (k1, initialisable, hp_W), one per keypoint of c0.  K: the row capacity, which numbers the created landmarks
    (L + p K + k0).
    -> dict(action=[per pair uint8], lm=[per pair int32], ids=[per camera int32], counts=[matched, created,
    re-initialised, observations])"""
    hp_W = np.asarray(hp_W, dtype=np.float64).reshape(-1, 4)
    L = len(hp_W)
    ids = [[int(v) if 0 <= int(v) < L else -1 for v in row] for row in ids_in]
    writer = [[None] * len(row) for row in ids_in]  # the pair that set an id in this call
    landmarks = {}

    def landmark(v):  # estimator.getLandmark / isLandmarkInitialised on the multiframe's view
        if v not in landmarks:
            landmarks[v] = [hp_W[v].copy(), bool(initialised[v]), False]
        return landmarks[v]

    def observable(which, p, c, k, lm, created_here):  # :2117-2122 / :2130-2135
        point, _, reset = landmark(lm)
        if reset:
            _count(census, "read_point_reset")
        if lm >= L and not created_here:
            _count(census, "read_point_created")
        hp_C = R.pose_inverse_times(tree, T_WC[c], point)
        head = -hp_C[:3] if hp_C[3] < 0 else hp_C[:3]  # projectHomogeneous
        st, proj = R.project(oracle, cams[c], head)
        if st != 0:
            _count(census, which + "_status")
            return False
        with np.errstate(all="ignore"):
            dx = np.float64(kps[c]["x"][k]) - proj[0]
            dy = np.float64(kps[c]["y"][k]) - proj[1]
            nrm = np.sqrt(dx * dx + dy * dy)
        if np.isnan(nrm):
            _count(census, which + "_nan")
            return False
        if not nrm < MAX_DISTANCE:
            _count(census, which + "_distance")
            return False
        _count(census, which + "_accepted")
        return True

    actions, lms = [], []
    counts = [0, 0, 0, 0]
    for p, (c0, c1) in enumerate(pairs):
        n0, n1 = len(kps[c0]), len(kps[c1])
        action = np.zeros(n0, np.uint8)
        lm_out = np.full(n0, -1, np.int32)
        rows = matches[p]
        for k0 in range(n0):
            k1 = int(rows["k1"][k0])
            if k1 < 0 or k1 >= n1:                                   # :2076
                continue
            counts[0] += 1
            id0, id1 = ids[c0][k0], ids[c1][k1]                      # :2081-2082 ("may change!!")
            for w in (writer[c0][k0], writer[c1][k1]):
                if w is not None:
                    _count(census, "read_id_same_pair" if w == p else "read_id_earlier_pair")
            initialisable = int(rows["initialisable"][k0]) != 0
            hps_W = np.array(rows["hp_W"][k0], dtype=np.float64)
            add0 = add1 = created = False
            a = 0
            if id0 >= 0 and id1 >= 0:                                # :2085
                lm = id0
                rec = landmark(id0)
                if not rec[1]:                                       # :2086
                    if initialisable:                                # :2088
                        rec[0], rec[1], rec[2] = hps_W, True, True   # setLandmark(id0, hps_W, true)
                        a |= REINIT
                        counts[2] += 1
                        _count(census, "both_reinit")
                    else:
                        _count(census, "both_not_initialisable")
                else:
                    _count(census, "both_initialised")
            elif id1 >= 0:                                           # :2093
                lm, add0 = id1, True
                _count(census, "only_id1")
            elif id0 >= 0:                                           # :2098
                lm, add1 = id0, True
                _count(census, "only_id0")
            else:
                if not keyframe:                                     # :2103
                    _count(census, "neither_not_keyframe")
                    continue
                _count(census, "neither_keyframe")
                lm = L + p * K + k0                                  # addLandmark(hps_W, initialisable)
                landmarks[lm] = [hps_W, initialisable, False]
                add0 = add1 = created = True
                a |= CREATE
                counts[1] += 1
            if add0 and observable("add0", p, c0, k0, lm, created):  # :2115
                ids[c0][k0] = lm
                writer[c0][k0] = p
                a |= OBS0
                counts[3] += 1
            if add1 and observable("add1", p, c1, k1, lm, created):  # :2128
                ids[c1][k1] = lm
                writer[c1][k1] = p
                a |= OBS1
                counts[3] += 1
            action[k0] = a
            lm_out[k0] = lm
        actions.append(action)
        lms.append(lm_out)
    return dict(action=actions, lm=lms, ids=[np.array(r, dtype=np.int32) for r in ids],
                counts=np.array(counts, dtype=np.int32))
