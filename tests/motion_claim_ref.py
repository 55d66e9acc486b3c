"""Reference for the frame-data part of Frontend::matchMotionStereo's insertion loop (Frontend.cpp:1915-1958) and for
the sweep over older frames built on it (:1773-1959), as okvfe_match_motion_stereo_blocks_batch_device restates them.
CPU only: numpy plus the CPU oracle's orc_match_motion_stereo.

    claim_loop     the literal transcription: a sequential loop over k0
    claim_closed   the closed form the kernel computes: per free k1 the smallest candidate k0
    contested_scene / sweep_scene / sweep_chain    the scenes of the tests and the reference chain over them

What the loop leaves out is estimator state: the re-checks of :1923-1933 (a skipped k0 carries k1 == -1, so they add
nothing here) and the landmark bookkeeping of :1940-1956, of which only "the current keypoint now carries a landmark"
(:1954) feeds back into the frame data."""
from __future__ import annotations

import dataclasses

import numpy as np

import gate_scenes as S
import oracle_lib as O


def claim_loop(rows, count0, matched1):
    """:1915-1958 on one pair's match rows.  rows: structured array with k1 and accepted (at least count0 rows);
    matched1: uint8 flags of the CURRENT frame ("landmarkId(im, k1) != 0") or None = all free.
    -> (claimed uint8[count0], n_claimed, matched1 after the loop -- a copy; None stays None)"""
    claimed = np.zeros(count0, dtype=np.uint8)
    taken = None if matched1 is None else np.array(matched1, dtype=np.uint8, copy=True)
    seen = set()  # with matched1 None the loop still hands a k1 out once (multiFrame1->setLandmarkId, :1954)
    ret_ctr = 0
    for k0 in range(count0):                      # :1916
        k1 = int(rows["k1"][k0])
        if k1 < 0 or not rows["accepted"][k0]:    # :1919 (mInfo.matching is set at :1903 only)
            continue
        if taken is not None:                     # :1935-1938
            if taken[k1]:
                continue
        elif k1 in seen:
            continue
        if taken is not None:                     # :1954
            taken[k1] = 1
        seen.add(k1)
        claimed[k0] = 1
        ret_ctr += 1                              # :1957
    return claimed, ret_ctr, taken


def claim_closed(rows, count0, matched1):
    """the same verdicts without the loop: for each free k1 the candidate with the smallest k0 wins"""
    k1 = np.asarray(rows["k1"][:count0], dtype=np.int64)
    cand = (k1 >= 0) & (np.asarray(rows["accepted"][:count0]) != 0)
    if matched1 is not None:
        m = np.asarray(matched1)
        cand &= m[np.where(cand, k1, 0)] == 0
    claimed = np.zeros(count0, dtype=np.uint8)
    k0s = np.flatnonzero(cand)
    if len(k0s):
        _, first = np.unique(k1[k0s], return_index=True)  # (k0s ascending: the first occurrence is the smallest k0)
        claimed[k0s[first]] = 1
    taken = None if matched1 is None else np.array(matched1, dtype=np.uint8, copy=True)
    if taken is not None:
        taken[k1[claimed != 0]] = 1
    return claimed, int(claimed.sum()), taken


def with_frame_size(cam, w, h):
    """the camera as a context of frame size w x h sees it (the projection's image bounds are the context's)"""
    return dataclasses.replace(cam, w=w, h=h)


def contested_scene(kind, n0=300, n1=300, seed=0, dup=0.25, **kw):
    """gate_scenes.pair_scene with a share `dup` of the older frame's rows replaced by copies of other rows of it
    (descriptor, keypoint and ray), so that two k0 choose one k1.  A copy inherits everything but its skip0 flag."""
    sc = S.pair_scene(kind, n0, n1, seed=seed, **kw)
    rng = np.random.default_rng([seed, 77, n0, n1])
    n_dup = int(round(dup * n0))
    if n_dup and n0 > 1:
        dst = rng.choice(n0, n_dup, replace=False)
        keep = np.setdiff1d(np.arange(n0), dst)
        src = rng.choice(keep, n_dup, replace=True)
        for k in ("d0", "kp0", "bp0", "bv0"):
            sc[k] = sc[k].copy()
            sc[k][dst] = sc[k][src]
    sc["name"] += "-dup"
    return sc


def match_rows(sc, skip0, matched1, cam=None):
    """the oracle's rows of a scene under the given flags"""
    return O.match_motion_stereo(sc["d0"], sc["kp0"], sc["bp0"], sc["bv0"], skip0, sc["d1"], sc["kp1"], sc["bp1"],
                                 sc["bv1"], matched1, sc["T0"], sc["T1"], cam or sc.get("oracle_cam", sc["cam"]),
                                 S.THRESHOLD)


def contest_stats(rows, matched1):
    """(contested free k1, uncontested claims, rows with k1 >= 0 and accepted == 0) of one pair"""
    cand = (rows["k1"] >= 0) & (rows["accepted"] != 0)
    if matched1 is not None:
        cand &= np.asarray(matched1)[np.where(cand, rows["k1"], 0)] == 0
    _, counts = np.unique(rows["k1"][cand], return_counts=True)
    return int((counts > 1).sum()), int((counts == 1).sum()), int(((rows["k1"] >= 0) & (rows["accepted"] == 0)).sum())


def older_view(sc, rng, share=0.7, dup=0.25):
    """another older frame of the same current frame: a random subset of the scene's older rows in random order, a
    quarter of them duplicated, with skip0 flags of its own -> dict with d0, kp0, bp0, bv0, skip0"""
    n0 = len(sc["kp0"])
    pick = rng.permutation(n0)[:max(1, int(share * n0))]
    n_dup = int(round(dup * len(pick)))
    if n_dup:
        pick = np.concatenate([pick, rng.choice(pick, n_dup, replace=True)])
        pick = pick[rng.permutation(len(pick))]
    return dict(d0=sc["d0"][pick], kp0=sc["kp0"][pick], bp0=sc["bp0"][pick], bv0=sc["bv0"][pick],
                skip0=(rng.random(len(pick)) < 0.1).astype(np.uint8))


def sweep_scene(cams, kinds, n_current=4, steps=3, n0=140, n1=160, seed=5):
    """A sweep: n_current current multiframes x len(cams) cameras = the current blocks (block c * len(cams) + m), and
    per step one older frame for each of them.  cams[m]: the camera of slot m (replaces the scene's own: the rays are
    re-derived by pair_scene only for its own camera, so a kind is used with the camera it was made for);
    kinds[m]: the pair_scene kind observed through camera m.
    -> dict(current=[scene per current block], older=[step][current block] -> older_view, matched1=[block] uint8)"""
    rng = np.random.default_rng([seed, 99])
    current, older = [], [[] for _ in range(steps)]
    for c in range(n_current):
        for m in range(len(cams)):
            sc = S.pair_scene(kinds[m], n0 + 7 * c, n1 + 5 * c + m, seed=seed + c)
            assert sc["cam"] == cams[m], "a scene kind goes with the camera it was observed through"
            current.append(sc)
            for j in range(steps):
                older[j].append(older_view(sc, rng))
    matched1 = [sc["matched1"].copy() for sc in current]
    return dict(current=current, older=older, matched1=matched1, n_cams=len(cams))


def sweep_chain(sw, cam_of=None):
    """The reference chain over a sweep_scene: per step and current block the oracle's rows under the matched1 flags
    the earlier steps left, then the insertion loop.  cam_of(scene) -> the oracle's camera (default: the scene's).
    -> (steps: [step][block] -> dict(rows, claimed, n_claimed), final matched1 per block)"""
    matched1 = [m.copy() for m in sw["matched1"]]
    out = []
    for step in sw["older"]:
        res = []
        for b, (sc, old) in enumerate(zip(sw["current"], step)):
            pair = dict(sc, **{k: old[k] for k in ("d0", "kp0", "bp0", "bv0")})
            rows = match_rows(pair, old["skip0"], matched1[b], cam_of(sc) if cam_of else None)
            claimed, n, matched1[b] = claim_loop(rows, len(rows), matched1[b])
            res.append(dict(rows=rows, claimed=claimed, n_claimed=n))
        out.append(res)
    return out, matched1
