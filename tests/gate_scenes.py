"""Scenes that drive the four gated matchers (matchStereo, matchMotionStereo, matchToMap,
matchToMapUninitialised) into every branch of their FP64 gate chain, and onto the knife edges of
the gates.  CPU only and seeded: everything here is numpy plus the CPU oracle; the GPU tier
(test_gpu_gate_census.py) and the CPU tier (test_gate_scenes_host.py) consume the same arrays.

    python tests/gate_scenes.py            census (label x matcher) over all scenes
    python tests/gate_scenes.py far        census of the scenes whose name contains "far"

A pair scene is a dict with the arrays of both images (desc, kp, bp, bv per side), the poses, the
focal lengths of the stereo call, the camera of the motion-stereo call and its skip0 / matched1
flags.  Descriptors are lightly perturbed copies of a dozen cluster centres, so most rows hold many
candidates under the Hamming threshold, most of them geometrically wrong; a share of image-1 rows
are exact copies of another row of their cluster (exact Hamming ties with different geometry), and
a few pairs sit at exactly threshold - 1 and threshold.
"""
from __future__ import annotations

import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:  # (run as a script: the package lives one level up)
    sys.path.insert(0, _ROOT)

import oracle_lib as O
from okvis2_amd import synth

THRESHOLD = 60  # the front-end's Hamming threshold in every shipped configuration
N_CLUSTERS = 12
PAIR_KINDS = ("identical", "rot01", "rot075", "base004", "base0099", "base0101", "far", "near",
              "general", "tumvi", "euroc")
# n1: 4 segments, 64-descriptor chunks, resident up to 256; n0: lanes of one 64-wide block
N1_SIZES = (0, 1, 3, 4, 5, 255, 256, 257, 260, 1500)
N0_SIZES = (1, 63, 64, 65)


def rodrigues(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def layer_size(octave):
    """keypoint size of a scale-space layer: 12 * scale(octave) (1, 1.5, 2, 3, ...)"""
    return 12.0 * ((3 << ((octave - 1) // 2)) / 2.0 if octave & 1 else float(1 << (octave // 2)))


def _flip_bits(row, bits):
    row = row.copy()
    for b in bits:
        row[b >> 3] ^= np.uint8(1 << (b & 7))
    return row


def _project(cam, p3):
    """(status, pixel): the oracle's projection; the 8-coefficient model, which the oracle does not carry,
    through its restatement tests/radtan8_ref.py"""
    if cam.dist_type == 3:
        import radtan8_ref
        st, pt, _ = radtan8_ref.project(cam, np.asarray(p3, dtype=np.float64)[None])
        return int(st[0]), pt[0]
    st, pt, _ = O.cam_project(cam, p3)
    return st, pt


def _backproject_keypoints(cam, kp):
    if cam.dist_type == 3:
        import radtan8_ref
        return radtan8_ref.backproject_keypoints(cam, kp)
    return O.backproject_keypoints(cam, kp)


def _pixels_to_points(cam, T, px, rng_range):
    """world points on the rays of pixels px (n, 2) of a camera at pose T, at the given ranges"""
    C, r = np.asarray(T[0]).reshape(3, 3), np.asarray(T[1])
    X = np.zeros((len(px), 3))
    kp = np.zeros(len(px), dtype=O.KEYPOINT_DTYPE)
    kp["x"], kp["y"] = px[:, 0], px[:, 1]
    dirs, valid = _backproject_keypoints(cam, kp)
    for i, p in enumerate(px):
        ok, d = bool(valid[i]), dirs[i]
        d = d / np.linalg.norm(d) if ok and np.linalg.norm(d) > 0 else np.array([0.0, 0.0, 1.0])
        X[i] = C @ (d * rng_range[i]) + r
    return X


def observe(cam, T, X, rng, noise, sizes_mixed=False):
    """keypoints of world points X seen from pose T; a point that does not project lands on a
    random pixel (clutter).  Returns (kp, bp, bv)."""
    C, r = np.asarray(T[0]).reshape(3, 3), np.asarray(T[1])
    Xc = (X - r) @ C
    n = len(X)
    kp = np.zeros(n, dtype=O.KEYPOINT_DTYPE)
    for i in range(n):
        st, pt = _project(cam, Xc[i])
        if st != 0:
            pt = (rng.uniform(2, cam.w - 2), rng.uniform(2, cam.h - 2))
        kp["x"][i], kp["y"][i] = pt
    if noise > 0:
        kp["x"] += rng.normal(0, noise, n).astype(np.float32)
        kp["y"] += rng.normal(0, noise, n).astype(np.float32)
    octave = rng.integers(0, 4, n) if sizes_mixed else np.zeros(n, dtype=np.int64)
    kp["octave"] = octave
    kp["size"] = [layer_size(int(o)) for o in octave]
    bp, bv = _backproject_keypoints(cam, kp) if n else (np.zeros((0, 3)), np.zeros(0, np.uint8))
    return kp, np.array(bp, dtype=np.float64), np.array(bv, dtype=np.uint8)


def _pair_geometry(kind):
    """(cam, T0, T1, (range_lo, range_hi), noise) of a pair scene"""
    cam = synth.euroc_config().cams[0]
    eye = np.eye(3)
    T0 = (eye.reshape(-1), np.zeros(3))
    rng_lo, rng_hi, noise = 2.0, 12.0, 0.3
    if kind == "identical":
        T0 = (rodrigues((0.3, -0.5, 0.8), 0.4).reshape(-1), np.array([0.7, -0.2, 0.1]))
        T1, noise = T0, 0.0
    elif kind == "rot01":
        T1 = (rodrigues((0.2, 1.0, 0.1), 0.1).reshape(-1), np.zeros(3))
    elif kind == "rot075":
        T1 = (rodrigues((0.1, 1.0, -0.2), 0.75).reshape(-1), np.zeros(3))
    elif kind == "base004":
        # up to 1.5 m and 0.1 px of noise (3e-4 rad over both rays): the rays of a true pair meet at more than
        # 2e-3 rad, which keeps hp_W of the plain triangulation within binary64's reach of 1e-9 (see "far")
        T1 = (eye.reshape(-1), np.array([0.004, 0.0, 0.0]))
        rng_lo, rng_hi, noise = 0.05, 1.5, 0.1
    elif kind == "base0099":
        T1 = (rodrigues((0, 1, 0), 0.01).reshape(-1), np.array([0.0099, 0.0, 0.0]))
        rng_lo, rng_hi, noise = 0.3, 10.0, 0.1  # (true pairs meet at >= 1e-3 rad; noise 3e-4: see "far")
    elif kind == "base0101":
        T1 = (rodrigues((0, 1, 0), 0.01).reshape(-1), np.array([0.0101, 0.0, 0.0]))
        rng_lo, rng_hi, noise = 0.3, 10.0, 0.1
    elif kind == "far":
        # 0.6 m and 0.05 px of noise (1.5e-4 rad over both rays): at 600 m the rays of a true pair still meet
        # at more than 5e-4 rad.  The triangulated point's condition is about 1 / sin^2 of that angle, so
        # binary64 (2^-53) keeps hp_W to a few 1e-10 relative: the longdouble restatement is compared at 1e-9,
        # which no arithmetic in binary64 can carry below ~3e-4 rad.  Every pair is still parallel by
        # cos 6 sigma (0.02 rad).
        T1 = (eye.reshape(-1), np.array([0.6, 0.0, 0.0]))
        rng_lo, rng_hi, noise = 30.0, 600.0, 0.05
    elif kind == "near":
        T1 = (rodrigues((0, 1, 0), -0.1).reshape(-1), np.array([0.11, 0.01, 0.0]))
        rng_lo, rng_hi = 0.12, 0.6
    elif kind == "general":
        C0 = rodrigues((0.5, -0.7, 0.4), 1.1)
        T0 = (C0.reshape(-1), np.array([3.0, -1.5, 0.8]))
        C1 = C0 @ rodrigues((0.6, 0.5, -0.6), 0.22)
        T1 = (C1.reshape(-1), T0[1] + C0 @ np.array([0.3, -0.05, 0.08]))
    elif kind == "tumvi":
        cam = synth.tumvi1024_config().cams[0]
        C0 = rodrigues((0.2, 0.3, 0.9), 0.5)
        T0 = (C0.reshape(-1), np.array([-1.0, 0.5, 0.2]))
        C1 = C0 @ rodrigues((0.1, 1.0, 0.2), 0.35)
        T1 = (C1.reshape(-1), T0[1] + C0 @ np.array([0.25, 0.02, 0.1]))
        rng_lo, rng_hi = 0.3, 8.0
    elif kind == "euroc":
        T1 = (rodrigues((0, 0, 1), 0.05).reshape(-1), np.array([0.35, 0.04, 0.02]))
    else:
        raise ValueError(kind)
    return cam, T0, T1, (rng_lo, rng_hi), noise


def pair_scene(kind, n0=300, n1=300, seed=0, mixed=False, invalid=0.0, nan_rays=0, radtan8=False):
    """One stereo / motion-stereo scene.  kind: see PAIR_KINDS.  mixed: octaves 0 .. 3 with sizes
    12 * scale(octave); invalid: share of back-projections flagged invalid on either side;
    nan_rays: number of zero-length back-projection vectors flagged VALID per side (NaN rays);
    radtan8: the 8-coefficient camera instead of the scene's own (observed through tests/radtan8_ref.py; the
    oracle's motion-stereo loop then runs with "oracle_cam", the same focal lengths without a distortion:
    its gates use fu and fv only, and its 4 px verdict is not the camera's -- see radtan8_accepted)."""
    rng = np.random.default_rng([seed, PAIR_KINDS.index(kind), n0, n1])
    cam, T0, T1, (lo, hi), noise = _pair_geometry(kind)
    if radtan8:
        cam = synth.radtan8_config().cams[0]
    N = max(n0, n1, 1)
    px = np.stack([rng.uniform(3, cam.w - 3, N), rng.uniform(3, cam.h - 3, N)], 1)
    X = _pixels_to_points(cam, T0, px, np.exp(rng.uniform(np.log(lo), np.log(hi), N)))
    kp0, bp0, bv0 = observe(cam, T0, X[:n0], rng, noise, mixed)
    if kind == "identical":
        m = min(n0, n1)
        kp1e, bp1e, bv1e = observe(cam, T1, X[m:n1], rng, noise, mixed)
        kp1 = np.concatenate([kp0[:m], kp1e])
        bp1 = np.concatenate([bp0[:m], bp1e]) if n1 else np.zeros((0, 3))
        bv1 = np.concatenate([bv0[:m], bv1e])
    else:
        kp1, bp1, bv1 = observe(cam, T1, X[:n1], rng, noise, mixed)
    cl = rng.integers(0, N_CLUSTERS, N)
    centres = rng.integers(0, 256, (N_CLUSTERS, 48), dtype=np.uint8)

    def perturbed(n):
        out = np.empty((n, 48), dtype=np.uint8)
        for i in range(n):
            out[i] = _flip_bits(centres[cl[i]], rng.choice(384, int(rng.integers(2, 11)), replace=False))
        return out

    d0, d1 = perturbed(n0), perturbed(n1)
    # exact ties: image-1 rows that copy another row of their cluster (different geometry, equal distance)
    for j in range(n1):
        if rng.random() < 0.15:
            same = np.flatnonzero(cl[:n1] == cl[j])
            d1[j] = d1[int(rng.choice(same))]
    # pairs at exactly THRESHOLD - 1 and THRESHOLD: fresh descriptors outside the clusters
    m = min(n0, n1)
    if m >= 16:
        for t, i in enumerate(range(3, 11)):
            d0[i] = rng.integers(0, 256, 48, dtype=np.uint8)
            d1[i] = _flip_bits(d0[i], rng.choice(384, THRESHOLD - 1 + (t & 1), replace=False))
    if invalid > 0:
        bv0[rng.random(n0) < invalid] = 0
        bv1[rng.random(n1) < invalid] = 0
    for side_bp, side_bv, n in ((bp0, bv0, n0), (bp1, bv1, n1)):
        for i in rng.choice(n, min(nan_rays, n), replace=False) if n else ():
            side_bp[i] = 0.0
            side_bv[i] = 1
    perm = rng.permutation(n1)
    d1, kp1, bp1, bv1 = d1[perm], kp1[perm], bp1[perm], bv1[perm]
    f0 = 0.5 * (cam.fu + cam.fv)
    f1 = f0 * 0.9976 if not mixed else f0 * 0.71  # f0 != f1; strongly so where the size classes mix
    name = f"{kind}-{n0}x{n1}" + ("-mixed" if mixed else "") + ("-invalid" if invalid else "") + \
        ("-nan" if nan_rays else "") + ("-radtan8" if radtan8 else "") + (f"-s{seed}" if seed else "")
    extra = {}
    if radtan8:
        import dataclasses
        extra["oracle_cam"] = dataclasses.replace(cam, dist_type=0, d=(0.0, 0.0, 0.0, 0.0))
    return dict(extra, name=name, kind=kind, cam=cam, d0=d0, kp0=kp0, bp0=bp0, bv0=bv0, d1=d1, kp1=kp1,
                bp1=bp1, bv1=bv1, T0=T0, T1=T1, f0=f0, f1=f1, mixed=mixed,
                skip0=(rng.random(n0) < 0.1).astype(np.uint8),
                matched1=(rng.random(n1) < 0.1).astype(np.uint8))


def _pair_specs():
    """every geometry at the base size with the input classes mixed in, then the size partitions"""
    out = []
    for i, kind in enumerate(PAIR_KINDS):
        out.append((kind, 300, 300, dict(mixed=i % 2 == 1, invalid=0.1 if i % 3 == 0 else 0.0,
                                         nan_rays=4 if i % 4 == 1 else 0)))
    out.append(("general", 300, 300, dict(seed=1, mixed=True, invalid=0.1, nan_rays=6)))
    out.append(("euroc", 200, 200, dict(seed=2, radtan8=True)))
    for n1 in N1_SIZES:
        out.append(("general", 65, n1, dict(seed=3, mixed=n1 % 2 == 1)))
    for n0 in N0_SIZES:
        out.append(("near", n0, 260, dict(seed=4)))
    return out


PAIR_SPECS = _pair_specs()  # (kind, n0, n1, keyword arguments) of pair_scene


def spec_id(spec):
    return "-".join(str(v) for v in spec[:3]) + "".join(f"-{k}{v:g}" for k, v in sorted(spec[3].items()) if v)


def pair_scenes():
    return [pair_scene(kind, n0, n1, **kw) for kind, n0, n1, kw in PAIR_SPECS]


def run_pair(oracle, sc, motion, census=None):
    if motion:
        return oracle.match_motion_stereo(sc["d0"], sc["kp0"], sc["bp0"], sc["bv0"], sc["skip0"], sc["d1"],
                                          sc["kp1"], sc["bp1"], sc["bv1"], sc["matched1"], sc["T0"], sc["T1"],
                                          sc.get("oracle_cam", sc["cam"]), THRESHOLD, census=census)
    return oracle.match_stereo(sc["d0"], sc["kp0"], sc["bp0"], sc["bv0"], sc["d1"], sc["kp1"], sc["bp1"],
                               sc["bv1"], sc["T0"], sc["T1"], sc["f0"], sc["f1"], THRESHOLD, census=census)


def radtan8_accepted(sc, rows):
    """The 4 px check of the winners in `rows`, recomputed with the restated 8-coefficient projection:
    1 / 0, or -1 where the verdict lies within 1e-6 of an edge (4 px, the image border)."""
    import radtan8_ref
    cam = sc["cam"]
    out = np.zeros(len(rows), dtype=np.int32)
    C1, r1 = np.asarray(sc["T1"][0]).reshape(3, 3), np.asarray(sc["T1"][1])
    for i in np.flatnonzero(rows["k1"] >= 0):
        hp = rows["hp_W"][i]
        hc = C1.T @ hp[:3] - (C1.T @ r1) * hp[3]
        head = -hc if hp[3] < 0 else hc
        st, pt, _ = radtan8_ref.project(cam, head[None])
        k1 = rows["k1"][i]
        e = np.hypot(float(sc["kp1"]["x"][k1]) - pt[0, 0], float(sc["kp1"]["y"][k1]) - pt[0, 1])
        edge = abs(e - 4.0) < 1e-6 or np.any(np.abs(pt[0]) < 1e-6) or np.any(np.abs(pt[0] - [cam.w, cam.h]) < 1e-6)
        out[i] = -1 if edge else int(st[0] == 0 and e < 4.0)
    return out


# ---- matchToMapUninitialised ---------------------------------------------------------------------
UNINIT_KINDS = ("base", "coincident", "close", "far", "identical", "tumvi")


def uninit_scene(kind, n_k=300, n_lm=400, seed=0):
    """Keypoint k observes landmark k (k < min(n_k, n_lm)).  coincident: a third of the observation
    centres equal the current camera centre (NaN epipolar normals); close: centres within 0.2 m of
    the point, and points within 0.2 m of the current centre; far: near-parallel rays; identical:
    the observing ray equals the current one."""
    rng = np.random.default_rng([seed, 100 + UNINIT_KINDS.index(kind), n_k, n_lm])
    cam = (synth.tumvi1024_config() if kind == "tumvi" else synth.euroc_config()).cams[0]
    focal = 0.5 * (cam.fu + cam.fv)
    C1 = rodrigues((0.3, 0.9, -0.2), 0.3)
    T1 = (C1.reshape(-1), np.array([0.25, -0.03, 0.05]))
    lo, hi = {"far": (40.0, 900.0), "close": (0.1, 0.6)}.get(kind, (0.5, 10.0))
    N = max(n_k, n_lm, 1)
    px = np.stack([rng.uniform(3, cam.w - 3, N), rng.uniform(3, cam.h - 3, N)], 1)
    X = _pixels_to_points(cam, T1, px, np.exp(rng.uniform(np.log(lo), np.log(hi), N)))
    kps, bp, bv = observe(cam, T1, X[:n_k], rng, 0.0 if kind == "identical" else 0.4)
    cl = rng.integers(0, N_CLUSTERS, N)
    centres = rng.integers(0, 256, (N_CLUSTERS, 48), dtype=np.uint8)
    desc = np.stack([_flip_bits(centres[cl[k]], rng.choice(384, int(rng.integers(2, 11)), replace=False))
                     for k in range(n_k)]) if n_k else np.zeros((0, 48), np.uint8)
    counts = rng.integers(1, 4, n_lm)
    counts[::23] = 0
    desc_begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    m = int(desc_begin[-1])
    pool = np.zeros((m, 48), dtype=np.uint8)
    r0, e0 = np.zeros((m, 3)), np.zeros((m, 3))
    for l in range(n_lm):
        for d in range(desc_begin[l], desc_begin[l + 1]):
            pool[d] = _flip_bits(centres[cl[l]], rng.choice(384, int(rng.integers(2, 11)), replace=False))
            r0[d] = T1[1] + rng.normal(0, 0.3, 3)
            u = rng.random()
            if kind == "coincident" and u < 0.33:
                r0[d] = T1[1]
            if kind == "close" and u < 0.4:
                r0[d] = X[l] + rng.normal(0, 0.08, 3)
            if kind == "identical" and u < 0.5:
                r0[d] = T1[1] if u < 0.25 else r0[d]
                ray = C1 @ (bp[l] / np.linalg.norm(bp[l])) if l < n_k and bv[l] else X[l] - T1[1]
            else:
                ray = X[l] - r0[d] + rng.normal(0, 0.003, 3) * np.linalg.norm(X[l] - r0[d])
            nr = np.linalg.norm(ray)
            e0[d] = ray / nr if nr > 0 else np.array([0.0, 0.0, 1.0])
    use = ((bv != 0) & (rng.random(n_k) > 0.1)).astype(np.uint8)
    previous = np.full(n_k, -1, dtype=np.int32)
    previous[::5] = np.arange(n_k)[::5] % max(n_lm, 1)
    previous[2::5] = (np.arange(n_k)[2::5] + 1) % max(n_lm, 1)
    name = f"uninit-{kind}-{n_k}x{n_lm}" + (f"-s{seed}" if seed else "")
    return dict(name=name, kind=kind, cam=cam, kps=kps, desc=desc, bp=bp, bv=bv, use=use, previous=previous,
                desc_begin=desc_begin, pool=pool, e0=e0, r0=r0, T1=T1, focal=focal)


UNINIT_SPECS = [(k, 300, 400, {}) for k in UNINIT_KINDS] + \
    [("base", n_k, 700, dict(seed=5)) for n_k in (0,) + N0_SIZES] + \
    [("far", 130, n_lm, dict(seed=6)) for n_lm in N1_SIZES]


def uninit_scenes():
    return [uninit_scene(kind, n_k, n_lm, **kw) for kind, n_k, n_lm, kw in UNINIT_SPECS]


def run_uninit(oracle, sc, census=None):
    return oracle.match_to_map_uninit(sc["desc"], sc["bp"], sc["use"], sc["previous"], sc["desc_begin"],
                                      sc["pool"], sc["e0"], sc["r0"], sc["T1"], sc["focal"], THRESHOLD,
                                      census=census)


# ---- matchToMap, 3-D landmarks: the float bounding-box prefilter and its edges ----------------------
def map_scene(kind, n_k=300, n_lm=600, seed=0, repr_thr=5.0):
    """kind:
    radius     projections at integer 3-4-5 offsets of their keypoint (dd == thr^2 exactly: passes, the
               test is a strict >) and one ulp outside (does not pass)
    disjoint   every wave's 64 keypoints sit in a box of their own
    outliers   keypoint coordinates negative, above 65535 and NaN mixed into waves of finite ones
    wildproj   projections NaN, +-inf and beyond float range
    crowded    landmarks with 0 descriptors and chunks of 64 landmarks with more than 192 descriptors
    """
    rng = np.random.default_rng([seed, 200 + ("radius", "disjoint", "outliers", "wildproj", "crowded").index(kind),
                                 n_k, n_lm])
    kps = np.zeros(n_k, dtype=O.KEYPOINT_DTYPE)
    kps["size"] = 12.0
    if kind == "disjoint":
        w = np.arange(n_k) // 64
        kps["x"] = 40.0 + 90.0 * (w % 8) + rng.uniform(0, 30, n_k)
        kps["y"] = 40.0 + 90.0 * (w // 8) + rng.uniform(0, 30, n_k)
    elif kind == "radius":
        kps["x"] = rng.integers(30, 720, n_k).astype(np.float32) + rng.choice([0.0, 0.25, 0.5], n_k)
        kps["y"] = rng.integers(30, 450, n_k).astype(np.float32) + rng.choice([0.0, 0.25, 0.5], n_k)
    else:
        kps["x"] = rng.uniform(30, 720, n_k)
        kps["y"] = rng.uniform(30, 450, n_k)
    cl = rng.integers(0, N_CLUSTERS, max(n_k, n_lm, 1))
    centres = rng.integers(0, 256, (N_CLUSTERS, 48), dtype=np.uint8)
    desc = np.stack([_flip_bits(centres[cl[k]], rng.choice(384, int(rng.integers(2, 11)), replace=False))
                     for k in range(n_k)]) if n_k else np.zeros((0, 48), np.uint8)
    counts = rng.integers(1, 4, n_lm)
    counts[::13] = 0
    if kind == "crowded":
        counts = rng.integers(0, 4, n_lm)
        counts[64:128] = rng.integers(3, 7, 64)   # > 192 descriptors in one chunk: the unstaged path
        counts[-40:] = rng.integers(4, 9, 40)
    desc_begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    m = int(desc_begin[-1])
    pool = np.stack([_flip_bits(centres[cl[np.searchsorted(desc_begin, d, side="right") - 1]],
                                rng.choice(384, int(rng.integers(2, 11)), replace=False))
                     for d in range(m)]) if m else np.zeros((0, 48), np.uint8)
    proj = np.stack([rng.uniform(0, 752, n_lm), rng.uniform(0, 480, n_lm)], 1)
    own = np.arange(n_lm) % max(n_k, 1)  # landmark l sits near keypoint l mod n_k
    if n_k:
        proj[:, 0] = kps["x"][own].astype(np.float64) + rng.normal(0, 0.6 * repr_thr + 1e-3, n_lm)
        proj[:, 1] = kps["y"][own].astype(np.float64) + rng.normal(0, 0.6 * repr_thr + 1e-3, n_lm)
    if kind == "radius" and n_k:
        offs = np.array([(3, 4), (-3, 4), (4, -3), (-4, -3), (5, 0), (0, -5)], dtype=np.float64) * (repr_thr / 5.0)
        for l in range(n_lm):
            o = offs[l % 6]
            x, y = float(kps["x"][own[l]]), float(kps["y"][own[l]])
            proj[l] = (x + o[0], y + o[1])          # dd == thr^2 exactly (all terms exact in binary64)
            if l % 3 == 1:                          # one ulp outside along the larger component
                i = int(abs(o[1]) > abs(o[0]))
                proj[l, i] = np.nextafter(proj[l, i], proj[l, i] + np.sign(o[i]) * 1e9)
            if l % 3 == 2:                          # one ulp inside
                i = int(abs(o[1]) > abs(o[0]))
                proj[l, i] = np.nextafter(proj[l, i], proj[l, i] - np.sign(o[i]) * 1e9)
    if kind == "outliers" and n_k:
        idx = rng.permutation(n_k)
        q = max(n_k // 12, 1)
        kps["x"][idx[:q]] = -rng.uniform(1, 300, len(idx[:q]))
        kps["y"][idx[q:2 * q]] = rng.uniform(65536, 2.0e5, len(idx[q:2 * q]))
        kps["x"][idx[2 * q:3 * q:2]] = np.nan
        kps["y"][idx[2 * q + 1:3 * q:2]] = np.nan
        kps["x"][idx[3 * q:3 * q + 3]] = (np.inf, -np.inf, 3.0e38)[:len(idx[3 * q:3 * q + 3])]
        # landmarks near the moved keypoints, so that they keep candidates
        for l in range(0, n_lm, 3):
            k = idx[l % (3 * q)]
            x, y = float(kps["x"][k]), float(kps["y"][k])
            if np.isfinite(x) and np.isfinite(y):
                proj[l] = (x + rng.normal(0, 2), y + rng.normal(0, 2))
    if kind == "wildproj":
        wild = [(np.nan, 100.0), (100.0, np.nan), (np.nan, np.nan), (np.inf, 50.0), (-np.inf, 50.0),
                (50.0, np.inf), (1.0e39, 100.0), (-1.0e300, 1.0e300), (3.5e38, -3.5e38), (1.0e-320, 0.0)]
        for l in range(0, n_lm, 4):
            proj[l] = wild[(l // 4) % len(wild)]
    use = (rng.random(n_k) > 0.12).astype(np.uint8)
    name = f"map-{kind}-{n_k}x{n_lm}-r{repr_thr:g}" + (f"-s{seed}" if seed else "")
    return dict(name=name, kind=kind, kps=kps, desc=desc, use=use, proj=proj, desc_begin=desc_begin, pool=pool,
                repr_thr=float(repr_thr))


MAP_SPECS = [("radius", 300, 600, dict(repr_thr=5.0)), ("radius", 300, 600, dict(repr_thr=20.0)),
             ("disjoint", 640, 900, dict(repr_thr=20.0)), ("outliers", 300, 600, dict(repr_thr=20.0)),
             ("outliers", 130, 300, dict(seed=1, repr_thr=150.0)), ("wildproj", 300, 600, dict(repr_thr=20.0)),
             ("crowded", 300, 600, dict(repr_thr=20.0)), ("outliers", 300, 600, dict(repr_thr=0.0, seed=4)),
             ("wildproj", 300, 600, dict(repr_thr=1.0e30)), ("outliers", 200, 300, dict(seed=2, repr_thr=1.0e30)),
             ("radius", 300, 300, dict(seed=3, repr_thr=0.0))] + \
    [("disjoint", n_k, 500, dict(seed=7, repr_thr=20.0)) for n_k in (1, 63, 64, 65)] + \
    [("radius", 100, n_lm, dict(seed=8, repr_thr=5.0)) for n_lm in (0, 1, 3, 4, 5, 255, 256, 257, 260, 1500)]


def map_scenes():
    return [map_scene(kind, n_k, n_lm, **kw) for kind, n_k, n_lm, kw in MAP_SPECS]


def run_map(oracle, sc, census=None):
    return oracle.match_to_map(sc["desc"], sc["kps"], sc["use"], sc["proj"], sc["desc_begin"], sc["pool"],
                               sc["repr_thr"], THRESHOLD, census=census)


# ---- knife edges -----------------------------------------------------------------------------------
def _ordered(x, dtype):
    """integer whose order is the order of the floating-point values (same-sign finite inputs suffice)"""
    bits = np.array([x], dtype=dtype).view(np.int64 if dtype == np.float64 else np.int32)[0]
    return int(bits)


def _from_ordered(i, dtype):
    return np.array([i], dtype=np.int64 if dtype == np.float64 else np.int32).view(dtype)[0]


def bisect_adjacent(f, a, b, dtype=np.float64, max_calls=70):
    """a, b > 0 of one sign with f(a) != f(b): two ADJACENT representable values (lo, hi), lo < hi,
    between them with f(lo) == f(min(a, b)) != f(hi).  At most max_calls calls."""
    a, b = (a, b) if a < b else (b, a)
    assert a > 0
    ia, ib = _ordered(a, dtype), _ordered(b, dtype)
    fa, fb = f(_from_ordered(ia, dtype)), f(_from_ordered(ib, dtype))
    assert fa != fb, "no edge between the end points"
    calls = 2
    while ib - ia > 1:
        im = (ia + ib) // 2
        fm = f(_from_ordered(im, dtype))
        calls += 1
        assert calls <= max_calls
        if fm == fa:
            ia = im
        else:
            ib = im
    return _from_ordered(ia, dtype), _from_ordered(ib, dtype)


# one edge per comparison that turns a verdict: the cos 2.6 sigma tests of both paths, cos 6 sigma, ee < 0.8, the
# depth in either camera against 0.05 (stereo) and 0.2 (motion), 4 px, lambda < 0.01.  ee < 0.5, tn < 0.01 and
# |det| <= 1e-12 have none: they choose a path, and no adjacent pair of inputs changes an output row through them.
KNIFE_GATES = ("cos26", "parcos26", "cos6", "ee08", "depth005", "depth02", "depth1_005", "depth1_02", "px4", "l001")


def _knife_single(gate, v, tilt=0.22):
    """the single-pair scene of a gate with its bisected input at v: (scene dict, motion?)"""
    cam = synth.euroc_config().cams[0]
    eye = np.eye(3)
    kp0 = np.zeros(1, dtype=O.KEYPOINT_DTYPE)
    kp1 = np.zeros(1, dtype=O.KEYPOINT_DTYPE)
    for kp in (kp0, kp1):
        kp["x"], kp["y"], kp["size"] = 367.0, 248.0, 12.0
    motion = gate in ("depth02", "depth1_02", "px4")
    P = np.array([0.0, 0.0, 0.5])  # the point, on the ray of kp0 (up to the camera model's rounding)
    ok, ray = O.cam_backproject(cam, (367.0, 248.0))
    ray = ray / np.linalg.norm(ray)
    T0 = (eye.reshape(-1), np.zeros(3))

    def looking_at(centre, target, spin=0.0):
        """pose at `centre` whose keypoint ray passes through target"""
        z = (target - centre) / np.linalg.norm(target - centre)
        axis = np.cross(ray, z)
        s = np.linalg.norm(axis)
        R = np.eye(3) if s < 1e-15 else rodrigues(axis, np.arctan2(s, float(ray @ z)))
        return (R.reshape(-1), np.asarray(centre, dtype=np.float64))

    if gate == "cos26":    # v: offset of camera 1 out of the epipolar plane -> skew rays
        P = ray * 0.5
        T1 = looking_at(np.array([0.1, 0.0, 0.0]), P)
        T1 = (T1[0], np.array([0.1, float(v), 0.0]))
    elif gate == "cos6":   # v: convergence angle of the two rays
        T1 = (rodrigues((0, 1, 0), -float(v)).reshape(-1), np.array([0.11, 0.0, 0.0]))
    elif gate == "ee08":   # v: angle between the rays, which meet at P
        P = ray * 1.0
        c = P - rodrigues((0, 1, 0), -float(v)) @ ray
        T1 = (rodrigues((0, 1, 0), -float(v)).reshape(-1), c)
    elif gate in ("depth005", "depth02"):  # v: camera 0 moves along its own ray towards P
        P = ray * 0.5
        T0 = (eye.reshape(-1), ray * float(v))
        T1 = looking_at(np.array([0.1, 0.0, 0.0]), P)
    elif gate in ("depth1_005", "depth1_02"):  # v: camera 1, rotated to look at P, moves along ITS ray towards P:
        P = ray * 0.5                          # the depth that turns is taken through the inverse of a rotated pose
        T1 = looking_at(np.array([0.1, 0.0, 0.0]), P)
        z = (P - T1[1]) / np.linalg.norm(P - T1[1])
        T1 = (T1[0], T1[1] + z * float(v))
    elif gate == "parcos26":  # v: angle between the rays, which meet 0.005 m ahead: lambda < 0.01 sends the pair to
        R1 = rodrigues((0, 1, 0), -float(v))  # midpoint_parallel, whose point lies on the bisector, v / 2 off each ray
        T1 = (R1.reshape(-1), ray * 0.005 - 0.005 * (R1 @ ray))
    elif gate == "px4":    # v: y of keypoint 1 (float32); size 24 keeps the triangulation valid to ~15 px
        P = ray * 2.0
        T1 = looking_at(np.array([0.3, 0.0, 0.0]), P)
        for kp in (kp0, kp1):
            kp["size"], kp["octave"] = 24.0, 2
        kp1["y"] = np.float32(v)
    elif gate == "l001":
        # The rays meet at lambda_0 = 0.009 + v in front of camera 0 and lambda_1 = 0.0101 in front of camera 1:
        # camera 1 slides along ray 0 by v.  Size class 7 (sigma 0.039): at 0.22 rad the pair is parallel by
        # cos 6 sigma, which spares it the depth gates (a point 0.01 m away fails every one of them), while the
        # fall-back of a lambda under 0.01 is invalid, as half of 0.22 rad exceeds 2.6 sigma: the verdict turns at
        # lambda_0 = 0.01.  With both lambdas near 0.01 the two products that make lambda_0 stay under 2^-6, so
        # lambda_0 moves in steps of its own ulp and can BE 0.01 (a camera further back cannot: steps of 16 ulps).
        for kp in (kp0, kp1):
            kp["size"], kp["octave"] = layer_size(7), 7
        R1 = rodrigues((0, 1, 0), -float(tilt))
        T1 = (R1.reshape(-1), ray * 0.009 - 0.0101 * (R1 @ ray) + ray * float(v))
    else:
        raise ValueError(gate)
    bp0, bv0 = O.backproject_keypoints(cam, kp0)
    bp1, bv1 = O.backproject_keypoints(cam, kp1)
    d = np.full((1, 48), 0x5A, dtype=np.uint8)
    f = 0.5 * (cam.fu + cam.fv)
    return dict(name=f"knife-{gate}", kind="knife", cam=cam, d0=d, kp0=kp0, bp0=bp0, bv0=bv0, d1=d.copy(), kp1=kp1,
                bp1=bp1, bv1=bv1, T0=T0, T1=T1, f0=f, f1=f, mixed=gate in ("px4", "l001"), skip0=np.zeros(1, np.uint8),
                matched1=np.zeros(1, np.uint8)), motion


_KNIFE_RANGE = {"cos26": (1e-4, 0.05, np.float64), "cos6": (1e-3, 0.2, np.float64), "ee08": (0.3, 1.0, np.float64),
                "depth005": (0.3, 0.49, np.float64), "depth02": (0.1, 0.45, np.float64),
                "depth1_005": (0.3, 0.49, np.float64), "depth1_02": (0.1, 0.45, np.float64),
                "parcos26": (0.005, 0.05, np.float64),
                "px4": (248.5, 262.0, np.float32), "l001": (0.0005, 0.0015, np.float64)}


def lambda0_binary64(sc, tree):
    """lambda_0 of triangulateFast for the single pair of sc as binary64 evaluates it, in the oracle's order of
    operations (tree: x0 + (x1 + x2), else left to right).  Python floats: IEEE binary64, no contraction."""
    import math

    def s3(p0, p1, p2):
        return p0 + (p1 + p2) if tree else (p0 + p1) + p2

    def dot(a, b):
        return s3(a[0] * b[0], a[1] * b[1], a[2] * b[2])

    def ray(T, bp):
        C = [float(x) for x in np.asarray(T[0]).reshape(-1)]
        v = [dot(C[0:3], bp), dot(C[3:6], bp), dot(C[6:9], bp)]
        n = math.sqrt(dot(v, v))
        return [v[0] / n, v[1] / n, v[2] / n]

    e1 = ray(sc["T0"], [float(x) for x in sc["bp0"][0]])
    e2 = ray(sc["T1"], [float(x) for x in sc["bp1"][0]])
    p1, p2 = [float(x) for x in sc["T0"][1]], [float(x) for x in sc["T1"][1]]
    t12 = [p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]]
    b0, b1 = dot(t12, e1), dot(t12, e2)
    a00, a10 = dot(e1, e1), dot(e1, e2)
    a01, a11 = -a10, -dot(e2, e2)
    det = a00 * a11 - a01 * a10
    invdet = 1.0 / det
    i00, i01 = a11 * invdet, -a01 * invdet
    return i00 * b0 + i01 * b1


def knife_edge(oracle, gate, copies=70):
    """Bisects the gate's input (under the oracle's CURRENT sum order) down to two adjacent representable
    values whose oracle rows carry different verdicts (k1, initialisable, accepted: hp_W moves with every
    step of the input, the verdict only at the edge), then embeds both sides in a batch of
    2 * copies keypoints per image (pair i of image 0 only matches row i of image 1: every pair has a
    descriptor of its own).  Returns (scene, motion, (lo, hi), calls).  The batch keeps the poses of the
    LOW side where the pose is the bisected input and so holds one side only for those gates; the other
    side is returned as a second scene: (scene_lo, scene_hi)."""
    lo0, hi0, dtype = _KNIFE_RANGE[gate]
    calls = [0]
    tilt = [0.22]

    def f(v):
        calls[0] += 1
        sc, motion = _knife_single(gate, v, tilt[0])
        row = run_pair(oracle, sc, motion)[0]
        return (int(row["k1"]), int(row["initialisable"]), int(row["accepted"]) if motion else 0)

    lo, hi = bisect_adjacent(f, lo0, hi0, dtype)
    if gate == "l001":
        # "<" and "<=" part ways at lambda_0 == 0.01 EXACTLY: the angle between the rays is stepped until the first
        # lambda_0 that is not under 0.01 IS 0.01 (binary64 replica above).  calls counts the last bisection.
        tree = bool(oracle.lib().orc_get_reduction())
        for step in range(400):
            if lambda0_binary64(_knife_single(gate, hi, tilt[0])[0], tree) == 0.01:
                break
            tilt[0] = 0.22 + 1.0e-6 * (step + 1)
            calls[0] = 0
            lo, hi = bisect_adjacent(f, lo0, hi0, dtype)
        else:
            raise AssertionError("no angle puts lambda_0 on 0.01")
    scenes = []
    for v in (lo, hi):
        sc, motion = _knife_single(gate, v, tilt[0])
        n = copies
        rng = np.random.default_rng(17)
        desc = rng.integers(0, 256, (n, 48), dtype=np.uint8)  # random rows: ~192 bits apart, far above the threshold
        out = dict(sc)
        for side in ("0", "1"):
            out["d" + side] = desc.copy()
            for k in ("kp", "bp", "bv"):
                out[k + side] = np.repeat(sc[k + side], n, axis=0)
        if gate == "px4":  # the keypoint is the bisected input: both sides alternate inside ONE batch
            other = _knife_single(gate, hi if v == lo else lo, tilt[0])[0]
            for k in ("kp1", "bp1", "bv1"):
                out[k][1::2] = other[k][0]
        out["skip0"] = np.zeros(n, np.uint8)
        out["matched1"] = np.zeros(n, np.uint8)
        out["name"] = f"knife-{gate}-{'lo' if v == lo else 'hi'}"
        scenes.append(out)
    return scenes, motion, (lo, hi), calls[0]


def all_census(oracle=O, match=""):
    """{matcher: counters} summed over the scenes whose name contains `match`"""
    tot = {m: oracle.new_census() for m in ("stereo", "motion", "uninit", "map")}
    for sc in pair_scenes():
        if match in sc["name"]:
            run_pair(oracle, sc, False, tot["stereo"])
            run_pair(oracle, sc, True, tot["motion"])
    for sc in uninit_scenes():
        if match in sc["name"]:
            run_uninit(oracle, sc, tot["uninit"])
    for sc in map_scenes():
        if match in sc["name"]:
            run_map(oracle, sc, tot["map"])
    return tot


def format_census(tot):
    labels = O.census_labels()
    lines = [f"{'label':<14}" + "".join(f"{m:>10}" for m in tot)]
    for i, lab in enumerate(labels):
        lines.append(f"{lab:<14}" + "".join(f"{int(tot[m][i]):>10}" for m in tot))
    return "\n".join(lines)


if __name__ == "__main__":
    print(format_census(all_census(match=sys.argv[1] if len(sys.argv) > 1 else "")))
