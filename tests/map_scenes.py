"""Landmark tables that drive matchToMap's landmark preparation (prepare_landmarks_kernel and
compact_landmarks_kernel of k_map.hip behind okvfe_match_to_map_landmarks; oracle:
orc_prepare_landmarks) into every branch of Frontend.cpp:1219-1359, onto the knife edges of its
comparisons, and through the chunk edges of the packing kernel.  CPU only and seeded: numpy plus the
CPU oracle.  The CPU tier (test_map_scenes_host.py) and the GPU tier (test_gpu_map_census.py)
consume the same tables.

    python tests/map_scenes.py            census (label x mode) over the general scenes
    python tests/map_scenes.py equi       census of the scenes whose name contains "equi"

A table is a dict in the layout of map_synth.make_map, valid for okvfe_match_to_map_landmarks as
include/okvfe.h documents it: cam, poses [(C, r)], T1, hp (n, 4), quality, obs_begin, obs_pose,
obs_desc, obs_bp, plus name.  Pose 0 of every general table is T1 bit for bit.

General scenes (general_scene): map_synth.make_map's random map of the scene's camera, extended by
directed landmarks.  A directed landmark sits at (range, polar angle, azimuth) in the current camera
and draws a recipe for its observation list; every observation has a pose of its own, placed at a
chosen view-point angle and range ratio relative to the landmark.

  cameras      euroc (radial-tangential), equi (Hilti, equidistant; polar angles to 2.6 rad: beyond 90 degrees),
               nodist (no distortion), radtan8 (8 coefficients: not in the oracle, see run_oracle)
  depth        |z| in {2, 5} x {1e-13, 1e-12} on both sides of the camera plane, on the axis (a point 1e-12 m from
               the centre) and off it; behind the camera; exactly at the centre; 1 mm from it
  hp[3]        1, 2, -1, 0.5 and 1e-300 (scaled point), 1e-300, 0.0 and -0.0 (point of order 1: 1e300 m away, resp. a
               direction)
  poses        pose 0 (= T1: r_W_old is r_W, the cosine 1 or one ulp above it), pure rotations of it, view-point angles
               around 0.6 rad, range ratios around 0.5 and 1.5, exact right / straight / opposite angles on the world axes
  quality      1, 0.3, 0.05, 1e-3, 1e-12, 0, -1, NaN
  lists        0, 1, 2, 3, 4, 6, 40 observations; scores ascending, descending, all equal (one pose), all exactly 0
               (pose 0 where the cosine is exactly 1); zero-length back-projections

Census of the committed general scenes (oracle, default summation order; the 8-coefficient scene through the
oracle's pinhole without a distortion):

    label               non-exclusive      exclusive
    head_negated                 1064           1064
    proj_invalid                  500            500
    proj_behind                   427            427
    proj_outside_kept             168            746
    proj_successful              5915           5915
    margin_u_low                  431            292
    margin_v_low                  345            205
    margin_u_high                 339            206
    margin_v_high                 275            109
    clamp_r                       333            334
    is3d_first                   3966           4357
    is3d_later                     93             95
    is3d_never                   1532           1680
    vp_reject                    6267              0
    vp_kept_excl                    0           7142
    scale_reject                 2723              0
    scale_kept_excl                 0           5970
    acos_tiny                       0            691
    acos_small                      0           1657
    acos_neg                        0           1674
    acos_pos                    22726          31270
    acos_above_one                245            253
    not_stored                   7989          16921
    not_stored_tie               2410           2635
    not_stored_ge1                  0           5269
    not_stored_nan                875           1382
    write_s0_o0                  4737           5476
    write_s0_o1                     0              0
    write_s0_o2                  1584           2060
    write_s1_o0                  3752           4552
    write_s1_o1                     0              0
    write_s1_o2                  1361           1733
    write_s2_o0                     0              0
    write_s2_o1                  2799           3562
    write_s2_o2                  1379           1875
    final_o0_stored               985            924
    final_o1                      953            990
    final_o2                     1440           1681
    final_o2_cropped             1359           1881

Knife edges (knife_edge): one scalar of a one-landmark table -- a landmark coordinate, a pose
translation, the quality -- is bisected until two ADJACENT binary64 values give different verdicts
in the oracle; both sides then sit in one table, side by side.  margin_*: the four reprojection
margins on a camera with dyadic intrinsics, where the kept side sits EXACTLY on -thr resp. w + thr;
z_invalid: |z| < 1e-12; cos10: the 3-D test; cos06; scale05, whose kept side is exactly 0.5; tie,
whose unstored side has exactly the worst slot's score; clamp: |r_W| < 0.01, which changes no output
(both branches meet there) and is bisected on the census.  `z > 0` has no adjacent pair: it is only
asked behind |z| >= 1e-12; z_sign_table() holds the nearest inputs of each side instead.

Packing scenes (packing_scene): the chunk loop of compact_landmarks_kernel at n_landmarks around the
multiples of 1024, with the 3-D landmarks all / none / first of each chunk / last of each chunk /
alternating / mixed with 1 and 2 pooled rows.  dictated_frame places one keypoint per pooled row of
every 3-D landmark at that landmark's projection, with that row as its descriptor: observation
descriptors are random, so the one match at distance 0 is dictated, and a wrong index_out, begin_out
or pool row of the packed set shows as another landmark or a distance above 0.
"""
from __future__ import annotations

import dataclasses
import functools
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:  # (run as a script: the package lives one level up)
    sys.path.insert(0, _ROOT)

import map_synth
import oracle_lib as O
from gate_scenes import bisect_adjacent, rodrigues
from okvis2_amd import synth

MODES = ((False, 20.0), (True, 150.0))  # (exclusive, reprojection threshold), as the existing map test
CAMERA_KINDS = ("euroc", "equi", "nodist", "radtan8")
# dyadic intrinsics: fu * x + cu is exact for the x of the margin knife edges
DYADIC_CAM = synth.Camera(640, 480, 512.0, 512.0, 256.0, 128.0, 0, (0.0, 0.0, 0.0, 0.0))
QUALITIES = (1.0, 0.3, 0.05, 1.0e-3, 1.0e-12, 0.0, -1.0, np.nan)


def camera(kind):
    if kind == "euroc":
        return synth.euroc_config().cams[0]
    if kind == "equi":
        return synth.hilti_config().cams[0]
    if kind == "nodist":
        return dataclasses.replace(synth.d455_config().cams[0], dist_type=0)
    if kind == "radtan8":
        return synth.radtan8_config().cams[0]
    raise ValueError(kind)


def oracle_camera(cam):
    """the camera the oracle runs with: the 8-coefficient model is not in the oracle, which then takes the same
    pinhole without a distortion (pooling does not see the camera model beyond the FoV check)"""
    return dataclasses.replace(cam, dist_type=0, d=(0.0, 0.0, 0.0, 0.0)) if cam.dist_type == 3 else cam


def _perp(e, rng):
    v = np.cross(e, rng.normal(size=3))
    n = np.linalg.norm(v)
    return v / n if n > 0 else np.array([1.0, 0.0, 0.0])


class _Table:
    def __init__(self, cam, T1, rng, base=None):
        self.cam, self.T1, self.rng = cam, T1, rng
        self.poses = [(np.array(T1[0], dtype=np.float64).copy(), np.array(T1[1], dtype=np.float64).copy())]
        self.hp, self.quality, self.n_obs = [], [], []
        self.obs_pose, self.obs_bp = [], []
        if base is not None:  # a map_synth map: its poses follow pose 0
            off = len(self.poses)
            self.poses += [(np.asarray(C, dtype=np.float64), np.asarray(r, dtype=np.float64)) for C, r in base["poses"]]
            self.hp += list(base["hp"])
            self.quality += list(base["quality"])
            self.n_obs += list(np.diff(base["obs_begin"]))
            self.obs_pose += list(base["obs_pose"] + off)
            self.obs_bp += list(base["obs_bp"])

    def pose(self, C, r):
        self.poses.append((np.asarray(C, dtype=np.float64).reshape(-1).copy(), np.asarray(r, dtype=np.float64).copy()))
        return len(self.poses) - 1

    def world(self, p_C):
        return np.asarray(self.T1[0]).reshape(3, 3) @ np.asarray(p_C, dtype=np.float64) + np.asarray(self.T1[1])

    def landmark(self, hp, quality, obs):
        """obs: [(pose index, back-projection)]"""
        self.hp.append(np.asarray(hp, dtype=np.float64))
        self.quality.append(float(quality))
        self.n_obs.append(len(obs))
        for pi, bp in obs:
            self.obs_pose.append(int(pi))
            self.obs_bp.append(np.asarray(bp, dtype=np.float64))

    def observe(self, p_W, angle, ratio, zero_bp=False):
        """a fresh pose whose centre sees p_W under `angle` to the current ray, at `ratio` times the current
        (clamped) range; returns (pose index, back-projection)"""
        rng = self.rng
        rw = np.asarray(p_W) - self.T1[1]
        rn = np.linalg.norm(rw)
        e = rw / rn if rn > 0 else np.array([0.0, 0.0, 1.0])
        d = rodrigues(_perp(e, rng), angle) @ e
        c = np.asarray(p_W) - ratio * max(0.01, rn) * d
        C = rodrigues(rng.normal(size=3), rng.uniform(0, 0.4)) @ np.asarray(self.T1[0]).reshape(3, 3)
        return self.at(C, c, p_W, zero_bp)

    def at(self, C, c, p_W, zero_bp=False):
        pi = self.pose(C, c)
        ray = np.asarray(C).reshape(3, 3).T @ (np.asarray(p_W) - c)
        n = np.linalg.norm(ray)
        bp = np.zeros(3) if zero_bp or not n > 0 else ray * self.rng.uniform(0.2, 3.0) / n
        return pi, bp

    def finish(self, name, desc_seed):
        n_obs = np.array(self.n_obs, dtype=np.int64)
        m = int(n_obs.sum())
        obs_desc = np.random.default_rng(desc_seed).integers(0, 256, (m, 48), dtype=np.uint8)
        return dict(name=name, cam=self.cam, poses=self.poses, T1=self.T1,
                    hp=np.array(self.hp, dtype=np.float64).reshape(-1, 4),
                    quality=np.array(self.quality, dtype=np.float64),
                    obs_begin=np.concatenate([[0], np.cumsum(n_obs)]).astype(np.int32),
                    obs_pose=np.array(self.obs_pose, dtype=np.int32),
                    obs_desc=obs_desc, obs_bp=np.array(self.obs_bp, dtype=np.float64).reshape(-1, 3))


def _current_pose(kind):
    # a dyadic centre: r1 + (0, 0, rho) is exact for the axis recipes.  radtan8: identity, so that hp_C = hp_W in
    # every summation order and the restated 8-coefficient projection is bit-comparable with the device's
    if kind == "radtan8":
        return (np.eye(3).reshape(-1), np.zeros(3))
    return (rodrigues((0.3, -0.5, 0.8), 0.2).reshape(-1), np.array([0.5, -0.25, 0.125]))


def _polar(rho, theta, phi):
    return rho * np.array([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)])


def _homogeneous(p_W, w, scaled=True):
    return np.concatenate([p_W * w if scaled else p_W, [w]])


def _observation_list(t, p_W, rng):
    """one recipe of the list above"""
    kind = rng.choice(["random", "ascending", "descending", "equal", "same", "wide", "edge"],
                      p=[0.34, 0.1, 0.12, 0.1, 0.04, 0.2, 0.1])
    n = int(rng.choice([0, 1, 2, 3, 4, 6, 40], p=[0.05, 0.1, 0.15, 0.2, 0.25, 0.15, 0.1]))
    zero = lambda: rng.random() < 0.05
    if kind == "ascending" or kind == "descending":
        a = np.sort(rng.uniform(0.03, 0.55, n))
        return [t.observe(p_W, x, 1.0, zero()) for x in (a if kind == "ascending" else a[::-1])]
    if kind == "equal":  # one pose seen n times: equal scores
        ob = t.observe(p_W, rng.uniform(0.05, 0.5), rng.uniform(0.7, 1.3))
        return [ob] * n
    if kind == "same":   # the current pose itself, with a genuine view before or after it at times
        obs = [(0, t.at(t.T1[0], t.T1[1], p_W)[1])] * n
        for i in range(0, n, 3):  # pure rotation: the current centre, another attitude
            obs[i] = t.at(rodrigues(rng.normal(size=3), rng.uniform(0.05, 0.5)) @ np.asarray(t.T1[0]).reshape(3, 3), t.T1[1], p_W)
        if n and rng.random() < 0.5:
            obs[int(rng.integers(0, n))] = t.observe(p_W, rng.uniform(0.05, 0.5), 1.0)
        return obs
    if kind == "wide":   # any view-point angle, any range ratio
        return [t.observe(p_W, rng.uniform(0, np.pi), np.exp(rng.uniform(np.log(0.2), np.log(4.0))), zero())
                for _ in range(n)]
    if kind == "edge":   # around 0.6 rad, around ratios 0.5 and 1.5
        return [t.observe(p_W, rng.uniform(0.52, 0.68) if i % 2 else rng.uniform(0.0, 0.3),
                          1.0 if i % 2 else rng.choice([0.5, 1.5]) + rng.normal(0, 0.03), zero()) for i in range(n)]
    return [t.observe(p_W, rng.uniform(0, 0.75), rng.uniform(0.4, 1.7), zero()) for _ in range(n)]


@functools.lru_cache(maxsize=None)  # (shared by the tests of a session: a table is never written to)
def general_scene(kind, seed=0, n_base=500, n_directed=900):
    rng = np.random.default_rng([seed, 300 + CAMERA_KINDS.index(kind)])
    cam = camera(kind)
    T1 = _current_pose(kind)
    base = map_synth.make_map(n_base, seed=11 + seed)
    t = _Table(cam, T1, rng, base)
    theta_in = 0.55 if kind != "equi" else 0.9
    for i in range(n_directed):
        u = rng.random()
        q = float(rng.choice(QUALITIES, p=[0.35, 0.1, 0.1, 0.15, 0.1, 0.07, 0.06, 0.07]))
        w = float(rng.choice([1.0, 2.0, -1.0, 0.5, 1.0e-300], p=[0.6, 0.1, 0.15, 0.1, 0.05]))
        if u < 0.5:      # inside or near the image
            p_C = _polar(np.exp(rng.uniform(0, np.log(12.0))), rng.uniform(0, theta_in), rng.uniform(0, 2 * np.pi))
        elif u < 0.8:    # out to and beyond 90 degrees: the margins, OutsideImage, Behind
            p_C = _polar(np.exp(rng.uniform(0, np.log(12.0))), rng.uniform(0.3, 2.6), rng.uniform(0, 2 * np.pi))
        elif u < 0.88:   # 1 mm to 2 cm from the centre: the clamp
            p_C = _polar(rng.choice([0.001, 0.004, 0.009, 0.02]), rng.uniform(0, theta_in), rng.uniform(0, 2 * np.pi))
        elif u < 0.91:   # on both sides of the camera plane, within and beyond 1e-12
            z = float(rng.choice([2e-13, 5e-13, 2e-12, 5e-12])) * float(rng.choice([-1.0, 1.0]))
            xy = rng.uniform(-1, 1, 2) * (0.4 * abs(z) if rng.random() < 0.6 else 1.0)
            p_C = np.array([xy[0], xy[1], z])
        else:
            p_C = None
        if p_C is None:
            v = rng.random()
            if v < 0.35:   # exactly at the camera centre
                t.landmark(_homogeneous(T1[1], w), q, _observation_list(t, T1[1] + [0, 0, 0.01], rng))
            elif v < 0.75: # a point of order 1 with a tiny or zero hp[3]: 1e300 m away, resp. a direction
                p_W = t.world(_polar(rng.uniform(1, 8), rng.uniform(0, theta_in), rng.uniform(0, 2 * np.pi)))
                t.landmark(_homogeneous(p_W, float(rng.choice([1.0e-300, 0.0, -0.0])), scaled=False), q,
                           _observation_list(t, p_W, rng))
            else:          # on the world axes through the (dyadic) current centre: cosines 0, 1 and -1 exactly
                rho = float(rng.choice([0.5, 1.0, 2.0, 4.0]))
                p_W = T1[1] + np.array([0.0, 0.0, rho])
                obs = []
                for _ in range(int(rng.integers(1, 6))):
                    d = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [0, 0, -1.0], [-1.0, 0, 0]][int(rng.integers(0, 5))])
                    obs.append(t.at(T1[0], p_W - float(rng.choice([0.5, 1.0, 1.25, 1.5])) * rho * d, p_W))
                t.landmark(_homogeneous(p_W, 1.0), q, obs)
            continue
        p_W = t.world(p_C)
        t.landmark(_homogeneous(p_W, w), q, _observation_list(t, p_W, rng))
    return t.finish(f"general-{kind}" + (f"-s{seed}" if seed else ""), [seed, 77, CAMERA_KINDS.index(kind)])


GENERAL_SPECS = [(k, 0) for k in CAMERA_KINDS] + [("euroc", 1), ("equi", 1)]


def general_scenes():
    return [general_scene(k, s) for k, s in GENERAL_SPECS]


def run_oracle(oracle, sc, exclusive, thr, census=None):
    return oracle.prepare_landmarks(sc["hp"], sc["quality"], sc["obs_begin"], sc["obs_pose"], sc["obs_bp"],
                                    sc["poses"], sc["T1"], oracle_camera(sc["cam"]), thr, exclusive, census=census)


# ---- the packing kernel ------------------------------------------------------------------------------
PACK_SIZES = (1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 3100)
PACK_PATTERNS = ("all", "none", "first", "last", "alternating", "mixed")


@functools.lru_cache(maxsize=None)
def packing_scene(n, pattern, seed=0):
    """n landmarks inside the image, four shared old poses half a metre around the current one: every observation is
    accepted in both modes.  3-D rows: quality 1 and 3 observations (2 pooled rows) or 2 (1 row); the others
    alternate between not 3-D yet (quality 1e-12) and no pooled view at all (1 or 0 observations)."""
    rng = np.random.default_rng([seed, 400 + PACK_PATTERNS.index(pattern), n])
    cam = camera("euroc")
    T1 = _current_pose("euroc")
    t = _Table(cam, T1, rng)
    C1 = np.asarray(T1[0]).reshape(3, 3)
    old = [t.pose(rodrigues((0, 1, 0), a) @ C1, T1[1] + C1 @ np.array(d))
           for a, d in ((0.02, (0.3, 0.0, 0.0)), (-0.03, (-0.4, 0.1, 0.0)), (0.01, (0.0, -0.35, 0.1)), (0.0, (0.5, 0.2, -0.1)))]
    last = {l for l in range(n) if l % 1024 == 1023 or l == n - 1}
    for l in range(n):
        p_C = np.array([rng.uniform(-0.6, 0.6), rng.uniform(-0.4, 0.4), 1.0]) * rng.uniform(3.0, 8.0)
        p_W = t.world(p_C)
        is3d = {"all": True, "none": False, "first": l % 1024 == 0, "last": l in last, "alternating": l % 2 == 0,
                "mixed": rng.random() < 0.6}[pattern]
        if is3d:
            n_obs, q = (2 if pattern == "mixed" and rng.random() < 0.5 else 3), 1.0
        else:
            n_obs, q = ((3, 1.0e-12) if l % 4 < 2 else (l % 2, 1.0))
        picks = rng.permutation(len(old))[:n_obs]
        obs = []
        for pi in picks:
            C, c = t.poses[old[pi]]
            ray = C.reshape(3, 3).T @ (p_W - c)
            obs.append((old[pi], ray / np.linalg.norm(ray)))
        t.landmark(_homogeneous(p_W, 1.0), q, obs)
    return t.finish(f"pack-{n}-{pattern}", [seed, 78, n, PACK_PATTERNS.index(pattern)])


def dictated_frame(oracle, sc, ref, clutter=0, seed=5):
    """One keypoint per pooled row of every 3-D landmark of `ref` (a prepare_landmarks result), at the landmark's
    projection, carrying that row: (kps, desc, use, landmark dictated per keypoint or -1).  clutter: further
    keypoints at random pixels with random descriptors, a tenth of all keypoints unused."""
    rng = np.random.default_rng([seed, len(sc["hp"])])
    idx = np.flatnonzero(ref["status"] == 1)
    own = np.repeat(idx, ref["n_desc"][idx])
    row = np.concatenate([ref["obs_rows"][l, :ref["n_desc"][l]] for l in idx]) if len(idx) else np.zeros(0, np.int64)
    n = len(own) + clutter
    kps = np.zeros(n, dtype=oracle.KEYPOINT_DTYPE)
    kps["size"] = 12.0
    kps["x"][:len(own)] = ref["projection"][own, 0]
    kps["y"][:len(own)] = ref["projection"][own, 1]
    kps["x"][len(own):] = rng.uniform(0, sc["cam"].w, clutter)
    kps["y"][len(own):] = rng.uniform(0, sc["cam"].h, clutter)
    desc = rng.integers(0, 256, (n, 48), dtype=np.uint8)
    desc[:len(own)] = sc["obs_desc"][row.astype(np.int64)]
    use = np.ones(n, dtype=np.uint8)
    want = np.concatenate([own, np.full(clutter, -1)]).astype(np.int32)
    if clutter:
        off = rng.random(n) < 0.1
        use[off] = 0
        want[off] = -1
    perm = rng.permutation(n)
    return kps[perm], desc[perm], use[perm], want[perm]


# ---- knife edges ---------------------------------------------------------------------------------------
KNIFE_EDGES = ("margin_u_low", "margin_v_low", "margin_u_high", "margin_v_high", "z_invalid", "cos10", "cos06",
               "scale05", "tie", "clamp")
# which mode an edge is bisected and checked in (cos06 and scale05 exist in a non-exclusive call only)
_IDENTITY = (np.eye(3).reshape(-1), np.zeros(3))


def _knife_table(edge, values, exclusive):
    """one landmark per value of the bisected scalar.  The camera looks along +z from the origin (identity pose)."""
    thr = dict(MODES)[exclusive]
    rng = np.random.default_rng(31)
    cam = DYADIC_CAM if edge.startswith("margin") else camera("euroc")
    t = _Table(cam, _IDENTITY, rng)
    eye = np.eye(3)

    def views(p_W, n=3, ratio=1.0):
        """n good views from poses of their own on a circle around the current ray"""
        return [t.at(eye, p_W - ratio * np.linalg.norm(p_W) * (rodrigues((np.cos(k), np.sin(k), 0.0), 0.1 + 0.05 * k)
                                                                  @ (p_W / np.linalg.norm(p_W))), p_W) for k in range(n)]
    for v in values:
        v = float(v)
        if edge.startswith("margin"):
            # v: the landmark's x (u edges) or y (v edges) at depth 1: kp = 512 * v + centre, exactly
            p = np.array([v, 0.0, 1.0]) if "_u_" in edge else np.array([0.0, v, 1.0])
            t.landmark(_homogeneous(p, 1.0), 1.0, views(p))
        elif edge == "z_invalid":  # v: the landmark's z, 1e-12 m in front of the centre; the views 1 cm away (the clamp)
            p = np.array([1.0e-14, -2.0e-14, v])
            t.landmark(_homogeneous(p, 1.0), 1.0,
                       [t.at(eye, -0.01 * (rodrigues((np.cos(k), np.sin(k), 0.0), 0.2 + 0.1 * k) @ np.array([0, 0, 1.0])), p)
                        for k in range(3)])
        elif edge == "cos10":      # v: the quality; one pose seen twice, 0.3 rad off the current ray
            p = np.array([0.3, -0.2, 5.0])
            ob = t.at(eye, p - np.linalg.norm(p) * (rodrigues((0, 1, 0), 0.3) @ (p / np.linalg.norm(p))), p)
            t.landmark(_homogeneous(p, 1.0), v, [ob, ob])
        elif edge == "cos06":      # v: x of the middle view's centre; cosVC = 5 / sqrt(v^2 + 25)
            p = np.array([0.0, 0.0, 5.0])
            g = views(p, 2)
            t.landmark(_homogeneous(p, 1.0), 1.0, [g[0], t.at(eye, np.array([v, 0.0, 0.0]), p), g[1]])
        elif edge == "scale05":    # v: how far the middle view stands behind the current centre, on the ray
            p = np.array([0.0, 0.0, 5.0])
            g = views(p, 2)
            t.landmark(_homogeneous(p, 1.0), 1.0, [g[0], t.at(eye, np.array([0.0, 0.0, -v]), p), g[1]])
        elif edge == "tie":        # views on the ray (acos(1) = 0: score = scale change), the fourth against the worst
            p = np.array([0.0, 0.0, 5.0])
            t.landmark(_homogeneous(p, 1.0), 1.0,
                       [t.at(eye, np.array([0.0, 0.0, -s]), p) for s in (0.5, 1.0, 1.5, v)])
        elif edge == "clamp":      # v: the landmark's range, on the axis
            p = np.array([0.0, 0.0, v])
            t.landmark(_homogeneous(p, 1.0), 1.0,
                       [t.at(eye, p - 0.012 * (rodrigues((np.cos(k), np.sin(k), 0.0), 0.2 + 0.1 * k) @ np.array([0, 0, 1.0])), p)
                        for k in range(3)])
        else:
            raise ValueError(edge)
    return t.finish(f"knife-{edge}", [9, KNIFE_EDGES.index(edge)]), thr


def _knife_range(edge, exclusive):
    thr = dict(MODES)[exclusive]
    c = DYADIC_CAM
    return {"margin_u_low": (-(c.cu + thr + 40) / c.fu, -(c.cu + thr - 40) / c.fu),
            "margin_v_low": (-(c.cv + thr + 40) / c.fv, -(c.cv + thr - 40) / c.fv),
            "margin_u_high": ((c.w + thr - c.cu - 40) / c.fu, (c.w + thr - c.cu + 40) / c.fu),
            "margin_v_high": ((c.h + thr - c.cv - 40) / c.fv, (c.h + thr - c.cv + 40) / c.fv),
            "z_invalid": (0.5e-12, 2.0e-12), "cos10": (1.0e-3, 1.0), "cos06": (3.0, 4.0), "scale05": (2.0, 3.0),
            "tie": (1.0, 2.0), "clamp": (0.005, 0.02)}[edge]


def knife_modes(edge):
    return (False,) if edge in ("cos06", "scale05") else (False, True)


def knife_verdict(oracle, sc, thr, exclusive, edge):
    """per landmark: what the edge turns.  clamp changes no output: the census says which side took 0.01."""
    if edge == "clamp":
        out = []
        for l in range(len(sc["hp"])):
            cen = oracle.new_prepare_census()
            run_oracle(oracle, _one(sc, l), exclusive, thr, cen)
            out.append((oracle.prepare_census_dict(cen)["clamp_r"],))
        return out
    r = run_oracle(oracle, sc, exclusive, thr)
    return [(int(r["status"][l]), int(r["n_desc"][l])) +
            tuple(int(x) - int(sc["obs_begin"][l]) if x >= 0 else -1 for x in r["obs_rows"][l])  # rows within the list
            for l in range(len(sc["hp"]))]


def _one(sc, l):
    """the table cut to landmark l"""
    a, b = int(sc["obs_begin"][l]), int(sc["obs_begin"][l + 1])
    out = dict(sc)
    out.update(hp=sc["hp"][l:l + 1], quality=sc["quality"][l:l + 1], obs_begin=np.array([0, b - a], np.int32),
               obs_pose=sc["obs_pose"][a:b], obs_desc=sc["obs_desc"][a:b], obs_bp=sc["obs_bp"][a:b])
    return out


def knife_edge(oracle, edge, exclusive, copies=33):
    """Bisects the edge's scalar under the oracle's CURRENT summation order.  Returns (table, thr, (lo, hi), calls):
    the table holds 2 * copies landmarks, lo and hi alternating (even rows lo)."""
    calls = [0]
    negative = _knife_range(edge, exclusive)[1] < 0

    def f(v):
        calls[0] += 1
        sc, thr = _knife_table(edge, [-v if negative else v], exclusive)
        return knife_verdict(oracle, sc, thr, exclusive, edge)[0][:2 if edge != "tie" else 5]

    a, b = _knife_range(edge, exclusive)
    lo, hi = bisect_adjacent(f, abs(a), abs(b))
    if negative:
        lo, hi = -hi, -lo
    sc, thr = _knife_table(edge, [lo, hi] * copies, exclusive)
    sc["name"] += "-excl" if exclusive else ""
    return sc, thr, (lo, hi), calls[0]


def z_sign_table():
    """`z > 0` is only asked for |z| >= 1e-12, so no two adjacent inputs straddle it.  The nearest of each side
    instead, at the centre of the image: z = +1e-12 (Successful), z = -1e-12 (Behind), and the former with all four
    of hp negated (hp_C[2] = -1e-12, and the head is negated back: Successful).  Rows cycle through the three."""
    rng = np.random.default_rng(32)
    t = _Table(camera("euroc"), _IDENTITY, rng)
    eye = np.eye(3)
    for i in range(48):
        z = (1.0e-12, -1.0e-12, 1.0e-12)[i % 3]
        p = np.array([1.0e-14, -2.0e-14, z])
        obs = [t.at(eye, -0.01 * (rodrigues((np.cos(k), np.sin(k), 0.0), 0.2 + 0.1 * k) @ np.array([0, 0, 1.0])), p)
               for k in range(3)]
        t.landmark(_homogeneous(p, -1.0 if i % 3 == 2 else 1.0), 1.0, obs)
    return t.finish("knife-z-sign", [9, 99])


# ---- census -----------------------------------------------------------------------------------------
def all_census(oracle=O, match=""):
    """{mode: counters} summed over the general scenes whose name contains `match`"""
    tot = {"non-exclusive": oracle.new_prepare_census(), "exclusive": oracle.new_prepare_census()}
    for sc in general_scenes():
        if match in sc["name"]:
            for exclusive, thr in MODES:
                run_oracle(oracle, sc, exclusive, thr, tot["exclusive" if exclusive else "non-exclusive"])
    return tot


def format_census(tot):
    labels = O.prepare_census_labels()
    lines = [f"{'label':<18}" + "".join(f"{m:>15}" for m in tot)]
    for i, lab in enumerate(labels):
        lines.append(f"{lab:<18}" + "".join(f"{int(tot[m][i]):>15}" for m in tot))
    return "\n".join(lines)


if __name__ == "__main__":
    print(format_census(all_census(match=sys.argv[1] if len(sys.argv) > 1 else "")))
