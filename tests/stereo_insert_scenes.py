"""Scenes for okvfe_stereo_insert_blocks_device (matchStereo's landmark bookkeeping, Frontend.cpp:2076-2141) and the
helpers that run them on the device.  Two kinds: rigs built from geometry (synth.py's EuRoC pair and Hilti extrinsics,
ransac_scenes.py's turned rigs, the four camera models; keypoints at projections of one point cloud, matcher rows derived
from which keypoints see the same point, with wrong and repeated k1, bad k1 and every kind of carried id mixed in) and
hand-built multiframes on undistorted cameras with a dyadic focal length, where the projection is exact.  Every scene is
one call: a table (hp, initialised), a rig, an ordered pair list and a batch of multiframes."""
import dataclasses
import functools

import numpy as np

import ransac_scenes as RS
import stereo_insert_ref as SR
from gate_scenes import bisect_adjacent, rodrigues
from okvis2_amd import capi, synth

K = 260            # keypoint capacity of the contexts: just above 256, so that the 256-row edge exists
W, H = 320, 240
L = 400            # rows of every scene's table
SENTINEL = -7
ACTION_SENTINEL = 0x77
PAST_COUNT_ROW = 5  # a valid table row in the landmark rows at or past a block's count: must be ignored
FLOOR = 16          # every census label is reached at least this often by the scenes together

I3 = np.eye(3).reshape(-1)


def camera(kind):
    """the camera models of ransac_scenes.py scaled to the W x H context"""
    if kind == "dyadic":  # undistorted, fu = fv = 256: u = 256 x / z + 160 is exact for dyadic x / z
        return dataclasses.replace(RS.camera("nodist"), w=W, h=H, fu=256.0, fv=256.0, cu=160.0, cv=120.0)
    base = RS.camera(kind)
    s = W / base.w
    return dataclasses.replace(base, w=W, h=H, fu=base.fu * s, fv=base.fv * s, cu=0.5 * W + 3.25, cv=0.5 * H - 2.5)


def all_pairs(n):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def rows(n):
    r = np.zeros(n, dtype=capi.STEREO_MATCH_DTYPE)
    r["k1"] = -1
    r["dist"] = 60
    return r


def keypoints(oracle, xy):
    kps = np.zeros(len(xy), dtype=oracle.KEYPOINT_DTYPE)
    if len(xy):
        xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
        kps["x"], kps["y"] = xy[:, 0], xy[:, 1]
    kps["size"] = 12.0
    return kps


def junk_points(rng, n):
    """table rows nothing sensible projects from: far off, behind, w of 0.0 / -0.0 / negative, NaN"""
    hp = np.concatenate([rng.uniform(-8, 8, (n, 3)), np.ones((n, 1))], axis=1)
    w = rng.choice(np.array([1.0, 1.0, 0.0, -0.0, -1.0, 0.5, np.nan]), n)
    hp[:, 3] = w
    hp[rng.random(n) < 0.1, 0] = np.nan
    return hp


# ---- rigs built from geometry ---------------------------------------------------------------------------------------
def rig_scene(oracle, name, cams, T_SC, pairs, counts, seed, keyframes=None, K=K, L=L, dense=False):
    """counts: per multiframe the keypoints per camera.  K, L: the keypoint capacity of the context and the rows of the
    table the scene is built for (default: the module's).  dense: every keypoint carries a table row of its own, no row
    is initialised, every k0 matches a k1 of its own and every match is initialisable (equal counts per multiframe), so
    that a pair's key table holds 2 count entries and every row whose first camera comes to the pair with its ids still
    untouched re-initialises its landmark into the overlay."""
    rng = np.random.default_rng(seed)
    n_cams, n_pts = len(cams), 300
    d = rng.normal(size=(n_pts, 3))
    d[: n_pts // 2, 2] = np.abs(d[: n_pts // 2, 2]) + 1.5  # half of the cloud in front of a forward-looking rig
    P = d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(2.5, 6.0, n_pts)[:, None]
    hp = np.concatenate([P, np.ones((n_pts, 1))], axis=1)
    scale = rng.choice(np.array([1.0, 1.0, 2.0, -1.0, 0.25]), n_pts)  # homogeneous: any non-zero multiple, sign included
    hp = np.concatenate([hp * scale[:, None], junk_points(rng, L - n_pts)])
    initialised = (rng.random(L) < 0.55).astype(np.uint8)
    if dense:
        initialised[:] = 0
    bad_ids = np.array([-2, L, L + 5, -1000, 2 ** 31 - 1], np.int64)
    mfs = []
    for mi, cnt in enumerate(counts):
        T_WS = (rodrigues(rng.normal(size=3), 0.03 * rng.random()), 0.05 * rng.normal(size=3))
        T_WC = [RS.compose(T_WS, T_SC[c]) for c in range(n_cams)]
        kps, ids, pt_of, kp_of = [], [], [], []
        own_rows = rng.permutation(L)[:sum(cnt)] if dense else None
        for c, cam in enumerate(cams):
            C, r = T_WC[c][0].reshape(3, 3), T_WC[c][1]
            xy, pts = [], []
            for j in rng.permutation(n_pts):
                if len(xy) >= cnt[c] * 4 // 5:
                    break
                st, pt = SR.R.project(oracle, cam, C.T @ (P[j] - r))
                if st != 0:
                    continue
                noise = rng.normal(0, 0.6, 2) if rng.random() < 0.85 else rng.normal(0, 4.0, 2)
                xy.append(pt + noise), pts.append(int(j))
            while len(xy) < cnt[c]:
                xy.append(rng.uniform((0, 0), (W, H))), pts.append(-1)
            k = keypoints(oracle, xy)
            nan = rng.random(cnt[c]) < 0.04
            k["x"][nan] = np.nan
            idc = np.full(cnt[c], -1, np.int64)
            u = rng.random(cnt[c])
            pts_a = np.array(pts, dtype=np.int64)
            own = (u < 0.35) & (pts_a >= 0)
            idc[own] = pts_a[own]                                   # the landmark the keypoint really sees
            other = (u >= 0.35) & (u < 0.45)
            idc[other] = rng.integers(0, L, int(other.sum()))       # any table row
            bad = (u >= 0.45) & (u < 0.5)
            idc[bad] = rng.choice(bad_ids, int(bad.sum()))          # outside [-1, L): read as none
            if dense:
                idc = own_rows[sum(cnt[:c]):sum(cnt[:c + 1])]
            kps.append(k), ids.append(idc.astype(np.int32)), pt_of.append(pts_a)
            kp_of.append({j: i for i, j in reversed(list(enumerate(pts))) if j >= 0})
        matches = []
        for c0, c1 in pairs:
            n0, n1 = cnt[c0], cnt[c1]
            r = rows(n0)
            hubs = rng.integers(0, n1, 4) if n1 else np.zeros(0, np.int64)
            if dense:
                assert n0 == n1
                k1_of = rng.permutation(n1)
            for k0 in range(n0):
                j = int(pt_of[c0][k0])
                u = rng.random()
                if dense:
                    k1, p = int(k1_of[k0]), P[j] if j >= 0 else rng.uniform(-4, 4, 3)
                elif j >= 0 and j in kp_of[c1] and u < 0.8:
                    k1, p = kp_of[c1][j], P[j] + rng.normal(0, 0.004, 3)
                elif n1 and u < 0.9:
                    k1 = int(rng.choice(hubs)) if rng.random() < 0.7 else int(rng.integers(0, n1))
                    p = P[j] if j >= 0 and rng.random() < 0.5 else rng.uniform(-4, 4, 3)
                elif u < 0.93:
                    k1, p = int(rng.choice([n1, K - 1, K, -5, 100000])), rng.uniform(-4, 4, 3)
                else:
                    continue
                r["k1"][k0], r["dist"][k0] = k1, int(rng.integers(0, 60))
                r["initialisable"][k0] = int(rng.choice([1, 7] if dense else [0, 1, 1, 7]))
                s = 1.0 if r["initialisable"][k0] else rng.choice([1.0, 0.5, -0.5])  # (not normalised when parallel)
                r["hp_W"][k0] = np.concatenate([p * s, [s]])
            matches.append(r)
        kf = True if keyframes is None else bool(keyframes[mi])
        mfs.append(dict(kps=kps, ids=ids, T_WC=T_WC, matches=matches, keyframe=kf))
    return dict(name=name, cams=cams, hp=hp, initialised=initialised, pairs=list(pairs), mfs=mfs, K=K)


# ---- the edges of the kernel's two open-addressed tables ---------------------------------------------------------------
MAX_LDS = 65280   # the call's limit on the LDS of one work-group


def lds_bytes(n_cams, Kc):
    """stereo_insert_lds_bytes restated: (bytes, log2 of the overlay's slots, log2 of the key table's slots) -- both
    tables have the first power of two ABOVE what they may hold (n_cams Kc re-initialising rows, 2 Kc keys)"""
    a = b = 1
    while (1 << a) <= n_cams * Kc:
        a += 1
    while (1 << b) <= 2 * Kc:
        b += 1
    return 4 * (n_cams * Kc + (1 << a) + 3 * Kc + (1 << b)), a, b


def largest_capacity(n_cams):
    """the largest keypoint capacity whose tables fit MAX_LDS"""
    return max(k for k in range(1, 4097) if lds_bytes(n_cams, k)[0] <= MAX_LDS)


def table_edge_scene(oracle, n_cams, Kc, seed=7):
    """one dense multiframe of full blocks on a rig of dyadic cameras in a ring of pairs (0, 1), (1, 2), ..., (n - 1, 0):
    every camera is once the first of a pair, so n_cams Kc rows re-initialise a landmark -- all the overlay may hold"""
    cams = [camera("dyadic")] * n_cams
    T_SC = [(I3.copy(), np.array([0.125 * c, 0.0, 0.0])) for c in range(n_cams)]
    pairs = [(c, (c + 1) % n_cams) for c in range(n_cams)]
    return rig_scene(oracle, "table-edge-%dx%d" % (n_cams, Kc), cams, T_SC, pairs, [(Kc,) * n_cams], seed, K=Kc,
                     L=n_cams * Kc + 77, dense=True)


def reference_of(oracle, tree, sc):
    """(per multiframe results, census) of a scene, uncached"""
    oracle.set_reduction(tree)
    census = SR.new_census()
    return [SR.stereo_insert(oracle, tree, sc["hp"], sc["initialised"], sc["cams"], sc["pairs"], sc["K"], mf["kps"],
                             mf["ids"], mf["T_WC"], mf["matches"], mf["keyframe"], census) for mf in sc["mfs"]], census


def euroc_T_SC():
    return [(I3.copy(), np.zeros(3)), (I3.copy(), np.array([synth.euroc_config().baseline, 0.0, 0.0]))]


@functools.lru_cache(maxsize=None)
def rig_scenes(oracle):
    hil = synth.hilti_config()
    out = [
        # EuRoC stereo: a not-keyframe multiframe between keyframes
        rig_scene(oracle, "euroc-stereo", [camera("euroc"), camera("euroc1")], euroc_T_SC(), [(0, 1)],
                  [(200, 180), (150, 170), (120, 90)], 1, keyframes=(1, 0, 1)),
        # the block sizes: 0, 1, 255, 256, 257 and K rows on either side
        rig_scene(oracle, "stereo-counts", [camera("nodist"), camera("radtan8")], euroc_T_SC(), [(0, 1)],
                  [(0, 7), (7, 0), (1, 1), (255, 256), (256, 255), (257, K), (K, 257), (K, K)], 2),
        # three cameras of Hilti's extrinsics, every pair; the four camera models over the two 3-camera rigs
        rig_scene(oracle, "hilti-3", [camera("equi"), camera("equi"), camera("radtan8")], hil.T_SC[:3], all_pairs(3),
                  [(140, 130, 120), (90, 100, 110)], 3, keyframes=(1, 0)),
        rig_scene(oracle, "turned-3", [camera("euroc"), camera("nodist"), camera("equi")],
                  RS.rig(("euroc", "nodist", "equi"))[1], all_pairs(3), [(160, 150, 140), (100, 0, 100)], 4),
        # Hilti's five cameras, nine pairs (every pair but (2, 4))
        rig_scene(oracle, "hilti-5", list(map(lambda c: camera("equi"), range(5))), hil.T_SC,
                  [pr for pr in all_pairs(5) if pr != (2, 4)], [(100, 90, 80, 70, 60), (60, 70, 80, 90, 100)], 5,
                  keyframes=(1, 1)),
        rig_scene(oracle, "turned-5", [camera(k) for k in ("euroc", "euroc1", "nodist", "equi", "radtan8")],
                  RS.rig(("euroc",) * 5)[1], all_pairs(5), [(90, 80, 70, 60, 50)], 6),
    ]
    return tuple(out)


# ---- hand-built multiframes -------------------------------------------------------------------------------------------
class Builder:
    """One multiframe on n dyadic cameras: camera c looks along z from (0.125 c, 0, 0).  Table rows are shared by the
    multiframes of a scene (Table)."""

    def __init__(self, oracle, table, n_cams=3, pairs=None, keyframe=True):
        self.oracle, self.table, self.n = oracle, table, n_cams
        self.pairs = all_pairs(n_cams) if pairs is None else pairs
        self.cams = [camera("dyadic")] * n_cams
        self.T_WC = [(I3.copy(), np.array([0.125 * c, 0.0, 0.0])) for c in range(n_cams)]
        self.xy = [[] for _ in range(n_cams)]
        self.ids = [[] for _ in range(n_cams)]
        self.rows = [[] for _ in self.pairs]
        self.keyframe = keyframe

    def proj(self, c, P):
        P = np.asarray(P, dtype=np.float64)
        return np.array([256.0 * (P[0] - 0.125 * c) / P[2] + 160.0, 256.0 * P[1] / P[2] + 120.0])

    def kp(self, c, P=None, off=(0.0, 0.0), lm=-1, xy=None):
        """a keypoint of camera c at the projection of P (+ off), carrying lm; -> its index"""
        xy = self.proj(c, P) + np.asarray(off) if xy is None else np.asarray(xy, dtype=np.float64)
        self.xy[c].append(xy), self.ids[c].append(lm)
        return len(self.xy[c]) - 1

    def row(self, p, k0, k1, hp, initialisable=1):
        hp = np.asarray(hp, dtype=np.float64)
        self.rows[p].append((k0, k1, initialisable, hp if len(hp) == 4 else np.concatenate([hp, [1.0]])))

    def build(self):
        kps = [keypoints(self.oracle, xy) for xy in self.xy]
        matches = []
        for p, (c0, c1) in enumerate(self.pairs):
            r = rows(len(kps[c0]))
            for k0, k1, ini, hp in self.rows[p]:
                assert r["k1"][k0] == -1, "one row per k0"
                r["k1"][k0], r["dist"][k0], r["initialisable"][k0], r["hp_W"][k0] = k1, 10, ini, hp
            matches.append(r)
        assert all(len(k) <= K for k in kps)
        return dict(kps=kps, ids=[np.array(i, dtype=np.int32) for i in self.ids], T_WC=self.T_WC, matches=matches,
                    keyframe=self.keyframe)


class Table:
    def __init__(self):
        self.hp, self.init = [], []

    def add(self, hp, initialised=True):
        hp = np.asarray(hp, dtype=np.float64)
        self.hp.append(hp if len(hp) == 4 else np.concatenate([hp, [1.0]]))
        self.init.append(1 if initialised else 0)
        assert len(self.hp) < L
        return len(self.hp) - 1

    def finish(self, last):
        """filled up to L rows with junk; row L - 1 is `last` (hp, initialised)"""
        rng = np.random.default_rng(77)
        n = L - 1 - len(self.hp)
        hp = np.concatenate([np.array(self.hp).reshape(-1, 4), junk_points(rng, n), np.asarray(last[0]).reshape(1, 4)])
        init = np.concatenate([np.array(self.init, np.uint8), (rng.random(n) < 0.5).astype(np.uint8),
                               np.array([last[1]], np.uint8)])
        return hp, init


def _grid(i, z=4.0):
    """point i of a lattice in front of all cameras, neighbours far more than 4 px apart"""
    return np.array([-1.25 + 0.25 * (i % 10), -0.75 + 0.25 * ((i // 10) % 7), z + 0.5 * (i // 70)])


def chain_mf(oracle, table, n, first):
    """chains of n rows on one k1, 18 of them shrunk to what fits K when n is 65: row j sits j x 0.05 px off, so a long
    chain crosses nothing, while every fourth follower sits 6 px off and fails the check"""
    b = Builder(oracle, table, 2)
    copies = 18 if n < 10 else 3
    for i in range(copies):
        P = _grid(i + 7 * n)
        k1 = b.kp(1, P)
        for j in range(n):
            off = (6.0, 0.0) if j % 4 == 3 else (0.05 * j, -0.03 * j)
            lm = -1
            if j == 0 and first == "succeeds":
                lm = table.add(P, initialised=i % 2 == 0)
            if j == 0 and first == "fails":
                lm = table.add(P + np.array([0.5, 0.0, 0.0]))  # 32 px off: add1 fails, the k1 stays free
            k0 = b.kp(0, P, off, lm)
            hp = P + np.array([0.0, 0.001 * j, 0.0])
            b.row(0, k0, k1, hp, initialisable=j % 3 != 2)
    return b.build()


def all_on_zero_mf(oracle, table):
    """every row of a full block matches k1 = 0"""
    b = Builder(oracle, table, 2)
    P = _grid(33)
    b.kp(1, P)
    for j in range(K):
        b.row(0, b.kp(0, P, (0.01 * j, 0.0) if j % 5 else (0.0, 5.0)), 0, P)
    return b.build()


def shared_landmark_mf(oracle, table, copies=18):
    """(a) two keypoints of image 0 carry one uninitialised landmark and match two k1 that both carry ids: the first
    re-initialises, the second finds it initialised; (b) a landmark carried by a k0 and by a k1 other than its match: the
    chain of that k1 reads the point row k0 re-set (entangled chains); (c) two k0 of one landmark, k1 free: both add1"""
    b = Builder(oracle, table, 2)
    for i in range(copies):
        P, Q = _grid(2 * i), _grid(2 * i + 1)
        P2 = P + np.array([0.0, 1.0 / 128.0, 0.0])  # 0.5 px from P at z = 4
        a = table.add(P, initialised=False)
        x, y = table.add(Q), table.add(Q, initialised=i % 2 == 0)
        # (a)
        k0a, k0b = b.kp(0, P, lm=a), b.kp(0, P, (1.0, 0.0), lm=a)
        b.row(0, k0a, b.kp(1, P, lm=x), P2, initialisable=1)
        b.row(0, k0b, b.kp(1, P, (0.0, 1.0), lm=y), P + np.array([1.0, 0.0, 0.0]), initialisable=1)
        # (b): a third k1 carries `a` and is matched by a k0 without a landmark: add0 reads the point (a) re-set
        k1c = b.kp(1, P, (0.5, 0.5), lm=a)
        b.row(0, b.kp(0, P2, (0.0, 0.0)), k1c, Q)
        b.row(0, b.kp(0, P, (0.0, -3.9)), k1c, Q)  # 3.9 px from P, 4.4 px from P2: only the re-set point rejects it
        # (c)
        u = table.add(Q, initialised=True)
        b.row(0, b.kp(0, Q, lm=u), b.kp(1, Q), Q)
        b.row(0, b.kp(0, Q, (0.5, 0.0), lm=u), b.kp(1, Q, (0.0, 0.5)), Q)
    return b.build()


def across_pairs_mf(oracle, table, copies=18, keyframe=True):
    """a creation in pair (0,1) (not initialisable) that pair (0,2) re-initialises with another point and pair (1,2)
    reads: the keypoint of camera 2 sits at the projection of the NEW point, 8 px from the old one's"""
    b = Builder(oracle, table, 3, keyframe=keyframe)
    for i in range(copies):
        P = _grid(i, z=4.0)
        Pn = P + np.array([0.0, 1.0 / 8.0, 0.0])  # 8 px off at z = 4
        ka, kb = b.kp(0, P), b.kp(1, P)
        b.row(0, ka, kb, P, initialisable=0)
        x = table.add(Pn)
        kc = b.kp(2, Pn, lm=x)
        b.row(1, ka, kc, Pn, initialisable=1 if i % 6 else 0)  # (every sixth stays as created: pair (1,2) then rejects)
        kd = b.kp(2, Pn, (0.25, 0.0))
        b.row(2, kb, kd, P)
    return b.build()


def bad_k1_and_ids_mf(oracle, table, last_row_point, copies=18):
    """k1 at and past count(c1) and negative; input ids of -1, -2, L - 1 and L on either side of a match"""
    b = Builder(oracle, table, 2)
    ids = (-1, -2, L - 1, L)
    for i in range(copies):
        P = last_row_point if i % 2 == 0 else _grid(i)
        id0, id1 = ids[i % 4], ids[(i // 4) % 4]
        b.row(0, b.kp(0, P, lm=id0), b.kp(1, P, lm=id1), P, initialisable=i % 3)
    n1 = len(b.xy[1])
    for i, k1 in enumerate((n1 - 1, n1, n1 + 1, K - 1, K, K + 1, 1 << 20, -1, -2, -(1 << 31), (1 << 31) - 1)):
        b.row(0, b.kp(0, _grid(40 + i), lm=(L - 1 if i % 2 else -1)), k1, _grid(40 + i))
    return b.build()


def failed_projection_mf(oracle, table, copies=18):
    """landmarks and triangulated points that do not project: behind the camera, hp[3] of 0.0 / -0.0 / negative, NaN; and
    keypoints with a NaN coordinate under a landmark that does project (the NaN norm adds nothing)"""
    b = Builder(oracle, table, 2)
    specials = ([0.1, 0.1, -3.0, 1.0], [0.1, 0.1, 3.0, 0.0], [0.1, 0.1, 3.0, -0.0], [-0.1, -0.1, -3.0, -1.0],
                [0.1, 0.1, -3.0, -1.0], [np.nan, 0.1, 3.0, 1.0], [0.1, 0.1, 3.0, np.nan], [0.1, 0.1, 1.0e-13, 1.0],
                [40.0, 0.1, 3.0, 1.0])
    for i in range(copies):
        hp = np.array(specials[i % len(specials)])
        P = np.array([0.1, 0.1, 3.0])
        t = table.add(hp)
        b.row(0, b.kp(0, P, lm=t), b.kp(1, P), P)            # only id0: add1 through the table's point
        b.row(0, b.kp(0, P), b.kp(1, P, lm=t), P)            # only id1: add0
        b.row(0, b.kp(0, P), b.kp(1, P), hp, initialisable=i % 2)  # creation from the special point: both
        g = _grid(i)
        u = table.add(g)
        nan0, nan1 = (np.nan, 100.0), (100.0, np.nan)
        b.row(0, b.kp(0, xy=nan0), b.kp(1, g, lm=u), g)      # add0 on a NaN keypoint
        b.row(0, b.kp(0, g, lm=u), b.kp(1, xy=nan1), g)      # add1 on a NaN keypoint
        b.row(0, b.kp(0, xy=nan1), b.kp(1, xy=nan0), g)      # creation: both NaN
    return b.build()


def edge_mf(oracle, tree, table):
    """the 4 px edge on camera 0 (at the origin: u = 256 x / z + 160 exactly): a keypoint exactly 4.0 px away adds
    nothing; a point coordinate bisected to two adjacent doubles with different verdicts"""
    b = Builder(oracle, table, 2)
    cam = b.cams[0]
    for i, (off, expect) in enumerate((((4.0, 0.0), False), ((0.0, -4.0), False), ((3.99999, 0.0), True),
                                       ((np.nextafter(np.float32(164.0), np.float32(0)) - 160.0, 0.0), True))):
        P = np.array([0.0, 0.0, 2.0 + i])  # projects to (160, 120) exactly
        t = table.add(P)
        k0 = b.kp(0, P, off)
        b.row(0, k0, b.kp(1, P, lm=t), P)
        b.expect = getattr(b, "expect", []) + [(k0, expect)]
    # bisection: keypoint at (163.5, 120); point (x, 0, 1): accepted while 256 x + 160 > 159.5
    kp = keypoints(oracle, [(163.5, 120.0)])

    def accepted(x):
        st, proj = SR.R.project(oracle, cam, SR.R.pose_inverse_times(tree, b.T_WC[0], [x - 1.0, 0.0, 1.0, 1.0])[:3])
        dx, dy = np.float64(kp["x"][0]) - proj[0], np.float64(kp["y"][0]) - proj[1]
        return bool(st == 0 and np.sqrt(dx * dx + dy * dy) < 4.0)

    lo, hi = bisect_adjacent(accepted, 1.0 - 1.0 / 256.0, 1.0)  # x - 1 in [-1/256, 0]: 159 .. 160
    assert accepted(lo) != accepted(hi) and np.nextafter(lo, 2.0) == hi
    for x in (lo, hi):
        t = table.add([x - 1.0, 0.0, 1.0, 1.0])
        k0 = b.kp(0, xy=(163.5, 120.0))
        b.row(0, k0, b.kp(1, [x - 1.0, 0.0, 1.0], lm=t), [0.0, 0.0, 1.0])
        b.expect.append((k0, accepted(x)))
    mf = b.build()
    mf["expect_obs0"] = b.expect
    return mf


@functools.lru_cache(maxsize=None)
def directed_scenes(oracle, tree):
    """the hand-built multiframes, grouped by rig into calls; the edge scene depends on the FP64 order"""
    out = []
    for first in ("succeeds", "fails", "creates"):
        table = Table()
        mfs = [chain_mf(oracle, table, n, first) for n in (2, 3, 65)]
        if first == "creates":
            mfs.append(all_on_zero_mf(oracle, table))
        hp, init = table.finish(([0.0, 0.0, 5.0, 1.0], 1))
        out.append(dict(name="chains-first-" + first, cams=[camera("dyadic")] * 2, hp=hp, initialised=init,
                        pairs=[(0, 1)], mfs=mfs))
    table = Table()
    last = np.array([0.25, -0.25, 5.0])
    mfs = [shared_landmark_mf(oracle, table), bad_k1_and_ids_mf(oracle, table, last), failed_projection_mf(oracle, table),
           edge_mf(oracle, tree, table)]
    hp, init = table.finish((np.concatenate([last, [1.0]]), 0))
    out.append(dict(name="shared-bad-failed-edge", cams=[camera("dyadic")] * 2, hp=hp, initialised=init, pairs=[(0, 1)],
                    mfs=mfs))
    table = Table()
    mfs = [across_pairs_mf(oracle, table), across_pairs_mf(oracle, table, keyframe=False), across_pairs_mf(oracle, table)]
    hp, init = table.finish(([0.0, 0.0, 5.0, 1.0], 1))
    out.append(dict(name="across-pairs", cams=[camera("dyadic")] * 3, hp=hp, initialised=init, pairs=all_pairs(3),
                    mfs=mfs))
    return tuple(out)


def all_scenes(oracle, tree):
    return rig_scenes(oracle) + directed_scenes(oracle, tree)


@functools.lru_cache(maxsize=None)
def reference(oracle, tree, name, all_keyframes=False):
    """(per multiframe results, census) of the scene called `name`, computed once; all_keyframes: what a call without
    keyframe flags must give"""
    sc = {s["name"]: s for s in all_scenes(oracle, tree)}[name]
    oracle.set_reduction(tree)
    census = SR.new_census()
    refs = [SR.stereo_insert(oracle, tree, sc["hp"], sc["initialised"], sc["cams"], sc["pairs"], K, mf["kps"], mf["ids"],
                             mf["T_WC"], mf["matches"], all_keyframes or mf["keyframe"], census) for mf in sc["mfs"]]
    return refs, census


# ---- GPU side ---------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        a = np.zeros((1,) + a.shape[1:], dtype=a.dtype)
    return torch.from_numpy(a).cuda()


def prepare(fe, sc, layout="multiframe-major", alias=False, optional=True, keyframe_flags=True, only=None):
    """the device tensors of one call over the multiframes `only` (default all); synchronises"""
    import torch
    from okvis2_amd import multigpu
    K = sc.get("K", globals()["K"])
    assert fe.max_keypoints == K
    mfs = sc["mfs"] if only is None else [sc["mfs"][i] for i in only]
    B, n_cams, n_pairs = len(mfs), len(sc["cams"]), len(sc["pairs"])
    strides = (n_cams, 1) if layout == "multiframe-major" else (1, B)
    bb = multigpu.block_layout(K)["total"]
    blocks = np.zeros((B * n_cams, bb), np.uint8)
    lm = np.full((B * n_cams, K), PAST_COUNT_ROW, np.int32)
    matches = np.zeros((n_pairs, B, K), dtype=capi.STEREO_MATCH_DTYPE)
    matches["k1"] = 3  # rows at or past the count: a valid-looking match that must not be read
    for m, mf in enumerate(mfs):
        for c in range(n_cams):
            n = len(mf["kps"][c])
            b = m * strides[0] + c * strides[1]
            blocks[b] = multigpu.pack_block_host(K, mf["kps"][c], np.zeros((n, 48), np.uint8), np.zeros((n, 3)),
                                                 np.zeros(n, np.uint8))
            lm[b, :n] = mf["ids"][c]
        for p, (c0, _) in enumerate(sc["pairs"]):
            matches[p, m, :len(mf["kps"][c0])] = mf["matches"][p]
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
    T = dict(blocks=_dev(blocks), lm=_dev(lm), matches=_dev(matches.view(np.uint8)), hp=_dev(sc["hp"]),
             initialised=_dev(sc["initialised"]), counts=full((B, 4), SENTINEL, torch.int32))
    T["lm_out"] = T["lm"] if alias else full(lm.shape, SENTINEL, torch.int32)
    if optional:
        T["action"] = full((n_pairs, B, K), ACTION_SENTINEL, torch.uint8)
        T["lm_row"] = full((n_pairs, B, K), SENTINEL, torch.int32)
    if keyframe_flags:
        T["keyframe"] = _dev(np.array([1 if mf["keyframe"] else 0 for mf in mfs], np.uint8))
    T.update(strides=strides, mfs=mfs, alias=alias, matches_np=matches)
    torch.cuda.synchronize()
    return T


def launch(fe, sc, T, stream=None):
    """the call alone: nothing here waits for the device"""
    mfs = T["mfs"]
    ptr = lambda k: T[k].data_ptr() if k in T else None
    tab = fe.make_landmark_table_device(len(sc["hp"]), 0, 0, T["hp"].data_ptr(), 0, 0, 0, 0, 0, 0)
    res = fe.make_stereo_insert_device(ptr("action"), ptr("lm_row"), ptr("lm_out"), ptr("counts"))
    fe.stereo_insert_blocks_device(tab, T["initialised"].data_ptr(), T["blocks"].data_ptr(), T["strides"][0],
                                   T["strides"][1], len(mfs), sc["pairs"], list(range(len(sc["cams"]))),
                                   [mf["T_WC"][c] for mf in mfs for c in range(len(sc["cams"]))], T["matches"].data_ptr(),
                                   T["lm"].data_ptr(), ptr("keyframe"), res, stream)


def launch_slice(fe, sc, T, first, count, stream=None):
    """the multiframes [first, first + count) of a prepared batch as a call of their own: blocks, landmark rows, counts
    and keyframe flags are the batch's, addressed through the base pointers and the batch's strides; the matcher rows
    (pair-major over the CALL's multiframes) are packed for the slice, and action / lm come back in the batch's arrays"""
    import torch
    n_cams, n_pairs = len(sc["cams"]), len(sc["pairs"])
    sm = T["strides"][0]
    at = lambda k, per: T[k].data_ptr() + first * per * T[k].element_size() if k in T else None
    d_matches = _dev(np.ascontiguousarray(T["matches_np"][:, first:first + count]).view(np.uint8))
    d_action = torch.full((n_pairs, count, K), ACTION_SENTINEL, dtype=torch.uint8, device="cuda")
    d_lm_row = torch.full((n_pairs, count, K), SENTINEL, dtype=torch.int32, device="cuda")
    tab = fe.make_landmark_table_device(len(sc["hp"]), 0, 0, T["hp"].data_ptr(), 0, 0, 0, 0, 0, 0)
    res = fe.make_stereo_insert_device(d_action.data_ptr(), d_lm_row.data_ptr(), at("lm_out", sm * K), at("counts", 4))
    mfs = T["mfs"][first:first + count]
    fe.stereo_insert_blocks_device(tab, T["initialised"].data_ptr(), at("blocks", sm * T["blocks"].shape[1]),
                                   T["strides"][0], T["strides"][1], count, sc["pairs"], list(range(n_cams)),
                                   [mf["T_WC"][c] for mf in mfs for c in range(n_cams)], d_matches.data_ptr(),
                                   at("lm", sm * K), at("keyframe", 1), res, stream)
    torch.cuda.synchronize()
    T["action"][:, first:first + count] = d_action
    T["lm_row"][:, first:first + count] = d_lm_row


def check(sc, T, refs, what):
    """every output of every multiframe against the restatement, byte for byte; rows past the counts untouched"""
    import torch
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in T.items() if isinstance(v, torch.Tensor)}
    past = PAST_COUNT_ROW if T["alias"] else SENTINEL
    for m, (mf, ref) in enumerate(zip(T["mfs"], refs)):
        w = (sc["name"],) + tuple(what) + (m,)
        assert got["counts"][m].tolist() == ref["counts"].tolist(), (w, got["counts"][m], ref["counts"])
        for c in range(len(sc["cams"])):
            b, n = m * T["strides"][0] + c * T["strides"][1], len(mf["kps"][c])
            diff = np.flatnonzero(got["lm_out"][b, :n] != ref["ids"][c])
            assert diff.size == 0, (w, c, "landmark_out", diff[:8], got["lm_out"][b, diff[:8]], ref["ids"][c][diff[:8]])
            assert np.all(got["lm_out"][b, n:] == past), (w, c, "landmark_out past the count")
        if "action" not in got:
            continue
        for p, (c0, _) in enumerate(sc["pairs"]):
            n = len(mf["kps"][c0])
            diff = np.flatnonzero(got["action"][p, m, :n] != ref["action"][p])
            assert diff.size == 0, (w, p, "action", diff[:8], got["action"][p, m, diff[:8]], ref["action"][p][diff[:8]])
            diff = np.flatnonzero(got["lm_row"][p, m, :n] != ref["lm"][p])
            assert diff.size == 0, (w, p, "lm", diff[:8], got["lm_row"][p, m, diff[:8]], ref["lm"][p][diff[:8]])
            assert np.all(got["action"][p, m, n:] == ACTION_SENTINEL) and np.all(got["lm_row"][p, m, n:] == SENTINEL), (w, p)
    return got
