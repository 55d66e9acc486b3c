"""The gated matchers' Hamming scan (k_match.hip, scan_top) on hand-built descriptors.

Frontend.match_stereo on host arrays reaches match_stereo_arrays_kernel and so match_stereo_rows; every field of
every row is compared byte for byte with the oracle (hp_W as u64).  Distances are known by construction: a side-1
descriptor is a query's descriptor with a chosen number of bits flipped, and two different queries' descriptors are
random, far above the threshold apart (checked).  Geometry comes from 3-D points seen by both EuRoC cameras: a
candidate that observes the query's own point passes the FP64 gate, one that observes a point some image rows away
does not, and one with bpv = 0 is refused before the gate.  Each directed case also states the row it expects, so
the oracle and the device are both held to the scan's contract:

  threshold   the sentinel: dist = threshold - 1 admitted, threshold and threshold + 1 not
  ties        equal distances across segments and inside one: the lowest k1 that passes the gate
  floor       the first scan's second key, then re-scans above a floor; successor keys at floor + 1 and floor + 2
  six keys    nine candidates of which eight are refused: every insertion slot used and overflowed, in both orders
  sizes       remainders of the unrolled body, resident and streamed segments, query blocks around 32 and 64
  full cap    the winner at index kp_cap - 1 of a 2500-keypoint context: the key's low bits
  skip flags  match_motion_stereo with the would-be winners flagged
"""
import functools
import math

import numpy as np
import pytest

from okvis2_amd import synth

import gpu_common as G

pytestmark = pytest.mark.gpu

FIELDS = ("k1", "dist", "initialisable", "pad")
GOOD, BAD_ROW, NO_BP = 0, 1, 2  # a candidate's geometry: the query's own point, another row's point, bpv = 0


@functools.lru_cache(maxsize=None)
def _world():
    """the EuRoC rig, a frontend, and a pool of 3-D points with their observations in both cameras: computed once"""
    import oracle_lib as O
    cfg = synth.euroc_config()
    fe = G.make_frontend(cfg)
    T0, T1 = synth.stereo_poses(cfg.baseline)
    # 20 x 20 points, one image row band (~17 px) per grid row, depths 3 .. 8 m
    gy, gx = np.meshgrid(np.arange(20), np.arange(20), indexing="ij")
    z = 3.0 + 5.0 * ((gx * 7 + gy * 3) % 20) / 19.0
    X = np.stack([(gx - 9.5) * 0.055 * z, (gy - 9.5) * 0.037 * z, z], -1).reshape(-1, 3)
    obs = []
    for cam, T in zip(cfg.cams, (T0, T1)):
        kp = np.zeros(len(X), dtype=O.KEYPOINT_DTYPE)
        kp["size"] = 12.0
        for i, p in enumerate(X - np.asarray(T[1])):
            st, pt, _ = O.cam_project(cam, p)
            assert st == 0, (i, st)
            kp["x"][i], kp["y"][i] = pt
        bp, bv = O.backproject_keypoints(cam, kp)
        assert bv.all()
        obs.append((kp, bp, bv))
    f = [0.5 * (c.fu + c.fv) for c in cfg.cams]
    return O, cfg, fe, (T0, T1), f, obs


def _flip(desc, nbits, start):
    """desc with nbits bits flipped from bit `start` on (cyclic): Hamming distance exactly nbits"""
    bits = np.unpackbits(desc)
    idx = (start + np.arange(nbits)) % bits.size
    bits[idx] ^= 1
    return np.packbits(bits)


class Scene:
    """n0 queries (query i observes pool point i), n1 side-1 slots filled with far-away descriptors until placed"""

    def __init__(self, n0, n1, seed):
        O, cfg, fe, T, f, obs = _world()
        rng = np.random.default_rng(seed)
        self.n0, self.n1 = n0, n1
        self.npool = len(obs[0][0])
        self.q = np.arange(n0) % self.npool
        self.d0 = rng.integers(0, 256, (n0, 48), dtype=np.uint8)
        self.d1 = rng.integers(0, 256, (n1, 48), dtype=np.uint8)
        self.p1 = (np.arange(n1) * 7 + 3) % self.npool  # the pool point a side-1 slot observes
        self.v1 = np.ones(n1, np.uint8)
        self.owner = np.full(n1, -1)  # the query a placed slot was derived from

    def put(self, k1, query, dist, kind, start=None):
        assert self.owner[k1] < 0, k1
        self.owner[k1] = query
        self.d1[k1] = _flip(self.d0[query], dist, 11 * k1 if start is None else start)
        own = self.q[query]
        self.p1[k1] = own if kind != BAD_ROW else (own + 5 * 20) % self.npool  # five grid rows away
        self.v1[k1] = 0 if kind == NO_BP else 1

    def arrays(self):
        O, cfg, fe, T, f, obs = _world()
        (kpA, bpA, bvA), (kpB, bpB, bvB) = obs
        a0 = (self.d0, kpA[self.q], bpA[self.q], bvA[self.q])
        a1 = (self.d1, kpB[self.p1], bpB[self.p1], self.v1)
        return a0, a1

    def check_far(self):
        """every descriptor pair that was not built as (query, its candidate) is far above any threshold used here"""
        x = self.d0[:, None, :] ^ self.d1[None, :, :]
        D = np.unpackbits(x, axis=2).sum(2)
        foreign = self.owner[None, :] != np.arange(self.n0)[:, None]
        assert (D[foreign] > 120).all(), int(D[foreign].min())

    def run(self, threshold=None):
        O, cfg, fe, T, f, obs = _world()
        self.check_far()
        a0, a1 = self.arrays()
        thr = cfg.match_threshold if threshold is None else threshold
        ref = O.match_stereo(*a0, *a1, T[0], T[1], f[0], f[1], thr)
        got = fe.match_stereo(*a0, *a1, T[0], T[1], f[0], f[1])
        assert len(got) == len(ref) == self.n0
        for name in FIELDS:
            assert np.array_equal(got[name], ref[name]), (name, np.flatnonzero(got[name] != ref[name])[:8])
        assert np.array_equal(got["hp_W"].view(np.uint64), ref["hp_W"].view(np.uint64))
        assert got.tobytes() == ref.tobytes()
        return ref


def _expect(ref, query, k1, dist):
    assert (int(ref["k1"][query]), int(ref["dist"][query])) == (k1, dist), (query, ref[query])


def test_threshold_edge():
    O, cfg, *_ = _world()
    thr = cfg.match_threshold
    s = Scene(6, 40, 1)  # per segment: 10
    # query 0: threshold - 1, threshold, threshold + 1, all geometrically consistent, in three segments
    s.put(31, 0, thr - 1, GOOD); s.put(2, 0, thr, GOOD); s.put(15, 0, thr + 1, GOOD)
    # query 1: its best sits AT the threshold
    s.put(5, 1, thr, GOOD); s.put(22, 1, thr + 1, GOOD)
    # query 2: threshold - 1 refused by the gate, nothing else below: the refused key must not come back as a match
    s.put(7, 2, thr - 1, BAD_ROW); s.put(8, 2, thr, GOOD)
    # query 3: distance 0 and the largest admissible distance side by side
    s.put(11, 3, thr - 1, GOOD); s.put(12, 3, 0, GOOD)
    ref = s.run()
    _expect(ref, 0, 31, thr - 1)
    _expect(ref, 1, -1, thr)
    _expect(ref, 2, -1, thr)
    _expect(ref, 3, 12, 0)
    _expect(ref, 4, -1, thr)  # no candidate in any segment
    _expect(ref, 5, -1, thr)


def test_ties():
    s = Scene(5, 40, 2)
    # query 0: three at distance 10 in segments 0, 1 and 3; the first has no back-projection
    s.put(3, 0, 10, NO_BP); s.put(17, 0, 10, GOOD); s.put(33, 0, 10, GOOD)
    # query 1: three at distance 9 inside segment 2; the first fails the gate
    s.put(21, 1, 9, BAD_ROW); s.put(22, 1, 9, GOOD); s.put(25, 1, 9, GOOD)
    # query 2: a tie between the last slot of segment 0 and the first of segment 1, both valid
    s.put(9, 2, 12, GOOD); s.put(10, 2, 12, GOOD)
    # query 3: identical descriptors (distance 0 twice) in one segment
    s.put(36, 3, 0, GOOD, start=0); s.put(38, 3, 0, GOOD, start=0)
    # query 4: a tie where the HIGHER segment's candidate is the only valid one
    s.put(1, 4, 7, BAD_ROW); s.put(39, 4, 7, GOOD)
    ref = s.run()
    _expect(ref, 0, 17, 10)
    _expect(ref, 1, 22, 9)
    _expect(ref, 2, 9, 12)
    _expect(ref, 3, 36, 0)
    _expect(ref, 4, 39, 7)


def test_floor_first_successor():
    s = Scene(6, 64, 3)  # per segment: 16
    # query 0: the two best are refused (no back-projection, gate), the third is valid: second key, then a re-scan
    s.put(4, 0, 5, NO_BP); s.put(9, 0, 6, BAD_ROW); s.put(2, 0, 7, GOOD)
    # query 1: refused key and successor differ only in k1, by one: the floor subtraction lands on 0
    s.put(20, 1, 8, NO_BP); s.put(21, 1, 8, BAD_ROW); s.put(22, 1, 8, GOOD)
    # query 2: ... by two: it lands on 1
    s.put(40, 2, 8, BAD_ROW); s.put(41, 2, 8, NO_BP); s.put(43, 2, 8, GOOD)
    # query 3: the successor sits BELOW the refused keys in k1 but one distance up
    s.put(60, 3, 3, NO_BP); s.put(61, 3, 3, NO_BP); s.put(50, 3, 4, GOOD)
    # query 4: everything above the floor is refused as well: the re-scan comes back empty
    s.put(5, 4, 2, NO_BP); s.put(6, 4, 3, BAD_ROW); s.put(7, 4, 4, NO_BP)
    # query 5: refused twice in segment 1 while segment 3 holds a worse but valid candidate
    s.put(17, 5, 1, BAD_ROW); s.put(18, 5, 2, NO_BP); s.put(55, 5, 30, GOOD)
    ref = s.run()
    _expect(ref, 0, 2, 7)
    _expect(ref, 1, 22, 8)
    _expect(ref, 2, 43, 8)
    _expect(ref, 3, 50, 4)
    _expect(ref, 4, -1, 60)
    _expect(ref, 5, 55, 30)


def test_six_key_rescan():
    O, cfg, *_ = _world()
    s = Scene(4, 128, 4)  # per segment: 32
    kinds = [NO_BP, BAD_ROW] * 4
    # query 0: nine below the threshold in segment 0, distances falling along k1: each key enters at the front
    for i in range(8):
        s.put(2 + 3 * i, 0, 40 - 4 * i, kinds[i])
    s.put(30, 0, 50, GOOD)
    # query 1: the same in segment 1 with distances rising along k1: each key enters at the back
    for i in range(8):
        s.put(33 + 3 * i, 1, 5 + 4 * i, kinds[i])
    s.put(63, 1, 55, GOOD)
    # query 2: mixed order with ties in segment 2, the valid one in the middle of the k1 range
    for k1, d in zip((64, 66, 69, 71, 80, 83, 90, 95), (20, 9, 20, 33, 9, 2, 33, 20)):
        s.put(k1, 2, d, NO_BP if k1 % 2 else BAD_ROW)
    s.put(75, 2, 34, GOOD)
    # query 3: all nine refused
    for i in range(9):
        s.put(97 + 3 * i, 3, 10 + (i * 5) % 9, kinds[i % 8])
    ref = s.run()
    _expect(ref, 0, 30, 50)
    _expect(ref, 1, 63, 55)
    _expect(ref, 2, 75, 34)
    _expect(ref, 3, -1, cfg.match_threshold)


def _dense_scene(n0, n1, seed):
    """side-1 slot j belongs to query j % n0 in round j // n0: several candidates per query over all segments, at mixed
    distances with ties; a third of them observe the query's point, the rest fail the gate or have no back-projection"""
    s = Scene(n0, n1, seed)
    for j in range(n1):
        kind = (GOOD, BAD_ROW, NO_BP, BAD_ROW, GOOD, BAD_ROW)[(j // n0 + j) % 6]
        s.put(j, j % n0, 2 + (j * 7) % 23, kind)
    return s


@pytest.mark.parametrize("n1", [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 300])
def test_sizes(n1):
    hits = 0
    for n0 in (1, 31, 32, 33, 63, 64, 65, 96, 97):
        ref = _dense_scene(n0, n1, 100 + n1).run()
        hits += int((ref["k1"] >= 0).sum())
        if n0 > n1:
            assert (ref["k1"][n1:] == -1).all()  # queries without any candidate
    assert hits > 0


def test_full_cap():
    O, cfg, fe0, T, f, obs = _world()
    cap = 2500
    fe = G.make_frontend(cfg, max_keypoints=cap)
    s = Scene(5, cap, 5)
    s.put(cap - 1, 0, 4, GOOD)   # the winner at the last index
    s.put(cap - 2, 0, 4, NO_BP)  # ... after a refused tie just below it
    s.put(1023, 0, 6, GOOD); s.put(1024, 0, 5, GOOD)
    s.put(0, 1, 3, GOOD); s.put(cap - 1 - 625, 1, 3, GOOD)  # first index against the last of segment 2
    s.put(2047, 2, 9, BAD_ROW); s.put(2048, 2, 9, GOOD)
    s.check_far()
    a0, a1 = s.arrays()
    ref = O.match_stereo(*a0, *a1, T[0], T[1], f[0], f[1], cfg.match_threshold)
    got = fe.match_stereo(*a0, *a1, T[0], T[1], f[0], f[1])
    for name in FIELDS:
        assert np.array_equal(got[name], ref[name]), name
    assert np.array_equal(got["hp_W"].view(np.uint64), ref["hp_W"].view(np.uint64))
    _expect(ref, 0, cap - 1, 4)
    _expect(ref, 1, 0, 3)
    _expect(ref, 2, 2048, 9)
    _expect(ref, 3, -1, cfg.match_threshold)


@pytest.mark.parametrize("n", [120, 400])  # segments resident in LDS / streamed in chunks
def test_motion_stereo_skip_flags(n):
    """matchMotionStereo, shaped like test_gpu_matchers.test_match_motion_stereo, with the flags set on the candidates
    that win without them: the scan has to pass over exactly those and bring the next key"""
    O, cfg, fe, *_ = _world()
    cam = cfg.cams[0]
    rng = np.random.default_rng(3)
    T0 = (np.eye(3).reshape(-1), np.zeros(3))
    th = 0.05
    Rz = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]])
    T1 = (Rz.reshape(-1), np.array([0.35, 0.04, 0.02]))
    X = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-0.8, 0.8, n), rng.uniform(2.5, 9, n)], 1)

    def observe(T):
        Xc = (X - np.asarray(T[1])) @ np.asarray(T[0]).reshape(3, 3)
        kp = np.zeros(n, dtype=O.KEYPOINT_DTYPE)
        kp["size"] = 12.0
        for i in range(n):
            st, pt, _ = O.cam_project(cam, Xc[i])
            kp["x"][i], kp["y"][i] = pt if st == 0 else (5.0, 5.0)
        bp, bv = O.backproject_keypoints(cam, kp)
        return kp, bp, bv

    kp0, bp0, bv0 = observe(T0)
    kp1, bp1, bv1 = observe(T1)
    d0 = rng.integers(0, 256, (n, 48), dtype=np.uint8)
    # two candidates per point on side 1: the point's own observation at distance 3 or 4 and a twin at 9, 10 or 11
    own = np.stack([_flip(d0[i], 3 + i % 2, 5 * i) for i in range(n)])
    twin = np.stack([_flip(d0[i], 9 + i % 3, 7 * i) for i in range(n)])
    perm = rng.permutation(2 * n)
    d1 = np.concatenate([own, twin])[perm]
    kp1, bp1, bv1 = (np.concatenate([a, a])[perm] for a in (kp1, bp1, bv1))

    def both(skip0, matched1):
        ref = O.match_motion_stereo(d0, kp0, bp0, bv0, skip0, d1, kp1, bp1, bv1, matched1, T0, T1, cam,
                                    cfg.match_threshold)
        got = fe.match_motion_stereo(cam, d0, kp0, bp0, bv0, skip0, d1, kp1, bp1, bv1, matched1, T0, T1)
        for name in ("k1", "dist", "initialisable", "accepted"):
            assert np.array_equal(got[name], ref[name]), name
        assert np.array_equal(got["hp_W"].view(np.uint64), ref["hp_W"].view(np.uint64))
        hit = ref["k1"] >= 0
        q = np.array([math.acos(c) for c in got["cos_quality"][hit]])  # libm acos, as the C++ host does
        assert np.array_equal(q, ref["quality"][hit])
        return ref

    free = both(None, None)
    won = free["k1"][free["k1"] >= 0]
    assert len(won) > n // 2
    matched1 = np.zeros(2 * n, np.uint8)
    matched1[won[::2]] = 1  # every other winner is taken already
    skip0 = np.zeros(n, np.uint8)
    skip0[::9] = 1
    flagged = both(skip0, matched1)
    hit = flagged["k1"] >= 0
    assert not matched1[flagged["k1"][hit]].any() and not skip0[hit].any()
    moved = hit & (free["k1"] >= 0) & (flagged["k1"] != free["k1"])
    assert moved.sum() > n // 8  # flagged winners were replaced by their successors
    assert (flagged["dist"][moved] >= free["dist"][moved]).all()
    # all flagged: nothing is left to scan
    none = both(None, np.ones(2 * n, np.uint8))
    assert (none["k1"] == -1).all()
