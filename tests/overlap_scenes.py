"""Scenes for the overlapFraction tests: per context about ten multiframes, built to hit what the kernel can get
wrong, and their restatement (overlap_ref.py), computed once per context and shared by the tests that need it.

Multiframes (index: what it is for)
  0  dense: camera 0 full (K keypoints), the others 226; ids from the shared pool
  1  sparse: 20 / 226 keypoints, ids from the pool
  2  sparse: 226 / 20 keypoints, fewer ids
  3  tiny: 1, 20, 0 ... keypoints
  4  no keypoints at all
  5  ids from a range nobody else uses: no common id with any other multiframe
  6  every keypoint has non-finite coordinates (nothing is painted): as side A with a common id the overlap is 0 / 0
  7  sparse; its only common id with 6 (NAN_ID) sits on a keypoint with NaN coordinates
  8  carries CROSS_ID in camera 0 only, other ids from the even half of the pool
  9  carries CROSS_ID in the LAST camera only, other ids from the odd half of the pool: (8, 9) have one common id, and
     with more than one camera only a set taken per multiframe finds it
Rows past a block's count hold ids that WOULD be common if they were read (pool ids, NAN_ID, CROSS_ID), and keypoint
bytes of 0xFF (NaN)."""
import numpy as np

import overlap_ref as OR
from okvis2_amd import capi, multigpu, synth

CONFIGS = {"euroc": (synth.euroc_config, 4), "tumvi1024": (synth.tumvi1024_config, 9),
           "hilti": (synth.hilti_config, 5), "mono640": (synth.mono640_config, 4)}
KPTRAD = OR.backend_kptrad()  # 0.095: 0.09 * 38 / 36
POOL = 400
NAN_ID = 1 << 50
CROSS_ID = (1 << 50) + 1
N_MULTIFRAMES = 10


def _camera(rng, w, h, n, ids):
    kps = np.zeros(n, dtype=capi.KEYPOINT_DTYPE)
    kps["x"] = rng.uniform(0, w - 0.5, n)
    kps["y"] = rng.uniform(0, h - 0.5, n)
    if n >= 20:  # the half-way values (cvRound: half to even), the far rim (centre outside the mask), the origin
        kps["x"][:8] = (5, 15, 25, 35, w - 0.5, 0, 45, w - 0.5)
        kps["y"][:8] = (5, 15, 35, 25, h - 0.5, 0, h - 0.5, 65)
    ids = np.asarray(ids, dtype=np.uint64).copy()
    if n > 40:
        ids[30:34] = ids[34]  # one landmark seen by several keypoints
    return kps, ids


def _ids(rng, n, frac, lo=1, hi=POOL, step=1):
    v = (lo + step * rng.integers(0, (hi - lo) // step + 1, n)).astype(np.uint64)
    v[rng.random(n) >= frac] = 0
    return v


def multiframes(cfg, K, seed=2341):
    rng = np.random.default_rng(seed)
    C, w, h = len(cfg.cams), cfg.w, cfg.h
    last = C - 1

    def sizes(*cycle):
        return [cycle[c % len(cycle)] for c in range(C)]
    mfs = []
    mfs.append([_camera(rng, w, h, n, _ids(rng, n, 0.6)) for n in sizes(K, 226)])
    mfs.append([_camera(rng, w, h, n, _ids(rng, n, 0.5)) for n in sizes(20, 226)])
    mfs.append([_camera(rng, w, h, n, _ids(rng, n, 0.3)) for n in sizes(226, 20)])
    mfs.append([_camera(rng, w, h, n, _ids(rng, n, 1.0)) for n in sizes(1, 20, 0)])
    mfs.append([_camera(rng, w, h, 0, np.zeros(0)) for _ in range(C)])
    mfs.append([_camera(rng, w, h, 20, _ids(rng, 20, 0.8, 1 << 40, (1 << 40) + 100)) for _ in range(C)])
    cams = []
    for c in range(C):  # 6: nothing of it can be painted
        kps, ids = _camera(rng, w, h, 3, [NAN_ID if c == 0 else 0, (1 << 41) + c, 0])
        kps["x"] = (np.nan, np.inf, 10.0)
        kps["y"] = (10.0, -np.inf, np.nan)
        cams.append((kps, ids))
    mfs.append(cams)
    cams = []
    for c in range(C):  # 7
        kps, ids = _camera(rng, w, h, 20, _ids(rng, 20, 0.5))
        if c == last:
            kps["x"][12], kps["y"][12], ids[12] = np.nan, 100.0, NAN_ID
        cams.append((kps, ids))
    mfs.append(cams)
    for own, half in ((0, 0), (last, 1)):  # 8 and 9
        cams = []
        for c in range(C):
            kps, ids = _camera(rng, w, h, 20, _ids(rng, 20, 0.7, 2 + half, POOL, 2))
            if c == own:
                kps["x"][15], kps["y"][15], ids[15] = 0.4 * w, 0.6 * h, CROSS_ID
            cams.append((kps, ids))
        mfs.append(cams)
    assert len(mfs) == N_MULTIFRAMES
    return mfs


def pack(mfs, K, stride_m, stride_c, seed=7):
    """The gather blocks and the landmark-id rows of the multiframes, block of (m, c) at m * stride_m + c * stride_c."""
    rng = np.random.default_rng(seed)
    M, C = len(mfs), len(mfs[0])
    L = multigpu.block_layout(K)
    blocks, ids = [None] * (M * C), np.zeros((M * C, K), dtype=np.uint64)
    for m, mf in enumerate(mfs):
        for c, (kps, fid) in enumerate(mf):
            b, n = m * stride_m + c * stride_c, len(kps)
            blocks[b] = multigpu.pack_block_host(K, kps, np.zeros((n, 48), np.uint8), np.zeros((n, 3)),
                                                 np.zeros(n, np.uint8))
            blocks[b][L["kps"] + n * 28:L["kps"] + K * 28] = 0xFF  # NaN coordinates past the count
            ids[b, :n] = fid
            planted = rng.integers(1, POOL + 1, K - n).astype(np.uint64)  # never read: common with many if they were
            planted[:2] = (NAN_ID, CROSS_ID)[:len(planted[:2])]
            ids[b, n:] = planted
    return np.stack(blocks), ids


_CACHE = {}


def reference(name):
    """(cfg, K, multiframes, {(a, b): overlap_ref.overlap_counts(...)}) for every ordered pair; computed once."""
    if name not in _CACHE:
        cfg = CONFIGS[name][0]()
        K = cfg.max_kpts
        mfs = multiframes(cfg, K)
        ref = {(a, b): OR.overlap_counts(cfg.w, cfg.h, mfs[a], mfs[b], KPTRAD)
               for a in range(len(mfs)) for b in range(len(mfs))}
        _CACHE[name] = (cfg, K, mfs, ref)
    return _CACHE[name]


def counts_array(ref, pairs):
    out = np.zeros(len(pairs), dtype=capi.OVERLAP_COUNTS_DTYPE)
    for i, p in enumerate(pairs):
        for field in OR.COUNT_FIELDS:
            out[field][i] = ref[tuple(p)][field]
    return out


def check_floors(name):
    """What the scenes must contain for the GPU comparison to mean something."""
    cfg, K, mfs, ref = reference(name)
    C = len(cfg.cams)
    ov = {p: r["overlap"] for p, r in ref.items()}
    assert sum(1 for v in ov.values() if 0.0 < v < 1.0) >= 16, name
    assert sum(1 for v in ov.values() if v == 0.0) >= 4, name
    assert sum(1 for v in ov.values() if np.isnan(v)) >= 1, name
    sizes = {len(k) for mf in mfs for k, _ in mf}
    assert {0, 1, 20, 226, K} <= sizes, (name, sizes)
    assert np.isnan(ov[(6, 7)]) and np.isnan(ov[(6, 6)]) and ov[(7, 6)] == 0.0  # common id, nothing painted on side A
    assert ref[(6, 7)]["n_matched"] == [1, 1] and ref[(6, 7)]["union_area"][0] == 0
    assert ref[(8, 9)]["n_matched"] == [1, 1] and 0.0 < ov[(8, 9)] < 1.0  # CROSS_ID, camera 0 against the last one
    assert all(ref[(5, b)]["n_matched"] == [0, 0] and ov[(5, b)] == 0.0 for b in range(len(mfs)) if b != 5)
    assert all(ref[(4, b)]["n_keypoints"][0] == 0 and ov[(4, b)] == 0.0 for b in range(len(mfs)))
    assert ov[(0, 0)] == ref[(0, 0)]["intersection_area"][0] / ref[(0, 0)]["union_area"][0]
    if C > 1:  # per image, cameras 0 and last of 8 and 9 share nothing
        a, b = set(mfs[8][0][1].tolist()), set(mfs[9][0][1].tolist())
        assert not (a & b) - {0}
