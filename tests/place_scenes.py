"""Scenes for okvfe_place_landmark_set, okvfe_place_claims_blocks_device and okvfe_place_consensus_blocks_device, for
contexts of K = ransac_scenes.K: old frames that reach every branch of the landmark set; hand-built k_min / dist_min
rows for the claims (collisions, the values of hp[3], empty blocks, k_min outside the count), the gate table and the
verdict table; chunk and landmark-count edges; and per rig of ransac_scenes.GENERAL_SPECS one general scene that goes
through the whole chain from descriptors.  CPU only up to `prepare` and the launches, which need torch and a GPU.
Test infrastructure only."""
import numpy as np

import place_ref as P
import ransac_scenes as S
from gate_scenes import bisect_adjacent
from okvis2_amd import synth

K = S.K
MATCH_THRESHOLD = synth.euroc_config().match_threshold
COPIES = 16
SENTINEL = S.SENTINEL
GATE_SENTINEL = 0x77


# ---- the landmark set ------------------------------------------------------------------------------------------------
def norm_edge(tree, base):
    """t_lo < t_hi adjacent doubles with norm(base t_lo) < 1e-12 <= norm(base t_hi) under the order `tree`"""
    lo, hi = bisect_adjacent(lambda t: bool(P.norm4(tree, base * t) < 1.0e-12), 0.25e-12, 4.0e-12)
    assert P.norm4(tree, base * lo) < 1.0e-12 <= P.norm4(tree, base * hi) and np.nextafter(lo, hi) == hi
    return lo, hi


def set_scene(seed=5, n_cams=2, n_general=120):
    """an old frame: per case COPIES landmarks (or keypoints) on top of general ones; ids scrambled and partly above 2^32"""
    rng = np.random.default_rng(seed)
    obs = [[] for _ in range(n_cams)]  # per camera: (id, hp, init)
    pool_ids = rng.permutation(np.arange(1, 4000))
    big = (np.uint64(1) << np.uint64(40))
    next_id = iter(int(v) + (int(big) if i % 3 == 0 else 0) for i, v in enumerate(pool_ids))
    good = lambda: np.append(rng.uniform(-5, 5, 3), 1.0) * rng.choice([1.0, 2.0, -1.0, 0.5])

    def add(c, lm_id, hp, init=1):
        obs[c].append((lm_id, np.asarray(hp, dtype=np.float64), init))

    for i in range(n_general):
        lm_id = next(next_id)
        for c in rng.choice(n_cams, rng.integers(1, n_cams + 1), replace=False):
            add(int(c), lm_id, good())
    for i in range(COPIES):
        c, d = i % n_cams, (i + 1) % n_cams
        add(c, 0, good())                                           # id 0
        add(c, next(next_id), good(), 0)                            # not initialised
        add(c, next(next_id), np.zeros(4))                          # norm exactly 0
        add(c, next(next_id), np.roll([1.0e-13, 0.0, 0.0, 0.0], i % 4))  # norm of 1e-13
        base = rng.normal(size=4)
        base /= np.linalg.norm(base)
        lo, hi = norm_edge(i % 2 == 0, base)                        # both sides of 1e-12, under either order
        add(c, next(next_id), base * lo)
        add(c, next(next_id), base * hi)
        add(c, next(next_id), np.array([np.nan, 1.0, 1.0, 1.0]))    # NaN norm: kept
        two = next(next_id)                                         # seen by two cameras (or twice, with one camera)
        h = good()
        add(c, two, h), add(d, two, h)
        twice = next(next_id)                                       # seen twice by one camera
        h = good()
        add(c, twice, h), add(c, twice, h)
        later = next(next_id)                                       # first observation filtered, a later one passing
        add(c, later, good(), 0), add(c, later, np.zeros(4)), add(d, later, good())
        differ = next(next_id)                                      # different hp: the first passing one wins
        add(c, differ, good()), add(d, differ, good()), add(c, differ, good())
    old = []
    for c in range(n_cams):
        n = len(obs[c])
        old.append(dict(ids=np.array([o[0] for o in obs[c]], dtype=np.uint64),
                        hp=np.array([o[1] for o in obs[c]], dtype=np.float64).reshape(n, 4),
                        init=np.array([o[2] for o in obs[c]], dtype=np.uint8),
                        desc=rng.integers(0, 256, (n, 48), dtype=np.uint8)))
    return old


def flat_old(old):
    """the arguments of okvfe_place_landmark_set: (n_kps, ids, hp, init, desc), camera-major"""
    return ([len(f["ids"]) for f in old], np.concatenate([f["ids"] for f in old]),
            np.concatenate([f["hp"] for f in old]), np.concatenate([f["init"] for f in old]),
            np.concatenate([f["desc"] for f in old]))


def same_set(got, ref, what):
    assert np.array_equal(got["ids"], ref["ids"]), (what, "ids")
    assert np.array_equal(got["hp"].view(np.uint64), ref["hp"].view(np.uint64)), (what, "hp")
    assert np.array_equal(got["desc_begin"], ref["desc_begin"]), (what, "desc_begin")
    assert np.array_equal(got["pool"], ref["pool"]), (what, "pool")


# ---- scenes with hand-built k_min / dist_min ---------------------------------------------------------------------------
def scene(name, cams, T_SC, hp, mfs, min_inliers=10):
    return dict(name=name, cams=cams, T_SC=T_SC, hp=np.ascontiguousarray(hp, dtype=np.float64).reshape(-1, 4), mfs=mfs,
                min_inliers=min_inliers)


def no_hits(n_cams, L):
    """what the matcher leaves where nothing is below the threshold"""
    return np.zeros((n_cams, L), np.int32), np.full((n_cams, L), MATCH_THRESHOLD, np.uint32)


def put(km, dm, hits, rng=None):
    """hits: (row, camera, keypoint)"""
    for row, c, k in hits:
        km[c, row] = k
        dm[c, row] = MATCH_THRESHOLD - 1 if rng is None else rng.integers(0, MATCH_THRESHOLD)
    return km, dm


def _frames(oracle, cams, T_SC, m, T_WS, sizes, rng, **kw):
    usable = S.usable_rows(m)
    return [S.make_frame(oracle, cam, S.compose(T_WS, T_SC[c]), m["p"], usable, sizes[c], rng, **kw)
            for c, cam in enumerate(cams)]


def _mf(frames, km, dm, H, valid=None, T_WS=None, ml=None, gate=None):
    return dict(frames=frames, kmin=km, dmin=dm, H=np.asarray(H, dtype=np.float64).reshape(-1, 12), valid=valid,
                T_WS=T_WS, ml=ml, gate=gate)


def claims_scene(oracle, seed=7):
    """2 cameras, L = 400.  Multiframe 0: per case COPIES rows -- no hit, a hit in one camera, hits in both, two and
    three rows on one keypoint, the values of hp[3], k_min outside the count (both sides).  Multiframe 1: the same hits
    against an empty second block."""
    m = S.table()
    cams, T_SC = S.rig(("euroc", "euroc1"))
    rng = np.random.default_rng(seed)
    hp = m["hp"].copy()
    L = len(hp)
    usable = [int(r) for r in S.usable_rows(m)]
    rows = iter(usable)
    take = lambda n: [next(rows) for _ in range(n)]
    counts = (K, 200)
    hits, kp = [], [iter(range(counts[0])), iter(range(counts[1]))]
    for r in take(COPIES):                                          # a hit in one camera
        hits.append((r, r % 2, next(kp[r % 2])))
    for r in take(COPIES):                                          # hits in both cameras
        hits += [(r, 0, next(kp[0])), (r, 1, next(kp[1]))]
    for i in range(COPIES):                                         # two and three rows on one keypoint
        c = i % 2
        k2, k3 = next(kp[c]), next(kp[c])
        hits += [(r, c, k2) for r in take(2)] + [(r, c, k3) for r in take(3)]
    for w in S.W_CASES:                                             # a claimed landmark with every value of hp[3]
        for r in take(COPIES):
            p = m["p"][r]
            hp[r] = np.array([p[0] * w, p[1] * w, p[2] * w, w]) if w == w and w != 0 else np.array([p[0], p[1], p[2], w])
            hits.append((r, 0, next(kp[0])))
    outside = take(COPIES)
    mfs = []
    for empty in (False, True):
        sizes = (counts[0], 0 if empty else counts[1])
        frames = _frames(oracle, cams, T_SC, m, m["T1"], sizes, rng)
        km, dm = put(*no_hits(2, L), hits, rng)
        for i, r in enumerate(outside):                             # below the threshold, k_min outside [0, count)
            km[1, r], dm[1, r] = (counts[1] + i, 3) if i % 2 else (-1 - i, 3)
        mfs.append(_mf(frames, km, dm, S.hypotheses(m["T1"], 12, rng, n_random=3), T_WS=m["T1"]))
    return scene("claims", cams, T_SC, hp, mfs)


def collide_all_scene(oracle, L=300, n_mf=8, seed=8):
    """every row of the set on one keypoint, in both cameras of every multiframe"""
    m = S.table()
    cams, T_SC = S.rig(("euroc", "euroc1"))
    rng = np.random.default_rng(seed)
    mfs = []
    for i in range(n_mf):
        frames = _frames(oracle, cams, T_SC, m, m["T1"], (40, 30), rng)
        km, dm = put(*no_hits(2, L), [(r, c, (7 * i + c) % 30) for r in range(L) for c in range(2)], rng)
        mfs.append(_mf(frames, km, dm, S.hypotheses(m["T1"], 4, rng, n_random=1), T_WS=m["T1"]))
    return scene("collide-all", cams, T_SC, m["hp"][:L], mfs)


GATE_TABLE = {
    10: (("nine in one camera each", (9, 9, 9), 0), ("three in both, four in one", (10, 7, 10), 0),
         ("two in both, six in one", (10, 8, 10), 2), ("ten, four with w = 0", (10, 10, 6), 1),
         ("ten, three with w = 0", (10, 10, 7), 2), ("twelve, six pairs colliding", (12, 12, 6), 1)),
    40: (("thirty-nine", (39, 39, 39), 0), ("forty", (40, 40, 40), 2)),
}
N_ZERO_W = 4  # rows 0 .. 3 of the gate scenes' sets have hp[3] == 0


def gate_scene(oracle, min_inliers, seed=9):
    """one multiframe per row of GATE_TABLE[min_inliers], 2 cameras"""
    m = S.table()
    cams, T_SC = S.rig(("euroc", "euroc1"))
    rng = np.random.default_rng(seed)
    good = [int(r) for r in S.usable_rows(m) if r >= N_ZERO_W]
    hp = m["hp"].copy()
    hp[:N_ZERO_W, 3] = 0.0
    one = lambda rows, k0=0: [(r, i % 2, k0 + i) for i, r in enumerate(rows)]
    both = lambda rows, k0: [(r, c, k0 + i) for i, r in enumerate(rows) for c in range(2)]
    if min_inliers == 10:
        specs = [one(good[:9]), both(good[:3], 100) + one(good[3:7]), both(good[:2], 100) + one(good[2:8]),
                 one(list(range(4)) + good[:6]), one(list(range(3)) + good[:7]),
                 [(r, 0, i // 2) for i, r in enumerate(good[:12])]]
    else:
        specs = [one(good[:39]), one(good[:40])]
    mfs = []
    for hits in specs:
        frames = _frames(oracle, cams, T_SC, m, m["T1"], (150, 150), rng)
        km, dm = put(*no_hits(2, len(hp)), hits)
        mfs.append(_mf(frames, km, dm, S.hypotheses(m["T1"], 6, rng, n_random=2), T_WS=m["T1"]))
    return scene("gate-%d" % min_inliers, cams, T_SC, hp, mfs, min_inliers)


# (min_inliers, n_corr, n_inliers) -> verdict
VERDICT_TABLE = {10: (((7, 7), 2), ((10, 10), 3), ((20, 14), 3), ((20, 13), 2), ((30, 21), 3), ((30, 20), 2),
                      ((14, 10), 3), ((15, 10), 2), ((6, 6), 1), ((0, 0), 1)),
                 5: (((7, 5), 3), ((7, 4), 2)),
                 40: (((57, 40), 3), ((58, 40), 2))}


def verdict_scene(oracle, min_inliers, H_of, valid=None, gates=None, seed=21):
    """one multiframe per VERDICT_TABLE[min_inliers] entry, one camera: n claimed keypoints of which i are inliers of the
    true pose (the landmarks of the others are copies moved a metre), as hand-built match_landmark rows.
    H_of(T_WS, rng) -> the hypotheses of every multiframe; gates: the gate_dev bytes or None"""
    m = S.table()
    cams, T_SC = S.rig(("euroc",))
    rng = np.random.default_rng(seed)
    T_WS = m["T1"]
    moved = m["hp"].copy()
    moved[:, :3] += np.array([1.0, 0.5, 0.0]) * moved[:, 3:4]
    hp = np.concatenate([m["hp"], moved])
    mfs = []
    for j, ((n, i), _) in enumerate(VERDICT_TABLE[min_inliers]):
        fr = _frames(oracle, cams, T_SC, m, T_WS, (n,), rng, wrong=0.0, none=0.0, noise=0.0)[0]
        fr["lm"][i:] += len(m["hp"])
        extra = _frames(oracle, cams, T_SC, m, T_WS, (5,), rng, wrong=0.0, none=1.0)[0]
        fr = {k: np.concatenate([fr[k], extra[k]]) for k in fr}  # (keypoints nothing claims)
        mfs.append(_mf([fr], None, None, H_of(T_WS, rng), valid, T_WS, ml=[fr["lm"].astype(np.int32)],
                       gate=None if gates is None else gates[j]))
    return scene("verdict-%d" % min_inliers, cams, T_SC, hp, mfs, min_inliers)


def true_first(T, rng):
    return np.array([S.pose_matrix(T), S.far_pose(T, rng)])


def chunk_scene(oracle, chunk, seed=31):
    """the five-camera rig; multiframes with exactly chunk - 1, chunk, chunk + 1, 2 chunk and 2 chunk + 1
    correspondences, as hand-built match_landmark rows"""
    m = S.table()
    cams, T_SC = S.rig("hilti")
    assert 2 * chunk + 1 <= len(cams) * K
    rng = np.random.default_rng(seed)
    mfs = []
    for total in (chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1):
        frames = _frames(oracle, cams, T_SC, m, m["T1"], (K, 100, K, K, 3), rng, wrong=0.3, none=0.0)
        left = total
        for fr in frames:
            n = min(len(fr["lm"]), left)
            fr["lm"][n:] = -1
            left -= n
        assert left == 0
        mfs.append(_mf(frames, None, None, S.hypotheses(m["T1"], 8, rng, n_random=2), T_WS=m["T1"],
                       ml=[f["lm"].astype(np.int32) for f in frames]))
    return scene("chunks", cams, T_SC, m["hp"], mfs)


L_EDGES = (0, 1, 255, 256, 257, 1025)


def landmark_count_scene(oracle, L, seed=41):
    """L rows with random hits (half of them) on the keypoints of 2 cameras, 2 multiframes"""
    m = S.table()
    cams, T_SC = S.rig(("euroc", "euroc1"))
    rng = np.random.default_rng([seed, L])
    hp = np.concatenate([rng.uniform(-5, 5, (L, 3)), rng.choice([1.0, 0.0, -1.0, 2.0], (L, 1), p=[0.7, 0.1, 0.1, 0.1])], axis=1)
    hp[:, :3] *= hp[:, 3:4]
    mfs = []
    for sizes in ((K, 31), (64, K)):
        frames = _frames(oracle, cams, T_SC, m, m["T1"], sizes, rng)
        km = np.stack([rng.integers(0, n, L) for n in sizes]).astype(np.int32).reshape(2, L)
        dm = rng.integers(MATCH_THRESHOLD - 20, MATCH_THRESHOLD + 20, (2, L)).astype(np.uint32)
        mfs.append(_mf(frames, km, dm, S.hypotheses(m["T1"], 5, rng, n_random=2), T_WS=m["T1"]))
    return scene("L-%d" % L, cams, T_SC, hp, mfs)


# ---- the whole chain from descriptors --------------------------------------------------------------------------------
def general_scene(oracle, spec, tree=True, seed=0, n_mf=3, n_hyp=50, n_landmarks=400):
    """An old frame over the landmarks of a map_synth table (its observations dealt to the rig's cameras, some ids 0 and
    some not initialised), its set, and n_mf multiframes whose keypoints sit at projections of set landmarks and carry a
    pool descriptor of that landmark with a few bits flipped; a share of the keypoints carries another landmark's."""
    m = S.table(n_landmarks)
    cams, T_SC = S.rig(spec)
    n_cams = len(cams)
    rng = np.random.default_rng([seed, n_cams, n_hyp])
    old = [dict(ids=[], hp=[], init=[], desc=[]) for _ in cams]
    for l in range(n_landmarks):
        for o in range(m["obs_begin"][l], m["obs_begin"][l + 1]):
            f = old[int(rng.integers(0, n_cams))]
            u = rng.random()
            f["ids"].append(0 if u < 0.05 else 1000 + 3 * l)
            f["hp"].append(m["hp"][l]), f["init"].append(0 if 0.05 <= u < 0.1 else 1), f["desc"].append(m["obs_desc"][o])
    old = [dict(ids=np.array(f["ids"], dtype=np.uint64), hp=np.array(f["hp"], dtype=np.float64).reshape(-1, 4),
                init=np.array(f["init"], dtype=np.uint8), desc=np.array(f["desc"], dtype=np.uint8).reshape(-1, 48))
           for f in old]
    lset = P.landmark_set(tree, old)
    L = len(lset["ids"])
    assert 100 <= L <= 400
    p_set = lset["hp"][:, :3] / lset["hp"][:, 3:4]
    usable = np.flatnonzero(np.abs(lset["hp"][:, 3]) >= 1.0e-8)
    mfs = []
    for i in range(n_mf):
        T_WS = (m["T1"][0].reshape(3, 3) @ S.rodrigues((0, 1, 0), 0.02 * i), m["T1"][1] + np.array([0.05 * i, 0.0, 0.0]))
        frames = []
        for c, cam in enumerate(cams):
            n = K if (i + c) % 3 == 0 else int(rng.integers(60, K))
            if i == 1 and c == n_cams - 1 and n_cams > 1:
                n = 0
            fr = S.make_frame(oracle, cam, S.compose(T_WS, T_SC[c]), p_set, usable, n, rng,
                              wrong=(0.1, 0.45, 0.25)[i % 3], none=0.2)
            for k in np.flatnonzero(fr["lm"] >= 0):
                row = int(rng.integers(lset["desc_begin"][fr["lm"][k]], lset["desc_begin"][fr["lm"][k] + 1]))
                flip = (rng.random(48) < 0.03) * rng.integers(1, 256, 48)
                fr["desc"][k] = lset["pool"][row] ^ flip.astype(np.uint8)
            frames.append(fr)
        km = np.zeros((n_cams, L), np.int32)
        dm = np.zeros((n_cams, L), np.uint32)
        for c, fr in enumerate(frames):
            km[c], dm[c] = oracle.verify_place(lset["pool"], lset["desc_begin"], fr["desc"], MATCH_THRESHOLD)
        valid = (rng.random(n_hyp) >= 0.1).astype(np.uint8)
        mfs.append(_mf(frames, km, dm, S.hypotheses(T_WS, n_hyp, rng), valid, T_WS))
    sc = scene("general-" + S.spec_id(spec), cams, T_SC, lset["hp"], mfs)
    sc.update(old=old, set=lset)
    return sc


# ---- the references ----------------------------------------------------------------------------------------------------
def claims_reference(sc, census=None):
    return [P.claim_stage(sc["hp"], [len(f["kps"]) for f in mf["frames"]], mf["kmin"], mf["dmin"], MATCH_THRESHOLD,
                          sc["min_inliers"], census) for mf in sc["mfs"]]


def consensus_reference(tree, sc, match_landmark, gates=None, use_valid=True, threshold=P.THRESHOLD):
    """match_landmark: per multiframe, per camera rows; gates: per multiframe the caller's gate, or None"""
    fus = [c.fu for c in sc["cams"]]
    return [P.consensus(tree, sc["hp"], mf["frames"], ml, fus, sc["T_SC"], mf["H"], mf["valid"] if use_valid else None,
                        None if gates is None else int(gates[i]), sc["min_inliers"], threshold)
            for i, (mf, ml) in enumerate(zip(sc["mfs"], match_landmark))]


# ---- GPU side ----------------------------------------------------------------------------------------------------------
def prepare(fe, sc, optional=True, alias=False, with_gate=True):
    """the device tensors of a claims + consensus chain over a scene (synchronises)"""
    import torch
    frames = [f for mf in sc["mfs"] for f in mf["frames"]]
    B, nh, L = len(sc["mfs"]), len(sc["mfs"][0]["H"]), len(sc["hp"])
    nb, Kc = len(frames), fe.max_keypoints
    blocks, _ = S.pack_frames(fe, [dict(f, lm=np.zeros(0, np.int32)) for f in frames])
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
    valid = None if sc["mfs"][0]["valid"] is None else np.stack([mf["valid"] for mf in sc["mfs"]]).astype(np.uint8)
    T = dict(blocks=S._dev(blocks), hp=S._dev(sc["hp"]), H=S._dev(np.stack([mf["H"] for mf in sc["mfs"]])),
             valid=None if valid is None else S._dev(valid))
    T["set"] = fe.make_place_set_device(L, T["hp"].data_ptr())
    ml = np.full((nb, Kc), S.PAST_COUNT_ROW, np.int32)  # (a valid row at or past the count: must be ignored)
    if sc["mfs"][0]["ml"] is not None:                   # hand-built claims
        for b, rows in enumerate(r for mf in sc["mfs"] for r in mf["ml"]):
            ml[b, :len(rows)] = rows
        gates = [mf["gate"] for mf in sc["mfs"]]
        T["gate"] = None if gates[0] is None else S._dev(np.array(gates, dtype=np.uint8))
    else:
        T["kmin"] = S._dev(np.concatenate([mf["kmin"] for mf in sc["mfs"]]).reshape(nb, L))
        T["dmin"] = S._dev(np.concatenate([mf["dmin"] for mf in sc["mfs"]]).reshape(nb, L).view(np.int32))  # (uint32 bits)
        T.update(n_matches=full((B,), SENTINEL, torch.int32), n_points=full((B,), SENTINEL, torch.int32),
                 n_corr_claims=full((B,), SENTINEL, torch.int32))
        T["gate"] = full((B,), GATE_SENTINEL, torch.uint8)
    T["ml"] = S._dev(ml)
    T["ml_in"] = ml
    T.update(n_corr=full((B,), SENTINEL, torch.int32), best=full((B,), SENTINEL, torch.int32),
             n_inl=full((B,), SENTINEL, torch.int32), accepted=full((B,), S.STATE_SENTINEL, torch.uint8),
             verdict=full((B,), GATE_SENTINEL, torch.uint8))
    if optional:
        T.update(hyp_inliers=full((B, nh), SENTINEL, torch.int32), state=full(ml.shape, S.STATE_SENTINEL, torch.uint8),
                 distance=full(ml.shape, S.DIST_SENTINEL, torch.float64),
                 lm_out=T["ml"] if alias else full(ml.shape, SENTINEL, torch.int32))
    T["use_gate"] = with_gate and T["gate"] is not None
    torch.cuda.synchronize()
    return T


def launch_claims(fe, sc, T, stream=None):
    res = fe.make_place_claims_device(T["n_matches"].data_ptr(), T["n_points"].data_ptr(), T["n_corr_claims"].data_ptr(),
                                      T["gate"].data_ptr(), T["ml"].data_ptr())
    fe.place_claims_blocks_device(T["set"], T["blocks"].data_ptr(), len(sc["mfs"]), len(sc["cams"]), T["kmin"].data_ptr(),
                                  T["dmin"].data_ptr(), sc["min_inliers"], res, stream)


def launch_consensus(fe, sc, T, use_valid=True, stream=None, threshold=P.THRESHOLD):
    ptr = lambda k: None if T.get(k) is None else T[k].data_ptr()
    res = fe.make_ransac_result_device(ptr("n_corr"), ptr("best"), ptr("n_inl"), ptr("accepted"), ptr("hyp_inliers"),
                                       ptr("state"), ptr("distance"), ptr("lm_out"))
    fe.place_consensus_blocks_device(T["set"], T["blocks"].data_ptr(), len(sc["mfs"]), list(range(len(sc["cams"]))),
                                     sc["T_SC"], ptr("ml"), ptr("gate") if T["use_gate"] else None, ptr("H"),
                                     ptr("valid") if use_valid else None, len(sc["mfs"][0]["H"]), sc["min_inliers"], res,
                                     ptr("verdict"), threshold, stream)


def download(T):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in T.items() if isinstance(v, torch.Tensor)}


def check_claims(sc, got, refs, what):
    """every output of the claims call; match_landmark rows at or past a block's count untouched.  `got` must have been
    downloaded before a consensus in place rewrote the rows."""
    n_cams = len(sc["cams"])
    for mi, (mf, ref) in enumerate(zip(sc["mfs"], refs)):
        head = tuple(int(got[k][mi]) for k in ("n_matches", "n_points", "n_corr_claims", "gate"))
        assert head == (ref["n_matches"], ref["n_points"], ref["n_corr"], ref["gate"]), (what, mi, head, ref["n_matches"],
                                                                                       ref["n_points"], ref["n_corr"], ref["gate"])
        for c in range(n_cams):
            b, n = mi * n_cams + c, len(mf["frames"][c]["kps"])
            assert np.array_equal(got["ml"][b, :n], ref["match_landmark"][c]), (what, mi, c, "match_landmark")
            assert np.all(got["ml"][b, n:] == S.PAST_COUNT_ROW), (what, mi, c, "match_landmark past the count")


def check_consensus(sc, got, refs, what, alias=False):
    """every output of the consensus call, FP64 as uint64 patterns; rows at or past a block's count untouched"""
    n_cams = len(sc["cams"])
    for mi, (mf, ref) in enumerate(zip(sc["mfs"], refs)):
        w = what + (mi,)
        head = tuple(int(got[k][mi]) for k in ("verdict", "n_corr", "best", "n_inl", "accepted"))
        want = (ref["verdict"], ref["n_corr"], ref["best"], ref["n_inliers"], ref["accepted"])
        assert head == want, (w, head, want)
        if "state" not in got:
            continue
        assert np.array_equal(got["hyp_inliers"][mi], ref["hyp_inliers"]), (w, got["hyp_inliers"][mi], ref["hyp_inliers"])
        for c in range(n_cams):
            b, n = mi * n_cams + c, len(mf["frames"][c]["kps"])
            assert np.array_equal(got["state"][b, :n], ref["state"][c]), (w, c, "state")
            assert np.all(got["state"][b, n:] == S.STATE_SENTINEL), (w, c, "state past the count")
            ds = ref["dist_set"][c]
            gd, rd = got["distance"][b, :n], ref["distance"][c]
            assert np.array_equal(gd[ds].view(np.uint64), rd[ds].view(np.uint64)), (w, c, "distance", gd[ds][:4], rd[ds][:4])
            assert np.all(gd[~ds] == S.DIST_SENTINEL) and np.all(got["distance"][b, n:] == S.DIST_SENTINEL), (w, c)
            lo = got["ml"] if alias else got["lm_out"]
            assert np.array_equal(lo[b, :n], ref["landmark_out"][c]), (w, c, "landmark_out")
            assert np.all(lo[b, n:] == (S.PAST_COUNT_ROW if alias else SENTINEL)), (w, c, "landmark_out past the count")
