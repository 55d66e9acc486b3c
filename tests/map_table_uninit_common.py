"""Shared by the tests of okvfe_match_to_map_table_uninitialised_blocks_device (the second pass of matchToMap over the
landmarks a frame's first pass left as not 3-D yet, for a batch of frames against one device-resident table): the
frames, the pose of the second pass, the per-frame reference, hand-built pools for the gate scenes, and the two calls.

The per-frame reference: map_table_common.reference (oracle.prepare_landmarks with the pose of the FIRST pass),
map_synth.packed_set of its status-2 landmarks with the e_W / r_W of the kept rows, oracle.match_to_map_uninit on that
set with the pose of the SECOND pass, the packed index mapped back to the table.  CPU only up to `prepare` / `run`."""
import numpy as np

import gate_scenes
import map_synth
import map_table_common as M
from gate_scenes import rodrigues

THRESHOLD = M.THRESHOLD
SENTINEL = M.SENTINEL
HS_FILL, CTR_FILL = 9, 123


def second_pose(pose):
    """pose_first turned 0.002 rad about the camera's y axis and moved (0.01, -0.005, 0.003) m"""
    C, r = np.asarray(pose[0], dtype=np.float64).reshape(3, 3), np.asarray(pose[1], dtype=np.float64)
    return (C @ rodrigues((0, 1, 0), 0.002)).reshape(-1), r + np.array([0.01, -0.005, 0.003])


def frame(oracle, sc, ref, cam, n, clutter, seed, n3d=0):
    """A frame of at most n + clutter keypoints for the second pass.  The first n sit at the first-pass projections of
    status-2 landmarks of `ref` (a prepare_landmarks result), one per pooled row (a random choice of n of them if there
    are more), and carry that row with about 3 % of its bytes disturbed; 30 % of them carry their owner as `previous`.
    clutter: keypoints at random pixels with random descriptors.  Back-projections are the oracle's; a tenth of all
    keypoints get backproj_valid = 0 and a NaN back-projection; use = 0 for a twentieth of the first n and a tenth of
    the clutter.  n3d: that many of the clutter keypoints sit at the projection of a 3-D (status-1) landmark instead and
    carry its first pooled row, so that the first pass matches them.
    -> dict(kps, desc, bp, bv, use, previous)"""
    rng = np.random.default_rng([seed, n, clutter, len(sc["hp"])])
    idx = np.flatnonzero(ref["status"] == 2)
    own = np.repeat(idx, ref["n_desc"][idx])
    row = np.concatenate([ref["obs_rows"][l, :ref["n_desc"][l]] for l in idx]) if len(idx) else np.zeros(0, np.int64)
    pick = np.sort(rng.permutation(len(own))[:n])
    own, row = own[pick], row[pick].astype(np.int64)
    m = len(own) + clutter
    kps = np.zeros(m, dtype=oracle.KEYPOINT_DTYPE)
    kps["size"] = 12.0
    kps["x"][:len(own)] = ref["projection"][own, 0]
    kps["y"][:len(own)] = ref["projection"][own, 1]
    kps["x"][len(own):] = rng.uniform(0, cam.w, clutter)
    kps["y"][len(own):] = rng.uniform(0, cam.h, clutter)
    desc = rng.integers(0, 256, (m, 48), dtype=np.uint8)
    flips = ((rng.random((len(own), 48)) < 0.03) * rng.integers(1, 256, (len(own), 48))).astype(np.uint8)
    if len(own):
        desc[:len(own)] = sc["obs_desc"][row] ^ flips
    if n3d:
        rng3 = np.random.default_rng([seed, n3d, 3])
        l3 = rng3.permutation(np.flatnonzero(ref["status"] == 1))[:min(n3d, clutter)]
        at = len(own) + np.arange(len(l3))
        kps["x"][at], kps["y"][at] = ref["projection"][l3, 0], ref["projection"][l3, 1]
        desc[at] = sc["obs_desc"][ref["obs_rows"][l3, 0]]
    previous = np.full(m, -1, np.int32)
    carried = rng.random(len(own)) < 0.3
    previous[:len(own)][carried] = own[carried]
    bp, bv = oracle.backproject_keypoints(cam, kps)
    bp, bv = bp.copy(), bv.copy()
    off = rng.random(m) < 0.1
    bv[off] = 0
    bp[off] = np.nan
    use = (rng.random(m) >= np.where(np.arange(m) < len(own), 0.05, 0.1)).astype(np.uint8)
    perm = rng.permutation(m)
    return dict(kps=kps[perm], desc=desc[perm], bp=bp[perm], bv=bv[perm], use=use[perm], previous=previous[perm])


def head(fr, n):
    return {k: v[:n] for k, v in fr.items()}


def reference(oracle, obs_desc, ref, fr, pose_second, cam, exclusive, with_use=True, with_previous=True, census=None):
    """-> (landmark as table row, distance, hp (n, 4), hp_set, already_matched) for one frame; ref: the pooling of the
    first pass (status, n_desc, obs_rows, e_W, r_W)"""
    n = len(fr["desc"])
    idx, _, begin, rows = map_synth.packed_set(dict(ref, projection=np.zeros((len(ref["status"]), 2))), obs_desc, 2)
    e0 = [ref["e_W"][l, d] for l in idx for d in range(ref["n_desc"][l])]
    r0 = [ref["r_W"][l, d] for l in idx for d in range(ref["n_desc"][l])]
    e0 = np.array(e0, dtype=np.float64).reshape(-1, 3)
    r0 = np.array(r0, dtype=np.float64).reshape(-1, 3)
    previous = fr["previous"] if with_previous else np.full(n, -1, np.int32)
    use = fr["use"] if with_use else np.ones(n, np.uint8)
    use_eff = ((fr["bv"] != 0) & (use != 0) & (bool(exclusive) | (previous < 0))).astype(np.uint8)
    packed_of = np.full(len(ref["status"]) + 1, -1, np.int32)  # (last entry: previous == -1)
    packed_of[idx] = np.arange(len(idx))
    prev_packed = packed_of[previous]
    bp = np.where(np.isnan(fr["bp"]), 0.0, fr["bp"])  # (rows the oracle must not read: use_eff is 0 there)
    assert not np.any(np.isnan(fr["bp"][use_eff != 0]))
    rl, rd, hp, hs, ctr = oracle.match_to_map_uninit(fr["desc"], bp, use_eff, prev_packed, begin, rows, e0, r0,
                                                     pose_second, 0.5 * (cam.fu + cam.fv), THRESHOLD, census=census)
    rl = np.where(rl >= 0, idx[np.maximum(rl, 0)], -1) if len(idx) else rl
    return rl.astype(np.int32), rd.astype(np.int32), hp, hs, int(ctr)


# ---- the gate scenes of gate_scenes.uninit_scene as a table and a pool ----------------------------------
def gate_pool(sc):
    """The landmarks of an uninit scene as what a first pass would have left: obs_desc = the scene's pool rows; rows
    truncated to min(count, 2) per landmark; status 2, but 1 for the landmarks with l % 7 == 3 (rows left in place) and
    0 for the empty ones.  -> (obs_desc, pool dict)"""
    begin = np.asarray(sc["desc_begin"], dtype=np.int64)
    L = len(begin) - 1
    count = begin[1:] - begin[:-1]
    pool = dict(status=np.full(L, 2, np.int32), n_desc=np.minimum(count, 2).astype(np.int32),
                obs_rows=np.full((L, 3), -1, np.int32), e_W=np.zeros((L, 2, 3)), r_W=np.zeros((L, 2, 3)))
    pool["status"][np.arange(L) % 7 == 3] = 1
    pool["status"][count == 0] = 0
    for l in range(L):
        for d in range(pool["n_desc"][l]):
            pool["obs_rows"][l, d] = begin[l] + d
            pool["e_W"][l, d] = sc["e0"][begin[l] + d]
            pool["r_W"][l, d] = sc["r0"][begin[l] + d]
    return np.ascontiguousarray(sc["pool"], dtype=np.uint8).reshape(-1, 48), pool


def gate_frame(sc, n=None):
    n = len(sc["desc"]) if n is None else n
    return dict(kps=sc["kps"][:n], desc=sc["desc"][:n], bp=sc["bp"][:n], bv=sc["bv"][:n], use=sc["use"][:n],
                previous=sc["previous"][:n])


def gate_census(oracle):
    """(census of the hand-built pools, census of the untruncated scenes), over gate_scenes.UNINIT_SPECS"""
    mine, theirs = oracle.new_census(), oracle.new_census()
    for spec in gate_scenes.UNINIT_SPECS:
        sc = gate_scenes.uninit_scene(spec[0], spec[1], spec[2], **spec[3])
        gate_scenes.run_uninit(oracle, sc, theirs)
        obs_desc, pool = gate_pool(sc)
        reference(oracle, obs_desc, pool, gate_frame(sc), sc["T1"], sc["cam"], True, census=mine)
    return mine, theirs


# ---- GPU side ------------------------------------------------------------------------------------------
class DescTable:
    """a device table of which the second pass reads obs_desc and n_landmarks alone (the gate scenes)"""

    def __init__(self, fe, obs_desc, n_landmarks):
        self.n_landmarks = int(n_landmarks)
        self.t = M._dev(np.ascontiguousarray(obs_desc, dtype=np.uint8).reshape(-1, 48))
        self.desc = fe.make_landmark_table_device(self.n_landmarks, len(obs_desc), 0, None, None, None, None,
                                                  self.t.data_ptr(), None, None)


def prepare(fe, L, frames, pool=None):
    """the device tensors of a batch: gather blocks (with back-projections), use and previous rows, the pool (filled
    with SENTINEL, or holding `pool`: a list of per-frame dicts) and the outputs of both passes filled with
    sentinels (synchronises)"""
    import torch
    from okvis2_amd import multigpu
    K, nf = fe.max_keypoints, len(frames)
    blocks = np.stack([multigpu.pack_block_host(K, fr["kps"], fr["desc"], fr["bp"], fr["bv"]) for fr in frames])
    use = np.zeros((nf, K), np.uint8)
    prev = np.full((nf, K), -1, np.int32)
    for f, fr in enumerate(frames):
        use[f, :len(fr["use"])] = fr["use"]
        prev[f, :len(fr["previous"])] = fr["previous"]
    T = dict(blocks=M._dev(blocks), use=M._dev(use), prev=M._dev(prev))
    for k in ("lm", "bd", "lm2", "bd2"):
        T[k] = torch.full((nf, K), SENTINEL, dtype=torch.int32, device="cuda")
    T["hp"] = torch.full((nf, K, 4), float(SENTINEL), dtype=torch.float64, device="cuda")
    T["hs"] = torch.full((nf, K), HS_FILL, dtype=torch.uint8, device="cuda")
    T["ctr"] = torch.full((nf,), CTR_FILL, dtype=torch.int32, device="cuda")
    for k in M.POOL_KEYS:
        dt = np.int32 if k in ("status", "n_desc", "obs_rows") else np.float64
        a = np.full((nf, max(L, 1)) + M.POOL_SHAPES[k], SENTINEL, dtype=dt)
        if pool is not None and k != "projection":
            for f in range(nf):
                a[f, :L] = pool[f][k]
        T[k] = M._dev(a)
    torch.cuda.synchronize()  # (the uploads above ran on torch's stream)
    return T


def pool_device(fe, T, projection=True):
    return fe.make_landmark_pool_device(*[T[k].data_ptr() if (k != "projection" or projection) else None
                                          for k in M.POOL_KEYS])


def launch_first(fe, tab, T, poses, cam_ids, thr, exclusive, with_use=True, stream=None):
    fe.match_to_map_table_blocks_device(tab.desc, T["blocks"].data_ptr(), len(T["lm"]), cam_ids, poses, thr, exclusive,
                                        T["use"].data_ptr() if with_use else None, pool_device(fe, T),
                                        T["lm"].data_ptr(), T["bd"].data_ptr(), stream)


def launch_second(fe, tab, T, poses, cam_ids, exclusive, with_use=True, previous="prev", stream=None):
    """the call alone: nothing here waits for the device.  previous: the name of the tensor passed as
    previous_landmark_dev ("prev": the frames' rows; "lm": the first pass's best_landmark_dev) or None"""
    fe.match_to_map_table_uninitialised_blocks_device(
        tab.desc, pool_device(fe, T, projection=False), T["blocks"].data_ptr(), len(T["lm2"]), cam_ids, poses,
        exclusive, T["use"].data_ptr() if with_use else None, T[previous].data_ptr() if previous else None,
        T["lm2"].data_ptr(), T["bd2"].data_ptr(), T["hp"].data_ptr(), T["hs"].data_ptr(), T["ctr"].data_ptr(), stream)


def collect(T, stream=None):
    import torch
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return {k: T[k].cpu().numpy() for k in ("lm", "bd", "lm2", "bd2", "hp", "hs", "ctr")}


def check_frame(got, f, n, ref, what):
    """frame f of a collected batch against its reference; rows at or past the keypoint count untouched"""
    rl, rd, hp, hs, ctr = ref
    lm2, bd2 = got["lm2"][f], got["bd2"][f]
    assert np.array_equal(lm2[:n], rl), (what, "landmark", np.flatnonzero(lm2[:n] != rl)[:8])
    assert np.array_equal(bd2[:n], rd), (what, "distance", np.flatnonzero(bd2[:n] != rd)[:8])
    assert np.array_equal(got["hs"][f, :n], hs), (what, "hp_set", np.flatnonzero(got["hs"][f, :n] != hs)[:8])
    M.same_f64(got["hp"][f, :n], hp, what + ("hps_W",))
    assert int(got["ctr"][f]) == ctr, (what, "already_matched", int(got["ctr"][f]), ctr)
    assert np.all(lm2[n:] == SENTINEL) and np.all(bd2[n:] == SENTINEL), (what, "rows past the count")
    assert np.all(got["hs"][f, n:] == HS_FILL) and np.all(got["hp"][f, n:] == float(SENTINEL)), (what, "rows past the count")
