"""Shared by the tests of okvfe_match_to_map_table_blocks_device (matchToMap from a device-resident landmark table, a
batch of frames): frames and their poses, the per-frame reference, the upload of a map_scenes.py table and the call.

The per-frame reference is the one of test_gpu_map_census.py: oracle.prepare_landmarks with the frame's pose and camera,
map_synth.packed_set of its status-1 landmarks, oracle.match_to_map on that set, the packed index mapped back to the
table.  CPU only up to `upload` / `run_batch`, which need torch and a GPU."""
import numpy as np

import map_scenes as S
import map_synth
from gate_scenes import rodrigues
from okvis2_amd import synth

THRESHOLD = synth.euroc_config().match_threshold
SENTINEL = -7
POOL_KEYS = ("status", "n_desc", "obs_rows", "projection", "e_W", "r_W")
POOL_SHAPES = {"status": (), "n_desc": (), "obs_rows": (3,), "projection": (2,), "e_W": (2, 3), "r_W": (2, 3)}


def scene_poses(sc):
    """The frame poses of a scene: its T1; one of the table's observing poses, bit for bit; T1 turned by pi about the
    camera's y axis; T1 moved by 0.5 m along the camera's x axis; and, so that a frame with an empty 3-D set exists for
    every camera model, T1 moved 1e6 m backwards (every landmark then sits on the optical axis of a camera whose views
    are all a million times closer: pruned without `exclusive`, and at the image centre at most otherwise)."""
    C, r = np.asarray(sc["T1"][0], dtype=np.float64).reshape(3, 3), np.asarray(sc["T1"][1], dtype=np.float64)
    pi = min(6, len(sc["poses"]) - 1)  # (general scenes: a keyframe pose of the map_synth arc, which faces the scene)
    Co, ro = sc["poses"][pi]
    return [(C.reshape(-1).copy(), r.copy()),
            (np.asarray(Co, dtype=np.float64).reshape(-1).copy(), np.asarray(ro, dtype=np.float64).copy()),
            ((C @ rodrigues((0, 1, 0), np.pi)).reshape(-1), r.copy()),
            (C.reshape(-1).copy(), r + C @ np.array([0.5, 0.0, 0.0])),
            (C.reshape(-1).copy(), r + C @ np.array([0.0, 0.0, -1.0e6]))]


def clutter_frame(oracle, sc, n, seed):
    """n keypoints at random pixels; descriptors are observation descriptors of the table with a few bits flipped (so a
    landmark that projects nearby matches at a small distance), a tenth of the keypoints unused"""
    rng = np.random.default_rng([seed, n, len(sc["hp"])])
    kps = np.zeros(n, dtype=oracle.KEYPOINT_DTYPE)
    kps["size"] = 12.0
    kps["x"] = rng.uniform(0, sc["cam"].w, n)
    kps["y"] = rng.uniform(0, sc["cam"].h, n)
    desc = rng.integers(0, 256, (n, 48), dtype=np.uint8)
    m = len(sc["obs_desc"])
    if m and n:
        flips = ((rng.random((n, 48)) < 0.03) * rng.integers(1, 256, (n, 48))).astype(np.uint8)
        own = rng.random(n) < 0.7
        desc[own] = (sc["obs_desc"][rng.integers(0, m, n)] ^ flips)[own]
    use = (rng.random(n) >= 0.1).astype(np.uint8)
    return kps, desc, use


def cut(frame, K):
    """a frame of more than K keypoints as consecutive frames of at most K"""
    kps, desc, use = frame[:3]
    return [(kps[a:a + K], desc[a:a + K], use[a:a + K]) for a in range(0, max(len(kps), 1), K)]


def reference(oracle, sc, pose, cam, exclusive, thr):
    """oracle pooling of the table for one (pose, camera)"""
    return S.run_oracle(oracle, dict(sc, T1=pose, cam=cam), exclusive, thr)


def reference_matches(oracle, sc, pool, thr, frame, use=None):
    kps, desc, u = frame[:3]
    if use is None:
        use = u
    idx, proj, begin, rows = map_synth.packed_set(pool, sc["obs_desc"], 1)
    rl, rd = oracle.match_to_map(desc, kps, use, proj, begin, rows, thr, THRESHOLD)
    rl = np.where(rl >= 0, idx[np.maximum(rl, 0)], -1) if len(idx) else rl
    return rl.astype(np.int32), rd.astype(np.int32)


def same_f64(got, ref, what):
    """uint64 patterns; where the oracle holds a NaN the device holds one too and nothing more is asked (the NaN-place
    rule of test_gpu_map_census.py)"""
    got, ref = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(ref, dtype=np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN places differ", np.argwhere(np.isnan(got) != nan)[:5])
    same = got.view(np.uint64) == ref.view(np.uint64)
    assert np.all(same | nan), (what, np.argwhere(~(same | nan))[:5])


def check_pool(got, ref, what):
    for k in ("status", "n_desc", "obs_rows"):
        assert np.array_equal(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:8])
    for k in ("projection", "e_W", "r_W"):
        same_f64(got[k], ref[k], what + (k,))


def table_arrays(sc):
    """the table as the contiguous host arrays of okvfe_landmark_table (poses: n_poses x 12 doubles, C then r)"""
    poses = np.array([np.concatenate([np.asarray(C, dtype=np.float64).reshape(-1), np.asarray(r, dtype=np.float64)])
                      for C, r in sc["poses"]], dtype=np.float64).reshape(-1, 12)
    return dict(hp=np.ascontiguousarray(sc["hp"], dtype=np.float64).reshape(-1, 4),
                quality=np.ascontiguousarray(sc["quality"], dtype=np.float64),
                obs_begin=np.ascontiguousarray(sc["obs_begin"], dtype=np.int32),
                obs_pose=np.ascontiguousarray(sc["obs_pose"], dtype=np.int32),
                obs_desc=np.ascontiguousarray(sc["obs_desc"], dtype=np.uint8).reshape(-1, 48),
                obs_bp=np.ascontiguousarray(sc["obs_bp"], dtype=np.float64).reshape(-1, 3), poses=poses)


# ---- GPU side ------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:  # (a zero-sized tensor has no address)
        a = np.zeros((1,) + a.shape[1:], dtype=a.dtype)
    return torch.from_numpy(a).cuda()


class DeviceTable:
    """a table in device memory: the tensors that own it and the okvfe_landmark_table_device over them"""

    def __init__(self, fe, sc, **override):
        a = table_arrays(sc)
        self.n_landmarks, self.n_observations, self.n_poses = len(a["hp"]), len(a["obs_pose"]), len(a["poses"])
        a.update(override)
        self.t = {k: _dev(v) for k, v in a.items()}
        self.desc = fe.make_landmark_table_device(
            self.n_landmarks, self.n_observations, self.n_poses,
            *[self.t[k].data_ptr() for k in ("hp", "quality", "obs_begin", "obs_pose", "obs_desc", "obs_bp", "poses")])


def prepare_batch(fe, tab, frames, with_pool=True):
    """the device tensors of a batch: gather blocks, use flags, outputs filled with SENTINEL (synchronises)"""
    import torch
    from okvis2_amd import multigpu
    K, nf, L = fe.max_keypoints, len(frames), tab.n_landmarks
    blocks = np.stack([multigpu.pack_block_host(K, kps, desc, np.zeros((len(kps), 3)), np.zeros(len(kps), np.uint8))
                       for kps, desc, _ in frames])
    use = np.zeros((nf, K), np.uint8)
    for f, fr in enumerate(frames):
        use[f, :len(fr[2])] = fr[2]
    T = dict(blocks=_dev(blocks), use=_dev(use),
             lm=torch.full((nf, K), SENTINEL, dtype=torch.int32, device="cuda"),
             bd=torch.full((nf, K), SENTINEL, dtype=torch.int32, device="cuda"))
    if with_pool:
        for k in POOL_KEYS:
            dt = torch.int32 if k in ("status", "n_desc", "obs_rows") else torch.float64
            T[k] = torch.full((nf, max(L, 1)) + POOL_SHAPES[k], SENTINEL, dtype=dt, device="cuda")
    torch.cuda.synchronize()  # (the uploads above ran on torch's stream)
    return T


def launch_batch(fe, tab, T, poses, cam_ids, thr, exclusive, with_use=True, stream=None):
    """the call alone: nothing here waits for the device"""
    pool_dev = fe.make_landmark_pool_device(*[T[k].data_ptr() for k in POOL_KEYS]) if "status" in T else None
    fe.match_to_map_table_blocks_device(tab.desc, T["blocks"].data_ptr(), len(T["lm"]), cam_ids, poses, thr, exclusive,
                                        T["use"].data_ptr() if with_use else None, pool_dev, T["lm"].data_ptr(),
                                        T["bd"].data_ptr(), stream)


def run_batch(fe, tab, frames, poses, cam_ids, thr, exclusive, with_use=True, with_pool=True, stream=None):
    """frames: [(kps, desc, use)].  Returns (lm, bd, pool or None, tensors): lm / bd (n_frames, K) with SENTINEL where
    the call wrote nothing; pool: dict of (n_frames, L, ...) arrays."""
    T = prepare_batch(fe, tab, frames, with_pool)
    launch_batch(fe, tab, T, poses, cam_ids, thr, exclusive, with_use, stream)
    return collect(T, tab.n_landmarks, stream)


def collect(T, L, stream=None):
    import torch
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    pool = {k: T[k].cpu().numpy()[:, :L] for k in POOL_KEYS} if "status" in T else None
    return T["lm"].cpu().numpy(), T["bd"].cpu().numpy(), pool, T


def check_frame(oracle, sc, ref, thr, frame, lm_row, bd_row, what, with_use=True):
    """one frame's rows against the reference; rows at or past the keypoint count untouched"""
    n = len(frame[0])
    rl, rd = reference_matches(oracle, sc, ref, thr, frame, None if with_use else np.ones(n, np.uint8))
    assert np.array_equal(lm_row[:n], rl), (what, np.flatnonzero(lm_row[:n] != rl)[:8])
    assert np.array_equal(bd_row[:n], rd), (what, np.flatnonzero(bd_row[:n] != rd)[:8])
    assert np.all(lm_row[n:] == SENTINEL) and np.all(bd_row[n:] == SENTINEL), (what, "rows past the count")
    return rl
