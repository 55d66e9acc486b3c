#!/usr/bin/env python3
"""What matchToMap from a device-resident landmark table costs (okvfe_match_to_map_table_blocks_device).

The table: 5000 landmarks in front of a twelve-keyframe arc, 1..5 observations each (about 3), seeded.  A frame: 700
keypoints, most of them at the projections of 3-D landmarks with a noisy copy of a pooled descriptor, seen from a
pose near the arc's end (64 distinct poses and frames, repeated to fill a batch).  EuRoC context, reprojection radius
20 px, not exclusive.  Everything is timed in ONE process, the two variants of a comparison alternating repetition by
repetition; a repetition is one call (or one batch call) that ends in a stream synchronisation, on the host clock.
Boxes differ by several per cent, so only the same-run comparison means anything.  Median and p10-p90 band over
`--reps` repetitions (at least 30); one JSON line per comparison.

  (a) B = 1    A  okvfe_match_to_map_landmarks: table upload, three host synchronisations, rows back on the host
               B  the new call on one gather block + one stream synchronisation (rows stay on the device)
               B' B plus the download of the two match rows
  (b) B = 256, 3072
               A  okvfe_match_to_map_blocks_device with frame 0's pooled set for all frames and per-frame projections
                  (what bench.py --workload map times: no preparation at all)
               B  the new call: exact per-frame preparation + packing + matching
               The difference is what the per-frame preparation costs; recorded, not gated.

    python tools/bench_map_table.py [--batches 256,3072] [--reps 30] [--landmarks 5000]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def make_table(n_landmarks, seed=1, n_poses=12):
    rng = np.random.default_rng(seed)
    poses = np.zeros((n_poses, 12))
    for i in range(n_poses):
        poses[i, :9] = rot_y(0.08 * (i - n_poses / 2)).reshape(-1)
        poses[i, 9:] = (0.25 * i - 1.5, 0.02 * i, 0.1 * np.sin(i))
    p = np.stack([rng.uniform(-6, 6, n_landmarks), rng.uniform(-3, 3, n_landmarks), rng.uniform(1.5, 12, n_landmarks)], 1)
    p[rng.random(n_landmarks) < 0.08, 2] *= -1.0
    hp = np.concatenate([p, np.ones((n_landmarks, 1))], 1)
    quality = rng.choice([1.0, 0.3, 0.05, 0.001], n_landmarks, p=[0.4, 0.3, 0.2, 0.1])
    n_obs = rng.integers(1, 6, n_landmarks)
    obs_begin = np.concatenate([[0], np.cumsum(n_obs)]).astype(np.int32)
    owner = np.repeat(np.arange(n_landmarks), n_obs)
    obs_pose = rng.integers(0, n_poses, len(owner)).astype(np.int32)
    ray = np.einsum("nji,nj->ni", poses[obs_pose, :9].reshape(-1, 3, 3), p[owner] - poses[obs_pose, 9:])
    obs_bp = ray * (rng.uniform(0.2, 3.0, len(owner)) / np.maximum(np.linalg.norm(ray, axis=1), 1e-9))[:, None]
    base = rng.integers(0, 256, (n_landmarks, 48), dtype=np.uint8)
    flips = ((rng.random((len(owner), 48)) < 0.04) * rng.integers(1, 256, (len(owner), 48))).astype(np.uint8)
    return dict(hp=hp, quality=quality, obs_begin=obs_begin, obs_pose=obs_pose, obs_desc=base[owner] ^ flips,
                obs_bp=np.ascontiguousarray(obs_bp), poses=poses)


def frame_poses(n):
    return [((rot_y(0.03) @ rot_y(0.003 * (f - n / 2))).reshape(-1).copy(),
             np.array([0.4 + 0.01 * f, 0.0, 0.3 + 0.002 * f])) for f in range(n)]


def band(x):
    x = np.asarray(x) * 1e3
    return {"median_ms": round(float(np.median(x)), 4), "p10_ms": round(float(np.percentile(x, 10)), 4),
            "p90_ms": round(float(np.percentile(x, 90)), 4)}


def timed(fns, reps, warmup=3):
    """fns: {name: callable that ends in a synchronisation}; alternating, `reps` repetitions each"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            t0 = time.perf_counter()
            f()
            out[k].append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", default="256,3072")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--landmarks", type=int, default=5000)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--threshold", type=float, default=20.0)
    args = ap.parse_args()
    if args.reps < 30:
        ap.error("--reps: at least 30")
    import torch
    from okvis2_amd import capi, multigpu, synth

    cfg = synth.euroc_config()
    K, L, thr = cfg.max_kpts, args.landmarks, args.threshold
    fe = capi.Frontend(cfg.w, cfg.h, cfg.uniformity_radius, 0, cfg.abs_threshold, K,
                       match_threshold=cfg.match_threshold, max_batch=1, num_cameras=1)
    fe.set_camera(0, cfg.cams[0])
    lib = capi.lib()
    tab = make_table(L)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in tab.items()}
    n_obs, n_poses = len(tab["obs_pose"]), len(tab["poses"])
    table_dev = fe.make_landmark_table_device(L, n_obs, n_poses, *[dev[k].data_ptr() for k in (
        "hp", "quality", "obs_begin", "obs_pose", "obs_desc", "obs_bp", "poses")])
    fe.landmark_table_check_device(table_dev)
    print(f"table: {L} landmarks, {n_obs} observations ({n_obs / L:.2f} each), "
          f"{sum(v.nbytes for v in tab.values()) / 1e6:.2f} MB; {K} keypoints per frame")

    # the distinct frames: a first pass (no keypoints) gives every pose's pooling, the keypoints are planted on it
    D = args.distinct
    poses = frame_poses(D)
    empty = np.stack([multigpu.pack_block_host(K, np.zeros(0, capi.KEYPOINT_DTYPE), np.zeros((0, 48), np.uint8),
                                               np.zeros((0, 3)), np.zeros(0, np.uint8))] * D)
    d_empty = torch.from_numpy(empty).cuda()
    st = torch.full((D, L), -1, dtype=torch.int32, device="cuda")
    nd = torch.zeros((D, L), dtype=torch.int32, device="cuda")
    rows = torch.zeros((D, L, 3), dtype=torch.int32, device="cuda")
    proj = torch.zeros((D, L, 2), dtype=torch.float64, device="cuda")
    scratch = torch.zeros((2, D, K), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    fe.match_to_map_table_blocks_device(table_dev, d_empty.data_ptr(), D, [0] * D, poses, thr, False, None,
                                        fe.make_landmark_pool_device(st.data_ptr(), nd.data_ptr(), rows.data_ptr(),
                                                                     proj.data_ptr()),
                                        scratch[0].data_ptr(), scratch[1].data_ptr(), stream)
    stream.synchronize()
    st_h, nd_h, rows_h, proj_h = (t.cpu().numpy() for t in (st, nd, rows, proj))
    rng = np.random.default_rng(7)
    frames, blocks = [], []
    for f in range(D):
        kps = np.zeros(K, dtype=capi.KEYPOINT_DTYPE)
        kps["size"] = 12.0
        kps["x"], kps["y"] = rng.uniform(30, cfg.w - 30, K), rng.uniform(30, cfg.h - 30, K)
        desc = rng.integers(0, 256, (K, 48), dtype=np.uint8)
        p = proj_h[f]
        vis = np.flatnonzero((st_h[f] == 1) & (p[:, 0] > 0) & (p[:, 0] < cfg.w) & (p[:, 1] > 0) & (p[:, 1] < cfg.h))
        obs = rng.permutation(vis)[:int(0.8 * K)]
        kps["x"][:len(obs)] = p[obs, 0] + rng.normal(0, 1.5, len(obs))
        kps["y"][:len(obs)] = p[obs, 1] + rng.normal(0, 1.5, len(obs))
        flips = ((rng.random((len(obs), 48)) < 0.04) * rng.integers(1, 256, (len(obs), 48))).astype(np.uint8)
        desc[:len(obs)] = tab["obs_desc"][rows_h[f, obs, 0]] ^ flips
        frames.append((kps, desc))
        blocks.append(multigpu.pack_block_host(K, kps, desc, np.zeros((K, 3)), np.ones(K, np.uint8)))
    n3 = (st_h == 1).sum(axis=1)
    print(f"3-D landmarks per frame: {n3.min()}..{n3.max()} of {L}")

    # ---- (a) B = 1 ------------------------------------------------------------------------------------------
    kps0, desc0 = frames[0]
    use0 = np.ones(K, np.uint8)
    P = (capi.Pose * n_poses)(*[capi.make_pose(r[:9], r[9:]) for r in tab["poses"]])
    host_table = capi.LandmarkTable(L, n_obs, n_poses, *[tab[k].ctypes.data for k in (
        "hp", "quality", "obs_begin", "obs_pose", "obs_desc", "obs_bp")], C.addressof(P))
    T1 = capi.make_pose(*poses[0])
    lm_h, bd_h = np.zeros(K, np.int32), np.zeros(K, np.int32)
    d_block = torch.from_numpy(blocks[0][None]).cuda()
    lm1 = torch.zeros((1, K), dtype=torch.int32, device="cuda")
    bd1 = torch.zeros((1, K), dtype=torch.int32, device="cuda")
    cam1, pose1 = (C.c_int32 * 1)(0), (capi.Pose * 1)(T1)
    raw = C.c_void_p(int(stream.cuda_stream))
    torch.cuda.synchronize()

    def a_host():
        s = lib.okvfe_match_to_map_landmarks(fe._h, 0, C.byref(host_table), C.byref(T1), C.c_double(thr), 0,
                                             capi._p(desc0), capi._p(kps0), capi._p(use0), K, None, capi._p(lm_h),
                                             capi._p(bd_h))
        assert s == 0, s

    def b_device():
        s = lib.okvfe_match_to_map_table_blocks_device(fe._h, C.byref(table_dev), capi._p(d_block.data_ptr()), 1, cam1,
                                                       pose1, C.c_double(thr), 0, None, None, capi._p(lm1.data_ptr()),
                                                       capi._p(bd1.data_ptr()), raw)
        assert s == 0, s
        lib.okvfe_stream_synchronize(raw)

    lm_b, bd_b = np.zeros(K, np.int32), np.zeros(K, np.int32)

    def b_device_download():
        b_device()
        lib.okvfe_copy_to_host(capi._p(lm_b), capi._p(lm1.data_ptr()), C.c_size_t(K * 4), raw)
        lib.okvfe_copy_to_host(capi._p(bd_b), capi._p(bd1.data_ptr()), C.c_size_t(K * 4), raw)
        lib.okvfe_stream_synchronize(raw)

    t = timed({"landmarks_host": a_host, "table_blocks": b_device, "table_blocks_download": b_device_download}, args.reps)
    assert np.array_equal(lm_h, lm_b) and np.array_equal(bd_h, bd_b), "the two routes disagree"
    res = {k: band(v) for k, v in t.items()}
    res.update(comparison="B=1", reps=args.reps, matches=int((lm_h >= 0).sum()),
               gain_ms=round(res["landmarks_host"]["median_ms"] - res["table_blocks"]["median_ms"], 4))
    print(json.dumps(res))

    # ---- (b) batches ----------------------------------------------------------------------------------------
    idx = np.flatnonzero(st_h[0] == 1)  # frame 0's pooled set, shared by every frame of variant A
    begin = np.concatenate([[0], np.cumsum(nd_h[0, idx])]).astype(np.int32)
    pool = np.concatenate([tab["obs_desc"][rows_h[0, l, :nd_h[0, l]]] for l in idx])
    d_begin, d_pool = torch.from_numpy(begin).cuda(), torch.from_numpy(np.ascontiguousarray(pool)).cuda()
    for B in [int(b) for b in args.batches.split(",")]:
        rep = [i % D for i in range(B)]
        d_blocks = torch.from_numpy(np.stack([blocks[i] for i in rep])).cuda()
        d_proj = torch.from_numpy(np.ascontiguousarray(np.stack([proj_h[i][idx] for i in rep]))).cuda()
        bposes = [poses[i] for i in rep]
        cams = (C.c_int32 * B)(*([0] * B))
        PB = (capi.Pose * B)(*[capi.make_pose(*p) for p in bposes])
        lm_a = torch.zeros((B, K), dtype=torch.int32, device="cuda")
        bd_a = torch.zeros((B, K), dtype=torch.int32, device="cuda")
        lm_n = torch.zeros((B, K), dtype=torch.int32, device="cuda")
        bd_n = torch.zeros((B, K), dtype=torch.int32, device="cuda")
        md = fe.make_map_device(len(idx), d_begin.data_ptr(), d_pool.data_ptr(), d_proj.data_ptr())
        torch.cuda.synchronize()

        def a_blocks():
            s = lib.okvfe_match_to_map_blocks_device(fe._h, capi._p(d_blocks.data_ptr()), B, None, C.byref(md),
                                                     C.c_double(thr), capi._p(lm_a.data_ptr()), capi._p(bd_a.data_ptr()), raw)
            assert s == 0, s
            lib.okvfe_stream_synchronize(raw)

        def b_table():
            s = lib.okvfe_match_to_map_table_blocks_device(fe._h, C.byref(table_dev), capi._p(d_blocks.data_ptr()), B,
                                                           cams, PB, C.c_double(thr), 0, None, None,
                                                           capi._p(lm_n.data_ptr()), capi._p(bd_n.data_ptr()), raw)
            assert s == 0, s
            lib.okvfe_stream_synchronize(raw)

        t = timed({"pooled_blocks": a_blocks, "table_blocks": b_table}, args.reps)
        res = {k: band(v) for k, v in t.items()}
        # frame 0 has the same pooled set in both: its rows agree once A's packed index is mapped to the table
        la = lm_a[0].cpu().numpy()
        la = np.where(la >= 0, idx[np.maximum(la, 0)], -1)
        assert np.array_equal(la, lm_n[0].cpu().numpy()), "frame 0 differs between the two routes"
        res.update(comparison=f"B={B}", reps=args.reps, matches_per_frame=round(float((lm_n >= 0).sum().item()) / B, 1),
                   preparation_ms=round(res["table_blocks"]["median_ms"] - res["pooled_blocks"]["median_ms"], 4),
                   per_frame_us=round(res["table_blocks"]["median_ms"] * 1e3 / B, 3))
        print(json.dumps(res))
        del d_blocks, d_proj, lm_a, bd_a, lm_n, bd_n
    fe.close()


if __name__ == "__main__":
    main()
