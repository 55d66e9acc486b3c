#!/usr/bin/env python3
"""What the second pass of matchToMap from a device-resident landmark table costs
(okvfe_match_to_map_table_uninitialised_blocks_device).

The workload of tools/bench_map_table.py: 5000 landmarks in front of a twelve-keyframe arc, 1..5 observations each
(about 3), 700 keypoints per frame, 64 distinct poses and frames repeated to fill a batch, EuRoC context, first pass
at 20 px, not exclusive.  A frame's keypoints sit at the projections of landmarks its first pass left as not 3-D yet
(status 2), with a noisy copy of a pooled descriptor and the ray to the landmark as back-projection; the rest is
clutter.  The second pass runs with the first pass's pose turned by 0.002 rad and moved by about a centimetre.
Everything is timed in ONE process, the variants of a comparison alternating repetition by repetition; a repetition is
one call (or one batch call) that ends in a stream synchronisation, on the host clock.  Boxes differ by several per
cent, so only the same-run comparison means anything.  Median and p10-p90 band over `--reps` repetitions (at least
30); one JSON line per comparison, and the status-2 set sizes the frames have.

  (a) B = 1    A  the host chain: the status-2 rows of the (already downloaded) pool compacted on the host, then
                  okvfe_match_to_map_uninitialised (upload, one kernel, rows back on the host)
               A' okvfe_match_to_map_uninitialised alone, on the set compacted beforehand
               B  the new call on one gather block and the pool the first pass left on the device + one stream
                  synchronisation (rows stay on the device)
  (b) B = 256, 3072
               A  okvfe_match_to_map_uninitialised_blocks_device with ONE pooled set for all frames: the set of the
                  frame whose status-2 set has the median size (it prepares nothing: the floor)
               B  the new call: every frame's own set, packed on the device, then matched
               The difference is the per-frame surcharge; recorded, not gated.

    python tools/bench_map_table_uninit.py [--batches 256,3072] [--reps 30] [--landmarks 5000]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_map_table import band, frame_poses, make_table, rot_y, timed  # noqa: E402


def second_pose(pose):
    C1, r1 = pose[0].reshape(3, 3), pose[1]
    return (C1 @ rot_y(0.002)).reshape(-1).copy(), r1 + np.array([0.01, -0.005, 0.003])


def compact(st, nd, rows, e_W, r_W, obs_desc):
    """the status-2 landmarks of one frame's pool as the packed set of okvfe_match_to_map_uninitialised (host)"""
    idx = np.flatnonzero(st == 2)
    n = nd[idx]
    begin = np.zeros(len(idx) + 1, np.int32)
    np.cumsum(n, out=begin[1:])
    keep = np.arange(2)[None, :] < n[:, None]
    return (idx, begin, obs_desc[rows[idx, :2][keep]], np.ascontiguousarray(e_W[idx][keep]),
            np.ascontiguousarray(r_W[idx][keep]))


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
    cam = cfg.cams[0]
    K, L, thr = cfg.max_kpts, args.landmarks, args.threshold
    focal = 0.5 * (cam.fu + cam.fv)
    fe = capi.Frontend(cfg.w, cfg.h, cfg.uniformity_radius, 0, cfg.abs_threshold, K,
                       match_threshold=cfg.match_threshold, max_batch=1, num_cameras=1)
    fe.set_camera(0, cam)
    lib = capi.lib()
    tab = make_table(L)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in tab.items()}
    n_obs, n_poses = len(tab["obs_pose"]), len(tab["poses"])
    table_dev = fe.make_landmark_table_device(L, n_obs, n_poses, *[dev[k].data_ptr() for k in (
        "hp", "quality", "obs_begin", "obs_pose", "obs_desc", "obs_bp", "poses")])
    fe.landmark_table_check_device(table_dev)
    print(f"table: {L} landmarks, {n_obs} observations ({n_obs / L:.2f} each); {K} keypoints per frame")

    # the distinct frames: a first pass (no keypoints) gives every pose's pooling, the keypoints are planted on it
    D = args.distinct
    poses = frame_poses(D)
    poses2 = [second_pose(p) for p in poses]
    empty = np.stack([multigpu.pack_block_host(K, np.zeros(0, capi.KEYPOINT_DTYPE), np.zeros((0, 48), np.uint8),
                                               np.zeros((0, 3)), np.zeros(0, np.uint8))] * D)
    d_empty = torch.from_numpy(empty).cuda()

    def pool_tensors(n):
        return dict(status=torch.full((n, L), -1, dtype=torch.int32, device="cuda"),
                    n_desc=torch.zeros((n, L), dtype=torch.int32, device="cuda"),
                    obs_rows=torch.zeros((n, L, 3), dtype=torch.int32, device="cuda"),
                    projection=torch.zeros((n, L, 2), dtype=torch.float64, device="cuda"),
                    e_W=torch.zeros((n, L, 2, 3), dtype=torch.float64, device="cuda"),
                    r_W=torch.zeros((n, L, 2, 3), dtype=torch.float64, device="cuda"))

    def pool_struct(t):
        return fe.make_landmark_pool_device(*[t[k].data_ptr() for k in ("status", "n_desc", "obs_rows", "projection",
                                                                        "e_W", "r_W")])

    pd = pool_tensors(D)
    scratch = torch.zeros((2, D, K), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    raw = C.c_void_p(int(stream.cuda_stream))
    fe.match_to_map_table_blocks_device(table_dev, d_empty.data_ptr(), D, [0] * D, poses, thr, False, None,
                                        pool_struct(pd), scratch[0].data_ptr(), scratch[1].data_ptr(), stream)
    stream.synchronize()
    ph = {k: v.cpu().numpy() for k, v in pd.items()}
    rng = np.random.default_rng(7)
    p_W = tab["hp"][:, :3] / tab["hp"][:, 3:4]
    frames, blocks = [], []
    for f in range(D):
        kps = np.zeros(K, dtype=capi.KEYPOINT_DTYPE)
        kps["size"] = 12.0
        kps["x"], kps["y"] = rng.uniform(30, cfg.w - 30, K), rng.uniform(30, cfg.h - 30, K)
        desc = rng.integers(0, 256, (K, 48), dtype=np.uint8)
        bp = np.stack([(kps["x"] - cam.cu) / cam.fu, (kps["y"] - cam.cv) / cam.fv, np.ones(K)], 1).astype(np.float64)
        p = ph["projection"][f]
        vis = np.flatnonzero((ph["status"][f] == 2) & (p[:, 0] > 0) & (p[:, 0] < cfg.w) & (p[:, 1] > 0) & (p[:, 1] < cfg.h))
        obs = rng.permutation(vis)[:int(0.8 * K)]
        kps["x"][:len(obs)] = p[obs, 0] + rng.normal(0, 1.5, len(obs))
        kps["y"][:len(obs)] = p[obs, 1] + rng.normal(0, 1.5, len(obs))
        flips = ((rng.random((len(obs), 48)) < 0.04) * rng.integers(1, 256, (len(obs), 48))).astype(np.uint8)
        desc[:len(obs)] = tab["obs_desc"][ph["obs_rows"][f, obs, 0]] ^ flips
        bp[:len(obs)] = (p_W[obs] - poses[f][1]) @ poses[f][0].reshape(3, 3)  # the ray to the landmark, camera frame
        frames.append((kps, desc, bp))
        blocks.append(multigpu.pack_block_host(K, kps, desc, bp, np.ones(K, np.uint8)))
    n2 = (ph["status"] == 2).sum(axis=1)
    rows2 = np.where(ph["status"] == 2, ph["n_desc"], 0).sum(axis=1)
    sizes = dict(status2_min=int(n2.min()), status2_median=int(np.median(n2)), status2_max=int(n2.max()),
                 pooled_rows_median=int(np.median(rows2)))
    print(f"status-2 landmarks per frame: {n2.min()}..{n2.max()} (median {int(np.median(n2))}) of {L}, "
          f"{int(np.median(rows2))} pooled rows at the median")

    def outputs(n):
        return dict(lm=torch.zeros((n, K), dtype=torch.int32, device="cuda"),
                    bd=torch.zeros((n, K), dtype=torch.int32, device="cuda"),
                    hp=torch.zeros((n, K, 4), dtype=torch.float64, device="cuda"),
                    hs=torch.zeros((n, K), dtype=torch.uint8, device="cuda"),
                    ctr=torch.zeros((n,), dtype=torch.int32, device="cuda"))

    def out_ptrs(o):
        return [capi._p(o[k].data_ptr()) for k in ("lm", "bd", "hp", "hs", "ctr")]

    fn = getattr(lib, "okvfe_match_to_map_table_uninitialised_blocks_device")

    # ---- (a) B = 1 ------------------------------------------------------------------------------------------
    kps0, desc0, bp0 = frames[0]
    use0, prev0 = np.ones(K, np.uint8), np.full(K, -1, np.int32)
    pool0 = {k: np.ascontiguousarray(v[0]) for k, v in ph.items()}
    T2 = capi.make_pose(*poses2[0])
    lm_h, bd_h, hp_h, hs_h = np.zeros(K, np.int32), np.zeros(K, np.int32), np.zeros((K, 4)), np.zeros(K, np.uint8)
    ctr_h = C.c_int32()
    d_block = torch.from_numpy(blocks[0][None]).cuda()
    pd1 = {k: v[:1].contiguous() for k, v in pd.items()}
    pool1 = pool_struct(pd1)
    o1 = outputs(1)
    cam1, pose1 = (C.c_int32 * 1)(0), (capi.Pose * 1)(T2)
    torch.cuda.synchronize()
    packed = {}

    def uninitialised(idx, begin, rows, e0, r0):
        s = lib.okvfe_match_to_map_uninitialised(fe._h, capi._p(desc0), capi._p(bp0), capi._p(use0), capi._p(prev0), K,
                                                 capi._p(begin), len(idx), capi._p(rows), capi._p(e0), capi._p(r0),
                                                 C.byref(T2), C.c_double(focal), capi._p(lm_h), capi._p(bd_h),
                                                 capi._p(hp_h), capi._p(hs_h), C.byref(ctr_h))
        assert s == 0, s

    def a_chain():
        packed["set"] = compact(pool0["status"], pool0["n_desc"], pool0["obs_rows"], pool0["e_W"], pool0["r_W"],
                                tab["obs_desc"])
        uninitialised(*packed["set"])

    def a_call_only():
        uninitialised(*packed["set"])

    def b_device():
        s = fn(fe._h, C.byref(table_dev), C.byref(pool1), capi._p(d_block.data_ptr()), 1, cam1, pose1, 0, None, None,
               *out_ptrs(o1), raw)
        assert s == 0, s
        lib.okvfe_stream_synchronize(raw)

    a_chain()
    t = timed({"host_compaction_and_uninitialised": a_chain, "uninitialised_alone": a_call_only,
               "table_uninitialised": b_device}, args.reps)
    idx0 = packed["set"][0]
    la = np.where(lm_h >= 0, idx0[np.maximum(lm_h, 0)], -1)
    assert np.array_equal(la, o1["lm"][0].cpu().numpy()) and np.array_equal(bd_h, o1["bd"][0].cpu().numpy()), \
        "the two routes disagree"
    assert np.array_equal(hp_h.view(np.uint64), o1["hp"][0].cpu().numpy().view(np.uint64))
    res = {k: band(v) for k, v in t.items()}
    res.update(comparison="B=1", reps=args.reps, matches=int((lm_h >= 0).sum()), status2=int(len(idx0)),
               gain_ms=round(res["host_compaction_and_uninitialised"]["median_ms"] - res["table_uninitialised"]["median_ms"], 4),
               below_chain_p10=bool(res["table_uninitialised"]["median_ms"] < res["host_compaction_and_uninitialised"]["p10_ms"]))
    res.update(sizes)
    print(json.dumps(res))

    # ---- (b) batches ----------------------------------------------------------------------------------------
    fm = int(np.argsort(n2)[len(n2) // 2])  # the frame whose status-2 set has the median size: shared by variant A
    idx, begin, rows, e0, r0 = compact(ph["status"][fm], ph["n_desc"][fm], ph["obs_rows"][fm], ph["e_W"][fm],
                                       ph["r_W"][fm], tab["obs_desc"])
    d_set = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (begin, rows, e0, r0)]
    md = fe.make_map_device(len(idx), d_set[0].data_ptr(), d_set[1].data_ptr(), None, d_set[2].data_ptr(),
                            d_set[3].data_ptr())
    for B in [int(b) for b in args.batches.split(",")]:
        rep = [(fm + i) % D for i in range(B)]  # (frame 0 of the batch is the owner of the shared set)
        d_blocks = torch.from_numpy(np.stack([blocks[i] for i in rep])).cuda()
        sel = torch.tensor(rep, device="cuda")
        pdB = {k: v.index_select(0, sel).contiguous() for k, v in pd.items() if k != "projection"}
        pdB["projection"] = pd["projection"][:1]  # (not read)
        poolB = pool_struct(pdB)
        cams = (C.c_int32 * B)(*([0] * B))
        PB = (capi.Pose * B)(*[capi.make_pose(*poses2[i]) for i in rep])
        oa, ob = outputs(B), outputs(B)
        torch.cuda.synchronize()

        def a_shared():
            s = lib.okvfe_match_to_map_uninitialised_blocks_device(
                fe._h, capi._p(d_blocks.data_ptr()), B, None, None, C.byref(md), PB, C.c_double(focal), *out_ptrs(oa), raw)
            assert s == 0, s
            lib.okvfe_stream_synchronize(raw)

        def b_table():
            s = fn(fe._h, C.byref(table_dev), C.byref(poolB), capi._p(d_blocks.data_ptr()), B, cams, PB, 0, None, None,
                   *out_ptrs(ob), raw)
            assert s == 0, s
            lib.okvfe_stream_synchronize(raw)

        t = timed({"shared_set_blocks": a_shared, "table_uninitialised": b_table}, args.reps)
        res = {k: band(v) for k, v in t.items()}
        # frame 0 has the same set in both: its rows agree once A's packed index is mapped to the table
        la = oa["lm"][0].cpu().numpy()
        la = np.where(la >= 0, idx[np.maximum(la, 0)], -1)
        assert np.array_equal(la, ob["lm"][0].cpu().numpy()), "frame 0 differs between the two routes"
        assert np.array_equal(oa["hp"][0].cpu().numpy().view(np.uint64), ob["hp"][0].cpu().numpy().view(np.uint64))
        res.update(comparison=f"B={B}", reps=args.reps, shared_set=int(len(idx)),
                   matches_per_frame=round(float((ob["lm"] >= 0).sum().item()) / B, 1),
                   surcharge_ms=round(res["table_uninitialised"]["median_ms"] - res["shared_set_blocks"]["median_ms"], 4),
                   per_frame_us=round(res["table_uninitialised"]["median_ms"] * 1e3 / B, 3))
        print(json.dumps(res))
        del d_blocks, pdB, oa, ob
    fe.close()


if __name__ == "__main__":
    main()
