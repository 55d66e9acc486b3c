#!/usr/bin/env python3
"""What batching matchMotionStereo buys: okvfe_match_motion_stereo_blocks_batch_device against a loop of
okvfe_match_motion_stereo_blocks_device calls, and the in-place sweep over older frames against the host chain.

Workload: EuRoC, 2 cameras, 700 keypoints per frame.  A static cloud of 4000 points 2 .. 12 m in front of the rig; 16
older and 16 current frames (camera = frame index % 2) each keep 700 of the points they see: the keypoint at the
radial-tangential projection with 0.3 px of noise, the ray to the point as back-projection, the point's descriptor with
about 3 % of its bytes disturbed.  Pair p matches older frame p % 16 against a copy of current frame p % 16 (every pair
has a current block of its own, as a call with claims requires); 10 % of the rows are flagged in skip0 and matched1.

Everything is timed in ONE process on one non-default stream, the variants of a comparison alternating repetition by
repetition, on the host clock around work that ends in a stream synchronisation; median and [p10, p90] over `--reps`
repetitions (at least 30); one JSON line per comparison.  Boxes differ by several per cent: only same-run comparisons
mean anything.  Before it is timed, the batched call's rows are compared with the loop's, byte for byte.
  (a) a loop of n_pairs B = 1 block calls (the parent's kernel, one launch per pair)
  (b) one batched call without claims
  (c) one batched call with claims (matched1_out restored outside the timed window)
  (d) a sweep over J = 6 older frames: six batched calls with claims, matched1 updated in place, one synchronisation --
      against the host chain it replaces: per step and pair a B = 1 call, the rows downloaded, the insertions resolved
      on the host (numpy), the pair's matched1 row uploaded.  The host chain runs `--host-reps` times where a repetition
      makes more than 4096 round trips.

    python tools/bench_motion_batch.py [--pairs 1,16,256,3072] [--reps 30]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 16       # distinct frames per side
J = 6        # older frames of a sweep


def band(x):
    x = np.asarray(x) * 1e3
    return {"median_ms": round(float(np.median(x)), 4), "p10_ms": round(float(np.percentile(x, 10)), 4),
            "p90_ms": round(float(np.percentile(x, 90)), 4)}


def rot_y(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def radtan(cam, x, y):
    k1, k2, p1, p2 = cam.d[:4]
    r = x * x + y * y
    rad = k1 * r + k2 * r * r
    return (x + x * rad + 2 * p1 * x * y + p2 * (r + 2 * x * x), y + y * rad + 2 * p2 * x * y + p1 * (r + 2 * y * y))


def make_frame(cam, T_WC, cloud, cloud_desc, K, rng):
    from okvis2_amd import capi
    pc = (cloud - T_WC[1]) @ T_WC[0].reshape(3, 3)
    front = np.flatnonzero(pc[:, 2] > 0.5)
    x, y = radtan(cam, pc[front, 0] / pc[front, 2], pc[front, 1] / pc[front, 2])
    u, v = cam.fu * x + cam.cu, cam.fv * y + cam.cv
    ok = (u > 2) & (u < cam.w - 2) & (v > 2) & (v < cam.h - 2) & (np.hypot(pc[front, 0], pc[front, 1]) / pc[front, 2] < 0.9)
    rows = rng.permutation(np.flatnonzero(ok))[:K]
    assert len(rows) == K, "the cloud is too thin for this pose"
    vis = front[rows]
    kps = np.zeros(K, dtype=capi.KEYPOINT_DTYPE)
    kps["size"] = 12.0
    kps["x"], kps["y"] = u[rows] + rng.normal(0, 0.3, K), v[rows] + rng.normal(0, 0.3, K)
    bp = (pc[vis] / pc[vis, 2:3]).astype(np.float64)
    flips = ((rng.random((K, 48)) < 0.03) * rng.integers(1, 256, (K, 48))).astype(np.uint8)
    return kps, cloud_desc[vis] ^ flips, bp


def resolve_host(rows, count0, taken):
    """the insertion loop's frame-data part on the host: per free k1 the smallest candidate k0; updates `taken`"""
    k1 = rows["k1"][:count0]
    cand = (k1 >= 0) & (rows["accepted"][:count0] != 0)
    cand &= taken[np.where(cand, k1, 0)] == 0
    k0s = np.flatnonzero(cand)
    if len(k0s):
        won, _ = np.unique(k1[k0s], return_index=True)
        taken[won] = 1
        return len(won)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", default="1,16,256,3072")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=5)
    args = ap.parse_args()
    if args.reps < 30:
        ap.error("--reps: at least 30")
    import torch
    from okvis2_amd import capi, multigpu, synth

    if not torch.cuda.is_available():
        sys.exit("no GPU: not measured")
    cfg = synth.euroc_config()
    cams, K = cfg.cams, cfg.max_kpts
    fe = capi.Frontend(cfg.w, cfg.h, cfg.uniformity_radius, 0, cfg.abs_threshold, K, match_threshold=cfg.match_threshold,
                       max_batch=1, num_cameras=2)
    for i, c in enumerate(cams):
        fe.set_camera(i, c)
    rng = np.random.default_rng(7)
    cloud = np.stack([rng.uniform(-9, 9, 4000), rng.uniform(-5, 5, 4000), rng.uniform(2, 12, 4000)], 1)
    cloud_desc = rng.integers(0, 256, (len(cloud), 48), dtype=np.uint8)
    T_SC = [np.zeros(3), np.array([0.11, 0.0, 0.0])]
    older, current, T_old, T_cur = [], [], [], []
    for i in range(D):
        for side, blocks, poses, x0 in ((0, older, T_old, -0.4), (1, current, T_cur, 0.3)):
            Cw = rot_y(0.02 * side + 0.004 * (i - D / 2))
            T = (Cw.reshape(-1).copy(), Cw @ T_SC[i % 2] + np.array([x0 + 0.03 * i, 0.01 * side, 0.02 * i * side]))
            kps, desc, bp = make_frame(cams[i % 2], T, cloud, cloud_desc, K, rng)
            blocks.append(multigpu.pack_block_host(K, kps, desc, bp, np.ones(K, np.uint8)))
            poses.append(T)
    stride = fe.gather_block_bytes()
    REC = capi.MOTION_MATCH_DTYPE.itemsize
    d_older = torch.from_numpy(np.stack(older)).cuda()
    stream = torch.cuda.Stream()
    sptr = stream.cuda_stream

    def alternate(fns, reps_of, warmup=2):
        """fns: {name: (prepare or None, run ending in a synchronisation)}; alternating; reps_of[name] repetitions"""
        out = {k: [] for k in fns}
        for r in range(-warmup, max(reps_of.values())):
            for k, (prep, run) in fns.items():
                if r >= reps_of[k]:
                    continue
                if prep:
                    prep()
                    stream.synchronize()
                t0 = time.perf_counter()
                run()
                dt = time.perf_counter() - t0
                if r >= 0:
                    out[k].append(dt)
        return out

    for n in [int(v) for v in args.pairs.split(",")]:
        cur = [p % D for p in range(n)]
        d_cur = torch.from_numpy(np.stack([current[c] for c in cur])).cuda()
        flags = np.random.default_rng(n)
        skip0 = (flags.random((J, n, K)) < 0.1).astype(np.uint8)
        m_init = (flags.random((n, K)) < 0.1).astype(np.uint8)
        d_skip0, d_m0 = torch.from_numpy(skip0).cuda(), torch.from_numpy(m_init).cuda()
        d_m = d_m0.clone()
        d_rows = torch.zeros((J, n, K, REC), dtype=torch.uint8, device="cuda")
        d_one = torch.zeros((n, K, REC), dtype=torch.uint8, device="cuda")
        d_claimed = torch.zeros((J, n, K), dtype=torch.uint8, device="cuda")
        d_n = torch.zeros((J, n), dtype=torch.int32, device="cuda")
        idx1 = np.arange(n, dtype=np.int32)
        cam_ids = np.array([c % 2 for c in cur], np.int32)
        T1 = [T_cur[c] for c in cur]
        step_idx0 = [np.array([(c + 2 * j) % D for c in cur], np.int32) for j in range(J)]
        step_T0 = [[T_old[i] for i in step_idx0[j]] for j in range(J)]
        torch.cuda.synchronize()

        def loop_b1(j=0, matched=None, out=None):
            matched, out = matched if matched is not None else d_m0, out if out is not None else d_one
            for p in range(n):
                fe.match_motion_stereo_blocks_device(
                    int(cam_ids[p]), d_older.data_ptr() + int(step_idx0[j][p]) * stride, d_cur.data_ptr() + p * stride,
                    d_skip0.data_ptr() + (j * n + p) * K, matched.data_ptr() + p * K, step_T0[j][p], T1[p],
                    out.data_ptr() + p * K * REC, sptr)

        def batched(j, matched, claim_out):
            claim = None
            if claim_out is not None:
                claim = dict(claimed=d_claimed[j].data_ptr(), n_claimed=d_n[j].data_ptr(), matched1_out=claim_out.data_ptr())
            fe.match_motion_stereo_blocks_batch_device(
                d_older.data_ptr(), D, d_cur.data_ptr(), n, step_idx0[j], idx1, cam_ids, step_T0[j], T1,
                d_skip0[j].data_ptr(), matched.data_ptr(), d_rows[j].data_ptr(), claim=claim, stream=sptr)

        # the same rows, byte for byte, before anything is timed
        loop_b1()
        batched(0, d_m0, None)
        stream.synchronize()
        assert torch.equal(d_one, d_rows[0]), "batched rows differ from the loop of B = 1 calls"
        hits = int((d_one.cpu().numpy().reshape(-1).view(capi.MOTION_MATCH_DTYPE)["k1"] >= 0).sum())

        def a_loop():
            loop_b1()
            stream.synchronize()

        def b_batch():
            batched(0, d_m0, None)
            stream.synchronize()

        def c_claims():
            batched(0, d_m, d_m)
            stream.synchronize()

        def restore():
            with torch.cuda.stream(stream):
                d_m.copy_(d_m0)

        t = alternate({"loop_b1": (None, a_loop), "batched": (None, b_batch), "batched_claims": (restore, c_claims)},
                      {"loop_b1": args.reps, "batched": args.reps, "batched_claims": args.reps})
        res = {k: band(v) for k, v in t.items()}
        res.update(comparison=f"one older frame, n_pairs={n}", reps=args.reps, matches_per_pair=round(hits / n, 1),
                   claims_per_pair=round(float(d_n[0].float().mean().item()), 1),
                   loop_over_batched=round(res["loop_b1"]["median_ms"] / res["batched"]["median_ms"], 2),
                   claims_plus_ms=round(res["batched_claims"]["median_ms"] - res["batched"]["median_ms"], 4))
        print(json.dumps(res), flush=True)

        # (d) the sweep
        def sweep_device():
            for j in range(J):
                batched(j, d_m, d_m)
            stream.synchronize()

        h_rows = np.zeros(K, dtype=capi.MOTION_MATCH_DTYPE)
        h_m = m_init.copy()
        host_claims = [0]

        def sweep_host():
            h_m[:] = m_init
            host_claims[0] = 0
            for j in range(J):
                for p in range(n):
                    fe.match_motion_stereo_blocks_device(
                        int(cam_ids[p]), d_older.data_ptr() + int(step_idx0[j][p]) * stride, d_cur.data_ptr() + p * stride,
                        d_skip0.data_ptr() + (j * n + p) * K, d_m.data_ptr() + p * K, step_T0[j][p], T1[p],
                        d_one.data_ptr() + p * K * REC, sptr)
                    fe_copy_to_host(h_rows, d_one.data_ptr() + p * K * REC)
                    host_claims[0] += resolve_host(h_rows, K, h_m[p])
                    fe_copy_to_device(d_m.data_ptr() + p * K, h_m[p])

        lib = capi.lib()

        def fe_copy_to_host(dst, src):
            st = lib.okvfe_copy_to_host(capi._p(dst), capi._p(src), capi.C.c_size_t(dst.nbytes), capi.C.c_void_p(sptr))
            st = st or lib.okvfe_stream_synchronize(capi.C.c_void_p(sptr))
            assert st == 0

        def fe_copy_to_device(dst, src):
            st = lib.okvfe_copy_to_device(capi._p(dst), capi._p(src), capi.C.c_size_t(src.nbytes), capi.C.c_void_p(sptr))
            st = st or lib.okvfe_stream_synchronize(capi.C.c_void_p(sptr))
            assert st == 0

        host_reps = args.reps if J * n <= 4096 else args.host_reps
        t = alternate({"sweep_device": (restore, sweep_device), "sweep_host_chain": (restore, sweep_host)},
                      {"sweep_device": args.reps, "sweep_host_chain": host_reps}, warmup=1)
        # the two sweeps hand out the same number of landmarks
        restore()
        sweep_device()
        dev_claims = int(d_n.sum().item())
        restore()
        stream.synchronize()
        sweep_host()
        stream.synchronize()
        res = {k: band(v) for k, v in t.items()}
        res.update(comparison=f"sweep over {J} older frames, n_pairs={n} per step", reps=args.reps, host_chain_reps=host_reps,
                   claims_device=dev_claims, claims_host=host_claims[0], same_claims=dev_claims == host_claims[0],
                   host_over_device=round(res["sweep_host_chain"]["median_ms"] / res["sweep_device"]["median_ms"], 2))
        print(json.dumps(res), flush=True)
        del d_cur, d_rows, d_one, d_claimed, d_n, d_skip0, d_m, d_m0
    fe.close()


if __name__ == "__main__":
    main()
