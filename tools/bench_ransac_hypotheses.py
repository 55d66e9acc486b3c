#!/usr/bin/env python3
"""What the pose hypotheses of the absolute-pose RANSAC cost on the device: okvfe_ransac3d2d_hypotheses_blocks_device
against what a caller could do before it existed.

Workload: that of tools/bench_map_ransac.py (5000 landmarks, multiframes of 2 EuRoC cameras with 700 keypoints each,
the landmark rows as the first pass wrote them, 30 % of the descriptors another landmark's), 50 hypotheses per
multiframe, 16 distinct multiframes repeated to fill a batch; multiframe m samples under the key m.

Everything is timed in ONE process, variants alternating repetition by repetition; median and [p10, p90] over `--reps`
repetitions (at least 30; the host path at most `--host-reps`); one JSON line per batch size B = 1 / 256 / 3072.
Boxes differ by several per cent: only same-run comparisons mean anything.
  launch          the launch alone, between device events on the call's stream
  call_sync       the call plus one stream synchronisation, on the host clock
  host_path       what was possible without the call: the landmark rows downloaded (one synchronisation), the
                  correspondences rebuilt with numpy, the samples drawn with the stated hash and every sample solved by
                  okvfe_p3p_hypothesis in a host loop, the hypotheses and their flags uploaded (a second
                  synchronisation).  The loop is Python around one ctypes call per hypothesis: a C++ caller's loop is
                  faster by the interpreter's share, which `host_solver_only` bounds from below (the ctypes calls alone
                  on prepared samples).

    python tools/bench_ransac_hypotheses.py [--batches 1,256,3072] [--reps 30] [--host-reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_map_ransac import compose, make_frame  # noqa: E402
from bench_map_table import band, make_table, rot_y  # noqa: E402

SEED = 0x0123456789ABCDEF
SQRT2 = np.array([0x3FF6A09E667F3BCD], dtype=np.uint64).view(np.float64)[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", default="1,256,3072")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--landmarks", type=int, default=5000)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--hypotheses", type=int, default=50)
    args = ap.parse_args()
    if args.reps < 30:
        ap.error("--reps: at least 30")
    import torch
    import ransac_hyp_ref as RH
    from okvis2_amd import capi, multigpu, synth

    cfg = synth.euroc_config()
    cams, K, L, nh, D = cfg.cams, cfg.max_kpts, args.landmarks, args.hypotheses, args.distinct
    fe = capi.Frontend(cfg.w, cfg.h, cfg.uniformity_radius, 0, cfg.abs_threshold, K, match_threshold=cfg.match_threshold,
                       max_batch=1, num_cameras=2)
    for i, c in enumerate(cams):
        fe.set_camera(i, c)
    tab = make_table(L)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in tab.items()}
    table_dev = fe.make_landmark_table_device(L, len(tab["obs_pose"]), len(tab["poses"]), *[dev[k].data_ptr() for k in (
        "hp", "quality", "obs_begin", "obs_pose", "obs_desc", "obs_bp", "poses")])
    fe.landmark_table_check_device(table_dev)
    T_SC = [(np.eye(3).reshape(-1), np.zeros(3)), (rot_y(0.01).reshape(-1).copy(), np.array([0.11, 0.0, 0.0]))]
    rng = np.random.default_rng(5)
    blocks, poses, frames = [], [], []
    for m in range(D):
        T_WS = ((rot_y(0.03) @ rot_y(0.003 * (m - D / 2))).reshape(-1).copy(), np.array([0.4 + 0.01 * m, 0.0, 0.3 + 0.002 * m]))
        for c in range(2):
            T_WC = compose(T_WS, T_SC[c])
            kps, desc, bp = make_frame(cams[c], cfg.w, cfg.h, T_WC, tab, K, rng)
            blocks.append(multigpu.pack_block_host(K, kps, desc, bp, np.ones(K, np.uint8)))
            poses.append(T_WC)
            frames.append((kps, bp))
    stream = torch.cuda.Stream()
    hp = np.asarray(tab["hp"], dtype=np.float64).reshape(-1, 4)
    n_obs = np.diff(np.asarray(tab["obs_begin"]))
    fus = [c.fu for c in cams]

    def host_samples(lm, B):
        """rows [2 B, K] -> per (multiframe, hypothesis) with four samples: (P [4, 3], f [4, 3], sigma, camera)"""
        out = []
        for m in range(B):
            cam_of, P, f, sg = [], [], [], []
            for c in range(2):
                rows = lm[2 * m + c]
                kps, bp = frames[2 * (m % D) + c]
                ok = (rows >= 0) & (rows < L)
                ok[ok] &= (n_obs[rows[ok]] >= 1) & ~(np.abs(hp[rows[ok], 3]) < 1.0e-8)
                k = np.flatnonzero(ok)
                h4 = hp[rows[k]]
                s = (0.8 * kps["size"][k].astype(np.float64)) / 12.0
                v = bp[k]
                P.append(h4[:, :3] / h4[:, 3:4])
                f.append(v / np.sqrt(v[:, 0] * v[:, 0] + (v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]))[:, None])   # (Eigen's order, the default)
                sg.append(((SQRT2 * s) * s) / (fus[c] * fus[c]))
                cam_of.append(np.full(len(k), c))
            cam_of, P, f, sg = np.concatenate(cam_of), np.concatenate(P), np.concatenate(f), np.concatenate(sg)
            for h in range(nh):
                pos = RH.sample(SEED, m, h, cam_of)
                out.append(None if pos[3] < 0 else (P[pos], f[pos], sg[pos[3]], int(cam_of[pos[0]])))
        return out

    for B in [int(b) for b in args.batches.split(",")]:
        rep = [2 * (i % D) + c for i in range(B) for c in range(2)]
        t = dict(blocks=torch.from_numpy(np.stack([blocks[i] for i in rep])).cuda(),
                 lm=torch.zeros((2 * B, K), dtype=torch.int32, device="cuda"),
                 bd=torch.zeros((2 * B, K), dtype=torch.int32, device="cuda"),
                 H=torch.zeros((B, nh, 12), dtype=torch.float64, device="cuda"),
                 valid=torch.zeros((B, nh), dtype=torch.uint8, device="cuda"),
                 H2=torch.zeros((B, nh, 12), dtype=torch.float64, device="cuda"),
                 valid2=torch.zeros((B, nh), dtype=torch.uint8, device="cuda"))
        ids = [i % 2 for i in range(2 * B)]
        torch.cuda.synchronize()
        fe.match_to_map_table_blocks_device(table_dev, t["blocks"].data_ptr(), 2 * B, ids, [poses[i] for i in rep], 20.0, False,
                                            None, None, t["lm"].data_ptr(), t["bd"].data_ptr(), stream)
        stream.synchronize()
        res = fe.make_ransac_hypotheses_device(t["H"].data_ptr(), t["valid"].data_ptr())

        def call():
            fe.ransac3d2d_hypotheses_blocks_device(table_dev, t["blocks"].data_ptr(), B, [0, 1], T_SC, t["lm"].data_ptr(), None,
                                                   SEED, nh, res, stream)

        def launch():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            stream.synchronize()
            return e0.elapsed_time(e1) * 1e-3

        def call_sync():
            t0 = time.perf_counter()
            call()
            stream.synchronize()
            return time.perf_counter() - t0

        host_H, host_valid = np.zeros((B, nh, 12)), np.zeros((B, nh), np.uint8)
        solver_only = []

        def host_path():
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                lm = t["lm"].cpu().numpy()                      # rows down, one synchronisation
            samples = host_samples(lm, B)
            t1 = time.perf_counter()
            for i, smp in enumerate(samples):
                if smp is None:
                    host_H[i // nh, i % nh], host_valid[i // nh, i % nh] = 0.0, 0
                else:
                    host_H[i // nh, i % nh], host_valid[i // nh, i % nh], _ = capi.p3p_hypothesis(smp[0], smp[1], smp[2], T_SC[smp[3]])
            solver_only.append(time.perf_counter() - t1)
            with torch.cuda.stream(stream):
                t["H2"].copy_(torch.from_numpy(host_H), non_blocking=True)       # hypotheses up
                t["valid2"].copy_(torch.from_numpy(host_valid), non_blocking=True)
            stream.synchronize()
            return time.perf_counter() - t0

        for _ in range(3):
            launch(), call_sync()
        out = dict(launch=[], call_sync=[], host_path=[])
        host_every = max(1, args.reps // max(1, args.host_reps))
        for r in range(args.reps):
            out["launch"].append(launch())
            out["call_sync"].append(call_sync())
            if r % host_every == 0 and len(out["host_path"]) < args.host_reps:
                out["host_path"].append(host_path())
        line = {k: band(v) for k, v in out.items()}
        same = bool(torch.equal(t["H"].view(torch.int64), t["H2"].view(torch.int64)) and torch.equal(t["valid"], t["valid2"]))
        line.update(comparison=f"hypotheses, B={B}", reps=args.reps, host_reps=len(out["host_path"]), n_hyp=nh,
                    host_solver_only=band(solver_only), valid_share=round(float(t["valid"].float().mean().item()), 3),
                    host_equals_device=same,
                    launch_us_per_multiframe=round(line["launch"]["median_ms"] * 1e3 / B, 3))
        print(json.dumps(line), flush=True)
        del t
    fe.close()


if __name__ == "__main__":
    main()
