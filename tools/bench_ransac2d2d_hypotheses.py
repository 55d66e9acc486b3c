#!/usr/bin/env python3
"""What the hypotheses of runRansac2d2d cost on the device: okvfe_ransac2d2d_hypotheses_blocks_device against what a
caller could do before it existed.

Workload: pairs of 2 EuRoC cameras, 700 keypoints a block, 300 correspondences per camera (a general motion with
parallax, a tenth of them wrong), 50 rotation-only and 50 relative-pose hypotheses per camera, 16 distinct pairs
repeated to fill a batch; pair p samples under the key p.

Everything is timed in ONE process, variants alternating repetition by repetition; median and [p10, p90] over `--reps`
repetitions (at least 30; the host path at most `--host-reps`); one JSON line per batch size B = 1 / 256 / 3072.
Boxes differ by several per cent: only same-run comparisons mean anything.
  launch          the launch alone, between device events on the call's stream
  call_sync       the call plus one stream synchronisation, on the host clock
  host_path       what is possible without the call: the landmark-id rows downloaded (one synchronisation), the
                  correspondences rebuilt with numpy, the samples drawn with the stated hash and every sample solved in
                  a host loop, the hypotheses and their flags uploaded (a second synchronisation).  The loop runs around
                  okvfe_twopt_rotation_hypothesis and okvfe_fivept_hypothesis, which arrive with the device call: before
                  it the library shipped no solver at all, so this is the path of a caller with solvers of the same
                  speed.  It is Python around two ctypes calls per hypothesis: a C++ caller's loop is faster by the
                  interpreter's share, which `host_solver_only` bounds from below (the ctypes calls alone on prepared
                  samples).

    python tools/bench_ransac2d2d_hypotheses.py [--batches 1,256,3072] [--reps 30] [--host-reps 3]
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

from bench_map_table import band  # noqa: E402

SEED = 0x0123456789ABCDEF


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", default="1,256,3072")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--hypotheses", type=int, default=50)
    ap.add_argument("--correspondences", type=int, default=300)
    args = ap.parse_args()
    if args.reps < 30:
        ap.error("--reps: at least 30")
    import torch
    import oracle_lib
    import ransac2d2d_hyp_ref as H2
    import ransac2d2d_ref as R2
    import ransac2d2d_scenes as S2
    from okvis2_amd import capi, multigpu, synth

    cfg = synth.euroc_config()
    cams, K, nh, D, n_corr = cfg.cams, cfg.max_kpts, args.hypotheses, args.distinct, args.correspondences
    fe = capi.Frontend(cfg.w, cfg.h, cfg.uniformity_radius, 0, cfg.abs_threshold, K, match_threshold=cfg.match_threshold,
                       max_batch=1, num_cameras=2)
    for i, c in enumerate(cams):
        fe.set_camera(i, c)
    rng = np.random.default_rng(5)
    frames = []   # per (distinct pair, camera): (fr0, fr1)
    for m in range(D):
        for c in range(2):
            nD = n_corr // 10
            fr0, fr1, _ = S2.hand_camera(oracle_lib, rng, 0, 0, n_corr - nD, nD, free0=K - n_corr, free1=K - n_corr)
            frames.append((fr0, fr1))
    pack = lambda fr: multigpu.pack_block_host(K, fr["kps"], fr["desc"], fr["bp"], fr["bpv"])
    b0, b1 = [pack(f[0]) for f in frames], [pack(f[1]) for f in frames]
    l0, l1 = [f[0]["lm"] for f in frames], [f[1]["lm"] for f in frames]
    stream = torch.cuda.Stream()
    fus = [c.fu for c in cams]

    def host_samples(lm0, lm1, B):
        """id rows [2 B, K] -> per (pair, camera): (corr, [(rotation positions, relative positions)] per hypothesis)"""
        out = []
        for p in range(B):
            for c in range(2):
                fr0, fr1 = frames[2 * (p % D) + c]
                corr = R2.correspondences(True, dict(fr0, lm=lm0[2 * p + c]), dict(fr1, lm=lm1[2 * p + c]), fus[c])
                n = len(corr["kA"])
                pos = [] if n < 10 else [(H2.sample(SEED, H2.fold_key(p, c, 0), h, n, 2), H2.sample(SEED, H2.fold_key(p, c, 1), h, n, 8))
                                         for h in range(nh)]
                out.append((corr, pos))
        return out

    for B in [int(b) for b in args.batches.split(",")]:
        rep = [2 * (i % D) + c for i in range(B) for c in range(2)]
        dev = lambda rows: torch.from_numpy(np.stack([rows[i] for i in rep])).cuda()
        t = dict(b0=dev(b0), b1=dev(b1), l0=dev(l0), l1=dev(l1))
        for name in ("", "2"):
            t["rot" + name] = torch.zeros((B, 2, nh, 9), dtype=torch.float64, device="cuda")
            t["rel" + name] = torch.zeros((B, 2, nh, 12), dtype=torch.float64, device="cuda")
            t["rotv" + name] = torch.zeros((B, 2, nh), dtype=torch.uint8, device="cuda")
            t["relv" + name] = torch.zeros((B, 2, nh), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        res = fe.make_ransac2d2d_hypotheses_device(t["rot"].data_ptr(), t["rotv"].data_ptr(), t["rel"].data_ptr(), t["relv"].data_ptr())
        mf = np.arange(B, dtype=np.int32)

        def call():
            fe.ransac2d2d_hypotheses_blocks_device(t["b0"].data_ptr(), B, t["b1"].data_ptr(), B, mf, mf, [0, 1], t["l0"].data_ptr(),
                                                   t["l1"].data_ptr(), None, 0, None, SEED, nh, res, stream)

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

        host = dict(rot=np.zeros((B, 2, nh, 9)), rel=np.zeros((B, 2, nh, 12)), rotv=np.zeros((B, 2, nh), np.uint8),
                    relv=np.zeros((B, 2, nh), np.uint8))
        solver_only = []

        def host_path():
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                lm0, lm1 = t["l0"].cpu().numpy(), t["l1"].cpu().numpy()          # rows down, one synchronisation
            samples = host_samples(lm0, lm1, B)
            t1 = time.perf_counter()
            for i, (corr, pos) in enumerate(samples):
                p, c = divmod(i, 2)
                for h, (p2, p8) in enumerate(pos):
                    host["rot"][p, c, h], host["rotv"][p, c, h] = capi.twopt_rotation_hypothesis(corr["b1"][p2], corr["b2"][p2])
                    host["rel"][p, c, h], host["relv"][p, c, h], _ = capi.fivept_hypothesis(
                        corr["b1"][p8], corr["b2"][p8], corr["s1"][p8[5:]], corr["s2"][p8[5:]])
            solver_only.append(time.perf_counter() - t1)
            with torch.cuda.stream(stream):
                for k, v in host.items():                                          # hypotheses up
                    t[k + "2"].copy_(torch.from_numpy(v), non_blocking=True)
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
        same = all(bool(torch.equal(t[k].view(torch.int64) if t[k].dtype == torch.float64 else t[k],
                                    t[k + "2"].view(torch.int64) if t[k].dtype == torch.float64 else t[k + "2"]))
                   for k in host)
        line.update(comparison=f"2d2d hypotheses, B={B}", reps=args.reps, host_reps=len(out["host_path"]), n_hyp=nh,
                    host_solver_only=band(solver_only), rel_valid_share=round(float(t["relv"].float().mean().item()), 3),
                    host_equals_device=same, launch_us_per_pair=round(line["launch"]["median_ms"] * 1e3 / B, 3))
        print(json.dumps(line), flush=True)
        del t
    fe.close()


if __name__ == "__main__":
    main()
