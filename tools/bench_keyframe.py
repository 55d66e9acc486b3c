#!/usr/bin/env python3
"""What the keyframe coverage call costs next to the launch it follows in the reference's per-frame order.

The yardstick is one okvfe_match_to_map_blocks_device launch over B gather blocks, set up as bench.py's map workload
(EuRoC context, 700 keypoints per frame, 5000 pooled landmarks with 1..3 descriptors, reprojection radius 20 px).
Timed in ONE process, alternating the two variants round by round:

  A   the matcher launch alone                                   (what a caller does today)
  B   the matcher launch + one okvfe_keyframe_coverage_blocks_device call on the same stream, with an id set

Per round `--steps` steps are queued and the stream is synchronised once (host clock); the medians over the rounds,
their difference, and the coverage launch's own time between two device events (no set / with a set) are printed,
then the B = 1 host seam okvfe_keyframe_coverage on its own (synchronous, host clock).  Boxes differ by several per
cent, so only the same-run difference B - A means anything.  One JSON line per batch size at the end of each block.

    python tools/bench_keyframe.py [--batches 256,3072] [--steps 20] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workload(torch, capi, synth, multigpu, B, distinct, seed=7):
    """bench.py run_map_workload's data, plus landmark ids: keypoint i of a frame carries landmark obs[i] + 1 with
    probability 0.4 (the frame's 'matched' keypoints), 0 otherwise."""
    cfg = synth.euroc_config()
    K, L = cfg.max_kpts, 5000
    fe = capi.Frontend(cfg.w, cfg.h, cfg.uniformity_radius, 0, cfg.abs_threshold, K,
                       match_threshold=cfg.match_threshold, max_batch=1, num_cameras=1)
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, 4, L)
    begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    pool = rng.integers(0, 256, (begin[-1], 48), dtype=np.uint8)
    lm_xy = np.stack([rng.uniform(-200, 952, L), rng.uniform(-150, 630, L)], 1)
    blocks, proj, ids = [], [], []
    for _ in range(min(distinct, B)):
        kps = np.zeros(K, dtype=capi.KEYPOINT_DTYPE)
        kps["x"] = rng.uniform(30, cfg.w - 30, K)
        kps["y"] = rng.uniform(30, cfg.h - 30, K)
        desc = rng.integers(0, 256, (K, 48), dtype=np.uint8)
        p = lm_xy + rng.normal(0, 2.0, (L, 2))
        vis = np.flatnonzero((p[:, 0] > 0) & (p[:, 0] < cfg.w) & (p[:, 1] > 0) & (p[:, 1] < cfg.h))
        obs = rng.permutation(vis)[:K]
        kps["x"][:len(obs)] = p[obs, 0] + rng.normal(0, 1.5, len(obs))
        kps["y"][:len(obs)] = p[obs, 1] + rng.normal(0, 1.5, len(obs))
        for i, l in enumerate(obs[::2]):
            desc[2 * i] = pool[begin[l]] ^ ((rng.random(48) < 0.04) * rng.integers(0, 256, 48)).astype(np.uint8)
        fid = np.zeros(K, dtype=np.uint64)
        fid[:len(obs)] = np.where(rng.random(len(obs)) < 0.4, obs + 1, 0)
        blocks.append(multigpu.pack_block_host(K, kps, desc, np.zeros((K, 3)), np.ones(K, np.uint8)))
        proj.append(p)
        ids.append(fid)
    rep = [i % len(blocks) for i in range(B)]
    d = {"blocks": torch.from_numpy(np.stack([blocks[i] for i in rep])).cuda(),
         "proj": torch.from_numpy(np.stack([proj[i] for i in rep])).cuda(),
         "ids": torch.from_numpy(np.stack([ids[i] for i in rep]).view(np.int64)).cuda(),
         "begin": torch.from_numpy(begin).cuda(), "pool": torch.from_numpy(pool).cuda(),
         "lm": torch.empty((B, K), dtype=torch.int32, device="cuda"),
         "bd": torch.empty((B, K), dtype=torch.int32, device="cuda"),
         "cov": torch.zeros((B, 6), dtype=torch.int32, device="cuda")}
    d["map"] = fe.make_map_device(L, d["begin"].data_ptr(), d["pool"].data_ptr(), d["proj"].data_ptr())
    host = (multigpu.unpack_block_host(blocks[0], K)[0], ids[0])
    return fe, cfg, K, d, host


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", default="256,3072")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--map-radius", type=float, default=20.0)
    args = ap.parse_args()
    import torch
    from okvis2_amd import capi, multigpu, synth
    if not torch.cuda.is_available():
        sys.exit("bench_keyframe.py needs the GPU: no timing is taken without one")
    for B in [int(b) for b in args.batches.split(",")]:
        fe, cfg, K, d, host = workload(torch, capi, synth, multigpu, B, args.distinct)
        st = torch.cuda.Stream()
        torch.cuda.synchronize()

        def matcher():
            fe.match_to_map_blocks_device(d["blocks"].data_ptr(), B, None, d["map"], args.map_radius,
                                          d["lm"].data_ptr(), d["bd"].data_ptr(), st)

        def coverage(with_set=True):  # the set: frame 0's own id rows, zeros included
            fe.keyframe_coverage_blocks_device(d["blocks"].data_ptr(), B, d["ids"].data_ptr(), d["cov"].data_ptr(),
                                               d["ids"].data_ptr() if with_set else None, K if with_set else 0,
                                               stream=st)

        def variant_a():
            matcher()

        def variant_b():
            matcher()
            coverage()

        def timed(fn):
            st.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            st.synchronize()
            return (time.perf_counter() - t0) * 1e3 / args.steps

        for _ in range(args.warmup):
            variant_b()
            coverage(False)
        ta, tb = [], []
        for _ in range(args.rounds):  # A B A B ...: both variants see the same box at the same time
            ta.append(timed(variant_a))
            tb.append(timed(variant_b))
        own = {}
        for with_set in (False, True):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st.synchronize()
            e0.record(st)
            for _ in range(args.steps):
                coverage(with_set)
            e1.record(st)
            st.synchronize()
            own[with_set] = e0.elapsed_time(e1) / args.steps
        a, b = statistics.median(ta), statistics.median(tb)
        cov = d["cov"].cpu().numpy()
        print(f"B = {B}: {K} keypoints per frame, mask {cfg.h // 10} x {cfg.w // 10}, {args.rounds} rounds of "
              f"{args.steps} steps, interleaved")
        print(f"  A  match_to_map_blocks_device alone      {a:9.4f} ms per step  (min {min(ta):.4f}, max {max(ta):.4f})")
        print(f"  B  ... + keyframe_coverage_blocks_device  {b:9.4f} ms per step  (min {min(tb):.4f}, max {max(tb):.4f})")
        print(f"  B - A                                     {b - a:9.4f} ms  ({100.0 * (b - a) / a:+.2f} % of A)")
        print(f"  coverage launch alone, device events      {own[False]:9.4f} ms without a set, {own[True]:.4f} ms with "
              f"a set of {K} ids")
        print(f"  per frame with a set: {1e3 * own[True] / B:.3f} us; matched / keypoints of frame 0: "
              f"{cov[0][1]} / {cov[0][0]}, intersection / union {cov[0][4]} / {cov[0][5]}")
        print(json.dumps({"batch": B, "step_ms": a, "step_plus_coverage_ms": b, "difference_ms": b - a,
                          "coverage_event_ms": own[True], "coverage_event_no_set_ms": own[False],
                          "rounds": args.rounds, "steps": args.steps}))
        if B == int(args.batches.split(",")[0]):  # the B = 1 host seam, once
            kps, fid = host
            for _ in range(5):
                fe.keyframe_coverage(kps, fid, fid)
            n = 200
            t0 = time.perf_counter()
            for _ in range(n):
                fe.keyframe_coverage(kps, fid, fid)
            seam = (time.perf_counter() - t0) * 1e3 / n
            print(f"  B = 1 host seam okvfe_keyframe_coverage ({K} keypoints, set of {K}): {seam:.4f} ms per call "
                  "(upload, launch, download, synchronise)")
            print(json.dumps({"batch": 1, "host_seam_ms": seam}))
        del fe, d
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
