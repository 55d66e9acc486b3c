#!/usr/bin/env python3
"""What the overlaps in front of the motion-stereo sweep cost: one okvfe_overlap_pairs_blocks_device launch against the
loop of coverage calls a caller had to queue before it existed.

Per size (EuRoC: 2 cameras, Hilti: 5 cameras; 700 keypoints per image, 40 % of them with a landmark from a pool the
multiframes share) and pair count (1, 20, 5120 = 20 candidate keyframes for 1, 1 and 256 current multiframes), in ONE
process, alternating the two variants round by round:

  A   per pair two okvfe_keyframe_coverage_blocks_device calls (side A with B's id rows as the set, side B with A's),
      one stream synchronisation, one download of the per-image records, the sums and the overlap in numpy
  B   one okvfe_overlap_pairs_blocks_device call, one stream synchronisation, one download of the counts,
      okvfe_overlap_fraction, and okvfe_motion_frame_order per current multiframe

okvfe_keyframe_coverage_blocks_device is the same entry point as before the overlap call was added, so A stands for
what a caller could do then.  Every image holds K keypoints, so A needs no zero-padding of the id rows.  Host clock
around queue + synchronise + download + host arithmetic; median [p10, p90] over the rounds.  One JSON line per case.

    python tools/bench_overlap.py [--configs euroc,hilti] [--pairs 1,20,5120] [--rounds 15]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CANDIDATES = 20


def scene(torch, capi, multigpu, cfg, n_current, seed=11):
    K, C = cfg.max_kpts, len(cfg.cams)
    M = CANDIDATES + n_current
    rng = np.random.default_rng(seed)
    blocks, ids = [], np.zeros((M * C, K), dtype=np.uint64)
    for b in range(M * C):
        kps = np.zeros(K, dtype=capi.KEYPOINT_DTYPE)
        kps["x"], kps["y"] = rng.uniform(0, cfg.w - 0.5, K), rng.uniform(0, cfg.h - 0.5, K)
        blocks.append(multigpu.pack_block_host(K, kps, np.zeros((K, 48), np.uint8), np.zeros((K, 3)), np.zeros(K, np.uint8)))
        ids[b] = np.where(rng.random(K) < 0.4, rng.integers(1, 4 * C * K, K), 0)
    return torch.from_numpy(np.stack(blocks)).cuda(), torch.from_numpy(ids.view(np.int64)).cuda(), M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="euroc,hilti")
    ap.add_argument("--pairs", default="1,20,5120")
    ap.add_argument("--rounds", type=int, default=15)
    args = ap.parse_args()
    import torch
    from okvis2_amd import capi, multigpu, synth
    makers = {"euroc": synth.euroc_config, "hilti": synth.hilti_config}
    kptrad = 0.09 * 38.0 / 36.0
    for name in args.configs.split(","):
        cfg = makers[name]()
        K, C = cfg.max_kpts, len(cfg.cams)
        fe = capi.Frontend(cfg.w, cfg.h, cfg.uniformity_radius, 0, cfg.abs_threshold, K,
                           match_threshold=cfg.match_threshold, max_batch=1, num_cameras=C)
        for n_pairs in (int(v) for v in args.pairs.split(",")):
            n_current = max(1, n_pairs // CANDIDATES)
            d_blocks, d_ids, M = scene(torch, capi, multigpu, cfg, n_current)
            pair_a = np.array([CANDIDATES + (i // CANDIDATES) % n_current for i in range(n_pairs)], dtype=np.int32)
            pair_b = np.array([i % CANDIDATES for i in range(n_pairs)], dtype=np.int32)
            frame_ids = np.arange(100, 100 + CANDIDATES, dtype=np.uint64)
            st = torch.cuda.Stream()
            d_cov = torch.zeros((n_pairs, 2, C, 6), dtype=torch.int32, device="cuda")
            d_counts = torch.zeros((n_pairs, 8), dtype=torch.int32, device="cuda")
            bb = d_blocks.shape[1]
            bp, ip, cp = d_blocks.data_ptr(), d_ids.data_ptr(), d_cov.data_ptr()

            def variant_a():
                for i in range(n_pairs):
                    a, b = int(pair_a[i]), int(pair_b[i])
                    for f, (own, other) in enumerate(((a, b), (b, a))):
                        fe.keyframe_coverage_blocks_device(bp + own * C * bb, C, ip + own * C * K * 8,
                                                           cp + (i * 2 + f) * C * 24, ip + other * C * K * 8, C * K,
                                                           kptrad, st)
                st.synchronize()
                rec = d_cov.cpu().numpy().reshape(-1, 6).view(capi.COVERAGE_DTYPE).reshape(n_pairs, 2, C)
                inter = rec["intersection_area"].sum(axis=2).astype(np.float64)
                union = rec["union_area"].sum(axis=2).astype(np.float64)
                with np.errstate(divide="ignore", invalid="ignore"):
                    o = inter / union
                ov = np.where(o[:, 1] < o[:, 0], o[:, 1], o[:, 0])
                return np.where(rec["n_matched"].sum(axis=2)[:, 0] == 0, 0.0, ov)

            def variant_b():
                fe.overlap_pairs_blocks_device(bp, C, 1, M, C, ip, pair_a, pair_b, d_counts.data_ptr(), None, kptrad, st)
                st.synchronize()
                counts = d_counts.cpu().numpy().view(capi.OVERLAP_COUNTS_DTYPE).reshape(-1)
                ov = capi.overlap_fraction(counts)
                for c0 in range(0, n_pairs - CANDIDATES + 1, CANDIDATES):
                    capi.motion_frame_order(ov[c0:c0 + CANDIDATES], frame_ids)
                return ov

            oa, ob = variant_a(), variant_b()  # warm-up, and the two must agree
            assert np.array_equal(oa.view(np.uint64), ob.view(np.uint64)), "variants disagree"
            ta, tb = [], []
            for _ in range(args.rounds):
                for fn, acc in ((variant_a, ta), (variant_b, tb)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    acc.append((time.perf_counter() - t0) * 1e3)
            qa, qb = (np.percentile(t, (50, 10, 90)) for t in (ta, tb))
            print(f"{name}: {C} cameras x {K} keypoints, {n_pairs} pairs, {args.rounds} rounds, interleaved")
            print(f"  A  {2 * n_pairs} coverage launches + sync + numpy     {qa[0]:9.4f} ms  [{qa[1]:.4f}, {qa[2]:.4f}]")
            print(f"  B  1 overlap launch + sync + host functions   {qb[0]:9.4f} ms  [{qb[1]:.4f}, {qb[2]:.4f}]")
            print(f"  A / B                                         {qa[0] / qb[0]:9.2f}")
            print(json.dumps({"config": name, "n_cams": C, "keypoints": K, "n_pairs": n_pairs, "rounds": args.rounds,
                              "loop_ms": [float(v) for v in qa], "single_ms": [float(v) for v in qb],
                              "mean_overlap": float(np.mean(ob))}))


if __name__ == "__main__":
    main()
