#!/usr/bin/env python3
"""What verifyRecognisedPlace costs on the device after its descriptor matching: okvfe_place_claims_blocks_device and
okvfe_place_consensus_blocks_device, against the chain an integrator had to build before they existed.

Workload: an old frame's landmark set of 1000 landmarks with 1.5 descriptors each, multiframes of 2 EuRoC cameras with
700 keypoints each, 50 hypotheses per multiframe (the true T_WS, 39 perturbed by up to 2 degrees / 5 cm, 10 random).  A
keypoint sits at the projection of a landmark with 0.5 px of noise and carries a noisy copy of that landmark's first
descriptor; 30 % of the descriptors are another landmark's.  16 distinct multiframes are repeated to fill a batch.

Every batch size is measured in ONE process of its own (a child of this one, under its own time limit), variants
alternating repetition by repetition; median and [p10, p90] over `--reps` repetitions (at least 30); one JSON line per
comparison.  Boxes differ by several per cent: only same-run comparisons mean anything.
  (a) the three launches alone (descriptor matching, claims, consensus), between device events on the call's stream
  (b) on the host clock, from the queued descriptor matching to the verdicts on the host:
      device    matching + claims + consensus on one stream, one synchronisation, the verdict bytes downloaded
      baseline  what the parent of this change offers: matching, k_min / dist_min downloaded, the `matches` map rebuilt
                in numpy (the last writer per keypoint), the rows uploaded, okvfe_ransac3d2d_consensus_blocks_device
                with a table that gives every landmark one observation, its counts downloaded, the verdict of
                Frontend.cpp:389 taken on the host.  (That kernel scores nothing below ten correspondences and the
                baseline cannot change it: its verdicts differ from the reference's between seven and nine.)

    python tools/bench_place_verify.py [--batches 1,256] [--reps 30]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_map_ransac import compose, hypotheses, make_frame  # noqa: E402
from bench_map_table import band, make_table, rot_y, timed  # noqa: E402

MIN_INLIERS = 10  # Frontend.cpp:823


def worker(B, args):
    import torch
    from okvis2_amd import capi, multigpu, synth

    cfg = synth.euroc_config()
    cams, K, L, nh, D = cfg.cams, args.keypoints, args.landmarks, args.hypotheses, args.distinct
    thr = cfg.match_threshold
    fe = capi.Frontend(cfg.w, cfg.h, cfg.uniformity_radius, 0, cfg.abs_threshold, K, match_threshold=thr, max_batch=1,
                       num_cameras=2)
    for i, c in enumerate(cams):
        fe.set_camera(i, c)
    rng = np.random.default_rng(5)
    tab = make_table(L)
    n_desc = 1 + (np.arange(L) % 2)  # 1.5 descriptors per landmark
    desc_begin = np.concatenate([[0], np.cumsum(n_desc)]).astype(np.int32)
    base = rng.integers(0, 256, (L, 48), dtype=np.uint8)
    owner = np.repeat(np.arange(L), n_desc)
    pool = base[owner] ^ ((rng.random((len(owner), 48)) < 0.04) * rng.integers(1, 256, (len(owner), 48))).astype(np.uint8)
    lset = dict(hp=tab["hp"], obs_begin=desc_begin, obs_desc=pool)  # (what make_frame reads of a table)
    T_SC = [(np.eye(3).reshape(-1), np.zeros(3)), (rot_y(0.01).reshape(-1).copy(), np.array([0.11, 0.0, 0.0]))]
    blocks, Hs = [], []
    for m in range(D):
        T_WS = ((rot_y(0.03) @ rot_y(0.003 * (m - D / 2))).reshape(-1).copy(), np.array([0.4 + 0.01 * m, 0.0, 0.3 + 0.002 * m]))
        for c in range(2):
            kps, desc, bp = make_frame(cams[c], cfg.w, cfg.h, compose(T_WS, T_SC[c]), lset, K, rng)
            blocks.append(multigpu.pack_block_host(K, kps, desc, bp, np.ones(K, np.uint8)))
        Hs.append(hypotheses(T_WS, nh, rng))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    zeros = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    nb = 2 * B
    t = dict(blocks=dev(np.stack([blocks[2 * (i % D) + c] for i in range(B) for c in range(2)])),
             H=dev(np.stack([Hs[i % D] for i in range(B)])), hp=dev(tab["hp"]), desc_begin=dev(desc_begin), pool=dev(pool),
             one_obs=dev(np.arange(L + 1, dtype=np.int32)), kmin=zeros((nb, L), torch.int32), dmin=zeros((nb, L), torch.int32),
             counts=zeros((3, B), torch.int32), gate=zeros((B,), torch.uint8), ml=zeros((nb, K), torch.int32),
             head=zeros((3, B), torch.int32), acc=zeros((B,), torch.uint8), verdict=zeros((B,), torch.uint8),
             rows=zeros((nb, K), torch.int32))
    md = fe.make_map_device(L, t["desc_begin"].data_ptr(), t["pool"].data_ptr())
    pset = fe.make_place_set_device(L, t["hp"].data_ptr())
    table = fe.make_landmark_table_device(L, L, 0, t["hp"].data_ptr(), 0, t["one_obs"].data_ptr(), 0, 0, 0, 0)
    claims_res = fe.make_place_claims_device(t["counts"][0].data_ptr(), t["counts"][1].data_ptr(), t["counts"][2].data_ptr(),
                                             t["gate"].data_ptr(), t["ml"].data_ptr())
    res = fe.make_ransac_result_device(t["head"][0].data_ptr(), t["head"][1].data_ptr(), t["head"][2].data_ptr(),
                                       t["acc"].data_ptr())
    stream = torch.cuda.Stream()
    pinned = dict(kmin=torch.zeros((nb, L), dtype=torch.int32).pin_memory(), dmin=torch.zeros((nb, L), dtype=torch.int32).pin_memory(),
                  rows=torch.zeros((nb, K), dtype=torch.int32).pin_memory(), head=torch.zeros((3, B), dtype=torch.int32).pin_memory(),
                  verdict=torch.zeros((B,), dtype=torch.uint8).pin_memory())
    counts = np.array([K] * nb)  # (every block is full)

    def match():
        fe.verify_place_blocks_device(t["blocks"].data_ptr(), nb, md, t["kmin"].data_ptr(), t["dmin"].data_ptr(), stream)

    def claims():
        fe.place_claims_blocks_device(pset, t["blocks"].data_ptr(), B, 2, t["kmin"].data_ptr(), t["dmin"].data_ptr(), MIN_INLIERS,
                                      claims_res, stream)

    def consensus():
        fe.place_consensus_blocks_device(pset, t["blocks"].data_ptr(), B, [0, 1], T_SC, t["ml"].data_ptr(), t["gate"].data_ptr(),
                                         t["H"].data_ptr(), None, nh, MIN_INLIERS, res, t["verdict"].data_ptr(), stream=stream)

    def device_chain():
        match(), claims(), consensus()
        with torch.cuda.stream(stream):
            pinned["verdict"].copy_(t["verdict"], non_blocking=True)
        stream.synchronize()
        return pinned["verdict"].numpy().copy()

    w = tab["hp"][:, 3]
    usable = ~(np.abs(w) < 1.0e-8)

    def baseline_chain():
        match()
        with torch.cuda.stream(stream):
            pinned["kmin"].copy_(t["kmin"], non_blocking=True)
            pinned["dmin"].copy_(t["dmin"], non_blocking=True)
        stream.synchronize()
        km, dm = pinned["kmin"].numpy(), pinned["dmin"].numpy()
        hit = (dm < thr) & (km >= 0) & (km < counts[:, None])
        rows = pinned["rows"].numpy()
        rows[:] = -1
        b, l = np.nonzero(hit)  # row-major: ascending landmark within a block, so the last writer is the largest row
        rows[b, km[b, l]] = l
        ctr = hit.reshape(B, 2, L).sum(axis=(1, 2))
        points = hit.reshape(B, 2, L).any(axis=1).sum(axis=1)
        claimed = rows.reshape(B, -1)
        n_corr = ((claimed >= 0) & usable[np.maximum(claimed, 0)]).sum(axis=1)
        with torch.cuda.stream(stream):
            t["rows"].copy_(pinned["rows"], non_blocking=True)
        fe.ransac3d2d_consensus_blocks_device(table, t["blocks"].data_ptr(), B, [0, 1], T_SC, t["rows"].data_ptr(),
                                              t["H"].data_ptr(), None, nh, res, remove_outliers=False, stream=stream)
        with torch.cuda.stream(stream):
            pinned["head"].copy_(t["head"], non_blocking=True)
        stream.synchronize()
        n_inl = pinned["head"].numpy()[2]
        with np.errstate(all="ignore"):
            verdict = np.where((ctr < MIN_INLIERS) | (points < 8), 0, np.where(n_corr < 7, 1, np.where(
                (n_inl < MIN_INLIERS) | (n_inl.astype(np.float64) / n_corr.astype(np.float64) < 0.7), 2, 3)))
        return verdict.astype(np.uint8)

    def by_events(fn):
        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            stream.synchronize()
            return e0.elapsed_time(e1) * 1e-3
        return run

    torch.cuda.synchronize()
    vd, vb = device_chain(), baseline_chain()
    device_chain()  # (the claims' rows again: the events below time the consensus on them)
    ev = {k: [] for k in ("match", "claims", "consensus")}
    fns = dict(match=by_events(match), claims=by_events(claims), consensus=by_events(consensus))
    for r in range(args.reps + 3):
        for k, f in fns.items():
            v = f()
            if r >= 3:
                ev[k].append(v)
    out = {k: band(v) for k, v in ev.items()}
    out.update(comparison=f"launch alone, B={B}", reps=args.reps, landmarks=L, pool_rows=int(desc_begin[-1]), keypoints=K,
               hypotheses=nh, matches_per_multiframe=round(float(t["counts"][0].float().mean().item()), 1),
               correspondences_per_multiframe=round(float(t["counts"][2].float().mean().item()), 1))
    print(json.dumps(out), flush=True)
    hc = timed({"device": device_chain, "baseline": baseline_chain}, args.reps)
    out = {k: band(v) for k, v in hc.items()}
    out.update(comparison=f"matching to verdicts on the host, B={B}", reps=args.reps,
               gain_ms=round(out["baseline"]["median_ms"] - out["device"]["median_ms"], 4),
               verdicts_device=np.bincount(vd, minlength=4).tolist(), verdicts_baseline=np.bincount(vb, minlength=4).tolist(),
               verdicts_equal=bool(np.array_equal(vd, vb)))
    print(json.dumps(out), flush=True)
    fe.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", default="1,256")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--landmarks", type=int, default=1000)
    ap.add_argument("--keypoints", type=int, default=700)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--hypotheses", type=int, default=50)
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds per batch size")
    ap.add_argument("--worker", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.reps < 30:
        ap.error("--reps: at least 30")
    if args.worker:
        return worker(args.worker, args)
    for B in [int(b) for b in args.batches.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", str(B), "--reps", str(args.reps), "--landmarks",
               str(args.landmarks), "--keypoints", str(args.keypoints), "--distinct", str(args.distinct), "--hypotheses",
               str(args.hypotheses)]
        try:
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:  # nothing more is started on the device after a step that failed
            print(json.dumps(dict(comparison=f"B={B}", error=f"the step ended with status {rc}")), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
