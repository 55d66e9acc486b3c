#!/usr/bin/env python3
"""What the consensus of runRansac2d2d costs on the device: okvfe_ransac2d2d_consensus_blocks_device.

Workload: pairs of multiframes of 2 EuRoC cameras with 700 keypoints each; about 300 keypoints per camera carry a
landmark id that both frames know (a translation of 0.25 m with parallax at 2 .. 8 m, 0.3 px of noise, 20 % of the
current ids swapped), 50 rotation-only and 50 relative-pose hypotheses per (pair, camera): the true model, 39
perturbed by up to 0.6 degrees, 10 random.  The back-projections are pinhole rays (a block's rays are data).  16
distinct pairs are repeated to fill a batch; landmark1_out is a buffer of its own, so every repetition sees the same
ids.

Everything is timed in ONE process, variants alternating repetition by repetition; median and [p10, p90] over `--reps`
repetitions (at least 30); one JSON line per comparison.  Boxes differ by several per cent: only same-run comparisons
mean anything.
  (a) the launch alone, between device events on the call's stream, at 1 / 256 / 3072 pairs; the achieved FP64 rate
      (180 FP64 operations per (hypothesis of both lists, correspondence): 51 of the rotation-only distance, 129 of
      the relative one) against the device's vector FP64 peak
  (b) the call plus one stream synchronisation, on the host clock
  (c) at `--host-pairs` pairs (default 1): what is possible without the call -- both frames' ids and gather blocks
      downloaded, the numpy restatement of tests/ransac2d2d_ref.py on the host, the current ids uploaded.  The host
      side is a PYTHON LOOP over hypotheses, not an optimised C++ one: the figure bounds the round trip from above
      and is flagged as such in the output.

    python tools/bench_ransac2d2d.py [--batches 1,256,3072] [--reps 30]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_map_table import band, timed  # noqa: E402

FLOP_PER_PAIR = 51 + 129
PEAK_FP64_TFLOPS = 78.6  # MI355X vector FP64 (AMD's data sheet)


def rodrigues(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1.0 - np.cos(angle)) * (Kx @ Kx)


def unit(t):
    return t / np.linalg.norm(t)


def make_camera_pair(cam, w, h, K, n_shared, R12, t12, rng):
    """(fr0, fr1): K keypoints each, n_shared of them on landmarks both frames carry"""
    from okvis2_amd import capi
    out = []
    px0 = np.stack([rng.uniform(5, w - 5, K), rng.uniform(5, h - 5, K)], 1)
    ray0 = np.stack([(px0[:, 0] - cam.cu) / cam.fu, (px0[:, 1] - cam.cv) / cam.fv, np.ones(K)], 1)
    P = ray0 / np.linalg.norm(ray0, axis=1, keepdims=True) * rng.uniform(2.0, 8.0, (K, 1))
    q = (P - t12) @ R12
    px1 = np.stack([cam.fu * q[:, 0] / q[:, 2] + cam.cu, cam.fv * q[:, 1] / q[:, 2] + cam.cv], 1) + rng.normal(0, 0.3, (K, 2))
    ids = rng.permutation(100000)[:K].astype(np.int32)
    lm0, lm1 = np.full(K, -1, np.int32), np.full(K, -1, np.int32)
    shared = rng.permutation(K)[:n_shared]
    lm0[shared] = ids[shared]
    lm1[shared] = ids[shared]
    swap = shared[rng.random(n_shared) < 0.2]
    lm1[swap] = ids[rng.permutation(swap)]
    order1 = rng.permutation(K)
    for px, lm in ((px0, lm0), (px1[order1], lm1[order1])):
        kps = np.zeros(K, dtype=capi.KEYPOINT_DTYPE)
        kps["x"], kps["y"], kps["size"] = px[:, 0], px[:, 1], 12.0
        bp = np.stack([(px[:, 0] - cam.cu) / cam.fu, (px[:, 1] - cam.cv) / cam.fv, np.ones(K)], 1)
        out.append(dict(kps=kps, desc=np.zeros((K, 48), np.uint8), bp=bp, bpv=np.ones(K, np.uint8), lm=lm))
    return out


def hypotheses(R12, t12, n, rng):
    rot, rel = [R12.reshape(9)], [np.concatenate([R12, unit(t12)[:, None]], 1).reshape(12)]
    for i in range(1, n):
        if i >= n - 10:
            Rm, t = rodrigues(rng.normal(size=3), rng.uniform(0, np.pi)), unit(rng.normal(size=3))
        else:
            s = rng.random()
            Rm, t = R12 @ rodrigues(rng.normal(size=3), np.deg2rad(0.6) * s), unit(unit(t12) + 0.1 * s * rng.normal(size=3))
        rot.append(Rm.reshape(9)), rel.append(np.concatenate([Rm, t[:, None]], 1).reshape(12))
    return np.array(rot), np.array(rel)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", default="1,256,3072")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--hypotheses", type=int, default=50)
    ap.add_argument("--shared", type=int, default=300)
    ap.add_argument("--host-pairs", type=int, default=1)
    args = ap.parse_args()
    if args.reps < 30:
        ap.error("--reps: at least 30")
    import torch
    import ransac2d2d_ref as R2
    from okvis2_amd import capi, multigpu, synth

    cfg = synth.euroc_config()
    cams, K, nh, D = cfg.cams, cfg.max_kpts, args.hypotheses, args.distinct
    fe = capi.Frontend(cfg.w, cfg.h, cfg.uniformity_radius, 0, cfg.abs_threshold, K, match_threshold=cfg.match_threshold,
                       max_batch=1, num_cameras=2)
    for i, c in enumerate(cams):
        fe.set_camera(i, c)
    rng = np.random.default_rng(5)
    pairs = []
    for m in range(D):
        R12 = rodrigues((1.0, 0.2, 0.01 * m), 0.02)
        t12 = np.array([0.25, 0.05 + 0.002 * m, -0.1])
        pair = []
        for c in range(2):
            fr0, fr1 = make_camera_pair(cams[c], cfg.w, cfg.h, K, args.shared, R12, t12, rng)
            rot, rel = hypotheses(R12, t12, nh, rng)
            pair.append(dict(fr0=fr0, fr1=fr1, rot_H=rot, rel_H=rel, rot_valid=None, rel_valid=None))
        pairs.append(pair)
    fus = [c.fu for c in cams]
    block = lambda f: multigpu.pack_block_host(K, f["kps"], f["desc"], f["bp"], f["bpv"])
    stream = torch.cuda.Stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def tensors(B):
        rep = [pairs[i % D] for i in range(B)]
        t = dict(b0=dev(np.stack([block(c["fr0"]) for p in rep for c in p])),
                 b1=dev(np.stack([block(c["fr1"]) for p in rep for c in p])),
                 lm0=dev(np.stack([c["fr0"]["lm"] for p in rep for c in p])),
                 lm1=dev(np.stack([c["fr1"]["lm"] for p in rep for c in p])),
                 rot=dev(np.stack([np.stack([c["rot_H"] for c in p]) for p in rep])),
                 rel=dev(np.stack([np.stack([c["rel_H"] for c in p]) for p in rep])),
                 out=torch.zeros((2 * B, K), dtype=torch.int32, device="cuda"),
                 cam=torch.zeros((5, B, 2), dtype=torch.int32, device="cuda"),
                 flags=torch.zeros((2, B, 2), dtype=torch.uint8, device="cuda"),
                 total=torch.zeros((B,), dtype=torch.int32, device="cuda"),
                 pair=torch.zeros((2, B), dtype=torch.uint8, device="cuda"))
        t["res"] = fe.make_ransac2d2d_result_device(*[t["cam"][i].data_ptr() for i in range(5)], t["flags"][0].data_ptr(),
                                                    t["flags"][1].data_ptr(), t["total"].data_ptr(), t["pair"][0].data_ptr(),
                                                    t["pair"][1].data_ptr(), landmark1_out_ptr=t["out"].data_ptr())
        t["mf"] = np.arange(B, dtype=np.int32)
        return t

    def call(t, B):
        fe.ransac2d2d_consensus_blocks_device(t["b0"].data_ptr(), B, t["b1"].data_ptr(), B, t["mf"], t["mf"], [0, 1],
                                              t["lm0"].data_ptr(), t["lm1"].data_ptr(), None, 0, t["rot"].data_ptr(), None,
                                              t["rel"].data_ptr(), None, nh, t["res"], stream=stream)

    def by_events(fn):
        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            stream.synchronize()
            return e0.elapsed_time(e1) * 1e-3
        return run

    def timed_events(fns, reps, warmup=3):
        for _ in range(warmup):
            for f in fns.values():
                f()
        out = {k: [] for k in fns}
        for _ in range(reps):
            for k, f in fns.items():
                out[k].append(f())
        return out

    for B in [int(b) for b in args.batches.split(",")]:
        t = tensors(B)
        torch.cuda.synchronize()

        def call_sync():
            call(t, B)
            stream.synchronize()

        ev = timed_events({"launch": by_events(lambda: call(t, B))}, args.reps)
        hc = timed({"call_and_sync": call_sync}, args.reps)
        n_corr = t["cam"][0].cpu().numpy().astype(np.int64)
        work = int(n_corr.sum()) * nh
        res = {"launch": band(ev["launch"]), "call_and_sync": band(hc["call_and_sync"])}
        tf = work * FLOP_PER_PAIR / (res["launch"]["median_ms"] * 1e-3) / 1e12
        res.update(comparison=f"okvfe_ransac2d2d_consensus_blocks_device, {B} pairs x 2 cameras", reps=args.reps,
                   correspondences_per_camera=round(float(n_corr.mean()), 1),
                   rot_inliers_per_camera=round(float(t["cam"][2].float().mean().item()), 1),
                   rel_inliers_per_camera=round(float(t["cam"][4].float().mean().item()), 1),
                   branches=np.bincount(t["flags"][0].cpu().numpy().reshape(-1), minlength=3).tolist(),
                   succeeded=int((t["total"] >= 0).sum().item()), fp64_tflops=round(tf, 3),
                   fp64_peak_share=round(tf / PEAK_FP64_TFLOPS, 4),
                   launch_us_per_pair=round(res["launch"]["median_ms"] * 1e3 / B, 3))
        print(json.dumps(res), flush=True)
        if B == args.host_pairs:
            def host_round_trip():
                b0, b1 = t["b0"].cpu().numpy(), t["b1"].cpu().numpy()
                l0, l1 = t["lm0"].cpu().numpy(), t["lm1"].cpu().numpy()
                out = np.empty_like(l1)
                for p in range(B):
                    cams_p = []
                    for c in range(2):
                        f0, f1 = (multigpu.unpack_block_host(b[2 * p + c], K) for b in (b0, b1))
                        src = pairs[p % D][c]
                        cams_p.append(dict(src, fr0=dict(kps=f0[0], bp=f0[2], bpv=f0[3], lm=l0[2 * p + c]),
                                           fr1=dict(kps=f1[0], bp=f1[2], bpv=f1[3], lm=l1[2 * p + c])))
                    ref = R2.run(True, cams_p, fus)
                    for c in range(2):
                        out[2 * p + c] = ref["cams"][c]["landmark1_out"]
                t["out"].copy_(torch.from_numpy(out), non_blocking=False)
                torch.cuda.synchronize()

            hh = timed({"device_call_and_sync": call_sync, "host_round_trip_python_loop": host_round_trip}, args.reps)
            res = {k: band(v) for k, v in hh.items()}
            res.update(comparison=f"{B} pair(s): the call + one synchronisation vs ids and blocks downloaded, the numpy "
                                  "restatement on the host, ids uploaded", reps=args.reps,
                       note="the host side is a Python loop over hypotheses: an upper bound of the round trip it stands for")
            print(json.dumps(res), flush=True)
        del t
    fe.close()


if __name__ == "__main__":
    main()
