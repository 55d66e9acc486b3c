#!/usr/bin/env python3
"""What the Hessian H of verifyRecognisedPlace costs on the device: okvfe_place_hessian_blocks_device behind the consensus,
against what an integrator had to do before the call existed.

Workload: that of tools/bench_place_verify.py -- a landmark set of 1000 landmarks, multiframes of 2 EuRoC cameras with
700 keypoints each, 50 hypotheses per multiframe; 16 distinct multiframes are repeated to fill a batch.  The matching,
the claims and the consensus (with its state rows) run once; the pose of a multiframe is its true T_WS turned by up to
0.01 rad and moved by 2 cm, as a solver would leave it.

Every batch size is measured in ONE process of its own (a child of this one, under its own time limit), variants
alternating repetition by repetition; median and [p10, p90] over `--reps` repetitions (at least 30); one JSON line per
comparison.  Boxes differ by several per cent: only same-run comparisons mean anything.
  (a) the launch alone, between device events on the call's stream (H and the counts only, and with both optional outputs)
  (b) on the host clock:
      device    the call, one synchronisation, H downloaded (288 bytes per multiframe)
      baseline  what the parent of this change offers: the consensus states, the claim rows and the gather blocks
                downloaded (timed at the full batch), then the terms rebuilt and evaluated on the host.  The host
                evaluation is the numpy restatement of the tests (tests/place_hessian_ref.py), timed on the distinct
                multiframes and scaled to the batch: an UPPER BOUND for a compiled host loop, not a measurement of one.

    python tools/bench_place_hessian.py [--batches 1,256,3072] [--reps 30]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_map_ransac import compose, hypotheses, make_frame  # noqa: E402
from bench_map_table import band, make_table, rot_y, timed  # noqa: E402

MIN_INLIERS = 10  # Frontend.cpp:823


def worker(B, args):
    import torch
    import oracle_lib
    import place_hessian_ref as PH
    import place_hessian_scenes as HS
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
    n_desc = 1 + (np.arange(L) % 2)
    desc_begin = np.concatenate([[0], np.cumsum(n_desc)]).astype(np.int32)
    base = rng.integers(0, 256, (L, 48), dtype=np.uint8)
    owner = np.repeat(np.arange(L), n_desc)
    pool = base[owner] ^ ((rng.random((len(owner), 48)) < 0.04) * rng.integers(1, 256, (len(owner), 48))).astype(np.uint8)
    lset = dict(hp=tab["hp"], obs_begin=desc_begin, obs_desc=pool)
    T_SC = [(np.eye(3).reshape(-1), np.zeros(3)), (rot_y(0.01).reshape(-1).copy(), np.array([0.11, 0.0, 0.0]))]
    prm = np.array([HS.pose7(T) for T in T_SC])
    blocks, Hs, poses = [], [], []
    for m in range(D):
        T_WS = ((rot_y(0.03) @ rot_y(0.003 * (m - D / 2))).reshape(-1).copy(), np.array([0.4 + 0.01 * m, 0.0, 0.3 + 0.002 * m]))
        for c in range(2):
            kps, desc, bp = make_frame(cams[c], cfg.w, cfg.h, compose(T_WS, T_SC[c]), lset, K, rng)
            blocks.append(multigpu.pack_block_host(K, kps, desc, bp, np.ones(K, np.uint8)))
        Hs.append(hypotheses(T_WS, nh, rng))
        poses.append(HS.refined(T_WS, rng))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    zeros = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    nb = 2 * B
    t = dict(blocks=dev(np.stack([blocks[2 * (i % D) + c] for i in range(B) for c in range(2)])),
             H=dev(np.stack([Hs[i % D] for i in range(B)])), hp=dev(tab["hp"]), desc_begin=dev(desc_begin), pool=dev(pool),
             poses=dev(np.stack([poses[i % D] for i in range(B)])), kmin=zeros((nb, L), torch.int32),
             dmin=zeros((nb, L), torch.int32), counts=zeros((3, B), torch.int32), gate=zeros((B,), torch.uint8),
             ml=zeros((nb, K), torch.int32), head=zeros((3, B), torch.int32), acc=zeros((B,), torch.uint8),
             verdict=zeros((B,), torch.uint8), state=zeros((nb, K), torch.uint8), Hm=zeros((B, 36), torch.float64),
             terms=zeros((2, B), torch.int32), residual=zeros((nb, K, 2), torch.float64),
             jacobian=zeros((nb, K, 12), torch.float64))
    md = fe.make_map_device(L, t["desc_begin"].data_ptr(), t["pool"].data_ptr())
    pset = fe.make_place_set_device(L, t["hp"].data_ptr())
    claims_res = fe.make_place_claims_device(t["counts"][0].data_ptr(), t["counts"][1].data_ptr(), t["counts"][2].data_ptr(),
                                             t["gate"].data_ptr(), t["ml"].data_ptr())
    res = fe.make_ransac_result_device(t["head"][0].data_ptr(), t["head"][1].data_ptr(), t["head"][2].data_ptr(),
                                       t["acc"].data_ptr(), state_ptr=t["state"].data_ptr())
    lean = fe.make_place_hessian_device(t["Hm"].data_ptr(), t["terms"][0].data_ptr(), t["terms"][1].data_ptr())
    rows = fe.make_place_hessian_device(t["Hm"].data_ptr(), t["terms"][0].data_ptr(), t["terms"][1].data_ptr(),
                                        t["residual"].data_ptr(), t["jacobian"].data_ptr())
    stream = torch.cuda.Stream()
    pinned = dict(Hm=torch.zeros((B, 36), dtype=torch.float64).pin_memory(),
                  state=torch.zeros((nb, K), dtype=torch.uint8).pin_memory(),
                  ml=torch.zeros((nb, K), dtype=torch.int32).pin_memory(),
                  blocks=torch.zeros(tuple(t["blocks"].shape), dtype=torch.uint8).pin_memory())
    # the chain up to the consensus, once: the rows the Hessian call reads
    fe.verify_place_blocks_device(t["blocks"].data_ptr(), nb, md, t["kmin"].data_ptr(), t["dmin"].data_ptr(), stream)
    fe.place_claims_blocks_device(pset, t["blocks"].data_ptr(), B, 2, t["kmin"].data_ptr(), t["dmin"].data_ptr(), MIN_INLIERS,
                                  claims_res, stream)
    fe.place_consensus_blocks_device(pset, t["blocks"].data_ptr(), B, [0, 1], T_SC, t["ml"].data_ptr(), t["gate"].data_ptr(),
                                     t["H"].data_ptr(), None, nh, MIN_INLIERS, res, t["verdict"].data_ptr(), stream=stream)
    stream.synchronize()

    def hessian(result):
        fe.place_hessian_blocks_device(pset, t["blocks"].data_ptr(), B, [0, 1], prm, t["poses"].data_ptr(), t["ml"].data_ptr(),
                                       t["state"].data_ptr(), t["verdict"].data_ptr(), result, stream)

    def device_chain():
        hessian(lean)
        with torch.cuda.stream(stream):
            pinned["Hm"].copy_(t["Hm"], non_blocking=True)
        stream.synchronize()
        return pinned["Hm"].numpy().copy()

    def downloads():
        with torch.cuda.stream(stream):
            for k in ("state", "ml", "blocks"):
                pinned[k].copy_(t[k], non_blocking=True)
        stream.synchronize()

    def host_terms():
        """the distinct multiframes through the numpy restatement (after `downloads`)"""
        st, ml, bl = pinned["state"].numpy(), pinned["ml"].numpy(), pinned["blocks"].numpy()
        verdict = t["verdict"].cpu().numpy()
        out = []
        for m in range(min(B, D)):
            frames = [dict(kps=multigpu.unpack_block_host(bl[2 * m + c], K)[0]) for c in range(2)]
            out.append(PH.evaluate(oracle_lib, True, tab["hp"], frames, [ml[2 * m], ml[2 * m + 1]], [st[2 * m], st[2 * m + 1]],
                                   cams, prm, poses[m % D], verdict[m] == 3))
        return out

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
    Hd = device_chain()
    downloads()
    t0 = time.perf_counter()
    refs = host_terms()
    host_s = (time.perf_counter() - t0) / len(refs)
    equal = all(HS.same_bytes(Hd[m].reshape(6, 6), r["H"]) for m, r in enumerate(refs))
    n_terms = t["terms"][0].cpu().numpy()
    ev = {k: [] for k in ("hessian", "hessian_with_rows")}
    fns = dict(hessian=by_events(lambda: hessian(lean)), hessian_with_rows=by_events(lambda: hessian(rows)))
    for r in range(args.reps + 3):
        for k, f in fns.items():
            v = f()
            if r >= 3:
                ev[k].append(v)
    out = {k: band(v) for k, v in ev.items()}
    out.update(comparison=f"launch alone, B={B}", reps=args.reps, landmarks=L, keypoints=K,
               terms_per_multiframe=round(float(n_terms.mean()), 1), verified=int((t["verdict"].cpu().numpy() == 3).sum()))
    print(json.dumps(out), flush=True)
    hc = timed({"device": device_chain, "downloads": downloads}, args.reps)
    out = {k: band(v) for k, v in hc.items()}
    upper = out["downloads"]["median_ms"] + 1e3 * host_s * B
    out.update(comparison=f"H on the host, B={B}", reps=args.reps, host_restatement_ms_per_multiframe=round(1e3 * host_s, 3),
               baseline_upper_bound_ms=round(upper, 3), H_equal_to_the_restatement=bool(equal),
               note="baseline_upper_bound_ms = downloads + B x the numpy restatement of one multiframe: an upper bound "
                    "for a compiled host loop")
    print(json.dumps(out), flush=True)
    fe.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", default="1,256,3072")
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
