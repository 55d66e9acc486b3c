#!/usr/bin/env python3
"""What the refinement of verifyRecognisedPlace's pose costs on the device: okvfe_place_refine_blocks_device behind the
consensus (3 + 2 x max_iterations short launches and the Hessian at the pose out), against the chain an integrator could
drive from the host before the call existed.

Workload: that of tools/bench_place_hessian.py -- a landmark set of 1000 landmarks, multiframes of 2 EuRoC cameras with
700 keypoints each, 50 hypotheses per multiframe; 16 distinct multiframes are repeated to fill a batch.  The matching,
the claims and the consensus (with its state rows and best_hypothesis) run once; the refinement starts at the winning
hypothesis, max_iterations 10.

Every batch size is measured in ONE process of its own (a child of this one, under its own time limit), variants
alternating repetition by repetition; median and [p10, p90] over `--reps` repetitions (at least 30); one JSON line per
comparison.  Boxes differ by several per cent: only same-run comparisons mean anything.
  (a) refine           the call alone, between device events on the call's stream (every output, H included)
  (b) on the host clock:
      refine_sync      the call, one synchronisation, poses, status and H downloaded
      host_chain_bound the chain possible without the call, as a LOWER BOUND only: per iterate a Hessian call with its
                       residual and Jacobian rows, one synchronisation, the download of the rows (K x 14 doubles per
                       block) and the upload of seven doubles per multiframe.  The number of iterates is the largest
                       number of evaluations the restatement (tests/place_refine_ref.py) needs for a multiframe of the
                       batch.  It contains NO host solve: it is a bound on the transfers and launches, not a host solver.

    python tools/bench_place_refine.py [--batches 1,256,3072] [--reps 30]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_map_ransac import compose, hypotheses, make_frame  # noqa: E402
from bench_map_table import band, make_table, rot_y, timed  # noqa: E402

MIN_INLIERS = 10  # Frontend.cpp:823


def worker(B, args):
    import torch
    import oracle_lib
    import place_hessian_scenes as HS
    import place_refine_ref as PR
    from okvis2_amd import capi, multigpu, synth

    cfg = synth.euroc_config()
    cams, K, L, nh, D, I = cfg.cams, args.keypoints, args.landmarks, args.hypotheses, args.distinct, args.max_iterations
    fe = capi.Frontend(cfg.w, cfg.h, cfg.uniformity_radius, 0, cfg.abs_threshold, K, match_threshold=cfg.match_threshold,
                       max_batch=1, num_cameras=2)
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
             kmin=zeros((nb, L), torch.int32), dmin=zeros((nb, L), torch.int32), counts=zeros((3, B), torch.int32),
             gate=zeros((B,), torch.uint8), ml=zeros((nb, K), torch.int32), head=zeros((3, B), torch.int32),
             acc=zeros((B,), torch.uint8), verdict=zeros((B,), torch.uint8), state=zeros((nb, K), torch.uint8),
             poses=zeros((B, 7), torch.float64), start=zeros((B, 7), torch.float64), cost=zeros((B, 2), torch.float64),
             Hm=zeros((B, 36), torch.float64), ints=zeros((5, B), torch.int32), terms=zeros((2, B), torch.int32),
             residual=zeros((nb, K, 2), torch.float64), jacobian=zeros((nb, K, 12), torch.float64))
    md = fe.make_map_device(L, t["desc_begin"].data_ptr(), t["pool"].data_ptr())
    pset = fe.make_place_set_device(L, t["hp"].data_ptr())
    claims_res = fe.make_place_claims_device(t["counts"][0].data_ptr(), t["counts"][1].data_ptr(), t["counts"][2].data_ptr(),
                                             t["gate"].data_ptr(), t["ml"].data_ptr())
    res = fe.make_ransac_result_device(t["head"][0].data_ptr(), t["head"][1].data_ptr(), t["head"][2].data_ptr(),
                                       t["acc"].data_ptr(), state_ptr=t["state"].data_ptr())
    out_dev = fe.make_place_refine_device(t["poses"].data_ptr(), t["ints"][0].data_ptr(), t["ints"][1].data_ptr(),
                                          t["ints"][2].data_ptr(), t["ints"][3].data_ptr(), t["cost"].data_ptr(),
                                          t["start"].data_ptr(), t["Hm"].data_ptr(), t["ints"][4].data_ptr())
    rows = fe.make_place_hessian_device(t["Hm"].data_ptr(), t["terms"][0].data_ptr(), t["terms"][1].data_ptr(),
                                        t["residual"].data_ptr(), t["jacobian"].data_ptr())
    stream = torch.cuda.Stream()
    pinned = dict(Hm=torch.zeros((B, 36), dtype=torch.float64).pin_memory(),
                  poses=torch.zeros((B, 7), dtype=torch.float64).pin_memory(),
                  status=torch.zeros((B,), dtype=torch.int32).pin_memory(),
                  residual=torch.zeros((nb, K, 2), dtype=torch.float64).pin_memory(),
                  jacobian=torch.zeros((nb, K, 12), dtype=torch.float64).pin_memory())
    # the chain up to the consensus, once: the rows and the winners the refinement reads
    fe.verify_place_blocks_device(t["blocks"].data_ptr(), nb, md, t["kmin"].data_ptr(), t["dmin"].data_ptr(), stream)
    fe.place_claims_blocks_device(pset, t["blocks"].data_ptr(), B, 2, t["kmin"].data_ptr(), t["dmin"].data_ptr(), MIN_INLIERS,
                                  claims_res, stream)
    fe.place_consensus_blocks_device(pset, t["blocks"].data_ptr(), B, [0, 1], T_SC, t["ml"].data_ptr(), t["gate"].data_ptr(),
                                     t["H"].data_ptr(), None, nh, MIN_INLIERS, res, t["verdict"].data_ptr(), stream=stream)
    stream.synchronize()

    def refine():
        fe.place_refine_blocks_device(pset, t["blocks"].data_ptr(), B, [0, 1], prm, t["H"].data_ptr(), nh,
                                      t["head"][1].data_ptr(), None, t["ml"].data_ptr(), t["state"].data_ptr(),
                                      t["verdict"].data_ptr(), I, out_dev, stream)

    def refine_sync():
        refine()
        with torch.cuda.stream(stream):
            pinned["poses"].copy_(t["poses"], non_blocking=True)
            pinned["status"].copy_(t["ints"][0], non_blocking=True)
            pinned["Hm"].copy_(t["Hm"], non_blocking=True)
        stream.synchronize()

    # the restatement on the distinct multiframes: the bytes to expect and the number of evaluations it needs
    refine_sync()
    ml, st, verdict = (t[k].cpu().numpy() for k in ("ml", "state", "verdict"))
    best = t["head"][1].cpu().numpy()
    n_eval, equal, statuses = [], True, []
    original = PR.accumulate
    for m in range(min(B, D)):
        calls = []
        PR.accumulate = lambda res_, jac_: (calls.append(1), original(res_, jac_))[1]
        try:
            frames = [dict(kps=multigpu.unpack_block_host(blocks[2 * m + c], K)[0]) for c in range(2)]
            ref = PR.refine(oracle_lib, True, tab["hp"], frames, [ml[2 * m], ml[2 * m + 1]], [st[2 * m], st[2 * m + 1]], cams,
                            prm, np.asarray(Hs[m]).reshape(nh, 12), int(best[m]), None, I, verdict[m] == 3)
        finally:
            PR.accumulate = original
        n_eval.append(len(calls))
        statuses.append(ref["status"])
        equal = equal and ref["status"] == int(pinned["status"][m]) and (
            ref["pose"] is None or (HS.same_bytes(pinned["poses"][m].numpy(), ref["pose"])
                                    and HS.same_bytes(pinned["Hm"][m].numpy().reshape(6, 6), ref["H"])))
    iterates = max(n_eval)
    up = torch.zeros((B, 7), dtype=torch.float64).pin_memory()

    def host_chain_bound():
        for _ in range(iterates):
            fe.place_hessian_blocks_device(pset, t["blocks"].data_ptr(), B, [0, 1], prm, t["start"].data_ptr(),
                                           t["ml"].data_ptr(), t["state"].data_ptr(), t["verdict"].data_ptr(), rows, stream)
            with torch.cuda.stream(stream):
                pinned["residual"].copy_(t["residual"], non_blocking=True)
                pinned["jacobian"].copy_(t["jacobian"], non_blocking=True)
            stream.synchronize()
            with torch.cuda.stream(stream):                         # (the next iterate of a host solver; none runs here)
                t["start"].copy_(up.copy_(pinned["poses"]), non_blocking=True)

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
    ev, f = [], by_events(refine)
    for r in range(args.reps + 3):
        v = f()
        if r >= 3:
            ev.append(v)
    out = dict(refine=band(ev), comparison=f"the call alone, B={B}", reps=args.reps, landmarks=L, keypoints=K,
               max_iterations=I, launches=3 + 2 * I + 1,
               terms_per_multiframe=round(float(t["ints"][3].cpu().numpy().mean()), 1),
               verified=int((verdict == 3).sum()), statuses_of_the_distinct=statuses, evaluations_of_the_distinct=n_eval,
               equal_to_the_restatement=bool(equal))
    print(json.dumps(out), flush=True)
    hc = timed({"refine_sync": refine_sync, "host_chain_bound": host_chain_bound}, args.reps)
    out = {k: band(v) for k, v in hc.items()}
    out.update(comparison=f"on the host clock, B={B}", reps=args.reps, iterates_of_the_bound=iterates,
               note="host_chain_bound = per iterate a Hessian call with rows + one synchronisation + the row download + a "
                    "seven-double upload per multiframe, no host solve: a LOWER BOUND for a host-driven chain, not a host solver")
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
    ap.add_argument("--max-iterations", type=int, default=10)
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
               str(args.hypotheses), "--max-iterations", str(args.max_iterations)]
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
