#!/usr/bin/env python3
"""What ImuError::propagation costs per frame next to the frontend's step: okvfe_imu_propagation_blocks_device against
the compiled host loop okvfe_imu_propagation over the same batch on one core.

Workload, EuRoC-like: IMU at 200 Hz with jitter, frames at 20 Hz (12 samples per multiframe: one before t_start, one
after t_end, t_start and t_end between samples), 2 cameras, moderate motion; 16 distinct multiframes repeated to fill a
batch of 1, 256 and 3072.

One process; the variants alternate repetition by repetition; median and [p10, p90] over --reps repetitions (at least
30); one JSON line per batch size.  Boxes differ by several per cent: only same-run comparisons mean anything.  For each
of the three forms (the mean only, with the Jacobian F, with the covariance P):
  launch_us   the launch alone, between device events on the call's stream
  device_us   on the host clock: the call, one synchronisation, and the download of what the form produces
  host_us     on the host clock: okvfe_imu_propagation over the same batch (host pointers, one core)

    python tools/bench_imu_propagation.py [--batches 1,256,3072] [--reps 30]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FORMS = dict(mean=(False, False), jacobian=(True, False), covariance=(True, True))
DISTINCT = 16


def workload(B):
    """(multiframes, T_SC_params): 12 samples at 200 Hz around a 50 ms frame interval"""
    import imu_scenes as SC
    rng = np.random.default_rng(2024)
    distinct = []
    for i in range(DISTINCT):
        mf = SC.multiframe("general", 4 * i + 1, rng, n=12)        # (an index that puts t_start between samples)
        ns = [int(t[0]) * 1000000000 + int(t[1]) for t in mf["ts"]]
        mf["t_start"] = SC.stamp(ns[0] + int(rng.integers(1, 4000000)))
        mf["t_end"] = SC.stamp(ns[10] + int(rng.integers(1, 4000000)))
        distinct.append(mf)
    return [distinct[i % DISTINCT] for i in range(B)], SC.scenes()[1]["T_SC_params"]


def stats(v):
    v = np.asarray(v) * 1e6
    return [round(float(np.median(v)), 2), round(float(np.percentile(v, 10)), 2), round(float(np.percentile(v, 90)), 2)]


def measure(fe, B, reps):
    import torch
    import imu_scenes as SC
    from okvis2_amd import capi
    mfs, T_SC = workload(B)
    samples, begin, states = SC.pack(mfs)
    n_cams = len(T_SC)
    shapes = dict(pose=(7, np.float64), speed_and_bias=(9, np.float64), n_propagated=(1, np.int32), status=(1, np.int32),
                  n_out_of_range=(1, np.int32), jacobian=(225, np.float64), covariance=(225, np.float64),
                  T_WC=(7 * n_cams, np.float64), gravity_C=(3 * n_cams, np.float32))
    host = {k: np.zeros((B, w), t) for k, (w, t) in shapes.items()}
    dev = {k: torch.zeros((B, w), dtype=getattr(torch, np.dtype(t).name), device="cuda") for k, (w, t) in shapes.items()}
    pinned = {k: torch.zeros((B, w), dtype=getattr(torch, np.dtype(t).name)).pin_memory() for k, (w, t) in shapes.items()}
    d_in = [torch.from_numpy(a).cuda() for a in (samples, begin, states)]
    prm = capi.make_imu_params(SC.PARAMS)
    T_SC_flat = np.ascontiguousarray(T_SC, np.float64).reshape(-1)
    stream = torch.cuda.Stream()

    def wanted(form):
        jacobian, covariance = FORMS[form]
        return [k for k in shapes if (k != "jacobian" or jacobian) and (k != "covariance" or covariance)]

    def result(ptrs, form):
        keys = wanted(form)
        return capi.make_imu_result(*[ptrs[k] if k in keys else None for k in shapes])

    res_dev = {f: result({k: t.data_ptr() for k, t in dev.items()}, f) for f in FORMS}
    res_host = {f: result({k: a.ctypes.data for k, a in host.items()}, f) for f in FORMS}

    def launch(form):
        fe.imu_propagation_blocks_device(prm, d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), B, T_SC,
                                         res_dev[form], stream=stream)

    def by_events(form):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        launch(form)
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) * 1e-3

    def device(form):
        t = time.perf_counter()
        launch(form)
        with torch.cuda.stream(stream):
            for k in wanted(form):
                pinned[k].copy_(dev[k], non_blocking=True)
        stream.synchronize()
        return time.perf_counter() - t

    fn = capi.lib().okvfe_imu_propagation

    def host_loop(form):
        t = time.perf_counter()
        st = fn(C.byref(prm), samples.ctypes.data_as(C.c_void_p), begin.ctypes.data_as(C.c_void_p),
                states.ctypes.data_as(C.c_void_p), B, n_cams, T_SC_flat.ctypes.data_as(C.c_void_p), 1, C.byref(res_host[form]))
        dt = time.perf_counter() - t
        assert st == 0
        return dt

    variants = [(kind, form, f) for form in FORMS for kind, f in (("launch_us", by_events), ("device_us", device),
                                                                   ("host_us", host_loop))]
    for _, form, f in variants:                                     # warm-up, and the two sides agree
        for _ in range(3):
            f(form)
    torch.cuda.synchronize()
    for k in wanted("covariance"):
        assert np.array_equal(pinned[k].numpy().view(np.uint8), host[k].view(np.uint8)), k
    times = {(kind, form): [] for kind, form, _ in variants}
    for _ in range(reps):
        for kind, form, f in variants:
            times[(kind, form)].append(f(form))
    out = dict(batch=B, samples_per_multiframe=12, cameras=n_cams, reps=reps, unit="us: median [p10, p90]")
    for form in FORMS:
        out[form] = {kind: stats(times[(kind, form)]) for kind in ("launch_us", "device_us", "host_us")}
        out[form]["host_over_device"] = round(out[form]["host_us"][0] / out[form]["device_us"][0], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,256,3072")
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    from okvis2_amd import capi
    fe = capi.Frontend(64, 64, 10.0, 0, 50, 10)
    try:
        for B in [int(b) for b in args.batches.split(",")]:
            print(json.dumps(measure(fe, B, max(args.reps, 30))), flush=True)
    finally:
        fe.close()


if __name__ == "__main__":
    main()
