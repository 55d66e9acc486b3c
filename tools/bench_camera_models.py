#!/usr/bin/env python3
"""EuRoC rig (radial-tangential, 4 coefficients) against the RADTAN8 rig (the reference's
8-coefficient test camera, synth.radtan8_config) on the bench's EuRoC step: 3072 stereo frames of
752x480 built from 256 distinct pairs, device-resident, detect + describe + matchStereo, timed with
HIP events.  Both rigs live in one process; after warm-up the steps alternate between them.  One
JSON line: stereo-frames/s per rig, the per-stage split of okvfe_profile_* (ms per step, from a
profiled pass of its own) and okvfe_pattern_kernel_class (the descriptor kernel class the rig's
Jacobian stretch selects).
Usage: python tools/bench_camera_models.py [--frames 3072] [--distinct 256] [--steps 10] [--warmup 3]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from okvis2_amd import capi, synth  # noqa: E402


def make_rig(cfg, frames, distinct, torch):
    _, base = bench.make_inputs(cfg, frames, distinct, 4242, tile=False)
    d_img = bench.tile_on_device(base, 2 * frames, torch.device("cuda"))
    fe = capi.Frontend(cfg.w, cfg.h, cfg.uniformity_radius, cfg.octaves, cfg.abs_threshold, cfg.max_kpts,
                       match_threshold=cfg.match_threshold, max_batch=2 * frames, num_cameras=2)
    for ci, cam in enumerate(cfg.cams):
        fe.set_camera(ci, cam)
    g = np.stack([[0.03 * ((i % 5) - 2), 1.0, 0.02 * ((i % 3) - 1)] for i in range(2 * distinct)])
    g = (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
    grav = np.concatenate([g] * (frames // distinct + 1))[:2 * frames]
    cam_ids = np.array([0, 1] * frames, dtype=np.int32)
    T0, T1 = synth.stereo_poses(cfg.baseline)
    f = [0.5 * (c.fu + c.fv) for c in cfg.cams]
    pairs = []
    for i in range(frames):
        sp = capi.StereoPair()
        sp.image0, sp.image1 = 2 * i, 2 * i + 1
        sp.T_WC0, sp.T_WC1 = capi.make_pose(*T0), capi.make_pose(*T1)
        sp.f0, sp.f1 = f[0], f[1]
        pairs.append(sp)
    pairs = (capi.StereoPair * frames)(*pairs)
    d_match = torch.zeros((frames, cfg.max_kpts, capi.STEREO_MATCH_DTYPE.itemsize), dtype=torch.uint8,
                          device="cuda")
    return dict(fe=fe, d_img=d_img, grav=grav, cam_ids=cam_ids, pairs=pairs, d_match=d_match, frames=frames)


def step(rig, stream):
    s = stream.cuda_stream
    rig["fe"].detect_describe_batch_device(rig["d_img"].data_ptr(), 2 * rig["frames"], rig["cam_ids"], rig["grav"], s)
    rig["fe"].match_stereo_batch_device(rig["pairs"], rig["d_match"].data_ptr(), s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3072)
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    stream = torch.cuda.Stream()
    rigs = {"euroc": make_rig(synth.euroc_config(), args.frames, args.distinct, torch),
            "radtan8": make_rig(synth.radtan8_config(), args.frames, args.distinct, torch)}
    with torch.cuda.stream(stream):
        for _ in range(args.warmup):
            for r in rigs.values():
                step(r, stream)
        stream.synchronize()
        times = {k: [] for k in rigs}
        for _ in range(args.steps):
            for k, r in rigs.items():  # alternated, so drifts of the box hit both rigs alike
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                step(r, stream)
                b.record(stream)
                b.synchronize()
                times[k].append(a.elapsed_time(b))
        out = {"frames_per_step": args.frames, "distinct": args.distinct, "steps": args.steps}
        for k, r in rigs.items():
            ms = float(np.median(times[k]))
            r["fe"].check_capacity(2 * args.frames)
            r["fe"].profile_enable(True)
            step(r, stream)
            stream.synchronize()
            prof = r["fe"].profile_read()
            r["fe"].profile_enable(False)
            counts = [r["fe"].download(i)[3] for i in range(0, 2 * args.distinct, 2 * args.distinct // 8)]
            out[k] = {"stereo_frames_per_s": args.frames / (ms / 1e3), "step_ms_median": ms,
                      "step_ms_min": float(np.min(times[k])),
                      "stage_ms": {s: v[0] for s, v in prof.items() if v[1] > 0},
                      "compact_ms_per_6144_images": prof["compact"][0] * 6144 / (2 * args.frames),
                      "pattern_kernel_class": r["fe"].pattern_kernel_class(),
                      "keypoints_per_image_sample": float(np.mean([len(c) for c in counts])),
                      "valid_backprojection_share": float(np.mean([c.mean() for c in counts]))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
