#!/usr/bin/env python3
"""What the step between matchToMap's two passes costs on the device: okvfe_ransac3d2d_consensus_blocks_device and
okvfe_remove_outliers_blocks_device.

Workload: the table of tools/bench_map_table.py (5000 landmarks), multiframes of 2 EuRoC cameras with 700 keypoints
each, 50 hypotheses per multiframe (the true T_WS, 39 perturbed by up to 2 degrees / 5 cm, 10 random).  A keypoint sits
at the radial-tangential projection of a landmark with 0.5 px of noise, carries a noisy copy of that landmark's first
observation descriptor and the ray to its pixel as back-projection; 30 % of the descriptors are another landmark's.
The landmark rows the new calls read are what the first pass (okvfe_match_to_map_table_blocks_device, 20 px, not
exclusive) wrote for these frames.  16 distinct multiframes are repeated to fill a batch.

Everything is timed in ONE process, variants alternating repetition by repetition; median and [p10, p90] over `--reps`
repetitions (at least 30); one JSON line per comparison.  Boxes differ by several per cent: only same-run comparisons
mean anything.
  (a) the consensus launch alone and the removeOutliers launch alone, between device events on the call's stream, at
      B = 1 / 256 / 3072 multiframes; the achieved FP64 rate of the consensus kernel (57 FP64 operations per
      (valid hypothesis, correspondence) pair: 27 multiplications, 25 additions and subtractions, 4 divisions and
      1 square root) against the device's vector FP64 peak
  (b) the step next to the call it follows, on the host clock with one stream synchronisation at the end: the first
      pass alone against first pass + consensus (in place) + removeOutliers (in place); the difference is the +ms
  (c) B = 1, one camera: the device consensus + one synchronisation against the host chain it replaces (tests/cpp/
      map_ransac_cli `host N`: match rows downloaded, correspondences rebuilt, 50 hypotheses scored by a plain C++
      loop, filtered rows uploaded)

    python tools/bench_map_ransac.py [--batches 1,256,3072] [--reps 30]
"""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_map_table import band, make_table, rot_y, timed  # noqa: E402

FLOP_PER_PAIR = 57
# MI355X vector FP64: half of the 157.3 TFLOPS FP32 vector rate of the chip-level table (AMD's data sheet: 78.6)
PEAK_FP64_TFLOPS = 78.6


def radtan(cam, x, y):
    k1, k2, p1, p2 = cam.d[:4]
    r = x * x + y * y
    rad = k1 * r + k2 * r * r
    return (x + x * rad + 2 * p1 * x * y + p2 * (r + 2 * x * x), y + y * rad + 2 * p2 * x * y + p1 * (r + 2 * y * y))


def rodrigues(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1.0 - np.cos(angle)) * (Kx @ Kx)


def compose(T_WS, T_SC):
    Cw, rw, Cs, rs = T_WS[0].reshape(3, 3), T_WS[1], T_SC[0].reshape(3, 3), T_SC[1]
    return (Cw @ Cs).reshape(-1).copy(), Cw @ rs + rw


def make_frame(cam, w, h, T_WC, tab, K, rng):
    p_W = tab["hp"][:, :3] / tab["hp"][:, 3:4]
    pc = (p_W - T_WC[1]) @ T_WC[0].reshape(3, 3)
    front = np.flatnonzero(pc[:, 2] > 0.5)
    x, y = radtan(cam, pc[front, 0] / pc[front, 2], pc[front, 1] / pc[front, 2])
    u, v = cam.fu * x + cam.cu, cam.fv * y + cam.cv
    ok = (u > 1) & (u < w - 1) & (v > 1) & (v < h - 1) & (np.hypot(pc[front, 0], pc[front, 1]) / pc[front, 2] < 1.0)
    rows = rng.permutation(np.flatnonzero(ok))[:K]  # positions in `front`
    vis = front[rows]
    from okvis2_amd import capi
    kps = np.zeros(K, dtype=capi.KEYPOINT_DTYPE)
    kps["size"] = 12.0
    kps["x"], kps["y"] = rng.uniform(5, w - 5, K), rng.uniform(5, h - 5, K)
    n = len(vis)
    kps["x"][:n] = u[rows] + rng.normal(0, 0.5, n)
    kps["y"][:n] = v[rows] + rng.normal(0, 0.5, n)
    bp = np.stack([(kps["x"] - cam.cu) / cam.fu, (kps["y"] - cam.cv) / cam.fv, np.ones(K)], 1).astype(np.float64)
    bp[:n] = pc[vis] / pc[vis, 2:3]
    desc = rng.integers(0, 256, (K, 48), dtype=np.uint8)
    owner = vis.copy()
    wrong = rng.random(n) < 0.3
    owner[wrong] = rng.integers(0, len(p_W), int(wrong.sum()))
    flips = ((rng.random((n, 48)) < 0.03) * rng.integers(1, 256, (n, 48))).astype(np.uint8)
    desc[:n] = tab["obs_desc"][tab["obs_begin"][owner]] ^ flips
    return kps, desc, bp


def hypotheses(T_WS, n, rng):
    Cw, rw = T_WS[0].reshape(3, 3), T_WS[1]
    out = [np.concatenate([Cw, rw[:, None]], 1).reshape(-1)]
    for i in range(1, n):
        if i >= n - 10:
            Ch, rh = rodrigues(rng.normal(size=3), rng.uniform(0, np.pi)), rng.uniform(-3, 3, 3)
        else:
            s = rng.random()
            Ch, rh = Cw @ rodrigues(rng.normal(size=3), np.deg2rad(2.0) * s), rw + 0.05 * s * rng.normal(size=3) / np.sqrt(3)
        out.append(np.concatenate([Ch, rh[:, None]], 1).reshape(-1))
    return np.array(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", default="1,256,3072")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--landmarks", type=int, default=5000)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--hypotheses", type=int, default=50)
    args = ap.parse_args()
    if args.reps < 30:
        ap.error("--reps: at least 30")
    import torch
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
    blocks, poses, Hs = [], [], []
    for m in range(D):
        T_WS = ((rot_y(0.03) @ rot_y(0.003 * (m - D / 2))).reshape(-1).copy(), np.array([0.4 + 0.01 * m, 0.0, 0.3 + 0.002 * m]))
        for c in range(2):
            T_WC = compose(T_WS, T_SC[c])
            kps, desc, bp = make_frame(cams[c], cfg.w, cfg.h, T_WC, tab, K, rng)
            blocks.append(multigpu.pack_block_host(K, kps, desc, bp, np.ones(K, np.uint8)))
            poses.append(T_WC)
        Hs.append(hypotheses(T_WS, nh, rng))
    stream = torch.cuda.Stream()

    def tensors(B, n_cams=2):
        rep = [(2 * (i % D) + c) if n_cams == 2 else 2 * (i % D) for i in range(B) for c in range(n_cams)]
        t = dict(blocks=torch.from_numpy(np.stack([blocks[i] for i in rep])).cuda(),
                 H=torch.from_numpy(np.stack([Hs[i % D] for i in range(B)])).cuda(),
                 lm=torch.zeros((B * n_cams, K), dtype=torch.int32, device="cuda"),
                 bd=torch.zeros((B * n_cams, K), dtype=torch.int32, device="cuda"),
                 lm0=torch.zeros((B * n_cams, K), dtype=torch.int32, device="cuda"),
                 out=torch.zeros((B * n_cams, K), dtype=torch.int32, device="cuda"),
                 head=torch.zeros((3, B), dtype=torch.int32, device="cuda"),
                 acc=torch.zeros((B,), dtype=torch.uint8, device="cuda"),
                 hyp=torch.zeros((B, nh), dtype=torch.int32, device="cuda"),
                 kept=torch.zeros((B * n_cams,), dtype=torch.int32, device="cuda"))
        t["poses"] = [poses[i] for i in rep]
        t["ids"] = [i % n_cams for i in range(B * n_cams)]
        return t

    def first_pass(t, dst):
        fe.match_to_map_table_blocks_device(table_dev, t["blocks"].data_ptr(), len(t["ids"]), t["ids"], t["poses"], 20.0,
                                            False, None, None, t[dst].data_ptr(), t["bd"].data_ptr(), stream)

    def consensus(t, B, n_cams, src, dst):
        res = fe.make_ransac_result_device(t["head"][0].data_ptr(), t["head"][1].data_ptr(), t["head"][2].data_ptr(),
                                           t["acc"].data_ptr(), t["hyp"].data_ptr(), None, None, t[dst].data_ptr())
        fe.ransac3d2d_consensus_blocks_device(table_dev, t["blocks"].data_ptr(), B, list(range(n_cams)), T_SC[:n_cams],
                                              t[src].data_ptr(), t["H"].data_ptr(), None, nh, res, stream=stream)

    def remove(t, src, dst):
        fe.remove_outliers_blocks_device(table_dev, t["blocks"].data_ptr(), len(t["ids"]), t["ids"], t["poses"],
                                         t[src].data_ptr(), t[dst].data_ptr(), t["kept"].data_ptr(), stream=stream)

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
        first_pass(t, "lm0")
        stream.synchronize()
        # (a) the launches alone, between device events
        ev = timed_events({"consensus": by_events(lambda: consensus(t, B, 2, "lm0", "out")),
                           "remove_outliers": by_events(lambda: remove(t, "lm0", "out"))}, args.reps)
        consensus(t, B, 2, "lm0", "out")
        stream.synchronize()
        n_corr = t["head"][0].cpu().numpy().astype(np.int64)
        pairs = int((n_corr * nh).sum())
        res = {k: band(v) for k, v in ev.items()}
        tf = pairs * FLOP_PER_PAIR / (res["consensus"]["median_ms"] * 1e-3) / 1e12
        res.update(comparison=f"launch alone, B={B}", reps=args.reps, correspondences_per_multiframe=round(float(n_corr.mean()), 1),
                   inliers_per_multiframe=round(float(t["head"][2].float().mean().item()), 1),
                   accepted=int(t["acc"].sum().item()), pairs=pairs, fp64_tflops=round(tf, 3),
                   fp64_peak_share=round(tf / PEAK_FP64_TFLOPS, 4),
                   consensus_us_per_multiframe=round(res["consensus"]["median_ms"] * 1e3 / B, 3),
                   remove_us_per_frame=round(res["remove_outliers"]["median_ms"] * 1e3 / (2 * B), 3))
        print(json.dumps(res))

        # (b) next to the first pass, host clock
        def a_first():
            first_pass(t, "lm")
            stream.synchronize()

        def b_chain():
            first_pass(t, "lm")
            consensus(t, B, 2, "lm", "lm")
            remove(t, "lm", "lm")
            stream.synchronize()

        hc = timed({"first_pass": a_first, "first_pass_consensus_removal": b_chain}, args.reps)
        res = {k: band(v) for k, v in hc.items()}
        res.update(comparison=f"step cost, B={B}", reps=args.reps, kept_per_frame=round(float(t["kept"].float().mean().item()), 1),
                   plus_ms=round(res["first_pass_consensus_removal"]["median_ms"] - res["first_pass"]["median_ms"], 4))
        print(json.dumps(res))
        del t

    # (c) B = 1, one camera: the device call + one synchronisation against the host chain of the CLI
    t = tensors(1, n_cams=1)
    torch.cuda.synchronize()
    first_pass(t, "lm0")
    stream.synchronize()

    def device_one():
        consensus(t, 1, 1, "lm0", "out")
        stream.synchronize()

    dv = band(timed({"device": device_one}, args.reps)["device"])
    cli = os.path.join(ROOT, "tests", "cpp", "map_ransac_cli")
    Lb = multigpu.block_layout(K)
    with tempfile.TemporaryDirectory() as tmp:
        req = os.path.join(tmp, "req.bin")
        cam = cams[0]
        with open(req, "wb") as f:
            f.write(struct.pack("<iii", cam.w, cam.h, cam.dist_type))
            f.write(struct.pack("<8d", cam.fu, cam.fv, cam.cu, cam.cv, *cam.d[:4]))
            f.write(struct.pack("<iii", K, cfg.match_threshold, 0))
            f.write(struct.pack("<d", 20.0))
            f.write(struct.pack("<iii", L, len(tab["obs_pose"]), len(tab["poses"])))
            for k, dt in (("hp", np.float64), ("quality", np.float64), ("obs_begin", np.int32), ("obs_pose", np.int32),
                          ("obs_desc", np.uint8), ("obs_bp", np.float64), ("poses", np.float64)):
                f.write(np.ascontiguousarray(tab[k], dtype=dt).tobytes())
            f.write(struct.pack("<iiiii", 1, len(blocks[0]), Lb["kps"], Lb["bp"], Lb["bpv"]))
            for _ in range(2):
                f.write(np.concatenate([poses[0][0], poses[0][1]]).astype(np.float64).tobytes())
            f.write(blocks[0].tobytes())
            f.write(np.ones(K, np.uint8).tobytes())
            f.write(np.concatenate([T_SC[0][0], T_SC[0][1]]).astype(np.float64).tobytes())
            f.write(struct.pack("<i", nh))
            f.write(np.ascontiguousarray(Hs[0], dtype=np.float64).tobytes())
        env = dict(os.environ)
        env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "okvis2_amd") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
        out = subprocess.run([cli, req, os.path.join(tmp, "resp.bin"), "host", str(max(args.reps, 50))], env=env,
                             capture_output=True, text=True)
    res = dict(comparison="B=1, one camera: device call + sync vs the host chain", device=dv)
    if out.returncode == 0 and out.stdout.startswith("host_chain_us"):
        w = out.stdout.split()
        head = t["head"].cpu().numpy()[:, 0]
        res.update(host_chain={"median_ms": round(float(w[1]) * 1e-3, 4), "p10_ms": round(float(w[2]) * 1e-3, 4),
                               "p90_ms": round(float(w[3]) * 1e-3, 4)},
                   host_verdict=[int(v) for v in w[4:7]], device_verdict=[int(v) for v in head],
                   gain_ms=round(float(w[1]) * 1e-3 - dv["median_ms"], 4))
    else:
        res.update(host_chain=None, note="map_ransac_cli failed: " + (out.stdout + out.stderr)[-300:])
    print(json.dumps(res))
    fe.close()


if __name__ == "__main__":
    main()
