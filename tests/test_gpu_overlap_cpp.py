"""GPU: the C++ host mirror's HipFrontend::overlapFraction (B = 1), overlapFractionBlocks (device-resident),
trackingQuality and motionStereoFrameOrder (okvis2_amd/host/okvfe_frontend.hpp), driven from a C++ program over a
request file on the EuRoC scene of overlap_scenes.py: counts equal, doubles equal as u64 bit patterns, to the
restatement of ViSlamBackend.cpp:2341-2427, :157-196 and Frontend.cpp:1742-1767 in overlap_ref.py.

PARITY UNPINNED for cv::circle and the point rounding (restated from OpenCV's published source, see keyframe_ref.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import keyframe_ref as R
import overlap_ref as OR
import overlap_scenes as S
from okvis2_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "cpp", "overlap_cli")


def _bits(values):
    return [struct.unpack("<Q", struct.pack("<d", float(v)))[0] for v in values]


def test_cpp_overlap_fraction_tracking_quality_and_sweep_order(tmp_path):
    assert os.path.exists(CLI), "run __graft_entry__.build() first"
    cfg, K, mfs, ref = S.reference("euroc")
    M, C, previous = len(mfs), len(cfg.cams), 1
    rng = np.random.default_rng(157)
    observed = [[(rng.random(len(kps)) < 0.7).astype(np.uint8) for kps, _ in mf] for mf in mfs]
    pairs = [(a, b) for a in range(M) for b in range(M)]
    frame_ids = np.array([40, 12, 77, 5, 63, 21, 90, 34, 58, 19], dtype=np.uint64)
    blocks, ids = S.pack(mfs, K, 1, M)  # camera-major
    req, resp = tmp_path / "req.bin", tmp_path / "resp.bin"
    with open(req, "wb") as f:
        f.write(struct.pack("<10i", C, cfg.w, cfg.h, K, M, len(pairs), 1, M, previous, blocks.shape[1]))
        f.write(struct.pack("<2d", -1.0, cfg.uniformity_radius))  # the mirror's own 0.09 * uniformityRadius / 36
        for mf, obs in zip(mfs, observed):
            for (kps, fid), o in zip(mf, obs):
                f.write(struct.pack("<i", len(kps)))
                f.write(kps.tobytes() + fid.tobytes() + o.tobytes())
        f.write(np.array([p[0] for p in pairs], np.int32).tobytes())
        f.write(np.array([p[1] for p in pairs], np.int32).tobytes())
        f.write(frame_ids.tobytes() + blocks.tobytes() + ids.tobytes())
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "okvis2_amd") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = subprocess.run([CLI, str(req), str(resp)], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(resp, "rb").read()
    n, off = len(pairs), 0

    def take(dtype, count):
        nonlocal off
        a = np.frombuffer(raw, dtype=dtype, count=count, offset=off)
        off += a.nbytes
        return a
    overlap, counts = take(np.float64, n), take(capi.OVERLAP_COUNTS_DTYPE, n)
    counts_dev, overlap_dev = take(capi.OVERLAP_COUNTS_DTYPE, n), take(np.float64, n)
    cov = take(capi.COVERAGE_DTYPE, n * 2 * C).reshape(n, 2, C)
    quality = take(np.float64, M)
    n_order = int(take(np.int32, 1)[0])
    order, threw = take(np.int32, n_order).tolist(), int(take(np.int32, 1)[0])
    assert off == len(raw)
    assert S.KPTRAD == 0.09 * cfg.uniformity_radius / 36.0
    want = S.counts_array(ref, pairs)
    want_overlap = _bits(ref[p]["overlap"] for p in pairs)
    for field in OR.COUNT_FIELDS:
        assert np.array_equal(counts[field], want[field]), ("overlapFraction", field)
        assert np.array_equal(counts_dev[field], want[field]), ("overlapFractionBlocks", field)
    assert _bits(overlap) == want_overlap and _bits(overlap_dev) == want_overlap
    assert any(np.isnan(overlap)) and sum(1 for v in overlap if 0 < v < 1) >= 16
    for field in R.COVERAGE_FIELDS:
        for i, p in enumerate(pairs):
            for side in range(2):
                assert cov[field][i, side].tolist() == [r[field] for r in ref[p]["per_image"][side]], (field, p, side)
    want_quality = [OR.tracking_quality(cfg.w, cfg.h, mf, obs, S.KPTRAD) for mf, obs in zip(mfs, observed)]
    assert _bits(quality) == _bits(want_quality)
    assert sum(1 for q in want_quality if q > 0.0) >= 3 and sum(1 for q in want_quality if q == 0.0) >= 2
    row = [ref[(previous, b)]["overlap"] for b in range(M)]
    assert order == OR.motion_frame_order(row, frame_ids, previous) and order[0] == previous and len(order) >= 3
    assert threw == 3
