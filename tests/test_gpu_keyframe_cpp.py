"""GPU: HipFrontend::doWeNeedANewKeyframe of the C++ host mirror (okvis2_amd/host/okvfe_frontend.hpp), driven from a
C++ program on a two-camera current multiframe and three other multiframes: verdict and overlap (as its u64 bit
pattern) equal to the numpy restatement of Frontend.cpp:1058-1167 in keyframe_ref.py.

PARITY UNPINNED for cv::circle and the point rounding (restated from OpenCV's published source, see keyframe_ref.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import keyframe_ref as R
from okvis2_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "cpp", "keyframe_cli")


def _multiframes(rng, w, h):
    def frame(n, ids):
        kps = np.zeros(n, dtype=capi.KEYPOINT_DTYPE)
        kps["x"], kps["y"] = rng.uniform(0, w - 0.5, n), rng.uniform(0, h - 0.5, n)
        return kps, np.asarray(ids, dtype=np.uint64)
    cur = [frame(40, np.where(rng.random(40) < 0.6, rng.integers(1, 1000, 40), 0)),
           frame(25, np.where(rng.random(25) < 0.5, rng.integers(1000, 2000, 25), 0))]
    pool = np.concatenate([i[i != 0] for _, i in cur])
    others = []
    for share, n in ((0.8, 30), (0.3, 45), (0.0, 20)):
        others.append([frame(n, np.where(rng.random(n) < share, rng.choice(pool, n), rng.integers(5000, 6000, n)))
                       for _ in range(2)])
    return cur, others


@pytest.mark.parametrize("threshold", [0.55, 0.6])
def test_cpp_do_we_need_a_new_keyframe(tmp_path, threshold):
    assert os.path.exists(CLI), "run __graft_entry__.build() first"
    w, h = 752, 480
    cur, others = _multiframes(np.random.default_rng(1167), w, h)
    req, resp = tmp_path / "req.bin", tmp_path / "resp.bin"
    with open(req, "wb") as f:
        f.write(struct.pack("<iiii", w, h, 2, len(others)))
        f.write(struct.pack("<f", threshold))
        for multiframe in [cur] + others:
            for kps, ids in multiframe:
                f.write(struct.pack("<i", len(kps)))
                f.write(kps.tobytes())
                f.write(ids.tobytes())
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "okvis2_amd") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = subprocess.run([CLI, str(req), str(resp)], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    need, overlap_bits, need_alone, overlap_alone_bits = struct.unpack("<iQiQ", open(resp, "rb").read())
    s = np.concatenate([i for _, i in cur])
    rc = [R.coverage(w, h, k, i) for k, i in cur]
    ro = [[R.coverage(w, h, k, i, s) for k, i in mf] for mf in others]
    want_need, want_overlap = R.decision(rc, ro, np.float32(threshold))
    assert 0.55 < want_overlap < 0.6  # the two thresholds straddle it: both verdicts are exercised
    assert bool(need) == want_need == (threshold == 0.6)
    assert overlap_bits == struct.unpack("<Q", struct.pack("<d", want_overlap))[0]
    assert (bool(need_alone), overlap_alone_bits) == (True, 0)  # no other frames: overlapOthers = 0.0
