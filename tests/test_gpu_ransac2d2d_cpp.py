"""GPU: the C++ host mirror (okvis2_amd/host/okvfe_frontend.hpp) of the consensus of runRansac2d2d --
HipFrontend::ransac2d2dBlocks with landmark1_out in place -- driven from a C++ program (tests/cpp/ransac2d2d_cli.cpp) on
a stream of its own: the one-camera general scene (hypothesis flags given) and the chunk scene (no flags) of
ransac2d2d_scenes.py against ransac2d2d_ref.py.  Integers for equality, distances as uint64 patterns; rows past a
frame's keypoint count keep the driver's fill bytes (the ids: the request's rows)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ransac2d2d_scenes as S2
from okvis2_amd import capi
from test_gpu_map_ransac_cpp import cli_env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "cpp", "ransac2d2d_cli")
K = S2.K
FILL = np.frombuffer(b"\xf9" * 4, dtype=np.int32)[0]


class _Cap:
    max_keypoints = K


def write_request(path, sc):
    cam = sc["cams"][0]
    b0, l0, b1, l1 = S2.pack(_Cap, sc)
    P, nh = len(sc["pairs"]), len(sc["pairs"][0][0]["rot_H"])
    stack = lambda key: np.stack([pair[0][key] for pair in sc["pairs"]])
    has_valid = sc["pairs"][0][0]["rot_valid"] is not None
    with open(path, "wb") as f:
        f.write(struct.pack("<iii", cam.w, cam.h, cam.dist_type))
        f.write(struct.pack("<8d", cam.fu, cam.fv, cam.cu, cam.cv, *cam.d[:4]))
        f.write(struct.pack("<ii", K, 60))
        f.write(struct.pack("<i", sc["n_landmarks"]))
        if sc["added"] is not None:
            f.write(np.ascontiguousarray(sc["added"], dtype=np.uint8).tobytes())
        f.write(struct.pack("<iii", P, P, b0.shape[1]))
        for a in (b0, b1, l0, l1):
            f.write(a.tobytes())
        f.write(struct.pack("<i", P))
        f.write(np.arange(P, dtype=np.int32).tobytes() * 2)
        f.write(struct.pack("<i", nh))
        f.write(stack("rot_H").astype(np.float64).tobytes())
        f.write(stack("rel_H").astype(np.float64).tobytes())
        f.write(struct.pack("<i", int(has_valid)))
        if has_valid:
            f.write(stack("rot_valid").astype(np.uint8).tobytes())
            f.write(stack("rel_valid").astype(np.uint8).tobytes())
    return P, nh, l1


@pytest.mark.parametrize("which", ("general", "chunks"))
def test_cpp_mirror(oracle, tmp_path, which):
    assert os.path.exists(CLI), "run __graft_entry__.build() first"
    if which == "general":
        sc = S2.general_scene(oracle, ("nodist",))
    else:
        sc = S2.chunk_scene(oracle, capi.Frontend._test_ransac2d2d_chunk_records())
    refs = S2.reference(True, sc)  # (a fresh process: the default order of the sums)
    req, resp = tmp_path / "req.bin", tmp_path / "resp.bin"
    P, nh, l1 = write_request(req, sc)
    out = subprocess.run([CLI, str(req), str(resp)], env=cli_env(), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(resp, "rb").read()
    sizes = [P * 20, P * 2, P * 4, P * 2, P * nh * 4, P * nh * 4, P * K * 4, P * K, P * K * 8, P * K * 4, 4]
    assert len(raw) == sum(sizes)
    parts, o = [], 0
    for n in sizes:
        parts.append(raw[o:o + n])
        o += n
    I = lambda i, *shape: np.frombuffer(parts[i], np.int32).reshape(*shape)
    U = lambda i, *shape: np.frombuffer(parts[i], np.uint8).reshape(*shape)
    head, flags, total, pair = I(0, 5, P), U(1, 2, P), I(2, P), U(3, 2, P)
    rh, lh, match1, state = I(4, P, nh), I(5, P, nh), I(6, P, K), U(7, P, K)
    dist, lm1 = np.frombuffer(parts[8], np.float64).reshape(P, K), I(9, P, K)
    assert struct.unpack("<i", parts[10])[0] == 1  # a hypothesis count that does not fit made ransac2d2dBlocks throw
    for p, (ref, entry) in enumerate(zip(refs, sc["pairs"])):
        c, cam = ref["cams"][0], entry[0]
        assert tuple(head[:, p]) == (c["n_corr"], c["rot_best"], c["rot_inliers"], c["rel_best"], c["rel_inliers"]), p
        assert tuple(flags[:, p]) == (c["branch"], c["removed"]), p
        assert (total[p], pair[0, p], pair[1, p]) == (ref["total_inliers"], ref["rotation_only"], ref["success"]), p
        assert np.array_equal(rh[p], c["rot_hyp_inliers"]) and np.array_equal(lh[p], c["rel_hyp_inliers"]), p
        n0, n1 = len(cam["fr0"]["kps"]), len(cam["fr1"]["kps"])
        assert np.array_equal(match1[p, :n0], c["match1"]) and np.all(match1[p, n0:] == FILL), p
        assert np.array_equal(state[p, :n0], c["state"]) and np.all(state[p, n0:] == 0xF9), p
        ds = c["dist_set"]
        assert np.array_equal(dist[p, :n0][ds].view(np.uint64), c["distance"][ds].view(np.uint64)), p
        assert np.array_equal(lm1[p, :n1], c["landmark1_out"]) and np.array_equal(lm1[p, n1:], l1[p, n1:]), p
    assert sum(r["success"] != 0 for r in refs) >= 1
