"""GPU: the C++ host mirror (okvis2_amd/host/okvfe_frontend.hpp) of the 2d2d hypotheses -- ransac2d2dHypothesesBlocks --
driven from a C++ program (tests/cpp/ransac2d2d_hyp_cli.cpp) on a stream of its own: the pairs of a one-camera scene
give what the restatement gives.  Outputs byte for byte."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ransac2d2d_hyp_scenes as HS
import ransac2d2d_scenes as S2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "cpp", "ransac2d2d_hyp_cli")
K = S2.K
N_HYP = 50


def cli_env():
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "okvis2_amd") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return env


class _Size:
    max_keypoints = K


@pytest.mark.parametrize("with_keys", (False, True), ids=("index keys", "key array"))
def test_cpp_hypotheses(oracle, tmp_path, with_keys):
    assert os.path.exists(CLI), "run __graft_entry__.build() first"
    oracle.set_reduction(True)                          # (a fresh process: the default order of the sums)
    sc = S2.general_scene(oracle, ("nodist",))
    cam, n_pairs = sc["cams"][0], len(sc["pairs"])
    keys = [90 + 11 * i for i in range(n_pairs)] if with_keys else list(range(n_pairs))
    b0, l0, b1, l1 = S2.pack(_Size, sc)
    req, resp = tmp_path / "req.bin", tmp_path / "resp.bin"
    with open(req, "wb") as f:
        f.write(struct.pack("<iii", cam.w, cam.h, cam.dist_type))
        f.write(struct.pack("<8d", cam.fu, cam.fv, cam.cu, cam.cv, *cam.d[:4]))
        f.write(struct.pack("<6i", K, n_pairs, b0.shape[1], N_HYP, int(with_keys), 0))
        f.write(b0.tobytes() + b1.tobytes() + l0.tobytes() + l1.tobytes())
        f.write(struct.pack("<Q", HS.SEED))
        if with_keys:
            f.write(np.array(keys, np.uint64).tobytes())
    out = subprocess.run([CLI, str(req), str(resp)], env=cli_env(), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(resp, "rb").read()
    n = n_pairs * N_HYP
    layout = (("rot_H", np.float64, 9), ("rot_valid", np.uint8, 1), ("rel_H", np.float64, 12), ("rel_valid", np.uint8, 1))
    tail = (("rot_samples", np.int32, 2), ("rel_samples", np.int32, 8), ("n_roots", np.int32, 1))
    got, o = {}, 0
    for key, dt, width in layout:
        size = n * width * np.dtype(dt).itemsize
        got[key] = np.frombuffer(raw[o:o + size], dt).reshape(n_pairs, N_HYP, *([width] if width > 1 else []))
        o += size
    n_corr = np.frombuffer(raw[o:o + 4 * n_pairs], np.int32)
    o += 4 * n_pairs
    for key, dt, width in tail:
        size = n * width * np.dtype(dt).itemsize
        got[key] = np.frombuffer(raw[o:o + size], dt).reshape(n_pairs, N_HYP, *([width] if width > 1 else []))
        o += size
    assert len(raw) == o + 4 and struct.unpack("<i", raw[o:])[0] == 1   # 65 hypotheses made the mirror throw
    refs = HS.reference(True, sc, keys=keys)
    for pi, ref in enumerate(refs):
        rc = ref[0]
        assert int(n_corr[pi]) == rc["n_corr"], ("cpp", pi)
        for key in got:
            assert np.array_equal(HS.bits(got[key][pi]), HS.bits(rc[key][:N_HYP])), ("cpp", pi, key)
    assert got["rel_valid"].any() and got["rot_valid"].any()
