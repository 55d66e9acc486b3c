"""GPU: the C++ host mirror (okvis2_amd/host/okvfe_frontend.hpp) of the pose hypotheses -- ransacHypothesesBlocks and
verifyPlaceHypothesesBlocks -- driven from a C++ program (tests/cpp/ransac_hyp_cli.cpp) on one stream: the multiframes of
a one-camera scene (the last with a gate of 0) give what the Python path gives, which test_gpu_ransac_hyp.py holds to
the restatement; here both are compared with the restatement directly.  Outputs byte for byte."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ransac_hyp_scenes as HS
import ransac_scenes as S
from okvis2_amd import multigpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "cpp", "ransac_hyp_cli")
K = S.K


def cli_env():
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "okvis2_amd") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return env


@pytest.mark.parametrize("with_keys", (False, True), ids=("index keys", "key array"))
def test_cpp_hypotheses(oracle, tmp_path, with_keys):
    assert os.path.exists(CLI), "run __graft_entry__.build() first"
    oracle.set_reduction(True)                          # (a fresh process: the default order of the sums)
    sc = S.general_scene(oracle, ("nodist",))
    cam, nf, nh = sc["cams"][0], len(sc["mfs"]), HS.N_HYP
    frames = [mf["frames"][0] for mf in sc["mfs"]]
    gates = [2] * (nf - 1) + [0]
    keys = [90 + 11 * i for i in range(nf)] if with_keys else list(range(nf))
    blocks = np.stack([multigpu.pack_block_host(K, fr["kps"], fr["desc"], fr["bp"], fr["bpv"]) for fr in frames])
    rows = np.full((nf, K), S.PAST_COUNT_ROW, np.int32)
    for i, fr in enumerate(frames):
        rows[i, :len(fr["lm"])] = fr["lm"]
    req, resp = tmp_path / "req.bin", tmp_path / "resp.bin"
    with open(req, "wb") as f:
        f.write(struct.pack("<iii", cam.w, cam.h, cam.dist_type))
        f.write(struct.pack("<8d", cam.fu, cam.fv, cam.cu, cam.cv, *cam.d[:4]))
        f.write(struct.pack("<6i", K, len(sc["hp"]), nf, blocks.shape[1], nh, int(with_keys)))
        f.write(sc["hp"].tobytes() + sc["obs_begin"].tobytes() + blocks.tobytes() + rows.tobytes())
        f.write(np.array(gates, np.uint8).tobytes())
        f.write(np.concatenate([np.asarray(sc["T_SC"][0][0]).reshape(-1), sc["T_SC"][0][1]]).astype(np.float64).tobytes())
        f.write(struct.pack("<Q", HS.SEED))
        if with_keys:
            f.write(np.array(keys, np.uint64).tobytes())
    out = subprocess.run([CLI, str(req), str(resp)], env=cli_env(), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(resp, "rb").read()
    sizes = [nf * nh * 96, nf * nh, nf * 4, nf * nh * 16, nf * nh * 4] * 2 + [4]
    assert len(raw) == sum(sizes)
    parts, o = [], 0
    for n in sizes:
        parts.append(raw[o:o + n])
        o += n
    assert struct.unpack("<i", parts[10])[0] == 1   # 65 hypotheses made ransacHypothesesBlocks throw
    for call, (place, g) in enumerate(((False, None), (True, gates))):
        refs = HS.reference(True, sc, nh, keys=keys, place=place, gates=g)
        p = parts[5 * call:5 * call + 5]
        H = np.frombuffer(p[0], np.float64).reshape(nf, nh, 12)
        valid = np.frombuffer(p[1], np.uint8).reshape(nf, nh)
        n_corr = np.frombuffer(p[2], np.int32)
        samples = np.frombuffer(p[3], np.int32).reshape(nf, nh, 4)
        n_sol = np.frombuffer(p[4], np.int32).reshape(nf, nh)
        for i, ref in enumerate(refs):
            w = ("cpp", "place" if place else "3d2d", i)
            assert HS.same_f64(H[i], ref["H"]) and np.array_equal(valid[i], ref["valid"]), w
            assert int(n_corr[i]) == ref["n_corr"] and np.array_equal(samples[i], ref["samples"]), w
            assert np.array_equal(n_sol[i], ref["n_solutions"]), w
        assert valid[0].any() and (not place or not valid[-1].any())
