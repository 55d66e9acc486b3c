"""GPU: the C++ host mirror (okvis2_amd/host/okvfe_frontend.hpp) of the loop-closure verification -- placeLandmarkSet,
uploadPlaceSet, verifyPlaceClaimsBlocks (descriptor matching + claims), verifyPlaceConsensusBlocks -- driven from a C++
program (tests/cpp/place_verify_cli.cpp) on one stream: the frames of the one-camera general scenes of place_scenes.py
(each frame a multiframe of its own), equal to what the Python path is held to (place_ref.py): integers for equality,
doubles as uint64 patterns; rows past a frame's keypoint count keep the driver's fill bytes."""
import os
import struct
import subprocess

import numpy as np
import pytest

import place_ref as P
import place_scenes as PS
from okvis2_amd import multigpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "cpp", "place_verify_cli")
K = PS.K
FILL = np.frombuffer(b"\xf9" * 4, dtype=np.int32)[0]


def write_request(path, sc, with_valid):
    cam, old = sc["cams"][0], sc["old"][0]
    frames = [mf["frames"][0] for mf in sc["mfs"]]
    blocks = np.stack([multigpu.pack_block_host(K, fr["kps"], fr["desc"], fr["bp"], fr["bpv"]) for fr in frames])
    C, r = sc["T_SC"][0]
    with open(path, "wb") as f:
        f.write(struct.pack("<iii", cam.w, cam.h, cam.dist_type))
        f.write(struct.pack("<8d", cam.fu, cam.fv, cam.cu, cam.cv, *cam.d[:4]))
        f.write(struct.pack("<iii", K, PS.MATCH_THRESHOLD, sc["min_inliers"]))
        f.write(struct.pack("<i", len(old["ids"])))
        for k in ("ids", "hp", "init", "desc"):
            f.write(np.ascontiguousarray(old[k]).tobytes())
        f.write(struct.pack("<ii", len(frames), blocks.shape[1]))
        f.write(blocks.tobytes())
        f.write(np.concatenate([np.asarray(C).reshape(-1), r]).astype(np.float64).tobytes())
        f.write(struct.pack("<ii", len(sc["mfs"][0]["H"]), int(with_valid)))
        f.write(np.stack([mf["H"] for mf in sc["mfs"]]).astype(np.float64).tobytes())
        if with_valid:
            f.write(np.stack([mf["valid"] for mf in sc["mfs"]]).astype(np.uint8).tobytes())


def cli_env():
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "okvis2_amd") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return env


@pytest.mark.parametrize("spec,with_valid", [(("nodist",), True), (("nodist",), False)], ids=["flags", "all-valid"])
def test_cpp_chain(oracle, tmp_path, spec, with_valid):
    assert os.path.exists(CLI), "run __graft_entry__.build() first"
    sc = PS.general_scene(oracle, spec, True)  # (a fresh process: the default order of the sums)
    req, resp = tmp_path / "req.bin", tmp_path / "resp.bin"
    write_request(req, sc, with_valid)
    out = subprocess.run([CLI, str(req), str(resp)], env=cli_env(), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(resp, "rb").read()
    L, rows = struct.unpack("<ii", raw[:8])
    nf, nh = len(sc["mfs"]), len(sc["mfs"][0]["H"])
    sizes = [L * 8, L * 32, (L + 1) * 4, rows * 48, nf * L * 4, nf * L * 4, nf * 12, nf, nf * K * 4, nf, nf * 12, nf,
             nf * nh * 4, nf * K, nf * K * 8, nf * K * 4, 4]
    assert len(raw) == 8 + sum(sizes)
    parts, o = [], 8
    for n in sizes:
        parts.append(raw[o:o + n])
        o += n
    I = lambda i, *shape: np.frombuffer(parts[i], np.int32).reshape(*shape)
    U8 = lambda i, *shape: np.frombuffer(parts[i], np.uint8).reshape(*shape)
    got_set = dict(ids=np.frombuffer(parts[0], np.uint64), hp=np.frombuffer(parts[1], np.float64).reshape(L, 4),
                   desc_begin=I(2, L + 1), pool=U8(3, rows, 48))
    PS.same_set(got_set, sc["set"], "cpp")
    kmin, dmin = I(4, nf, L), np.frombuffer(parts[5], np.uint32).reshape(nf, L)
    counts, gate, ml, verdict = I(6, 3, nf), U8(7, nf), I(8, nf, K), U8(9, nf)
    head, acc, hyp = I(10, 3, nf), U8(11, nf), I(12, nf, nh)
    state, dist, lo = U8(13, nf, K), np.frombuffer(parts[14], np.float64).reshape(nf, K), I(15, nf, K)
    assert struct.unpack("<i", parts[16])[0] == 1  # a hypothesis count that does not fit made the consensus call throw
    verdicts = []
    for f, mf in enumerate(sc["mfs"]):
        cl, co = P.verify(True, sc["hp"], mf["frames"], mf["kmin"], mf["dmin"], PS.MATCH_THRESHOLD, [sc["cams"][0].fu],
                          sc["T_SC"], mf["H"], mf["valid"] if with_valid else None, sc["min_inliers"])
        n = len(mf["frames"][0]["kps"])
        assert np.array_equal(kmin[f], mf["kmin"][0]) and np.array_equal(dmin[f], mf["dmin"][0]), f
        assert (counts[0, f], counts[1, f], counts[2, f], gate[f]) == (cl["n_matches"], cl["n_points"], cl["n_corr"], cl["gate"]), f
        assert np.array_equal(ml[f, :n], cl["match_landmark"][0]) and np.all(ml[f, n:] == FILL), f
        assert (verdict[f], head[0, f], head[1, f], head[2, f], acc[f]) == \
            (co["verdict"], co["n_corr"], co["best"], co["n_inliers"], co["accepted"]), f
        assert np.array_equal(hyp[f], co["hyp_inliers"]), f
        assert np.array_equal(state[f, :n], co["state"][0]) and np.all(state[f, n:] == 0xF9), f
        ds = co["dist_set"][0]
        assert np.array_equal(dist[f, :n][ds].view(np.uint64), co["distance"][0][ds].view(np.uint64)), f
        assert np.array_equal(lo[f, :n], co["landmark_out"][0]) and np.all(lo[f, n:] == FILL), f
        verdicts.append(co["verdict"])
    assert 3 in verdicts
