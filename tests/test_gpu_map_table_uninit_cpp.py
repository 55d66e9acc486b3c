"""GPU: HipFrontend::matchToMapUninitialisedBlocks of the C++ host mirror (okvis2_amd/host/okvfe_frontend.hpp) after
HipFrontend::matchToMapBlocks on the same stream, driven from a C++ program (tests/cpp/map_table_uninit_cli.cpp) on
one small scene: a table of 129 landmarks and four frames (two of the scene's pose, one of a moved pose, an empty
one), against the per-frame reference of map_table_uninit_common.py.  Landmark, distance, hp_set and already_matched
for equality, hps_W as uint64 patterns; rows past a frame's keypoint count keep the driver's fill bytes."""
import os
import struct
import subprocess

import numpy as np
import pytest

import map_scenes as S
import map_table_common as M
import map_table_uninit_common as U
from okvis2_amd import multigpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "cpp", "map_table_uninit_cli")
K = 256
FILL = np.frombuffer(b"\xf9" * 4, dtype=np.int32)[0]


@pytest.mark.parametrize("exclusive,thr", S.MODES)
def test_cpp_match_to_map_uninitialised_blocks(oracle, tmp_path, exclusive, thr):
    assert os.path.exists(CLI), "run __graft_entry__.build() first"
    sc = S.packing_scene(129, "mixed")
    cam = sc["cam"]
    T1 = (np.asarray(sc["T1"][0], dtype=np.float64).reshape(-1), np.asarray(sc["T1"][1], dtype=np.float64))
    moved = (T1[0], T1[1] + np.array([0.05, -0.02, 0.01]))
    poses1 = [T1, T1, moved, moved]
    poses2 = [U.second_pose(p) for p in poses1]
    refs = [M.reference(oracle, sc, p, cam, exclusive, thr) for p in poses1]
    rows = int(refs[0]["n_desc"][refs[0]["status"] == 2].sum())
    assert 20 < rows < K - 40
    frames = [U.frame(oracle, sc, refs[0], cam, rows, K - rows, 1), U.frame(oracle, sc, refs[1], cam, rows, 30, 2),
              U.frame(oracle, sc, refs[2], cam, rows, 65 - min(rows, 65), 3), U.frame(oracle, sc, refs[3], cam, 0, 0, 4)]
    assert len(frames[0]["desc"]) == K and len(frames[3]["desc"]) == 0
    a = M.table_arrays(sc)
    nl, nf = len(a["hp"]), len(frames)
    blocks = np.stack([multigpu.pack_block_host(K, fr["kps"], fr["desc"], fr["bp"], fr["bv"]) for fr in frames])
    use = np.zeros((nf, K), np.uint8)
    prev = np.full((nf, K), -1, np.int32)
    for f, fr in enumerate(frames):
        use[f, :len(fr["use"])] = fr["use"]
        prev[f, :len(fr["previous"])] = fr["previous"]
    req, resp = tmp_path / "req.bin", tmp_path / "resp.bin"
    with open(req, "wb") as f:
        f.write(struct.pack("<iii", cam.w, cam.h, cam.dist_type))
        f.write(struct.pack("<8d", cam.fu, cam.fv, cam.cu, cam.cv, *cam.d[:4]))
        f.write(struct.pack("<iii", K, M.THRESHOLD, int(exclusive)))
        f.write(struct.pack("<d", thr))
        f.write(struct.pack("<iii", nl, len(a["obs_pose"]), len(a["poses"])))
        for k in ("hp", "quality", "obs_begin", "obs_pose", "obs_desc", "obs_bp", "poses"):
            f.write(a[k].tobytes())
        f.write(struct.pack("<ii", nf, blocks.shape[1]))
        for C, r in poses1 + poses2:
            f.write(np.concatenate([C, r]).astype(np.float64).tobytes())
        f.write(blocks.tobytes())
        f.write(use.tobytes())
        f.write(prev.tobytes())
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "okvis2_amd") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = subprocess.run([CLI, str(req), str(resp)], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(resp, "rb").read()
    sizes = [nf * K * 4, nf * nl * 4, nf * K * 4, nf * K * 4, nf * K * 32, nf * K, nf * 4, 4]
    assert len(raw) == sum(sizes)
    parts, o = [], 0
    for n in sizes:
        parts.append(raw[o:o + n])
        o += n
    status = np.frombuffer(parts[1], np.int32).reshape(nf, nl)
    got = dict(lm2=np.frombuffer(parts[2], np.int32).reshape(nf, K), bd2=np.frombuffer(parts[3], np.int32).reshape(nf, K),
               hp=np.frombuffer(parts[4], np.float64).reshape(nf, K, 4), hs=np.frombuffer(parts[5], np.uint8).reshape(nf, K),
               ctr=np.frombuffer(parts[6], np.int32))
    assert struct.unpack("<i", parts[7])[0] == 1  # a pose too many made matchToMapUninitialisedBlocks throw
    hits = 0
    for f, fr in enumerate(frames):
        n = len(fr["desc"])
        assert np.array_equal(status[f], refs[f]["status"]), f
        rl, rd, hp, hs, ctr = U.reference(oracle, sc["obs_desc"], refs[f], fr, poses2[f], cam, exclusive)
        assert np.array_equal(got["lm2"][f, :n], rl) and np.array_equal(got["bd2"][f, :n], rd), f
        assert np.array_equal(got["hs"][f, :n], hs) and int(got["ctr"][f]) == ctr, f
        M.same_f64(got["hp"][f, :n], hp, ("cpp", f))
        assert np.all(got["lm2"][f, n:] == FILL) and np.all(got["bd2"][f, n:] == FILL), f
        assert np.all(got["hs"][f, n:] == 0xF9), f
        hits += int((rl >= 0).sum())
    assert hits > 30
