"""GPU: HipFrontend::uploadLandmarkTable and HipFrontend::matchToMapBlocks of the C++ host mirror
(okvis2_amd/host/okvfe_frontend.hpp), driven from a C++ program (tests/cpp/map_table_cli.cpp) on one small scene: a
table of 129 landmarks, four frames (the dictated frame, a frame seen from a moved pose, an empty frame, clutter),
against the per-frame reference of test_gpu_map_census.py (map_table_common.py).  Matches, status and obs_rows for
equality, projections as uint64 patterns; rows past a frame's keypoint count keep the driver's fill bytes."""
import os
import struct
import subprocess

import numpy as np
import pytest

import map_scenes as S
import map_table_common as M
from okvis2_amd import multigpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "cpp", "map_table_cli")
K = 256
FILL = np.frombuffer(b"\xf9" * 4, dtype=np.int32)[0]


@pytest.mark.parametrize("exclusive,thr", S.MODES)
def test_cpp_upload_landmark_table_and_match_to_map_blocks(oracle, tmp_path, exclusive, thr):
    assert os.path.exists(CLI), "run __graft_entry__.build() first"
    sc = S.packing_scene(129, "mixed")
    cam = sc["cam"]
    T1 = (np.asarray(sc["T1"][0], dtype=np.float64).reshape(-1), np.asarray(sc["T1"][1], dtype=np.float64))
    moved = (T1[0], T1[1] + np.array([0.05, -0.02, 0.01]))
    ref = M.reference(oracle, sc, T1, cam, exclusive, thr)
    kps, desc, use, want = S.dictated_frame(oracle, sc, ref, clutter=40)
    assert len(kps) <= K and (want >= 0).sum() > 60
    empty = (kps[:0], desc[:0], use[:0])
    frames = [(kps, desc, use), (kps, desc, use), empty, M.clutter_frame(oracle, sc, K, 3)]
    poses = [T1, moved, moved, T1]
    a = M.table_arrays(sc)
    nl, nf = len(a["hp"]), len(frames)
    blocks = np.stack([multigpu.pack_block_host(K, k, d, np.zeros((len(k), 3)), np.zeros(len(k), np.uint8))
                       for k, d, _ in frames])
    use_all = np.zeros((nf, K), np.uint8)
    for f, fr in enumerate(frames):
        use_all[f, :len(fr[2])] = fr[2]
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
        for C, r in poses:
            f.write(np.concatenate([C, r]).astype(np.float64).tobytes())
        f.write(blocks.tobytes())
        f.write(use_all.tobytes())
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "okvis2_amd") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = subprocess.run([CLI, str(req), str(resp)], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(resp, "rb").read()
    sizes = [nf * K * 4, nf * K * 4, nf * nl * 4, nf * nl * 12, nf * nl * 16, 4]
    assert len(raw) == sum(sizes)
    parts, o = [], 0
    for n in sizes:
        parts.append(raw[o:o + n])
        o += n
    lm = np.frombuffer(parts[0], np.int32).reshape(nf, K)
    bd = np.frombuffer(parts[1], np.int32).reshape(nf, K)
    status = np.frombuffer(parts[2], np.int32).reshape(nf, nl)
    rows = np.frombuffer(parts[3], np.int32).reshape(nf, nl, 3)
    proj = np.frombuffer(parts[4], np.float64).reshape(nf, nl, 2)
    assert struct.unpack("<i", parts[5])[0] == 1  # the malformed table made uploadLandmarkTable throw
    hits = 0
    for f, fr in enumerate(frames):
        r = M.reference(oracle, sc, poses[f], cam, exclusive, thr)
        n = len(fr[0])
        rl, rd = M.reference_matches(oracle, sc, r, thr, fr)
        assert np.array_equal(lm[f, :n], rl) and np.array_equal(bd[f, :n], rd), f
        assert np.all(lm[f, n:] == FILL) and np.all(bd[f, n:] == FILL), f
        assert np.array_equal(status[f], r["status"]) and np.array_equal(rows[f], r["obs_rows"]), f
        M.same_f64(proj[f], r["projection"], ("cpp", f))
        hits += int((rl >= 0).sum())
    told = want >= 0
    assert np.array_equal(lm[0, :len(want)][told], want[told]) and hits > 100
