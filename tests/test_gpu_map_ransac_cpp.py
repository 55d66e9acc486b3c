"""GPU: the C++ host mirror (okvis2_amd/host/okvfe_frontend.hpp) of the whole matchToMap chain -- matchToMapBlocks,
ransac3d2dBlocks with landmark_out in place, removeOutliersBlocks in place, matchToMapUninitialisedBlocks with the
filtered rows as `previous` -- driven from a C++ program (tests/cpp/map_ransac_cli.cpp) on one stream: three frames of
one camera (each a multiframe of its own; the last one empty) against the reference chain of
ransac_scenes.chain_scene.  Integers for equality, distances and hps_W as uint64 patterns; rows past a frame's keypoint
count keep the driver's fill bytes."""
import os
import struct
import subprocess

import numpy as np
import pytest

import map_scenes
import map_table_common as M
import ransac_scenes as S
from gate_scenes import rodrigues
from okvis2_amd import multigpu, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "cpp", "map_ransac_cli")
K = 512
FILL = np.frombuffer(b"\xf9" * 4, dtype=np.int32)[0]


def write_request(path, ch, exclusive, thr, kp_cap=K):
    """the request file of map_ransac_cli for the blocks of a one-camera chain scene"""
    cam, frames = ch["cams"][0], ch["frames"]
    a = M.table_arrays(ch["sc"])
    nf = len(frames)
    L = multigpu.block_layout(kp_cap)
    blocks = np.stack([multigpu.pack_block_host(kp_cap, fr["kps"], fr["desc"], fr["bp"], fr["bv"]) for fr in frames])
    use = np.zeros((nf, kp_cap), np.uint8)
    for f, fr in enumerate(frames):
        use[f, :len(fr["use"])] = fr["use"]
    with open(path, "wb") as f:
        f.write(struct.pack("<iii", cam.w, cam.h, cam.dist_type))
        f.write(struct.pack("<8d", cam.fu, cam.fv, cam.cu, cam.cv, *cam.d[:4]))
        f.write(struct.pack("<iii", kp_cap, M.THRESHOLD, int(exclusive)))
        f.write(struct.pack("<d", thr))
        f.write(struct.pack("<iii", len(a["hp"]), len(a["obs_pose"]), len(a["poses"])))
        for k in ("hp", "quality", "obs_begin", "obs_pose", "obs_desc", "obs_bp", "poses"):
            f.write(a[k].tobytes())
        f.write(struct.pack("<iiiii", nf, blocks.shape[1], L["kps"], L["bp"], L["bpv"]))
        for C, r in ch["poses1"] + ch["poses2"]:
            f.write(np.concatenate([np.asarray(C).reshape(-1), r]).astype(np.float64).tobytes())
        f.write(blocks.tobytes())
        f.write(use.tobytes())
        f.write(np.concatenate([np.asarray(ch["T_SC"][0][0]).reshape(-1), ch["T_SC"][0][1]]).astype(np.float64).tobytes())
        f.write(struct.pack("<i", ch["H"].shape[1]))
        f.write(np.ascontiguousarray(ch["H"], dtype=np.float64).tobytes())
    return len(a["hp"]), nf


def mono_chain(oracle, tree, exclusive, thr, sizes=((120, 200), (60, 150), (0, 0))):
    T_SC = [(rodrigues((0, 1, 0), 0.01).reshape(-1), np.array([0.05, 0.0, 0.01]))]
    return S.chain_scene(oracle, tree, exclusive, thr, cams=[synth.euroc_config().cams[0]], T_SC=T_SC, sizes=sizes)


def cli_env():
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "okvis2_amd") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return env


@pytest.mark.parametrize("exclusive,thr", map_scenes.MODES)
def test_cpp_chain(oracle, tmp_path, exclusive, thr):
    assert os.path.exists(CLI), "run __graft_entry__.build() first"
    ch = mono_chain(oracle, True, exclusive, thr)  # (a fresh process: the default order of the sums)
    frames = ch["frames"]
    assert len(frames[2]["desc"]) == 0 and all(len(f["desc"]) <= K for f in frames)
    req, resp = tmp_path / "req.bin", tmp_path / "resp.bin"
    nl, nf = write_request(req, ch, exclusive, thr)
    nh = ch["H"].shape[1]
    out = subprocess.run([CLI, str(req), str(resp)], env=cli_env(), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(resp, "rb").read()
    sizes = [nf * K * 4, nf * 12, nf, nf * nh * 4, nf * K, nf * K * 8, nf * 4, nf * K * 4, nf * K * 4, nf * K * 32, nf * K,
             nf * 4, 4]
    assert len(raw) == sum(sizes)
    parts, o = [], 0
    for n in sizes:
        parts.append(raw[o:o + n])
        o += n
    I = lambda i, *shape: np.frombuffer(parts[i], np.int32).reshape(*shape)
    lm, head, acc, hyp = I(0, nf, K), I(1, 3, nf), np.frombuffer(parts[2], np.uint8), I(3, nf, nh)
    state, dist = np.frombuffer(parts[4], np.uint8).reshape(nf, K), np.frombuffer(parts[5], np.float64).reshape(nf, K)
    kept = I(6, nf)
    got = dict(lm2=I(7, nf, K), bd2=I(8, nf, K), hp=np.frombuffer(parts[9], np.float64).reshape(nf, K, 4),
               hs=np.frombuffer(parts[10], np.uint8).reshape(nf, K), ctr=I(11, nf))
    assert struct.unpack("<i", parts[12])[0] == 1  # a hypothesis count that does not fit made ransac3d2dBlocks throw
    accepted = 0
    for f, fr in enumerate(frames):
        n, cons = len(fr["desc"]), ch["cons"][f]
        assert (head[0, f], head[1, f], head[2, f], acc[f]) == (cons["n_corr"], cons["best"], cons["n_inliers"], cons["accepted"]), f
        assert np.array_equal(hyp[f], cons["hyp_inliers"]), f
        assert np.array_equal(state[f, :n], cons["state"][0]) and np.all(state[f, n:] == 0xF9), f
        ds = cons["dist_set"][0]
        assert np.array_equal(dist[f, :n][ds].view(np.uint64), cons["distance"][0][ds].view(np.uint64)), f
        filtered, k = ch["removed"][f]
        assert np.array_equal(lm[f, :n], filtered) and np.all(lm[f, n:] == FILL) and kept[f] == k, f
        rl, rd, hp, hs, ctr = ch["second"][f]
        assert np.array_equal(got["lm2"][f, :n], rl) and np.array_equal(got["bd2"][f, :n], rd), f
        assert np.array_equal(got["hs"][f, :n], hs) and int(got["ctr"][f]) == ctr, f
        M.same_f64(got["hp"][f, :n], hp, ("cpp", f))
        assert np.all(got["lm2"][f, n:] == FILL) and np.all(got["hs"][f, n:] == 0xF9), f
        accepted += cons["accepted"]
    assert accepted >= 1 and ch["cons"][2]["n_corr"] == 0
