"""GPU: okvfe_place_hessian_blocks_device (place_hessian_kernel) against the restatement place_hessian_ref.py, byte for
byte and under both orders of the FP64 sums: H, n_terms, n_singular and the optional residual and minimal-Jacobian rows
as uint64 patterns (a NaN standing for any NaN), no term exempt; rows that are no terms keep their sentinels.  Scenes:
place_hessian_scenes.py (rigs of 1, 2 and 5 cameras over the four camera models in batches of 1, 3 and 17; the directed
scene of the census; term counts around the kernel's chunk; blocks of 0, 1 and K keypoints; odd poses), the whole chain
from descriptors on a side stream, and the C++ mirror through tests/cpp/place_hessian_cli."""
import dataclasses
import os
import struct
import subprocess

import numpy as np
import pytest

import gpu_common as G
import place_hessian_ref as PH
import place_hessian_scenes as HS
import place_ref as P
import place_scenes as PS
import ransac_scenes as S
from okvis2_amd import capi, multigpu, synth

pytestmark = [pytest.mark.gpu]
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "cpp", "place_hessian_cli")
_FRONTENDS = {}


def _frontend(cams, n_set=None, K=HS.K):
    """a context of the first camera's size with K keypoints whose first n_set slots hold `cams`"""
    n_set = len(cams) if n_set is None else n_set
    key = tuple((c.w, c.h, c.fu, c.fv, c.cu, c.cv, c.dist_type, tuple(c.d)) for c in cams) + (n_set, K)
    if key not in _FRONTENDS:
        cfg = dataclasses.replace(synth.euroc_config(), w=cams[0].w, h=cams[0].h, cams=list(cams), max_kpts=K)
        fe = G.make_frontend(cfg)
        for i, c in enumerate(cams[:n_set]):
            fe.set_camera(i, c)
        _FRONTENDS[key] = fe
    return _FRONTENDS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_frontends():
    yield
    while _FRONTENDS:
        _FRONTENDS.popitem()[1].close()


def _tree(fp64_order):
    return fp64_order == "eigen_tree"


_SCENES, _REFS = {}, {}


def _scene(oracle, kind, *args):
    """the scenes are built once and shared by the tests and both orders of the sums"""
    key = (kind,) + args
    if key not in _SCENES:
        _SCENES[key] = getattr(HS, kind + "_scene")(oracle, *args)
        _SCENES[key]["key"] = key
    return _SCENES[key]


def _refs(oracle, sc, tree, use_verdict=True):
    """... and so is the reference of a scene under an order"""
    key = (sc["key"], tree, use_verdict)
    if key not in _REFS:
        _REFS[key] = HS.reference(oracle, tree, sc, use_verdict)
    return _REFS[key]


def _run(oracle, sc, tree, what, use_verdict=True, optional=True, residual=True, jacobian=True):
    fe = _frontend(sc["cams"])
    assert fe.max_keypoints == HS.K
    refs = _refs(oracle, sc, tree, use_verdict)
    T = HS.prepare(fe, sc, optional=optional)
    HS.launch(fe, sc, T, use_verdict=use_verdict, residual=residual, jacobian=jacobian)
    return refs, HS.check(sc, T, refs, what, residual=residual, jacobian=jacobian)


@pytest.mark.parametrize("spec", S.GENERAL_SPECS, ids=S.spec_id)
def test_general_scenes(oracle, fp64_order, spec):
    """rigs of 1, 2 and 5 cameras over the four camera models, batches of 1, 3 and 17 multiframes"""
    sc = _scene(oracle, "general", spec)
    refs, got = _run(oracle, sc, _tree(fp64_order), (sc["name"], fp64_order))
    assert len(refs) == HS.BATCH[spec] and refs[0]["n_terms"] >= 16
    assert not np.isnan(got["H"]).any() and np.all(got["H"][[mf["verdict"] != 3 for mf in sc["mfs"]]] == 0.0)


def test_directed_scene_of_the_census(oracle, fp64_order):
    tree = _tree(fp64_order)
    sc = _scene(oracle, "directed")
    refs, got = _run(oracle, sc, tree, (sc["name"], fp64_order))
    n_cams = len(sc["cams"])
    assert got["n_terms"].tolist() == [n_cams * HS.COPIES * 16, 0, 0, n_cams * HS.COPIES * 16]
    assert got["n_singular"].tolist() == [n_cams * HS.COPIES * 5, 0, 0, n_cams * HS.COPIES * 4]
    assert np.isnan(got["H"][0]).all() and not got["H"][1:3].any()
    # verdict_dev NULL: every multiframe counts
    refs, got = _run(oracle, sc, tree, (sc["name"], fp64_order, "verdict NULL"), use_verdict=False)
    assert got["n_terms"].tolist() == [n_cams * HS.COPIES * 16] * 4


def test_ring_edges(oracle, fp64_order):
    chunk = capi.Frontend._test_place_hessian_chunk_terms()
    totals = (chunk - 1, chunk, chunk + 1, 600)
    sc = _scene(oracle, "term_count", totals)
    refs, got = _run(oracle, sc, _tree(fp64_order), (sc["name"], fp64_order))
    assert got["n_terms"].tolist() == list(totals) and len(sc["cams"]) == 5
    sc = _scene(oracle, "block_size")
    refs, got = _run(oracle, sc, _tree(fp64_order), (sc["name"], fp64_order))
    assert got["n_terms"].tolist() == [1 + HS.K, HS.K + 1, 1 + HS.K, 0, 3] and not got["H"][3].any()


def test_optional_outputs(oracle, fp64_order):
    """outputs NULL; sentinel-filled outputs untouched at rows that are no terms and past a block's count (checked by
    every call of HS.check); unverified multiframes give zeros"""
    tree = _tree(fp64_order)
    sc = _scene(oracle, "general", ("euroc", "euroc1"), 5)
    what = (sc["name"], fp64_order)
    _run(oracle, sc, tree, what + ("H and counts only",), optional=False)
    _run(oracle, sc, tree, what + ("residual only",), jacobian=False)
    refs, got = _run(oracle, sc, tree, what + ("jacobian only",), residual=False)
    assert [mf["verdict"] for mf in sc["mfs"]][2] != 3 and not got["H"][2].any() and got["n_terms"][2] == 0


def test_poses(oracle, fp64_order):
    sc = _scene(oracle, "pose")
    refs, got = _run(oracle, sc, _tree(fp64_order), (sc["name"], fp64_order))
    H = got["H"]
    assert not np.isnan(H[:3]).any() and np.isnan(H[3]).any() and np.isnan(H[4]).all()
    assert got["n_singular"].tolist() == [0] * 5 and len(set(got["n_terms"].tolist())) == 1


def test_whole_chain_on_a_side_stream(oracle, fp64_order):
    """descriptors -> okvfe_verify_place_blocks_device -> claims -> consensus -> this call, queued on one side stream with
    nothing waited for in between; the result equals the chain of the references"""
    tree = _tree(fp64_order)
    sc = PS.general_scene(oracle, ("euroc", "euroc1"), tree)
    cams = sc["cams"]
    fe = _frontend(cams, K=PS.K)
    fus = [c.fu for c in cams]
    rng = np.random.default_rng(77)
    poses = np.stack([HS.refined(mf["T_WS"], rng) for mf in sc["mfs"]])
    prm = np.array([HS.pose7(T) for T in sc["T_SC"]])
    T = PS.prepare(fe, sc)
    T["pool"], T["desc_begin"] = S._dev(sc["set"]["pool"]), S._dev(sc["set"]["desc_begin"])
    T["kmin"].fill_(-5), T["dmin"].fill_(12345)
    B, nb = len(sc["mfs"]), T["blocks"].shape[0]
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
    T.update(poses=S._dev(poses), Hm=full((B, 36), HS.H_SENTINEL, torch.float64),
             n_terms=full((B,), HS.COUNT_SENTINEL, torch.int32), n_singular=full((B,), HS.COUNT_SENTINEL, torch.int32),
             residual=full((nb, PS.K, 2), HS.ROW_SENTINEL, torch.float64),
             jacobian=full((nb, PS.K, 12), HS.ROW_SENTINEL, torch.float64))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    md = fe.make_map_device(len(sc["set"]["ids"]), T["desc_begin"].data_ptr(), T["pool"].data_ptr())
    fe.verify_place_blocks_device(T["blocks"].data_ptr(), nb, md, T["kmin"].data_ptr(), T["dmin"].data_ptr(), stream)
    PS.launch_claims(fe, sc, T, stream)
    PS.launch_consensus(fe, sc, T, stream=stream)
    res = fe.make_place_hessian_device(T["Hm"].data_ptr(), T["n_terms"].data_ptr(), T["n_singular"].data_ptr(),
                                       T["residual"].data_ptr(), T["jacobian"].data_ptr())
    fe.place_hessian_blocks_device(T["set"], T["blocks"].data_ptr(), B, [0, 1], prm, T["poses"].data_ptr(),
                                   T["ml"].data_ptr(), T["state"].data_ptr(), T["verdict"].data_ptr(), res, stream)
    stream.synchronize()
    got = PS.download(T)
    verdicts = []
    for mi, mf in enumerate(sc["mfs"]):
        cl, co = P.verify(tree, sc["hp"], mf["frames"], mf["kmin"], mf["dmin"], PS.MATCH_THRESHOLD, fus, sc["T_SC"], mf["H"],
                          mf["valid"], sc["min_inliers"])
        ref = PH.evaluate(oracle, tree, sc["hp"], mf["frames"], cl["match_landmark"], co["state"], cams, prm, poses[mi],
                          co["verdict"] == 3)
        verdicts.append(co["verdict"])
        assert int(got["verdict"][mi]) == co["verdict"]
        assert (int(got["n_terms"][mi]), int(got["n_singular"][mi])) == (ref["n_terms"], ref["n_singular"]), mi
        assert ref["n_terms"] == (co["n_inliers"] if co["verdict"] == 3 else 0)
        assert HS.same_bytes(got["Hm"][mi].reshape(6, 6), ref["H"]), (mi, got["Hm"][mi], ref["H"])
        for c in range(len(cams)):
            b = mi * len(cams) + c
            term = np.zeros(PS.K, bool)
            term[ref["rows"][c]] = True
            assert HS.same_bytes(got["residual"][b][term], ref["residual"][c]), (mi, c)
            assert HS.same_bytes(got["jacobian"][b][term], ref["jacobian"][c]), (mi, c)
            assert np.all(got["residual"][b][~term] == HS.ROW_SENTINEL) and np.all(got["jacobian"][b][~term] == HS.ROW_SENTINEL)
    assert 3 in verdicts


def test_argument_errors_and_an_empty_batch(oracle):
    sc = _scene(oracle, "general", ("euroc", "euroc1"), 2)
    fe = _frontend(sc["cams"])
    T = HS.prepare(fe, sc)
    p = T["H"].data_ptr()
    res = fe.make_place_hessian_device(p, T["n_terms"].data_ptr(), T["n_singular"].data_ptr())
    good = dict(place_set=T["set"], blocks_ptr=T["blocks"].data_ptr(), n_multiframes=2, cam_ids=[0, 1],
                T_SC_params=sc["T_SC_params"], poses_ptr=T["poses"].data_ptr(), match_landmark_ptr=T["ml"].data_ptr(),
                state_ptr=T["state"].data_ptr(), verdict_ptr=None, result=res)
    bad = (dict(place_set=None), dict(blocks_ptr=None), dict(n_multiframes=-1), dict(cam_ids=[], T_SC_params=[]),
           dict(cam_ids=[0, 1, 0], T_SC_params=np.zeros((3, 7))), dict(poses_ptr=None), dict(match_landmark_ptr=None),
           dict(state_ptr=None), dict(result=None), dict(place_set=fe.make_place_set_device(-1, T["hp"].data_ptr())),
           dict(place_set=fe.make_place_set_device(5, None)), dict(result=fe.make_place_hessian_device(None, p, p)),
           dict(result=fe.make_place_hessian_device(p, None, p)), dict(result=fe.make_place_hessian_device(p, p, None)))
    for change in bad:
        with pytest.raises(capi.OkvfeError) as e:
            fe.place_hessian_blocks_device(**dict(good, **change))
        assert e.value.status == capi.ERR_INVALID_ARGUMENT, change
    fe.place_hessian_blocks_device(**dict(good, n_multiframes=0))
    torch.cuda.synchronize()
    assert np.all(T["H"].cpu().numpy() == HS.H_SENTINEL) and np.all(T["n_terms"].cpu().numpy() == HS.COUNT_SENTINEL)
    assert np.all(T["residual"].cpu().numpy() == HS.ROW_SENTINEL)
    half = _frontend(sc["cams"], n_set=1)  # a slot without intrinsics: the frame and the slot are named
    with pytest.raises(capi.OkvfeError) as e:
        half.place_hessian_blocks_device(**good)
    assert e.value.status == capi.ERR_NOT_READY and "frame 1: camera slot 1" in str(e.value), str(e.value)


def test_cpp_mirror(oracle, tmp_path):
    """HipFrontend::verifyPlaceHessianBlocks through tests/cpp/place_hessian_cli (a fresh process: the default order of
    the sums): the same bytes as the restatement; rows the call leaves alone keep the driver's fill bytes"""
    assert os.path.exists(CLI), "run __graft_entry__.build() first"
    sc = _scene(oracle, "general", ("nodist",), 3)
    refs = _refs(oracle, sc, True)
    cam, K, nf = sc["cams"][0], HS.K, len(sc["mfs"])
    frames = [mf["frames"][0] for mf in sc["mfs"]]
    blocks = np.stack([multigpu.pack_block_host(K, fr["kps"], fr["desc"], fr["bp"], fr["bpv"]) for fr in frames])
    ml, st = np.full((nf, K), S.PAST_COUNT_ROW, np.int32), np.full((nf, K), 2, np.uint8)
    for b, mf in enumerate(sc["mfs"]):
        ml[b, :len(mf["ml"][0])], st[b, :len(mf["state"][0])] = mf["ml"][0], mf["state"][0]
    req, resp = tmp_path / "req.bin", tmp_path / "resp.bin"
    with open(req, "wb") as f:
        f.write(struct.pack("<iii", cam.w, cam.h, cam.dist_type))
        f.write(struct.pack("<8d", cam.fu, cam.fv, cam.cu, cam.cv, *cam.d[:4]))
        f.write(struct.pack("<ii", K, len(sc["hp"])))
        f.write(sc["hp"].tobytes())
        f.write(struct.pack("<ii", nf, blocks.shape[1]))
        f.write(blocks.tobytes())
        f.write(sc["T_SC_params"][0].astype(np.float64).tobytes())
        f.write(np.stack([mf["pose"] for mf in sc["mfs"]]).astype(np.float64).tobytes())
        f.write(ml.tobytes() + st.tobytes())
        f.write(struct.pack("<i", 1))
        f.write(np.array([mf["verdict"] for mf in sc["mfs"]], dtype=np.uint8).tobytes())
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "okvis2_amd") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = subprocess.run([CLI, str(req), str(resp)], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(resp, "rb").read()
    sizes = [nf * 288, nf * 8, nf * K * 16, nf * K * 96, 4]
    assert len(raw) == sum(sizes)
    parts, o = [], 0
    for n in sizes:
        parts.append(raw[o:o + n])
        o += n
    H = np.frombuffer(parts[0], np.float64).reshape(nf, 6, 6)
    counts = np.frombuffer(parts[1], np.int32).reshape(2, nf)
    res = np.frombuffer(parts[2], np.float64).reshape(nf, K, 2)
    jac = np.frombuffer(parts[3], np.float64).reshape(nf, K, 12)
    fill = np.frombuffer(b"\xf9" * 8, dtype=np.float64)[0]
    assert struct.unpack("<i", parts[4])[0] == 1  # a negative number of multiframes made the call throw
    for mi, ref in enumerate(refs):
        assert (int(counts[0, mi]), int(counts[1, mi])) == (ref["n_terms"], ref["n_singular"]), mi
        assert HS.same_bytes(H[mi], ref["H"]), mi
        term = np.zeros(K, bool)
        term[ref["rows"][0]] = True
        assert HS.same_bytes(res[mi][term], ref["residual"][0]) and HS.same_bytes(jac[mi][term], ref["jacobian"][0]), mi
        assert np.all(res[mi][~term].view(np.uint64) == fill.view(np.uint64)), mi
        assert np.all(jac[mi][~term].view(np.uint64) == fill.view(np.uint64)), mi
    assert refs[0]["n_terms"] >= 16 and refs[2]["n_terms"] == 0
