"""GPU: okvfe_place_refine_blocks_device (k_place_refine.hip: the start, evaluation and step kernels around
place_refine_dev.h) against the restatement place_refine_ref.py, byte for byte and under both orders of the FP64 sums:
poses, start_poses, status, n_iterations, n_accepted, n_terms, cost and H as uint64 patterns (a NaN standing for any NaN),
no multiframe exempt; the rows of an unverified multiframe and two records behind every output keep their sentinels.
Scenes: every scene of test_place_refine_ref._scenes and the wild scene on the 8-coefficient model; the start given as a
pose; verdict_dev NULL; max_iterations 0 and 1; every optional output NULL in turn; the call twice on one stream; the 16
noisy and 16 far multiframes tiled to 63, 64, 65 and 257 (the lane and wave edges of the per-multiframe kernels); the
whole chain from descriptors on a side stream; argument errors; and the C++ mirror through tests/cpp/place_refine_cli."""
import dataclasses
import os
import struct
import subprocess

import numpy as np
import pytest

import batch_scale as BS
import gpu_common as G
import place_hessian_scenes as HS
import place_ref as P
import place_refine_device as RD
import place_refine_ref as PR
import place_refine_scenes as RS
import place_scenes as PS
import ransac_scenes as S
from okvis2_amd import capi, multigpu, synth

pytestmark = [pytest.mark.gpu]
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "cpp", "place_refine_cli")
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
    _SCENES.clear(), _REFS.clear(), _PREPARED.clear()
    torch.cuda.empty_cache()


def _tree(fp64_order):
    return fp64_order == "eigen_tree"


def _chunk():
    return capi.Frontend._test_place_hessian_chunk_terms()


# the scenes of test_place_refine_ref._scenes, by the name they carry there, and the wild scene on the RADTAN8 camera
SCENE_MAKERS = dict([("general-" + S.spec_id(spec), (lambda o, spec=spec: RS.general_scene(o, spec))) for spec in S.GENERAL_SPECS],
                    truth=RS.truth_scene, wild=RS.wild_scene, no_term=RS.no_term_scene, far=RS.far_scene,
                    noisy=RS.noisy_scene, term_count=lambda o: RS.term_count_scene(o, (_chunk() - 1, _chunk(), _chunk() + 1, 600)),
                    block_size=RS.block_size_scene, directed=RS.directed_scene, conversion=RS.conversion_scene,
                    wild_rt8=RS.wild_rt8_scene)
_SCENES, _REFS, _PREPARED = {}, {}, {}


def _scene(oracle, kind):
    """the scenes are built once and shared by the tests and both orders of the sums"""
    if kind not in _SCENES:
        _SCENES[kind] = SCENE_MAKERS[kind](oracle)
        _SCENES[kind]["key"] = kind
    return _SCENES[kind]


def _refs(oracle, sc, tree, **kw):
    """... and so is the reference of a scene under an order and a variant"""
    key = (sc["key"], tree) + tuple(sorted(kw.items()))
    if key not in _REFS:
        _REFS[key] = RS.reference(oracle, tree, sc, **kw)
    return _REFS[key]


def _prepared(sc):
    """the device tensors of a scene, uploaded once; the outputs are refilled with sentinels before every call"""
    if sc["key"] not in _PREPARED:
        fe = _frontend(sc["cams"])
        assert fe.max_keypoints == HS.K
        _PREPARED[sc["key"]] = (fe, RD.prepare(fe, sc))
    fe, T = _PREPARED[sc["key"]]
    RD.fresh_outputs(T, len(sc["mfs"]))
    return fe, T


def _run(oracle, sc, tree, what, without=(), stream=None, **kw):
    refs = _refs(oracle, sc, tree, **kw)
    fe, T = _prepared(sc)
    RD.launch(fe, sc, T, without=without, stream=stream, **kw)
    if stream is not None:
        stream.synchronize()
    return refs, RD.check(RD.download(T), refs, what, without=without)


@pytest.mark.parametrize("kind", list(SCENE_MAKERS))
def test_scenes(oracle, fp64_order, kind):
    sc = _scene(oracle, kind)
    refs, got = _run(oracle, sc, _tree(fp64_order), (sc["name"], fp64_order))
    statuses = [r["status"] for r in refs]
    if kind.startswith("general"):
        assert len(refs) in (1, 3, 17) and (1 in statuses or 2 in statuses)
    if kind == "term_count":
        assert got["n_terms_out"][:4].tolist() == [_chunk() - 1, _chunk(), _chunk() + 1, 600]
    if kind == "block_size":
        assert got["n_terms_out"][:5].tolist() == [1 + HS.K, HS.K + 1, 1 + HS.K, 0, 3] and statuses[3] == 3
    if kind == "no_term":
        assert statuses == [3] * 16 + [0] * 8
    if kind == "directed":
        assert statuses == [4, 0, 0, 4] + [4] * RS.BAD_BEST
        assert np.isnan(got["poses_out"][4:4 + RS.BAD_BEST]).all() and not np.isnan(got["poses_out"][0]).any()
        assert got["n_terms_out"][4] == got["n_terms_out"][3] > 0          # a bad winner is still evaluated
    if kind in ("far", "wild"):
        assert any(r["n_accepted"] < r["n_iterations"] for r in refs)
    if kind == "far":
        assert sc["max_iterations"] == 20
    if kind == "noisy":
        assert all(s in (1, 2) for s in statuses) and 1 in statuses and min(r["n_accepted"] for r in refs) >= 1
    if kind == "conversion":
        assert len(refs) == 64


def test_start_given_as_a_pose(oracle, fp64_order):
    """initial_poses_dev in place of the hypotheses, which are NULL: an unnormalised quaternion is a start like any other"""
    base = _scene(oracle, "noisy")
    sc = dict(base, key="noisy-initial", mfs=[dict(mf, initial=np.concatenate([
        PR.start_pose(mf["hyp"][mf["best"]])[:3], (1.0 + 0.25 * i) * PR.start_pose(mf["hyp"][mf["best"]])[3:]]))
        for i, mf in enumerate(base["mfs"])])
    _SCENES.setdefault(sc["key"], sc)
    sc = _SCENES[sc["key"]]
    refs, got = _run(oracle, sc, _tree(fp64_order), (sc["key"], fp64_order), use_initial=True)
    assert all(HS.same_bytes(r["start_pose"], mf["initial"]) for r, mf in zip(refs, sc["mfs"]))
    assert all(r["status"] in (1, 2) for r in refs)


@pytest.mark.parametrize("kind", ["directed", "no_term"])
def test_verdict_null(oracle, fp64_order, kind):
    """verdict_dev NULL: every multiframe counts"""
    sc = _scene(oracle, kind)
    refs, got = _run(oracle, sc, _tree(fp64_order), (sc["name"], fp64_order, "verdict NULL"), use_verdict=False)
    assert 0 not in [r["status"] for r in refs] and 0 in [r["status"] for r in _refs(oracle, sc, _tree(fp64_order))]


@pytest.mark.parametrize("max_iterations", [0, 1])
def test_iteration_limits(oracle, fp64_order, max_iterations):
    sc = _scene(oracle, "noisy")
    refs, got = _run(oracle, sc, _tree(fp64_order), (sc["name"], fp64_order, max_iterations), max_iterations=max_iterations)
    assert got["n_iterations"][:len(refs)].tolist() == [max_iterations] * len(refs)
    assert [r["status"] for r in refs] == [2] * len(refs)
    if max_iterations == 0:
        assert HS.same_bytes(got["poses_out"][:len(refs)], got["start_poses"][:len(refs)])


def test_optional_outputs_and_the_call_twice(oracle, fp64_order):
    """every optional output NULL in turn (it keeps its sentinels, the others their bytes); then the call twice on one
    stream without a wait in between: the workspace is reused in order and the bytes are the same"""
    tree = _tree(fp64_order)
    sc = _SCENES.setdefault("general-5", dict(RS.general_scene(oracle, ("euroc", "euroc1"), n_mf=5), key="general-5"))
    assert [mf["verdict"] for mf in sc["mfs"]][2] != 3
    for key in RD.OPTIONAL:
        _run(oracle, sc, tree, (sc["name"], fp64_order, "without", key), without=(key,))
    _run(oracle, sc, tree, (sc["name"], fp64_order, "required only"), without=RD.OPTIONAL)
    refs = _refs(oracle, sc, tree)
    fe, T = _prepared(sc)
    stream = torch.cuda.Stream()
    T2 = RD.fresh_outputs(dict(T), len(refs))
    RD.launch(fe, sc, T, stream=stream)
    RD.launch(fe, sc, T2, stream=stream)
    stream.synchronize()
    first, second = RD.download(T), RD.download(T2)
    RD.check(first, refs, (sc["name"], fp64_order, "first of two"))
    RD.check(second, refs, (sc["name"], fp64_order, "second of two"))
    assert all(np.array_equal(first[k].view(np.uint8), second[k].view(np.uint8)) for k in RD.OUTPUTS)


def test_lane_and_wave_edges(oracle, fp64_order):
    """the 16 noisy and 16 far multiframes (one rig, one landmark table) tiled to 63, 64, 65 and 257 multiframes, in the
    modular order and in a shuffle that moves every index: a lane per multiframe in work-groups of one wave"""
    tree = _tree(fp64_order)
    noisy, far = _scene(oracle, "noisy"), _scene(oracle, "far")
    assert np.array_equal(noisy["hp"], far["hp"]) and np.array_equal(noisy["T_SC_params"], far["T_SC_params"])
    both = _SCENES.setdefault("noisy+far", dict(far, key="noisy+far", name="noisy+far", mfs=noisy["mfs"] + far["mfs"]))
    assert both["max_iterations"] == 20 and len(both["mfs"]) == 32
    refs = _refs(oracle, both, tree)                                # once per distinct multiframe
    assert {r["status"] for r in refs} <= {1, 2} and any(r["n_accepted"] < r["n_iterations"] for r in refs)
    fe = _frontend(both["cams"])
    for n in (63, 64, 65, 257):
        for name, order in zip(("modular", "shuffled"), BS.placements(n, len(refs))):
            sc, rf = BS.tile(both, n, refs, order)
            T = RD.prepare(fe, sc)
            RD.launch(fe, sc, T)
            RD.check(RD.download(T), rf, (both["name"], fp64_order, n, name))


def test_whole_chain_on_a_side_stream(oracle, fp64_order):
    """descriptors -> okvfe_verify_place_blocks_device -> claims -> consensus (best_hypothesis stays on the device) ->
    this call, queued on one side stream with nothing waited for in between; the result equals the chain of the references"""
    tree = _tree(fp64_order)
    sc = PS.general_scene(oracle, ("euroc", "euroc1"), tree, n_mf=7)   # (seven: three verified, one of them converges)
    cams = sc["cams"]
    fe = _frontend(cams, K=PS.K)
    fus = [c.fu for c in cams]
    prm = np.array([HS.pose7(T) for T in sc["T_SC"]])
    T = PS.prepare(fe, sc)
    T["pool"], T["desc_begin"] = S._dev(sc["set"]["pool"]), S._dev(sc["set"]["desc_begin"])
    T["kmin"].fill_(-5), T["dmin"].fill_(12345)
    B, nb, nh = len(sc["mfs"]), T["blocks"].shape[0], len(sc["mfs"][0]["H"])
    O = RD.fresh_outputs({}, B)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    md = fe.make_map_device(len(sc["set"]["ids"]), T["desc_begin"].data_ptr(), T["pool"].data_ptr())
    fe.verify_place_blocks_device(T["blocks"].data_ptr(), nb, md, T["kmin"].data_ptr(), T["dmin"].data_ptr(), stream)
    PS.launch_claims(fe, sc, T, stream)
    PS.launch_consensus(fe, sc, T, stream=stream)
    res = fe.make_place_refine_device(*[O[k].data_ptr() for k in RD.OUTPUTS])
    fe.place_refine_blocks_device(T["set"], T["blocks"].data_ptr(), B, [0, 1], prm, T["H"].data_ptr(), nh,
                                  T["best"].data_ptr(), None, T["ml"].data_ptr(), T["state"].data_ptr(),
                                  T["verdict"].data_ptr(), PR.MAX_ITERATIONS_DEFAULT, res, stream)
    stream.synchronize()
    got = PS.download(T)
    refs = []
    for mi, mf in enumerate(sc["mfs"]):
        cl, co = P.verify(tree, sc["hp"], mf["frames"], mf["kmin"], mf["dmin"], PS.MATCH_THRESHOLD, fus, sc["T_SC"], mf["H"],
                          mf["valid"], sc["min_inliers"])
        assert int(got["verdict"][mi]) == co["verdict"] and int(got["best"][mi]) == co["best"]
        refs.append(PR.refine(oracle, tree, sc["hp"], mf["frames"], cl["match_landmark"], co["state"], cams, prm,
                              np.asarray(mf["H"]).reshape(nh, 12), co["best"], None, PR.MAX_ITERATIONS_DEFAULT,
                              co["verdict"] == 3))
    RD.check(RD.download(O), refs, ("chain", fp64_order))
    assert {r["status"] for r in refs} == {0, 1, 2}


def test_argument_errors_and_an_empty_batch(oracle):
    sc = _SCENES.setdefault("general-2", dict(RS.general_scene(oracle, ("euroc", "euroc1"), n_mf=2), key="general-2"))
    fe, T = _prepared(sc)
    T["initial"] = T["poses"]
    p, q = T["poses_out"].data_ptr(), T["status"].data_ptr()
    res = fe.make_place_refine_device(p, q)
    good = dict(place_set=T["set"], blocks_ptr=T["blocks"].data_ptr(), n_multiframes=2, cam_ids=[0, 1],
                T_SC_params=sc["T_SC_params"], hypotheses_ptr=T["hyp"].data_ptr(), n_hyp=RS.N_HYP,
                best_hypothesis_ptr=T["best"].data_ptr(), initial_poses_ptr=None, match_landmark_ptr=T["ml"].data_ptr(),
                state_ptr=T["state"].data_ptr(), verdict_ptr=None, max_iterations=3, result=res)
    bad = (dict(place_set=None), dict(blocks_ptr=None), dict(n_multiframes=-1), dict(cam_ids=[], T_SC_params=[]),
           dict(cam_ids=[0, 1, 0], T_SC_params=np.zeros((3, 7))), dict(hypotheses_ptr=None), dict(best_hypothesis_ptr=None),
           dict(n_hyp=-1), dict(match_landmark_ptr=None), dict(state_ptr=None), dict(result=None), dict(max_iterations=-1),
           dict(max_iterations=65), dict(place_set=fe.make_place_set_device(-1, T["hp"].data_ptr())),
           dict(place_set=fe.make_place_set_device(5, None)), dict(result=fe.make_place_refine_device(None, q)),
           dict(result=fe.make_place_refine_device(p, None)))
    for change in bad:
        with pytest.raises(capi.OkvfeError) as e:
            fe.place_refine_blocks_device(**dict(good, **change))
        assert e.value.status == capi.ERR_INVALID_ARGUMENT, change
    # the hypotheses may be NULL if and only if the initial poses are given
    fe.place_refine_blocks_device(**dict(good, hypotheses_ptr=None, best_hypothesis_ptr=None, n_hyp=0, n_multiframes=0,
                                         initial_poses_ptr=T["initial"].data_ptr()))
    fe.place_refine_blocks_device(**dict(good, n_multiframes=0))
    torch.cuda.synchronize()
    got = RD.download(T)
    assert all(np.all(got[k] == fill) for k, (_, _, fill) in RD.OUTPUTS.items())
    fe.place_refine_blocks_device(**dict(good, max_iterations=64))  # the largest limit: 131 launches, most of them idle
    refs = _refs(oracle, sc, True, use_verdict=False, max_iterations=64)
    RD.check(RD.download(T), refs, ("64 iterations",), without=RD.OPTIONAL)
    assert max(r["n_iterations"] for r in refs) < 64
    half = _frontend(sc["cams"], n_set=1)  # a slot without intrinsics: the frame and the slot are named
    with pytest.raises(capi.OkvfeError) as e:
        half.place_refine_blocks_device(**good)
    assert e.value.status == capi.ERR_NOT_READY and "frame 1: camera slot 1" in str(e.value), str(e.value)


def test_cpp_mirror(oracle, tmp_path):
    """HipFrontend::verifyPlaceRefineBlocks through tests/cpp/place_refine_cli (a fresh process: the default order of
    the sums): the same bytes as the restatement; rows the call leaves alone keep the driver's fill bytes"""
    assert os.path.exists(CLI), "run __graft_entry__.build() first"
    sc = _SCENES.setdefault("general-nodist-3", dict(RS.general_scene(oracle, ("nodist",), n_mf=3), key="general-nodist-3"))
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
        f.write(struct.pack("<ii", RS.N_HYP, sc["max_iterations"]))
        f.write(np.stack([mf["hyp"] for mf in sc["mfs"]]).astype(np.float64).tobytes())
        f.write(np.array([mf["best"] for mf in sc["mfs"]], dtype=np.int32).tobytes())
        f.write(ml.tobytes() + st.tobytes())
        f.write(struct.pack("<i", 1))
        f.write(np.array([mf["verdict"] for mf in sc["mfs"]], dtype=np.uint8).tobytes())
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "okvis2_amd") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = subprocess.run([CLI, str(req), str(resp)], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(resp, "rb").read()
    sizes = [nf * 56, nf * 56, nf * 16, nf * 288, nf * 20, 4]
    assert len(raw) == sum(sizes)
    parts, o = [], 0
    for n in sizes:
        parts.append(raw[o:o + n])
        o += n
    poses, starts = (np.frombuffer(parts[i], np.float64).reshape(nf, 7) for i in (0, 1))
    cost = np.frombuffer(parts[2], np.float64).reshape(nf, 2)
    H = np.frombuffer(parts[3], np.float64).reshape(nf, 6, 6)
    counts = np.frombuffer(parts[4], np.int32).reshape(5, nf)
    fill = np.frombuffer(b"\xf9" * 8, dtype=np.float64)[0]
    assert struct.unpack("<i", parts[5])[0] == 1  # a negative number of multiframes made the call throw
    for mi, ref in enumerate(refs):
        assert counts[:4, mi].tolist() == [ref["status"], ref["n_iterations"], ref["n_accepted"], ref["n_terms"]], mi
        assert HS.same_bytes(H[mi], ref["H"]) and HS.same_bytes(cost[mi], ref["cost"]), mi
        if ref["status"] == 0:
            assert np.all(poses[mi].view(np.uint64) == fill.view(np.uint64)), mi
            assert np.all(starts[mi].view(np.uint64) == fill.view(np.uint64)), mi
        else:
            assert HS.same_bytes(poses[mi], ref["pose"]) and HS.same_bytes(starts[mi], ref["start_pose"]), mi
    assert [r["status"] for r in refs][2] == 0 and refs[0]["status"] in (1, 2)
