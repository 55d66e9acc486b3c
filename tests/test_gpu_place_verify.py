"""GPU: okvfe_place_claims_blocks_device (place_claims_kernel) and okvfe_place_consensus_blocks_device
(ransac_consensus_kernel under its kPlace policy) against the transcription place_ref.py, byte for byte and under both
orders of the FP64 sums: counts, gates, claimed rows, verdicts, states and landmark rows for equality, distances as
uint64 patterns, no row exempt; rows at or past a block's keypoint count keep their sentinels.  Scenes: place_scenes.py
(hand-built k_min / dist_min for the directed cases, the gate and verdict tables, the chunk and landmark-count edges;
one general scene per rig through the whole chain from descriptors; two candidate sets on one stream)."""
import dataclasses

import numpy as np
import pytest

import gpu_common as G
import place_ref as P
import place_scenes as PS
import ransac_scenes as S
from okvis2_amd import capi, synth

pytestmark = [pytest.mark.gpu]
torch = pytest.importorskip("torch")

_FRONTENDS = {}


def _frontend(cams, n_set=None):
    """a context of the first camera's size with K = ransac_scenes.K whose first n_set slots hold `cams`"""
    n_set = len(cams) if n_set is None else n_set
    key = tuple((c.w, c.h, c.fu, c.fv, c.cu, c.cv, c.dist_type, tuple(c.d)) for c in cams) + (n_set,)
    if key not in _FRONTENDS:
        cfg = dataclasses.replace(synth.euroc_config(), w=cams[0].w, h=cams[0].h, cams=list(cams), max_kpts=S.K)
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


def _chain(fe, sc, tree, what, optional=True, alias=False, with_gate=True, use_valid=True):
    """claims, then consensus on the claimed rows, each against the reference"""
    cl_refs = PS.claims_reference(sc)
    T = PS.prepare(fe, sc, optional=optional, alias=alias, with_gate=with_gate)
    PS.launch_claims(fe, sc, T)
    got = PS.download(T)
    PS.check_claims(sc, got, cl_refs, what)
    co_refs = PS.consensus_reference(tree, sc, [r["match_landmark"] for r in cl_refs],
                                     [r["gate"] for r in cl_refs] if with_gate else None, use_valid)
    PS.launch_consensus(fe, sc, T, use_valid=use_valid)
    got = PS.download(T)
    PS.check_consensus(sc, got, co_refs, what, alias=alias)
    return cl_refs, co_refs, got


def _consensus(fe, sc, tree, what, optional=True, alias=False, use_valid=True):
    """consensus alone on hand-built match_landmark rows (and gates, where the scene has them)"""
    gates = None if sc["mfs"][0]["gate"] is None else [mf["gate"] for mf in sc["mfs"]]
    refs = PS.consensus_reference(tree, sc, [mf["ml"] for mf in sc["mfs"]], gates, use_valid)
    T = PS.prepare(fe, sc, optional=optional, alias=alias)
    PS.launch_consensus(fe, sc, T, use_valid=use_valid)
    got = PS.download(T)
    PS.check_consensus(sc, got, refs, what, alias=alias)
    return refs, got


def test_directed_claims(oracle, fp64_order):
    tree = _tree(fp64_order)
    sc = PS.claims_scene(oracle)
    fe = _frontend(sc["cams"])
    assert fe.max_keypoints == PS.K
    cl, co, _ = _chain(fe, sc, tree, (sc["name"], fp64_order))
    assert cl[0]["gate"] == 2 and co[0]["verdict"] >= 2
    _chain(fe, sc, tree, (sc["name"], fp64_order, "in place"), alias=True)
    _chain(fe, sc, tree, (sc["name"], fp64_order, "verdicts only, gate NULL"), optional=False, with_gate=False)
    allsc = PS.collide_all_scene(oracle)
    cl, _, _ = _chain(fe, allsc, tree, (allsc["name"], fp64_order))
    assert all(r["n_matches"] == 2 * len(allsc["hp"]) for r in cl)


@pytest.mark.parametrize("min_inliers", sorted(PS.GATE_TABLE))
def test_gate_table(oracle, fp64_order, min_inliers):
    sc = PS.gate_scene(oracle, min_inliers)
    cl, co, got = _chain(_frontend(sc["cams"]), sc, _tree(fp64_order), (sc["name"], fp64_order))
    assert got["gate"].tolist() == [g for _, _, g in PS.GATE_TABLE[min_inliers]]
    assert [tuple(int(got[k][i]) for k in ("n_matches", "n_points", "n_corr_claims")) for i in range(len(cl))] == \
        [c for _, c, _ in PS.GATE_TABLE[min_inliers]]
    assert [min(int(v), 2) for v in got["verdict"]] == got["gate"].tolist()
    # without the gate the kernel's own count decides: a multiframe of gate 0 with seven correspondences is scored
    _chain(_frontend(sc["cams"]), sc, _tree(fp64_order), (sc["name"], fp64_order, "gate NULL"), with_gate=False)


def test_verdict_table(oracle, fp64_order):
    tree = _tree(fp64_order)
    far_twice = lambda T, rng: np.array([S.far_pose(T, rng)] * 2)
    thrice = lambda T, rng: np.array([S.pose_matrix(T), S.pose_matrix(T), S.far_pose(T, rng)])
    for min_inliers, table in PS.VERDICT_TABLE.items():
        sc = PS.verdict_scene(oracle, min_inliers, PS.true_first)
        fe = _frontend(sc["cams"])
        what = (sc["name"], fp64_order)
        refs, got = _consensus(fe, sc, tree, what)
        assert got["verdict"].tolist() == [v for _, v in table], (what, got["verdict"].tolist())
        assert got["n_corr"].tolist() == [n for (n, _), _ in table]
        assert got["n_inl"].tolist() == [i if v >= 2 else 0 for (_, i), v in table]
        assert got["accepted"].tolist() == [int(v == 3) for _, v in table]
        _consensus(fe, sc, tree, what + ("in place",), alias=True)
        _consensus(fe, sc, tree, what + ("verdicts only",), optional=False)
        refs, got = _consensus(fe, PS.verdict_scene(oracle, min_inliers, far_twice), tree, what + ("zero inliers",))
        assert got["best"].tolist() == [-1] * len(table) and set(got["verdict"].tolist()) <= {1, 2}
        refs, got = _consensus(fe, PS.verdict_scene(oracle, min_inliers, thrice, valid=np.array([0, 1, 1], np.uint8)), tree,
                               what + ("winner off",))
        assert got["best"].tolist() == [1 if v >= 2 else -1 for _, v in table]
        gates = [j % 3 for j in range(len(table))]
        refs, got = _consensus(fe, PS.verdict_scene(oracle, min_inliers, PS.true_first, gates=gates), tree, what + ("gates",))
        assert got["verdict"].tolist() == [0 if g == 0 else v for g, (_, v) in zip(gates, table)]


def test_chunk_edges(oracle, fp64_order):
    chunk = capi.Frontend._test_ransac_chunk_records()
    sc = PS.chunk_scene(oracle, chunk)
    refs, got = _consensus(_frontend(sc["cams"]), sc, _tree(fp64_order), (sc["name"], fp64_order))
    assert got["n_corr"].tolist() == [chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1]


@pytest.mark.parametrize("L", PS.L_EDGES)
def test_landmark_count_edges(oracle, fp64_order, L):
    sc = PS.landmark_count_scene(oracle, L)
    _chain(_frontend(sc["cams"]), sc, _tree(fp64_order), (sc["name"], fp64_order))


def _match_setup(sc, T):
    """the set's descriptors in device memory; k_min / dist_min overwritten with values no matcher writes (synchronises)"""
    T["pool"], T["desc_begin"] = S._dev(sc["set"]["pool"]), S._dev(sc["set"]["desc_begin"])
    T["kmin"].fill_(-5), T["dmin"].fill_(12345)
    torch.cuda.synchronize()


def _match(fe, sc, T, stream=None):
    """okvfe_verify_place_blocks_device over the scene's blocks into T's k_min / dist_min: the call alone"""
    md = fe.make_map_device(len(sc["set"]["ids"]), T["desc_begin"].data_ptr(), T["pool"].data_ptr())
    fe.verify_place_blocks_device(T["blocks"].data_ptr(), T["blocks"].shape[0], md, T["kmin"].data_ptr(),
                                  T["dmin"].data_ptr(), stream)


@pytest.mark.parametrize("spec", S.GENERAL_SPECS, ids=S.spec_id)
def test_general_scene_through_the_whole_chain(oracle, fp64_order, spec):
    """descriptors -> okvfe_verify_place_blocks_device (= oracle.verify_place) -> claims -> consensus over hypotheses
    around the true pose, equal to place_ref.verify"""
    tree = _tree(fp64_order)
    sc = PS.general_scene(oracle, spec, tree)
    fe = _frontend(sc["cams"])
    what = (sc["name"], fp64_order)
    fus = [c.fu for c in sc["cams"]]
    refs = [P.verify(tree, sc["hp"], mf["frames"], mf["kmin"], mf["dmin"], PS.MATCH_THRESHOLD, fus, sc["T_SC"], mf["H"],
                     mf["valid"], sc["min_inliers"]) for mf in sc["mfs"]]
    T = PS.prepare(fe, sc)
    _match_setup(sc, T)
    _match(fe, sc, T)
    PS.launch_claims(fe, sc, T)
    PS.launch_consensus(fe, sc, T)
    got = PS.download(T)
    L = len(sc["hp"])
    assert np.array_equal(got["kmin"], np.concatenate([mf["kmin"] for mf in sc["mfs"]]).reshape(-1, L)), what
    assert np.array_equal(got["dmin"].view(np.uint32), np.concatenate([mf["dmin"] for mf in sc["mfs"]]).reshape(-1, L)), what
    PS.check_claims(sc, got, [r[0] for r in refs], what)
    PS.check_consensus(sc, got, [r[1] for r in refs], what)
    assert int((got["state"] == 2).sum()) >= S.STATE_FLOOR and int((got["state"] == 1).sum()) >= S.STATE_FLOOR
    # the variants of the call on the same rows
    _chain(fe, sc, tree, what + ("in place",), alias=True)
    _chain(fe, sc, tree, what + ("verdicts only",), optional=False)
    _chain(fe, sc, tree, what + ("gate NULL",), with_gate=False)
    _chain(fe, sc, tree, what + ("hyp_valid NULL",), use_valid=False)


def test_two_candidates_on_one_stream(oracle, fp64_order):
    """two candidate old frames: match, claims and consensus of each queued on a side stream with nothing waited for in
    between; the verdicts are read once at the end"""
    tree = _tree(fp64_order)
    spec = ("euroc", "euroc1")
    scs = [PS.general_scene(oracle, spec, tree, seed=s) for s in (0, 1)]
    fe = _frontend(scs[0]["cams"])
    fus = [c.fu for c in scs[0]["cams"]]
    Ts = [PS.prepare(fe, sc, alias=True) for sc in scs]
    stream = torch.cuda.Stream()
    for sc, T in zip(scs, Ts):
        _match_setup(sc, T)
    for sc, T in zip(scs, Ts):
        _match(fe, sc, T, stream)
        PS.launch_claims(fe, sc, T, stream)
        PS.launch_consensus(fe, sc, T, stream=stream)
    stream.synchronize()
    for sc, T in zip(scs, Ts):
        refs = [P.verify(tree, sc["hp"], mf["frames"], mf["kmin"], mf["dmin"], PS.MATCH_THRESHOLD, fus, sc["T_SC"], mf["H"],
                         mf["valid"], sc["min_inliers"]) for mf in sc["mfs"]]
        got = PS.download(T)
        assert [int(got[k][i]) for i in range(3) for k in ("n_matches", "n_points", "n_corr_claims", "gate")] == \
            [r[0][k] for r in refs for k in ("n_matches", "n_points", "n_corr", "gate")]
        PS.check_consensus(sc, got, [r[1] for r in refs], (sc["name"], "side stream"), alias=True)


def test_argument_errors_and_an_empty_batch(oracle):
    sc = PS.gate_scene(oracle, 40)
    fe = _frontend(sc["cams"])
    T = PS.prepare(fe, sc)
    claims = fe.make_place_claims_device(*[T[k].data_ptr() for k in ("n_matches", "n_points", "n_corr_claims", "gate", "ml")])
    good = dict(place_set=T["set"], blocks_ptr=T["blocks"].data_ptr(), n_multiframes=2, n_cams=2, k_min_ptr=T["kmin"].data_ptr(),
                dist_min_ptr=T["dmin"].data_ptr(), min_inliers=40, result=claims)
    p = T["ml"].data_ptr()
    bad = (dict(place_set=None), dict(blocks_ptr=None), dict(n_multiframes=-1), dict(n_cams=0), dict(k_min_ptr=None),
           dict(dist_min_ptr=None), dict(min_inliers=-1), dict(result=None),
           dict(place_set=fe.make_place_set_device(-1, T["hp"].data_ptr())), dict(place_set=fe.make_place_set_device(5, None)),
           dict(result=fe.make_place_claims_device(p, p, p, None, p)), dict(result=fe.make_place_claims_device(p, p, p, p, None)))
    for change in bad:
        with pytest.raises(capi.OkvfeError) as e:
            fe.place_claims_blocks_device(**dict(good, **change))
        assert e.value.status == capi.ERR_INVALID_ARGUMENT, change
    fe.place_claims_blocks_device(**dict(good, n_multiframes=0))
    res = fe.make_ransac_result_device(*[T[k].data_ptr() for k in ("n_corr", "best", "n_inl", "accepted")])
    cgood = dict(place_set=T["set"], blocks_ptr=T["blocks"].data_ptr(), n_multiframes=2, cam_ids=[0, 1], poses_T_SC=sc["T_SC"],
                 match_landmark_ptr=T["ml"].data_ptr(), gate_ptr=None, hypotheses_ptr=T["H"].data_ptr(), hyp_valid_ptr=None,
                 n_hyp=6, min_inliers=40, result=res, verdict_ptr=T["verdict"].data_ptr())
    cbad = (dict(place_set=None), dict(blocks_ptr=None), dict(n_multiframes=-1), dict(cam_ids=[], poses_T_SC=[]),
            dict(cam_ids=[0, 1, 0], poses_T_SC=sc["T_SC"] + sc["T_SC"][:1]), dict(match_landmark_ptr=None),
            dict(hypotheses_ptr=None), dict(n_hyp=0), dict(n_hyp=capi.RANSAC_MAX_HYPOTHESES + 1), dict(min_inliers=-1),
            dict(threshold=float("nan")), dict(threshold=-1.0), dict(result=None), dict(verdict_ptr=None),
            dict(result=fe.make_ransac_result_device(T["n_corr"].data_ptr(), None, T["n_inl"].data_ptr(), T["accepted"].data_ptr())))
    for change in cbad:
        with pytest.raises(capi.OkvfeError) as e:
            fe.place_consensus_blocks_device(**dict(cgood, **change))
        assert e.value.status == capi.ERR_INVALID_ARGUMENT, change
    fe.place_consensus_blocks_device(**dict(cgood, n_multiframes=0))
    got = PS.download(T)
    for k in ("n_matches", "n_points", "n_corr_claims", "n_corr", "best", "n_inl"):
        assert np.all(got[k] == PS.SENTINEL), k
    assert np.all(got["gate"] == PS.GATE_SENTINEL) and np.all(got["verdict"] == PS.GATE_SENTINEL)
    assert np.all(got["ml"] == T["ml_in"])
    half = _frontend(sc["cams"], n_set=1)  # a slot without intrinsics: the frame and the slot are named
    with pytest.raises(capi.OkvfeError) as e:
        half.place_consensus_blocks_device(**cgood)
    assert e.value.status == capi.ERR_NOT_READY and "frame 1: camera slot 1" in str(e.value), str(e.value)


def test_the_largest_keypoint_capacity_and_the_refusal_beyond_it():
    """the claims table is one int per keypoint in LDS and is not tiled: a context of 12288 rows works up to its last
    keypoint, one of 16384 rows is refused before anything is launched"""
    L, thr = 700, PS.MATCH_THRESHOLD
    hp = np.tile(np.array([1.0, 2.0, 3.0, 1.0]), (L, 1))
    for per_layer, ok in ((3072, True), (4096, False)):  # (octaves = 2: four layers of `per_layer` rows each)
        fe = capi.Frontend(128, 128, 10.0, 2, 50, per_layer, match_threshold=thr)
        try:
            Kb = fe.max_keypoints
            assert (Kb <= capi.PLACE_CLAIMS_MAX_KEYPOINTS) == ok and Kb == 4 * per_layer
            block = np.zeros(fe.gather_block_bytes(), np.uint8)
            block[:4] = np.array([Kb], np.int32).view(np.uint8)  # a full block: the claims read nothing else of it
            rng = np.random.default_rng(per_layer)
            km = rng.integers(Kb - 300, Kb, L).astype(np.int32)  # collisions among the last 300 keypoints
            km[:3] = Kb - 1
            dm = rng.integers(thr - 5, thr + 5, L).astype(np.int32)
            dm[:3] = 0
            ref = P.claim_stage(hp, [Kb], [km], [dm], thr, 10)
            d = dict(block=S._dev(block), hp=S._dev(hp), km=S._dev(km), dm=S._dev(dm),
                     counts=torch.full((3,), PS.SENTINEL, dtype=torch.int32, device="cuda"),
                     gate=torch.full((1,), PS.GATE_SENTINEL, dtype=torch.uint8, device="cuda"),
                     ml=torch.full((Kb,), PS.SENTINEL, dtype=torch.int32, device="cuda"))
            torch.cuda.synchronize()
            res = fe.make_place_claims_device(d["counts"][0:].data_ptr(), d["counts"][1:].data_ptr(), d["counts"][2:].data_ptr(),
                                              d["gate"].data_ptr(), d["ml"].data_ptr())
            call = lambda: fe.place_claims_blocks_device(fe.make_place_set_device(L, d["hp"].data_ptr()), d["block"].data_ptr(), 1,
                                                         1, d["km"].data_ptr(), d["dm"].data_ptr(), 10, res)
            if ok:
                call()
                torch.cuda.synchronize()
                assert d["counts"].cpu().tolist() == [ref["n_matches"], ref["n_points"], ref["n_corr"]] and ref["gate"] == 2
                assert int(d["gate"].cpu()[0]) == 2 and np.array_equal(d["ml"].cpu().numpy(), ref["match_landmark"][0])
                assert ref["match_landmark"][0][Kb - 1] >= 2 and ref["n_matches"] > ref["n_corr"] > 100
            else:
                with pytest.raises(capi.OkvfeError) as e:
                    call()
                assert e.value.status == capi.ERR_UNSUPPORTED and "12288" in str(e.value)
                torch.cuda.synchronize()
                assert np.all(d["counts"].cpu().numpy() == PS.SENTINEL) and np.all(d["ml"].cpu().numpy() == PS.SENTINEL)
        finally:
            fe.close()
