"""CPU: the boundary of okvfe_place_landmark_set, okvfe_place_claims_blocks_device and
okvfe_place_consensus_blocks_device (Frontend::verifyRecognisedPlace around its descriptor matching): exported, declared,
bound; argument errors that need no device; the pipelined-lanes audit classifies both device entry points as joining;
the host helper against the transcription (place_ref.py) on every set scene under both orders of the sum; and the
scenes the GPU tier feeds the kernels (place_scenes.py) hold their census floors, the gate table and the verdict table
on the reference alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import place_ref as P
import place_scenes as PS
import ransac_scenes as S
from okvis2_amd import capi
from test_capi_join_audit import classify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("okvfe_place_landmark_set", "okvfe_place_claims_blocks_device", "okvfe_place_consensus_blocks_device")
FLOOR = 16
TREES = (True, False)


def test_symbols_exported_declared_and_bound():
    lib = C.CDLL(capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "okvfe.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in capi.EXPORTS
    assert "#define OKVFE_ABI_VERSION 8" in header
    assert "typedef struct okvfe_place_set_device" in code and "typedef struct okvfe_place_claims_device" in code
    for method in ("place_landmark_set", "place_claims_blocks_device", "place_consensus_blocks_device",
                   "make_place_set_device", "make_place_claims_device"):
        assert callable(getattr(capi.Frontend, method)), method
    assert [len(getattr(capi.lib(), n).argtypes) for n in NAMES] == [15, 10, 17]
    assert C.sizeof(capi.PlaceClaimsDevice) == 5 * C.sizeof(C.c_void_p)
    assert C.sizeof(capi.PlaceSetDevice) == 2 * C.sizeof(C.c_void_p)
    # the header says what stays with the caller, and what is refused
    for text in ("non-maximum suppression", "gp3p", "adaptive stop", "ceres refinement", "Hessian H",
                 "attemptLoopClosure", "PARITY UNPINNED: opengv's winner rule", "12288", "packets of two"):
        assert text in header, text
    mirror = open(os.path.join(ROOT, "okvis2_amd", "host", "okvfe_frontend.hpp")).read()
    for name in NAMES:
        assert name + "(" in mirror
    for text in ("class DevicePlaceSet", "placeLandmarkSet(", "verifyPlaceClaimsBlocks(", "verifyPlaceConsensusBlocks("):
        assert text in mirror, text
    assert "place_verify_cli.cpp" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    mk = open(os.path.join(ROOT, "okvis2_amd", "csrc", "Makefile")).read()
    assert "k_place.hip" in mk and "capi_place.cpp" in mk


def test_null_and_negative_arguments_are_invalid_before_any_device_work():
    lib = capi.lib()
    buf = (C.c_int32 * 64)()
    a = C.addressof(buf)
    pset = capi.Frontend.make_place_set_device(0, None)
    claims = capi.Frontend.make_place_claims_device(a, a, a, a, a)
    res = capi.Frontend.make_ransac_result_device(a, a, a, a)
    cams = (C.c_int32 * 1)(0)
    pose = capi.make_pose(np.eye(3).reshape(-1), np.zeros(3))
    f, g = getattr(lib, NAMES[1]), getattr(lib, NAMES[2])
    assert f(None, C.byref(pset), buf, 1, 1, buf, buf, 10, C.byref(claims), None) == capi.ERR_INVALID_ARGUMENT
    assert g(None, C.byref(pset), buf, 1, 1, cams, C.byref(pose), buf, None, buf, None, 1, 16.0, 10, C.byref(res), buf,
             None) == capi.ERR_INVALID_ARGUMENT
    # the host helper: NULL outputs, negative counts, an order that does not exist
    h = getattr(lib, NAMES[0])
    one = (C.c_int32 * 1)(0)
    nl, nr = C.c_int32(-1), C.c_int32(-1)
    ok = lambda *args: h(*args)
    assert ok(1, one, None, None, None, None, 1, None, None, buf, 0, None, 0, C.byref(nl), C.byref(nr)) == 0
    assert (nl.value, nr.value, buf[0]) == (0, 0, 0)
    assert ok(1, one, None, None, None, None, 2, None, None, buf, 0, None, 0, C.byref(nl), C.byref(nr)) == capi.ERR_INVALID_ARGUMENT
    assert ok(-1, one, None, None, None, None, 1, None, None, buf, 0, None, 0, C.byref(nl), C.byref(nr)) == capi.ERR_INVALID_ARGUMENT
    assert ok(1, one, None, None, None, None, 1, None, None, None, 0, None, 0, C.byref(nl), C.byref(nr)) == capi.ERR_INVALID_ARGUMENT
    assert ok(1, one, None, None, None, None, 1, None, None, buf, 0, None, 0, None, C.byref(nr)) == capi.ERR_INVALID_ARGUMENT
    neg = (C.c_int32 * 1)(-3)
    assert ok(1, neg, None, None, None, None, 1, None, None, buf, 0, None, 0, C.byref(nl), C.byref(nr)) == capi.ERR_INVALID_ARGUMENT
    four = (C.c_int32 * 1)(4)  # keypoints without arrays
    assert ok(1, four, None, None, None, None, 1, None, None, buf, 0, None, 0, C.byref(nl), C.byref(nr)) == capi.ERR_INVALID_ARGUMENT


def test_both_device_entry_points_join_the_pipelined_lanes():
    joins, missing, unclassified = classify()
    for name in NAMES[1:]:
        assert name in joins
    assert not missing and not unclassified


def test_the_consensus_is_a_policy_of_the_one_kernel():
    src = open(os.path.join(ROOT, "okvis2_amd", "csrc", "k_ransac.hip")).read()
    assert src.count("void ransac_consensus_kernel(") == 1 and src.count("template <bool kTree, bool kPlace>") == 2
    assert src.count("double ransac_distance(") == 1 and src.count("void invert_hypothesis(") == 1
    assert src.count("auto score = ") == 1 and src.count("s_rec[kRansacRing]") == 1
    assert "ransac_consensus_kernel<true, true>" in src and "ransac_consensus_kernel<false, true>" in src


def test_fractions_of_the_verdict_table_in_float64():
    """7 / 10, 14 / 20 and 21 / 30 are not < 0.7 in float64 (Frontend.cpp:389 lets them pass; :2243 does not)"""
    for i, n in ((7, 10), (14, 20), (21, 30)):
        assert not np.float64(i) / np.float64(n) < 0.7
        assert not np.float64(i) / np.float64(n) > 0.7
    assert np.float64(13) / np.float64(20) < 0.7 and np.float64(20) / np.float64(30) < 0.7
    assert not np.float64(10) / np.float64(14) < 0.7 and np.float64(10) / np.float64(15) < 0.7
    assert not np.float64(40) / np.float64(57) < 0.7 and np.float64(40) / np.float64(58) < 0.7
    assert not np.float64(5) / np.float64(7) < 0.7 and np.float64(4) / np.float64(7) < 0.7


@pytest.mark.parametrize("tree", TREES)
def test_landmark_set_against_the_transcription(oracle, tree):
    census = P.new_census(P.SET_CENSUS)
    for old in (PS.set_scene(), PS.set_scene(seed=6, n_cams=5), PS.set_scene(seed=7, n_cams=1, n_general=10)):
        ref = P.landmark_set(tree, old, census)
        got = capi.place_landmark_set(*PS.flat_old(old), eigen_tree=tree)
        PS.same_set(got, ref, (tree, len(old)))
        assert np.all(np.diff(ref["ids"].astype(np.int64)) > 0) and ref["desc_begin"][-1] == len(ref["pool"])
    print(census)
    for key in P.SET_CENSUS:
        assert census[key] >= FLOOR, (key, census)
    for spec in S.GENERAL_SPECS:  # the sets of the general scenes
        sc = PS.general_scene(oracle, spec, tree)
        PS.same_set(capi.place_landmark_set(*PS.flat_old(sc["old"]), eigen_tree=tree), sc["set"], (tree, spec))
    # an empty old frame
    empty = capi.place_landmark_set([0, 0], np.zeros(0, np.uint64), np.zeros((0, 4)), np.zeros(0, np.uint8), np.zeros((0, 48), np.uint8))
    assert len(empty["ids"]) == 0 and empty["desc_begin"].tolist() == [0]


def test_the_norm_edge_separates_under_its_own_order():
    """the bisected pairs are adjacent doubles, one landmark filtered and one kept, under the order they were made for"""
    rng = np.random.default_rng(3)
    for tree in TREES:
        for _ in range(8):
            base = rng.normal(size=4)
            lo, hi = PS.norm_edge(tree, base / np.linalg.norm(base))
            old = [dict(ids=np.array([5, 6], np.uint64), hp=np.array([base / np.linalg.norm(base) * lo, base / np.linalg.norm(base) * hi]),
                        init=np.ones(2, np.uint8), desc=np.zeros((2, 48), np.uint8))]
            got = capi.place_landmark_set(*PS.flat_old(old), eigen_tree=tree)
            assert got["ids"].tolist() == [6], (tree, lo, hi)


def test_landmark_set_capacity():
    old = PS.set_scene()
    n_kps, ids, hp, init, desc = PS.flat_old(old)
    ref = P.landmark_set(True, old)
    L, R = len(ref["ids"]), len(ref["pool"])
    nk = np.array(n_kps, np.int32)
    out_ids, out_hp, out_db, out_pool = np.zeros(L, np.uint64), np.zeros((L, 4)), np.full(L + 1, -9, np.int32), np.zeros((R, 48), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    nl, nr = C.c_int32(0), C.c_int32(0)
    f = capi.lib().okvfe_place_landmark_set
    for cap_l, cap_r in ((L - 1, R), (L, R - 1), (0, 0)):
        st = f(len(nk), p(nk), p(ids), p(hp), p(init), p(desc), 1, p(out_ids), p(out_hp), p(out_db), cap_l, p(out_pool), cap_r,
               C.byref(nl), C.byref(nr))
        assert st == capi.ERR_CAPACITY and (nl.value, nr.value) == (L, R) and np.all(out_db == -9)
    st = f(len(nk), p(nk), p(ids), p(hp), p(init), p(desc), 1, p(out_ids), p(out_hp), p(out_db), L, p(out_pool), R, C.byref(nl), C.byref(nr))
    assert st == 0 and np.array_equal(out_db, ref["desc_begin"]) and np.array_equal(out_pool, ref["pool"])


def test_claim_scenes_reach_every_branch(oracle):
    census = P.new_census(P.CLAIM_CENSUS)
    sc = PS.claims_scene(oracle)
    refs = PS.claims_reference(sc, census)
    allsc = PS.collide_all_scene(oracle)
    all_refs = PS.claims_reference(allsc, census)
    print(census)
    for key in P.CLAIM_CENSUS:
        assert census[key] >= FLOOR, (key, census)
    L = len(allsc["hp"])
    for ref in all_refs:  # the largest row wins, the losers still count
        assert (ref["n_matches"], ref["n_points"]) == (2 * L, L)
        assert all(int((ml >= 0).sum()) == 1 and ml.max() == L - 1 for ml in ref["match_landmark"])
    a, b = refs
    assert a["gate"] == 2 and a["n_matches"] > a["n_points"] > 0 and a["n_corr"] < int(sum((ml >= 0).sum() for ml in a["match_landmark"]))
    assert len(b["match_landmark"][1]) == 0 and b["n_matches"] < a["n_matches"]
    assert census["w_below_1e-8"] >= 4 * PS.COPIES and census["w_nan"] >= PS.COPIES and census["w_negative"] >= 2 * PS.COPIES


@pytest.mark.parametrize("min_inliers", sorted(PS.GATE_TABLE))
def test_gate_table(oracle, min_inliers):
    refs = PS.claims_reference(PS.gate_scene(oracle, min_inliers))
    assert len(refs) == len(PS.GATE_TABLE[min_inliers])
    for (name, counts, gate), ref in zip(PS.GATE_TABLE[min_inliers], refs):
        assert (ref["n_matches"], ref["n_points"], ref["n_corr"]) == counts and ref["gate"] == gate, (name, ref)


@pytest.mark.parametrize("tree", TREES)
def test_verdict_table(oracle, tree):
    for min_inliers, table in PS.VERDICT_TABLE.items():
        sc = PS.verdict_scene(oracle, min_inliers, PS.true_first)
        ml = [mf["ml"] for mf in sc["mfs"]]
        refs = PS.consensus_reference(tree, sc, ml)
        for ((n, i), verdict), ref in zip(table, refs):
            assert (ref["n_corr"], ref["n_inliers"], ref["verdict"]) == (n, i if verdict >= 2 else 0, verdict), (min_inliers, n, i, ref["n_inliers"], ref["verdict"])
            assert ref["best"] == (0 if verdict >= 2 else -1) and ref["accepted"] == int(verdict == 3)
            removed = int((ref["landmark_out"][0] == -1).sum()) - int((sc["mfs"][refs.index(ref)]["ml"][0] == -1).sum())
            assert removed == (n - i if verdict == 3 else 0)
            if verdict < 2:
                assert np.all(ref["hyp_inliers"] == -1) and np.all(ref["state"][0] <= 1)
        # every hypothesis with zero inliers
        none = PS.consensus_reference(tree, PS.verdict_scene(oracle, min_inliers, lambda T, rng: np.array([S.far_pose(T, rng)] * 2)), ml)
        for ((n, i), _), ref in zip(table, none):
            assert (ref["verdict"], ref["best"], ref["n_inliers"]) == ((2, -1, 0) if n >= P.MIN_CORR else (1, -1, 0))
            assert ref["hyp_inliers"].tolist() == ([0, 0] if n >= P.MIN_CORR else [-1, -1])
        # the would-be winner switched off: the copy behind it wins with the same count
        thrice = lambda T, rng: np.array([S.pose_matrix(T), S.pose_matrix(T), S.far_pose(T, rng)])
        off = PS.consensus_reference(tree, PS.verdict_scene(oracle, min_inliers, thrice, valid=np.array([0, 1, 1], np.uint8)), ml)
        for ((n, i), verdict), ref in zip(table, off):
            assert ref["verdict"] == verdict and ref["best"] == (1 if verdict >= 2 else -1)
            assert ref["hyp_inliers"][0] == -1
        # gate_dev of 0 and of 1 passed through: 0 ends the multiframe, 1 leaves the verdict to the kernel's own count
        gates = [j % 3 for j in range(len(table))]
        gated = PS.consensus_reference(tree, sc, ml, gates)
        for g, ((n, i), verdict), ref in zip(gates, table, gated):
            assert ref["verdict"] == (0 if g == 0 else verdict) and ref["n_corr"] == n
            if g == 0:
                assert ref["best"] == -1 and ref["n_inliers"] == 0 and np.all(ref["hyp_inliers"] == -1)


def test_chunk_and_landmark_count_edges(oracle):
    chunk = capi.Frontend._test_ransac_chunk_records()
    sc = PS.chunk_scene(oracle, chunk)
    refs = PS.consensus_reference(True, sc, [mf["ml"] for mf in sc["mfs"]])
    assert [r["n_corr"] for r in refs] == [chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1]
    assert all(r["best"] >= 0 for r in refs) and len(sc["cams"]) == 5
    for L in PS.L_EDGES:
        sc = PS.landmark_count_scene(oracle, L)
        refs = PS.claims_reference(sc)
        assert len(sc["hp"]) == L
        if L >= 255:
            assert all(r["n_matches"] > r["n_points"] >= 100 and r["n_corr"] >= 20 for r in refs), L
        if L == 0:
            assert all((r["n_matches"], r["n_points"], r["n_corr"], r["gate"]) == (0, 0, 0, 0) for r in refs)


@pytest.mark.parametrize("tree", TREES)
def test_general_scenes_hold_a_mix_of_verdicts(oracle, tree):
    verdicts, collisions = [], 0
    for spec in S.GENERAL_SPECS:
        sc = PS.general_scene(oracle, spec, tree)
        assert len(sc["hp"]) <= 400 and len(sc["mfs"]) == 3 and len(sc["mfs"][0]["H"]) <= 50
        census = P.new_census(P.CLAIM_CENSUS)
        for mf in sc["mfs"]:
            cl, co = P.verify(tree, sc["hp"], mf["frames"], mf["kmin"], mf["dmin"], PS.MATCH_THRESHOLD,
                              [c.fu for c in sc["cams"]], sc["T_SC"], mf["H"], mf["valid"], sc["min_inliers"], census=census)
            verdicts.append(co["verdict"])
            if co["verdict"] >= 2:
                assert int(sum((s == 2).sum() for s in co["state"])) >= FLOOR, sc["name"]
        collisions += census["loser_counted"]
    print(verdicts, collisions)
    assert verdicts.count(3) >= 3 and verdicts.count(2) >= 3
