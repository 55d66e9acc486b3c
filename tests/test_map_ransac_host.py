"""CPU: the boundary of okvfe_ransac3d2d_consensus_blocks_device and okvfe_remove_outliers_blocks_device (what
Frontend::matchToMap does between its two matcher passes, on device-resident batches): exported, declared, bound;
argument errors that need no device; the pipelined-lanes audit classifies both as joining; the distance exists once in
k_ransac.hip and the pose-inverse helper once in k_map.hip; and the scenes the GPU tier feeds them (ransac_scenes.py)
hold their census floors, their verdict tables and the margin cap on the reference alone (ransac_ref.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ransac_ref as R
import ransac_scenes as S
from okvis2_amd import capi
from test_capi_join_audit import classify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("okvfe_ransac3d2d_consensus_blocks_device", "okvfe_remove_outliers_blocks_device")
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
    assert "typedef struct okvfe_ransac_result_device" in code
    assert callable(capi.Frontend.ransac3d2d_consensus_blocks_device)
    assert callable(capi.Frontend.remove_outliers_blocks_device)
    assert len(getattr(capi.lib(), NAMES[0]).argtypes) == 15 and len(getattr(capi.lib(), NAMES[1]).argtypes) == 11
    assert C.sizeof(capi.RansacResultDevice) == 8 * C.sizeof(C.c_void_p)
    # the texts no longer list the step as missing, and say what is not restated
    assert "Not covered: RANSAC" not in header
    assert "PARITY UNPINNED: opengv" in header and "adaptive stop" in header


def test_null_arguments_are_invalid_before_any_device_work():
    lib = capi.lib()
    t = capi.Frontend.make_landmark_table_device(0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    buf = (C.c_int32 * 64)()
    res = capi.Frontend.make_ransac_result_device(C.addressof(buf), C.addressof(buf), C.addressof(buf), C.addressof(buf))
    cams = (C.c_int32 * 1)(0)
    pose = capi.make_pose(np.eye(3).reshape(-1), np.zeros(3))
    f = getattr(lib, NAMES[0])
    assert f(None, C.byref(t), buf, 1, 1, cams, C.byref(pose), buf, buf, None, 1, 16.0, 1, C.byref(res), None) == \
        capi.ERR_INVALID_ARGUMENT
    g = getattr(lib, NAMES[1])
    assert g(None, C.byref(t), buf, 1, cams, C.byref(pose), 4.0, buf, buf, buf, None) == capi.ERR_INVALID_ARGUMENT


def test_both_entry_points_join_the_pipelined_lanes():
    joins, missing, unclassified = classify()
    for name in NAMES:
        assert name in joins
    assert not missing and not unclassified


def test_one_copy_of_the_distance_and_of_the_pose_inverse():
    src = open(os.path.join(ROOT, "okvis2_amd", "csrc", "k_ransac.hip")).read()
    assert src.count("double ransac_distance(") == 1
    assert src.count("= ransac_distance<kTree>(") == 2  # the scoring loop and the final sweep
    assert src.count("rep[i] / n - b[i]") == 1 and src.count("bool make_correspondence(") == 1
    ops = open(os.path.join(ROOT, "okvis2_amd", "csrc", "fp64_ops.h")).read()
    assert ops.count("double sum4(") == 1 and "double sum4" not in src
    kmap = open(os.path.join(ROOT, "okvis2_amd", "csrc", "k_map.hip")).read()
    assert kmap.count("void pose_inverse_times(") == 1
    assert kmap.count("hh[i] + (-cr[i]) * hp[3]") == 1
    assert kmap.count("pose_inverse_times(") == 3  # the definition, prepare_landmark, remove_outliers_frames_kernel
    mk = open(os.path.join(ROOT, "okvis2_amd", "csrc", "Makefile")).read()
    assert "k_ransac.hip" in mk and "capi_ransac.cpp" in mk


def test_fractions_of_the_verdict_table_in_float64():
    """7 / 10, 14 / 20 and 21 / 30 are not > 0.7 in float64; 15 / 20 and 10 / 10 are"""
    for i, n in ((7, 10), (14, 20), (21, 30)):
        assert not np.float64(i) / np.float64(n) > 0.7
    assert np.float64(15) / np.float64(20) > 0.7 and np.float64(9) / np.float64(12) > 0.7


@pytest.mark.parametrize("tree", TREES)
def test_general_scenes_margins_and_census(oracle, tree):
    """float64 and longdouble agree on every verdict whose margin exceeds 1e-9 relative, at most 1 % of the verdicts
    sit inside that margin, and the scenes hold a mix of accepted and rejected multiframes"""
    total = inside = 0
    census = R.new_census()
    accepted = []
    for spec in S.GENERAL_SPECS:
        sc = S.general_scene(oracle, spec)
        refs = S.reference(tree, sc, census=census)
        for want in (1, 2):  # what test_gpu_map_ransac.py asks of the device's states, on the reference alone
            have = sum(int((st == want).sum()) for ref in refs for st in ref["state"])
            assert have >= S.STATE_FLOOR, (sc["name"], want, have)
        for mf, ref in zip(sc["mfs"], refs):
            v64, vld, margin = R.margins(tree, mf["H"], ref["corr"], sc["T_SC"])
            clear = margin > 1.0e-9
            assert np.array_equal(v64[clear], vld[clear]), sc["name"]
            total += margin.size
            inside += int((~clear).sum())
            accepted.append(ref["accepted"])
            if sum(len(f["kps"]) for f in mf["frames"]):  # (a one-camera rig's empty block is a multiframe of its own)
                assert ref["n_corr"] >= 25, (sc["name"], ref["n_corr"])
            else:
                assert ref["n_corr"] == 0 and ref["best"] == -1
    print("verdicts", total, "inside the margin", inside, "accepted", accepted, census)
    assert total > 20000 and inside <= 0.01 * total
    assert sum(accepted) >= 3 and len(accepted) - sum(accepted) >= 3
    for key in ("no_landmark", "correspondence", "duplicate_landmark"):
        assert census[key] >= FLOOR, (key, census)


@pytest.mark.parametrize("tree", TREES)
def test_directed_scene_reaches_every_branch(oracle, tree):
    census = R.new_census()
    sc = S.directed_scene(oracle)
    ref = S.reference(tree, sc, census=census)[0]
    print(census)
    for key in R.CENSUS:
        assert census[key] >= FLOOR, (key, census)
    assert census["w_below_1e-8"] >= 4 * 2 * S.DIRECTED_COPIES  # nextafter below, 0.0, -0.0, the negative small one
    assert census["nan_distance"] >= 2 * S.DIRECTED_COPIES + 2 * S.DIRECTED_COPIES  # the centre and the NaN hp[3]
    assert ref["best"] > 0 and ref["hyp_inliers"][0] >= 0


@pytest.mark.parametrize("tree", TREES)
def test_knife_edges_flip_one_verdict(oracle, tree):
    sc = S.knife_translation(oracle, tree)
    ref = S.reference(tree, sc)[0]
    assert ref["n_corr"] == 13 and ref["hyp_inliers"][0] == ref["hyp_inliers"][1] + 1 >= 10
    assert ref["dist"][0, 0] < R.THRESHOLD <= ref["dist"][1, 0] and np.all((ref["dist"][0] < 16) == (ref["dist"][1] < 16)[None] | (np.arange(13) == 0))
    H = sc["mfs"][0]["H"]
    assert np.nextafter(H[0][3], H[1][3]) == H[1][3] and np.array_equal(np.delete(H[0], 3), np.delete(H[1], 3))
    sc = S.knife_size(oracle, tree)
    ref = S.reference(tree, sc)[0]
    sizes = sc["mfs"][0]["frames"][0]["kps"]["size"]
    assert np.nextafter(sizes[0], sizes[1]) == sizes[1]
    assert ref["n_corr"] == 14 and list(ref["state"][0][:2]) == [1, 2] and ref["hyp_inliers"][0] == 13


@pytest.mark.parametrize("tree", TREES)
def test_verdict_table(oracle, tree):
    true_first = lambda T, rng: np.array([S.pose_matrix(T), S.far_pose(T, rng)])
    sc = S.verdict_scene(oracle, true_first)
    refs = S.reference(tree, sc)
    for case, ref in zip(S.VERDICT_CASES, refs):
        assert ref["n_corr"] == case[0]
        assert (ref["best"], ref["n_inliers"], ref["accepted"]) == S.VERDICT_EXPECT[case], (case, ref["best"], ref["n_inliers"])
        removed = sum(int((lo == -1).sum()) - int((f["lm"] == -1).sum()) for lo, f in zip(ref["landmark_out"], sc["mfs"][refs.index(ref)]["frames"]))
        assert removed == (case[0] - case[1] if ref["accepted"] else 0), case
    # equal counts: the first wins; a better one later wins; nothing beats zero
    twice = S.reference(tree, S.verdict_scene(oracle, lambda T, rng: np.array([S.pose_matrix(T)] * 2)))
    assert [r["best"] for r in twice[1:]] == [0] * 6
    later = S.reference(tree, S.verdict_scene(oracle, lambda T, rng: np.array([S.far_pose(T, rng), S.pose_matrix(T)])))
    assert [r["best"] for r in later[1:]] == [1] * 6
    none = S.reference(tree, S.verdict_scene(oracle, lambda T, rng: np.array([S.far_pose(T, rng)] * 2)))
    assert all(r["best"] == -1 and r["n_inliers"] == 0 and not r["accepted"] for r in none)
    assert all(list(r["hyp_inliers"]) == [0, 0] for r in none[1:]) and list(none[0]["hyp_inliers"]) == [-1, -1]
    invalid = S.reference(tree, S.verdict_scene(oracle, true_first, valid=np.zeros(2, np.uint8)))
    assert all(r["best"] == -1 and list(r["hyp_inliers"]) == [-1, -1] for r in invalid)


def test_chunk_scene_counts(oracle):
    chunk = capi.Frontend._test_ransac_chunk_records()
    sc = S.chunk_scene(oracle, chunk)
    refs = S.reference(True, sc)
    assert [r["n_corr"] for r in refs] == [chunk - 1, chunk, chunk + 1, 2 * chunk + 1]
    assert all(r["best"] >= 0 for r in refs)


@pytest.mark.parametrize("tree", TREES)
def test_remove_outliers_scenes(oracle, tree):
    census = dict.fromkeys(R.REMOVE_CENSUS, 0)
    sc = S.remove_scene(oracle)
    refs = S.remove_reference(oracle, tree, sc, census=census)
    assert all(10 <= k for _, k in refs[:-1]) and refs[-1][1] == 0
    st = S.remove_status_scene(oracle)
    S.remove_reference(oracle, tree, st, census=census)
    print(census)
    for key in R.REMOVE_CENSUS:
        assert census[key] >= FLOOR, (key, census)
    edge, keep, drop = S.remove_edge_scene(oracle, tree)
    assert np.nextafter(drop, keep) == keep
    assert S.remove_reference(oracle, tree, edge, keep)[0][1] == 3 and S.remove_reference(oracle, tree, edge, drop)[0][1] == 0


def test_chain_scene_exercises_every_step(oracle):
    """the reference chain of test_gpu_map_ransac_chain.py: the first pass matches enough keypoints, the consensus
    accepts and removes outliers, removeOutliers removes more, and the second pass still matches"""
    import map_scenes
    for exclusive, thr, tree in [m + (t,) for m in map_scenes.MODES for t in TREES]:
        ch = S.chain_scene(oracle, tree, exclusive, thr)
        cons = ch["cons"][0]
        matched = sum(int((f >= 0).sum()) for f in ch["first"])
        after_ransac = sum(int((lo >= 0).sum()) for lo in cons["landmark_out"])
        after_remove = sum(k for _, k in ch["removed"])
        hits2 = sum(int((s[0] >= 0).sum()) for s in ch["second"])
        print(exclusive, matched, cons["n_corr"], cons["n_inliers"], cons["accepted"], after_ransac, after_remove, hits2)
        assert cons["accepted"] == 1 and cons["n_corr"] >= 100
        assert matched > after_ransac > after_remove >= 50 and hits2 >= 30


def test_cpp_chain_scene_and_mirror(oracle):
    """the one-camera chain of test_gpu_map_ransac_cpp.py accepts at least one multiframe on the reference alone, and
    the host mirror declares both methods"""
    import map_scenes
    from test_gpu_map_ransac_cpp import K, mono_chain
    for exclusive, thr in map_scenes.MODES:
        ch = mono_chain(oracle, True, exclusive, thr)
        print([(c["n_corr"], c["n_inliers"], c["accepted"]) for c in ch["cons"]], [k for _, k in ch["removed"]])
        assert sum(c["accepted"] for c in ch["cons"]) >= 1 and all(len(f["desc"]) <= K for f in ch["frames"])
        assert sum(int((s[0] >= 0).sum()) for s in ch["second"]) >= 30
    mirror = open(os.path.join(ROOT, "okvis2_amd", "host", "okvfe_frontend.hpp")).read()
    assert "void ransac3d2dBlocks(" in mirror and "void removeOutliersBlocks(" in mirror
    for name in NAMES:
        assert name + "(" in mirror
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "map_ransac_cli.cpp" in entry
