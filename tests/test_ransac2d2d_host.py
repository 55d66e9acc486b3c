"""CPU: the boundary of okvfe_ransac2d2d_consensus_blocks_device (the consensus of Frontend::runRansac2d2d on device
batches): exported, declared, bound; argument errors that need no device; the pipelined-lanes audit classifies it as
joining; each distance exists once in k_ransac2d2d.hip; and the scenes the GPU tier feeds it (ransac2d2d_scenes.py)
hold their census floors, their decision table, their knife edges and the margin cap on the reference alone
(ransac2d2d_ref.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ransac2d2d_ref as R2
import ransac2d2d_scenes as S2
from okvis2_amd import capi
from test_capi_join_audit import classify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "okvfe_ransac2d2d_consensus_blocks_device"
FLOOR = 16
TREES = (True, False)


def _header():
    return open(os.path.join(ROOT, "include", "okvfe.h")).read()


def test_symbol_exported_declared_and_bound():
    lib = C.CDLL(capi.LIB_PATH)
    header = _header()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert hasattr(lib, NAME) and hasattr(lib, "okvfe_test_ransac2d2d_chunk_records")
    assert re.search(r"\b%s\s*\(" % NAME, code) and NAME in capi.EXPORTS
    assert "okvfe_test_ransac2d2d_chunk_records" not in header
    assert "#define OKVFE_ABI_VERSION 8" in header
    assert "typedef struct okvfe_ransac2d2d_result_device" in code
    assert callable(capi.Frontend.ransac2d2d_consensus_blocks_device)
    assert callable(capi.Frontend.make_ransac2d2d_result_device)
    assert len(getattr(capi.lib(), NAME).argtypes) == 23
    assert C.sizeof(capi.Ransac2d2dResultDevice) == 16 * C.sizeof(C.c_void_p)
    n_members = len(re.findall(r"\*\s*\w+;", re.search(r"typedef struct okvfe_ransac2d2d_result_device \{(.*?)\}", code, re.S).group(1)))
    assert n_members == 16


def test_header_texts():
    header = _header()
    flat = re.sub(r"\s*\n \*\s*", " ", header)
    # the motion sweep no longer leaves runRansac2d2d with the caller
    assert not re.search(r"runRansac2d2d[^.]*stay with the caller", flat)
    assert "The consensus of runRansac2d2d (:1964-1969, before initialisation only) is okvfe_ransac2d2d_consensus_blocks_device" in flat
    # the duplicate-current-multiframe rule and the ceiling on K are documented
    assert "With landmark1_out a current multiframe may appear in at most one pair of a call (OKVFE_ERR_INVALID_ARGUMENT" in flat
    assert "K = max_keypoints <= %d, beyond that OKVFE_ERR_UNSUPPORTED" % capi.RANSAC2D2D_MAX_KEYPOINTS in flat
    # the two PARITY UNPINNED notes of this call
    doc = flat[flat.index("before initialisation: the consensus of runRansac2d2d"):flat.index("typedef struct okvfe_ransac2d2d_result_device")]
    assert doc.count("PARITY UNPINNED") == 2 and "triangulate2" in doc and "winner rule" in doc
    for word in ("sampler", "twopt_rotationOnly", "Stewenius", "adaptive stop", "removeObservation", ":2378-2384",
                 "rotationOnly_tmp"):
        assert word in doc, word


def test_null_arguments_are_invalid_before_any_device_work():
    f = getattr(capi.lib(), NAME)
    buf = (C.c_int32 * 64)()
    a = C.addressof(buf)
    res = capi.Frontend.make_ransac2d2d_result_device(*[a] * 10)
    one = (C.c_int32 * 1)(0)
    assert f(None, buf, 1, buf, 1, 1, one, one, 1, one, buf, buf, None, 0, buf, None, buf, None, 1, 9.0, 1,
             C.byref(res), None) == capi.ERR_INVALID_ARGUMENT


def test_the_entry_point_joins_the_pipelined_lanes():
    joins, missing, unclassified = classify()
    assert NAME in joins and not missing and not unclassified


def test_one_copy_of_each_distance_and_both_files_in_the_makefile():
    src = open(os.path.join(ROOT, "okvis2_amd", "csrc", "k_ransac2d2d.hip")).read()
    assert src.count("double rotation_only_distance(") == 1 and src.count("double relative_pose_distance(") == 1
    assert src.count("= rotation_only_distance<kTree>(") == 2   # the scoring loop and the final sweep
    assert src.count("= relative_pose_distance<kTree>(") == 2
    assert src.count("void make_correspondence2(") == 1 and src.count("make_correspondence2<kTree>(") == 2
    assert src.count("(q1 * 0.5) / s1 + (q2 * 0.5) / s2") == 1 and src.count("1.0 / det") == 1
    ops = open(os.path.join(ROOT, "okvis2_amd", "csrc", "fp64_ops.h")).read()
    assert ops.count("double sum4(") == 1 and "double sum4" not in src and "k_ransac.hip\"" not in src
    mk = open(os.path.join(ROOT, "okvis2_amd", "csrc", "Makefile")).read()
    assert "k_ransac2d2d.hip" in mk and "capi_ransac2d2d.cpp" in mk


def test_fractions_of_the_decision_table_in_float32():
    """8 / 10, 12 / 15 and 16 / 20 are 0.8f, not above it; 17 / 20 is above; a float64 ratio would decide 12 / 15
    the same way but the reference compares floats"""
    f = np.float32
    for i, n in ((8, 10), (12, 15), (16, 20)):
        assert f(i) / f(n) == f(0.8) and not f(i) / f(n) > f(0.8)
    assert f(17) / f(20) > f(0.8) and f(17) / f(20) < f(18) / f(20)
    assert np.float64(f(0.8)) > np.float64(0.8)  # 0.8f lies above the double 0.8: in double arithmetic 16 / 20 > 0.8f would still be false
    assert f(10) / f(10) > f(0) / f(10) and not f(0) / f(20) > f(0) / f(20)


@pytest.mark.parametrize("tree", TREES)
def test_directed_scene_reaches_every_branch(oracle, tree):
    census = R2.new_census()
    sc = S2.directed_scene(oracle)
    refs = S2.reference(tree, sc, census=census)
    print(census)
    for key in R2.CENSUS:
        assert census[key] >= FLOOR, (key, census)
    assert sum(r["total_inliers"] >= 0 for r in refs) == len(refs)  # every pair of the plan has a succeeding camera


@pytest.mark.parametrize("tree", TREES)
def test_decision_table(oracle, tree):
    sc = S2.decision_scene(oracle)
    refs = S2.reference(tree, sc)
    for case, ref in zip(S2.DECISION_CASES, refs):
        c = ref["cams"][0]
        n, rot, rel = case
        assert c["n_corr"] == n, case
        if n >= 10:
            assert (c["rot_inliers"], c["rel_inliers"]) == (rot, rel), (case, c["rot_inliers"], c["rel_inliers"])
            assert c["rot_best"] == (0 if rot else -1) and c["rel_best"] == (0 if rel else -1), case
        else:
            assert (c["rot_best"], c["rot_inliers"], c["rel_best"], c["rel_inliers"]) == (-1, 0, -1, 0)
            assert np.all(c["rot_hyp_inliers"] == -1) and np.all(c["state"][c["match1"] >= 0] == 1)
        got = (c["branch"], ref["success"], ref["total_inliers"], ref["rotation_only"])
        assert got == S2.DECISION_EXPECT[case], (case, got)
        assert ref["cams"][1]["branch"] == 0 and ref["cams"][1]["n_corr"] == 0
        fr1 = sc["pairs"][refs.index(ref)][0]["fr1"]
        kicked = int((c["landmark1_out"] != fr1["lm"]).sum())
        taken = rot if c["branch"] == 1 else rel
        assert kicked == (n - taken if ref["success"] else 0), (case, kicked)
    for ref, want in zip(refs[len(S2.DECISION_CASES):], S2.ORDER_EXPECT):
        assert [c["removed"] for c in ref["cams"]] == want["removed"]
        assert (ref["total_inliers"], ref["rotation_only"], ref["success"]) == (want["total"], want["rotation_only"], want["success"])
    # equal counts: the first wins; a better one later wins; no inlier anywhere; all-invalid lists
    n_single = len(S2.DECISION_CASES)
    twice = S2.reference(tree, S2.decision_scene(oracle, "twice"))
    later = S2.reference(tree, S2.decision_scene(oracle, "better later"))
    for case, a, b in zip(S2.DECISION_CASES, twice[:n_single], later[:n_single]):
        n, rot, rel = case
        if n >= 10:
            assert (a["cams"][0]["rot_best"], a["cams"][0]["rel_best"]) == (0 if rot else -1, 0 if rel else -1)
            assert (b["cams"][0]["rot_best"], b["cams"][0]["rel_best"]) == (1 if rot else -1, 1 if rel else -1)
            assert a["total_inliers"] == b["total_inliers"] == S2.DECISION_EXPECT[case][2]
    for kind, invalid in (("far", False), ("true first", True)):
        for ref in S2.reference(tree, S2.decision_scene(oracle, kind, invalid)):
            assert (ref["total_inliers"], ref["rotation_only"], ref["success"]) == (-1, 1, 0)
            assert all(c["rot_best"] == -1 and c["rel_best"] == -1 and c["branch"] in (0, 2) for c in ref["cams"])
            if invalid:
                assert all(np.all(c["rot_hyp_inliers"] == -1) for c in ref["cams"])


@pytest.mark.parametrize("tree", TREES)
def test_knife_edges_flip_one_count(oracle, tree):
    sc = S2.knife_rotation(oracle, tree)
    cam = sc["pairs"][0][0]
    c = S2.reference(tree, sc)[0]["cams"][0]
    lo, hi = cam["fr0"]["kps"]["size"][cam["probes"]]
    assert np.nextafter(lo, hi) == hi
    assert c["n_corr"] == 14 and c["branch"] == 1 and c["rot_inliers"] == 13 and c["rel_inliers"] == 0
    assert list(c["state"][cam["probes"]]) == [1, 2]
    d = c["distance"][cam["probes"]]
    assert d[1] < R2.THRESHOLD <= d[0]
    sc = S2.knife_relative(oracle, tree)
    cam = sc["pairs"][0][0]
    c = S2.reference(tree, sc)[0]["cams"][0]
    H = cam["rel_H"]
    assert np.nextafter(H[0][7], H[1][7]) == H[1][7] and np.array_equal(np.delete(H[0], 7), np.delete(H[1], 7))
    assert c["n_corr"] == 13 and c["branch"] == 2 and c["rot_inliers"] == 0
    assert c["rel_hyp_inliers"][0] == c["rel_hyp_inliers"][1] + 1 >= 10
    col = list(c["corr"]["kA"]).index(cam["probe"])
    assert c["rel_dist"][0, col] < R2.THRESHOLD <= c["rel_dist"][1, col]
    same = (c["rel_dist"][0] < R2.THRESHOLD) == (c["rel_dist"][1] < R2.THRESHOLD)
    assert np.all(same | (np.arange(13) == col))


def test_chunk_and_edge_scene_counts(oracle):
    chunk = capi.Frontend._test_ransac2d2d_chunk_records()
    refs = S2.reference(True, S2.chunk_scene(oracle, chunk))
    assert [r["cams"][0]["n_corr"] for r in refs] == [chunk - 1, chunk, chunk + 1, 2 * chunk + 1]
    assert all(r["cams"][0]["rel_best"] == 0 and r["cams"][0]["removed"] == 1 for r in refs)
    refs = S2.reference(True, S2.edge_scene(oracle))
    assert [r["cams"][0]["n_corr"] for r in refs] == [0, 0, 1, S2.K]
    assert refs[3]["success"] and refs[2]["total_inliers"] == -1


@pytest.mark.parametrize("tree", TREES)
def test_general_scenes_margins_and_outcomes(oracle, tree):
    """float64 and longdouble agree on every inlier verdict whose relative margin to the threshold exceeds 1e-9, at most
    1 % of the verdicts sit inside that margin, and at least three pairs end in each of: branch 1 with success,
    branch 2 with success, -1"""
    total = inside = 0
    ends = dict(rotation=0, relative=0, failed=0)
    census = R2.new_census()
    for spec in S2.GENERAL_SPECS:
        sc = S2.general_scene(oracle, spec)
        refs = S2.reference(tree, sc, census=census)
        for pair, ref in zip(sc["pairs"], refs):
            for cam, rc in zip(pair, ref["cams"]):
                v64, vld, margin = R2.margins(tree, cam["rot_H"], cam["rel_H"], rc["corr"])
                clear = margin > 1.0e-9
                assert np.array_equal(v64[clear], vld[clear]), sc["name"]
                assert not np.any(v64[np.isnan(margin)])  # (a NaN distance is an outlier in both)
                total += margin.size
                inside += int((~clear & ~np.isnan(margin)).sum())
                if len(cam["fr0"]["kps"]):
                    assert rc["n_corr"] >= 25, (sc["name"], rc["n_corr"])
            if ref["total_inliers"] < 0:
                ends["failed"] += 1
            elif ref["success"] & 2:
                ends["relative"] += 1
            else:
                ends["rotation"] += 1
            print(sc["name"], [(c["n_corr"], c["rot_inliers"], c["rel_inliers"], c["branch"]) for c in ref["cams"]],
                  ref["total_inliers"], ref["rotation_only"], ref["success"])
    print("verdicts", total, "inside the margin", inside, ends, census)
    assert total > 20000 and inside <= 0.01 * total
    assert min(ends.values()) >= 3, ends
    for key in ("no_id_1", "no_id_0", "id_not_in_map", "duplicate_id_in_current", "removed_row"):
        assert census[key] >= FLOOR, (key, census)


def test_the_mirror_and_the_driver_are_declared():
    mirror = open(os.path.join(ROOT, "okvis2_amd", "host", "okvfe_frontend.hpp")).read()
    assert "void ransac2d2dBlocks(" in mirror and NAME + "(" in mirror
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "ransac2d2d_cli.cpp" in entry
