"""CPU: the boundary of matchToMap from a device-resident landmark table (okvfe_landmark_table_check_device,
okvfe_match_to_map_table_blocks_device): exported, declared, bound; argument errors that need no device; the
pipelined-lanes audit classifies both as joining; the slicing arithmetic of the workspace; and the frames / poses the
GPU tier feeds it (map_table_common.py) meet that tier's conditions on the oracle alone."""
import ctypes as C
import os
import re

import numpy as np

import map_scenes as S
import map_table_common as M
from okvis2_amd import capi, synth
from test_capi_join_audit import classify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("okvfe_landmark_table_check_device", "okvfe_match_to_map_table_blocks_device")


def test_symbols_exported_declared_and_bound():
    lib = C.CDLL(capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "okvfe.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in capi.EXPORTS
    for n in ("okvfe_landmark_table_device", "okvfe_landmark_pool_device"):
        assert re.search(r"\}\s*%s\s*;" % n, code), n
    assert "#define OKVFE_ABI_VERSION 8" in header
    for attr in ("make_landmark_table_device", "landmark_table_check_device", "match_to_map_table_blocks_device"):
        assert callable(getattr(capi.Frontend, attr)), attr
    assert C.sizeof(capi.LandmarkTableDevice) == C.sizeof(capi.LandmarkTable) == 3 * 4 + 4 + 7 * 8
    assert C.sizeof(capi.LandmarkPoolDevice) == 6 * 8
    assert hasattr(lib, "okvfe_test_set_map_table_workspace_limit")  # the test hook: exported, not declared
    assert "okvfe_test_set_map_table_workspace_limit" not in header


def test_null_context_or_table_is_an_invalid_argument():
    lib = capi.lib()
    t = capi.Frontend.make_landmark_table_device(0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    assert lib.okvfe_landmark_table_check_device(None, C.byref(t), None) == capi.ERR_INVALID_ARGUMENT
    assert lib.okvfe_landmark_table_check_device(None, None, None) == capi.ERR_INVALID_ARGUMENT
    cams = (C.c_int32 * 1)(0)
    pose = capi.make_pose(np.eye(3).reshape(-1), np.zeros(3))
    buf = (C.c_int32 * 4)()
    args = (C.byref(t), buf, 1, cams, C.byref(pose), C.c_double(20.0), 0, None, None, buf, buf, None)
    assert lib.okvfe_match_to_map_table_blocks_device(None, *args) == capi.ERR_INVALID_ARGUMENT
    assert lib.okvfe_match_to_map_table_blocks_device(None, None, *args[1:]) == capi.ERR_INVALID_ARGUMENT


def test_both_entry_points_join_the_pipelined_lanes():
    joins, missing, unclassified = classify()
    for n in NAMES:
        assert n in joins, n
    assert not missing and not unclassified


def _slice_frames(per_frame, limit, n_frames):
    """okvfe_ctx.h: map_table_slice_frames"""
    fit = limit // per_frame if per_frame else n_frames
    return min(max(fit, 1), min(max(n_frames, 1), 65535))


def test_slicing_arithmetic_matches_the_source():
    src = open(os.path.join(ROOT, "okvis2_amd", "csrc", "okvfe_ctx.h")).read()
    body = src[src.index("inline int map_table_slice_frames"):]
    body = body[:body.index("\n}\n")]
    assert "limit / per_frame" in body and "65535" in body and "std::max<size_t>(fit, 1)" in body
    K = 700
    per_frame = 5000 * 32 + K * 4 + 4
    assert per_frame <= 5000 * 40  # the workspace budget: at most 40 bytes per (frame, landmark) pair
    assert _slice_frames(per_frame, 1 << 30, 3072) == 3072          # 3072 x 5000 fits in 1 GiB: one slice
    assert _slice_frames(per_frame, 1 << 30, 8192) == (1 << 30) // per_frame  # does not: slices
    assert _slice_frames(per_frame, 100, 64) == 1                    # never fewer than one frame
    assert _slice_frames(1500 * 32 + K * 4 + 4, 5 * (1500 * 32 + K * 4 + 4) + 100, 64) == 5  # the GPU tier's case
    assert _slice_frames(4, 1 << 30, 100000) == 65535               # a launch's grid.y
    assert _slice_frames(per_frame, 1 << 30, 1) == 1


def test_kernels_share_one_copy_of_the_preparation():
    """the reference's FP64 expression order exists once: both kernels call prepare_landmark"""
    src = open(os.path.join(ROOT, "okvis2_amd", "csrc", "k_map.hip")).read()
    assert src.count("acos_fixed(cosVC)") == 1
    for kernel in ("void prepare_landmarks_kernel(", "void prepare_landmarks_frames_kernel("):
        body = src[src.index(kernel):]
        assert "prepare_landmark<kRT8>(" in body[:body.index("\n}\n")], kernel


def test_scene_batches_meet_the_gpu_tiers_conditions(oracle):
    """on the oracle alone: every general scene dictates at least 100 matches for its first pose and has a frame whose
    3-D set is empty; the observing pose is one of the table's, bit for bit"""
    K = synth.euroc_config().max_kpts
    for spec in S.GENERAL_SPECS:
        sc = S.general_scene(*spec)
        P = M.scene_poses(sc)
        assert any(np.array_equal(P[1][0], np.asarray(C).reshape(-1)) and np.array_equal(P[1][1], r)
                   for C, r in sc["poses"][1:])
        empty = 0
        for exclusive, thr in S.MODES:
            refs = [M.reference(oracle, sc, p, S.oracle_camera(sc["cam"]), exclusive, thr) for p in P]
            want = S.dictated_frame(oracle, sc, refs[0], clutter=200)[3]
            assert (want >= 0).sum() >= 100, (spec, exclusive)
            assert len(want) > K  # (the dictated frame is cut into several frames)
            empty += sum(1 for r in refs if not (r["status"] == 1).any())
            assert (refs[1]["status"] == 1).sum() > 20 and (refs[3]["status"] == 1).sum() > 20, (spec, exclusive)
        assert empty >= 1, spec
