"""CPU: the boundary of okvfe_match_to_map_table_uninitialised_blocks_device (the second pass of matchToMap from a
device-resident landmark table, batched): exported, declared, bound; argument errors that need no device; the
pipelined-lanes audit classifies it as joining; the gate chain exists once in k_match.hip; and the frames and hand-built
pools the GPU tier feeds it (map_table_uninit_common.py) meet that tier's conditions on the oracle alone."""
import ctypes as C
import os
import re

import numpy as np

import map_scenes as S
import map_table_common as M
import map_table_uninit_common as U
from okvis2_amd import capi, synth
from test_capi_join_audit import classify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "okvfe_match_to_map_table_uninitialised_blocks_device"


def test_symbol_exported_declared_and_bound():
    lib = C.CDLL(capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "okvfe.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert hasattr(lib, NAME)
    assert re.search(r"\b%s\s*\(" % NAME, code)
    assert NAME in capi.EXPORTS
    assert "#define OKVFE_ABI_VERSION 8" in header
    assert callable(getattr(capi.Frontend, "match_to_map_table_uninitialised_blocks_device"))
    assert len(getattr(capi.lib(), NAME).argtypes) == 16
    mirror = open(os.path.join(ROOT, "okvis2_amd", "host", "okvfe_frontend.hpp")).read()
    assert "void matchToMapUninitialisedBlocks(" in mirror and NAME + "(" in mirror
    # the texts no longer list the second pass as missing
    assert "Not covered: the second pass" not in header
    assert "input of a later, batched pass" not in header


def test_null_context_or_table_is_an_invalid_argument():
    lib = capi.lib()
    t = capi.Frontend.make_landmark_table_device(0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    pool = capi.Frontend.make_landmark_pool_device()
    cams = (C.c_int32 * 1)(0)
    pose = capi.make_pose(np.eye(3).reshape(-1), np.zeros(3))
    buf = (C.c_int32 * 16)()
    args = (C.byref(t), C.byref(pool), buf, 1, cams, C.byref(pose), 0, None, None, buf, buf, buf, buf, buf, None)
    f = getattr(lib, NAME)
    assert f(None, *args) == capi.ERR_INVALID_ARGUMENT
    assert f(None, None, *args[1:]) == capi.ERR_INVALID_ARGUMENT


def test_the_entry_point_joins_the_pipelined_lanes():
    joins, missing, unclassified = classify()
    assert NAME in joins
    assert not missing and not unclassified


def _kernel_body(src, name):
    body = src[src.index("void %s(" % name):]
    return body[:body.index("\n}\n")]


def test_one_copy_of_the_gate_and_the_fold():
    """the reference's FP64 expression order of the gate exists once: both kernels call the shared functions"""
    src = open(os.path.join(ROOT, "okvis2_amd", "csrc", "k_match.hip")).read()
    assert src.count("nn[i] = n0[i] + n0[i]") == 1
    assert src.count("if (r.np_dist < best)") == 1  # the fold of the ranges
    assert src.count("bool uninit_gate(") == 1 and src.count("void uninit_visit(") == 1
    assert src.count("void uninit_fold_and_store(") == 1
    for kernel in ("match_to_map_uninit_kernel", "match_to_map_table_uninit_kernel"):
        body = _kernel_body(src, kernel)
        assert "uninit_visit(" in body and "uninit_fold_and_store(" in body, kernel
        assert "triangulate_fast(" not in body and "cross3(" not in body, kernel
    assert "uninit_gate(" in _kernel_body(src, "uninit_visit")
    pack = open(os.path.join(ROOT, "okvis2_amd", "csrc", "k_map.hip")).read()
    assert "void pack_uninit_frames_kernel(" in pack


def test_workspace_budget():
    """16 bytes per (frame, landmark) pair plus 4 per frame, sliced by the first pass's arithmetic"""
    src = open(os.path.join(ROOT, "okvis2_amd", "csrc", "okvfe_internal.h")).read()
    assert "static_assert(sizeof(MapUninitPacked) == 16" in src
    api = open(os.path.join(ROOT, "okvis2_amd", "csrc", "capi_map.cpp")).read()
    body = api[api.index("okvfe_status %s(" % NAME):]
    body = body[:body.index("\n}\n")]
    assert "nl * sizeof(MapUninitPacked) + sizeof(int32_t)" in body
    assert "map_table_slice_frames(per_frame, ctx->map_table_ws_limit, n_frames)" in body
    assert "map_table_workspace(" in body and "pick_stream(" in body and "ring_release(" in body


def test_scene_frames_meet_the_gpu_tiers_conditions(oracle):
    """On the oracle alone: with the frames of map_table_uninit_common.frame and the second pose, every general scene
    except radtan8 yields, in both modes, at least 100 matched keypoints of which at least 80 carry an hp, and
    already_matched >= 30.  Without `exclusive` a keypoint that carries a landmark does not take part (Frontend.cpp:1630)
    and the counter is zero by construction, so the counter is the one of the exclusive second pass on the same first
    pass, in both modes."""
    K = synth.euroc_config().max_kpts
    low = [10 ** 9] * 3
    for spec in S.GENERAL_SPECS:
        if spec[0] == "radtan8":
            continue
        sc = S.general_scene(*spec)
        P = M.scene_poses(sc)
        for exclusive, thr in S.MODES:
            ref = M.reference(oracle, sc, P[0], S.oracle_camera(sc["cam"]), exclusive, thr)
            fr = U.frame(oracle, sc, ref, sc["cam"], K - 100, 100, 1)
            assert len(fr["kps"]) <= K
            lm, _, _, hs, ctr = U.reference(oracle, sc["obs_desc"], ref, fr, U.second_pose(P[0]), sc["cam"], exclusive)
            ctr_x = U.reference(oracle, sc["obs_desc"], ref, fr, U.second_pose(P[0]), sc["cam"], True)[4]
            got = (int((lm >= 0).sum()), int(hs.sum()), ctr_x)
            print(spec, exclusive, got, ctr)
            low = [min(a, b) for a, b in zip(low, got)]
            assert got[0] >= 100 and got[1] >= 80 and got[2] >= 30, (spec, exclusive, got)
            assert exclusive or ctr == 0
            assert np.all(hs[lm < 0] == 0)
    print("minima", low)


def test_hand_built_gate_pools_reach_every_label(oracle):
    """the gate scenes through hand-built pools (rows truncated to two per landmark, a seventh of the landmarks
    status 1, the empty ones status 0) still reach every census label the untruncated scenes reach, 100 times each"""
    mine, theirs = U.gate_census(oracle)
    labels = oracle.census_labels()
    reached = [lab for lab, t in zip(labels, theirs) if t > 0]
    assert len(reached) == 17, reached
    for lab, m, t in zip(labels, mine, theirs):
        assert (m > 0) == (t > 0), lab
        if t > 0:
            assert m >= 100, (lab, int(m))
