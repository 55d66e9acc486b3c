"""CPU: the boundary of okvfe_place_hessian_blocks_device (the Hessian H of Frontend::verifyRecognisedPlace and its
terms): exported, declared, bound; argument errors that need no device; the pipelined-lanes audit classifies it as
joining.  And the restatement the GPU tier is compared with (place_hessian_ref.py) on its own: its minimal Jacobian
against central differences of its residual under PoseManifold::plus, the census floors of the scenes
(place_hessian_scenes.py), the symmetry of H, the defined NaN rows and the unverified multiframes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import place_hessian_ref as PH
import place_hessian_scenes as HS
import ransac_scenes as S
from okvis2_amd import capi
from test_capi_join_audit import classify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "okvfe_place_hessian_blocks_device"
FLOOR = 16
TREES = (True, False)


def test_symbol_exported_declared_and_bound():
    lib = C.CDLL(capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "okvfe.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert hasattr(lib, NAME) and re.search(r"\b%s\s*\(" % NAME, code) and NAME in capi.EXPORTS
    assert "#define OKVFE_ABI_VERSION 8" in header and capi.ABI_VERSION == 8
    assert "typedef struct okvfe_place_hessian_device" in code
    assert len(getattr(capi.lib(), NAME).argtypes) == 13
    assert C.sizeof(capi.PlaceHessianDevice) == 5 * C.sizeof(C.c_void_p)
    assert [n for n, _ in capi.PlaceHessianDevice._fields_] == ["H", "n_terms", "n_singular", "residual", "jacobian_minimal"]
    for method in ("place_hessian_blocks_device", "make_place_hessian_device"):
        assert callable(getattr(capi.Frontend, method)), method
    assert "okvfe_test_place_hessian_chunk_terms" in capi.TEST_HOOKS and "okvfe_test_place_hessian_chunk_terms" not in header
    assert capi.Frontend._test_place_hessian_chunk_terms() >= 64
    # the header says what the call defines where the reference reads indeterminate memory, and what it leaves out
    for text in ("DEFINED DEVIATION", "n_singular", "fabs(head[2]) < 1.0e-12", "not a positive finite number",
                 "PARITY UNPINNED: they are Eigen's", "PoseManifold::minusJacobian", "no tree over the terms"):
        assert text in header, text
    mirror = open(os.path.join(ROOT, "okvis2_amd", "host", "okvfe_frontend.hpp")).read()
    assert NAME + "(" in mirror and "verifyPlaceHessianBlocks(" in mirror
    assert "place_hessian_cli.cpp" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "k_place_hessian.hip" in open(os.path.join(ROOT, "okvis2_amd", "csrc", "Makefile")).read()


def test_a_null_context_is_invalid_before_any_device_work():
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    pset = capi.Frontend.make_place_set_device(0, None)
    res = capi.Frontend.make_place_hessian_device(a, a, a)
    cams = (C.c_int32 * 1)(0)
    f = getattr(capi.lib(), NAME)
    assert f(None, C.byref(pset), buf, 1, 1, cams, buf, buf, buf, buf, None, C.byref(res), None) == capi.ERR_INVALID_ARGUMENT
    assert f(None, None, None, -1, 0, None, None, None, None, None, None, None, None) == capi.ERR_INVALID_ARGUMENT


def test_the_entry_point_joins_the_pipelined_lanes():
    joins, missing, unclassified = classify()
    assert NAME in joins and not missing and not unclassified


@pytest.fixture(scope="module")
def general(oracle):
    return {spec: HS.general_scene(oracle, spec, n_mf=1) for spec in S.GENERAL_SPECS}


# Largest relative deviation measured on these scenes (four camera models, 1010 terms, both orders of the sums), with
# the step 1e-6 and the deviation of a term taken as max |analytic - numeric| / max |analytic| over its 2 x 6 entries:
# 5.3e-9 (5.264e-9 and 5.255e-9 under the two orders).  The bound is ten times that, 5.3e-8, far below the 1e-4 of the
# reference's own analytic-versus-numeric camera tests (okvis_cv/test/TestPinholeCamera.cpp).
JACOBIAN_BOUND = 5.3e-8


@pytest.mark.parametrize("tree", TREES)
def test_minimal_jacobian_against_central_differences(oracle, general, tree):
    """d residual / d delta of PoseManifold::plus(pose, delta) at delta = 0, by central differences of the restatement's
    own residual"""
    h = 1.0e-6
    worst, n_terms, n_negated = 0.0, 0, 0
    for spec, sc in general.items():
        mf = sc["mfs"][0]
        at = lambda pose: PH.evaluate(oracle, tree, sc["hp"], mf["frames"], mf["ml"], mf["state"], sc["cams"],
                                      sc["T_SC_params"], pose)
        ref = at(mf["pose"])
        assert ref["n_singular"] == 0 and ref["n_terms"] >= FLOOR
        num = [np.zeros((len(r), 2, 6)) for r in ref["rows"]]
        for i in range(6):
            d = np.zeros(6)
            d[i] = h
            hi, lo = at(PH.pose_plus(mf["pose"], d)), at(PH.pose_plus(mf["pose"], -d))
            for c in range(len(sc["cams"])):
                num[c][:, :, i] = (hi["residual"][c] - lo["residual"][c]) / (2.0 * h)
        for c in range(len(sc["cams"])):
            ana = ref["jacobian"][c].reshape(-1, 2, 6).copy()
            if not len(ana):
                continue
            # projectHomogeneous negates the head of a point with w < 0 and hands back the Jacobian of the negated head
            # (PinholeCamera.hpp:514-524): the reference's analytic Jacobian of such a term is minus the derivative
            negated = sc["hp"][mf["ml"][c][ref["rows"][c]], 3] < 0
            n_negated += int(negated.sum())
            ana[negated] = -ana[negated]
            dev = np.abs(ana - num[c]).max(axis=(1, 2)) / np.abs(ana).max(axis=(1, 2))
            worst = max(worst, float(dev.max()))
            n_terms += len(ana)
    print("largest relative deviation %.3e over %d terms, %d of them with w < 0" % (worst, n_terms, n_negated))
    assert n_terms >= 400 and n_negated >= FLOOR and worst < JACOBIAN_BOUND, worst


def test_scenes_reach_every_branch(oracle):
    census = PH.new_census()
    sc = HS.directed_scene(oracle)
    refs = HS.reference(oracle, True, sc, census=census)
    print(census)
    for key in PH.CENSUS:
        assert census[key] >= FLOOR, (key, census)
    verified, rejected, few, other = refs
    n_cams = len(sc["cams"])
    # the singular depths and the four bad sizes of every camera, and nothing else, are the defined NaN rows
    assert verified["n_singular"] == n_cams * HS.COPIES * (1 + len(HS.BAD_SIZES))
    assert other["n_singular"] == n_cams * HS.COPIES * len(HS.BAD_SIZES)  # (at another pose no depth is singular)
    assert verified["n_terms"] == n_cams * HS.COPIES * 16 and np.all(np.isnan(verified["H"]))
    for c in range(n_cams):
        nan = np.isnan(verified["jacobian"][c]).all(axis=1)
        assert np.array_equal(nan, np.isnan(verified["residual"][c]).all(axis=1))
        assert int(nan.sum()) == HS.COPIES * (1 + len(HS.BAD_SIZES))
        assert not np.isnan(verified["jacobian"][c][~nan]).any()
        assert np.all(verified["jacobian"][c].reshape(-1, 2, 6)[~nan][:, :, :3].any(axis=(1, 2)))
    # not verified: zeros, whatever the rows say
    for ref in (rejected, few):
        assert ref["n_terms"] == 0 and ref["n_singular"] == 0 and not ref["H"].any()
    # the general scenes: a mix of verdicts, terms in every camera, blocks of K and of 0 keypoints
    for spec in S.GENERAL_SPECS:
        g = HS.general_scene(oracle, spec)
        assert len(g["mfs"]) == HS.BATCH[spec]
        refs = HS.reference(oracle, True, g)
        assert refs[0]["n_terms"] >= FLOOR and all(r["n_singular"] == 0 for r in refs)
        assert [r["n_terms"] > 0 for r in refs] == [mf["verdict"] == 3 for mf in g["mfs"]]
        sizes = {len(f["kps"]) for mf in g["mfs"] for f in mf["frames"]}
        assert HS.K in sizes and (0 in sizes or len(g["cams"]) == 1)
    assert sorted(HS.BATCH.values()) == [1, 3, 3, 17] and sorted(len(S.rig(s)[0]) for s in HS.BATCH) == [1, 1, 2, 5]


@pytest.mark.parametrize("tree", TREES)
def test_hessian_is_symmetric_byte_for_byte(oracle, general, tree):
    for sc in list(general.values()) + [HS.pose_scene(oracle)]:
        for ref in HS.reference(oracle, tree, sc):
            H = ref["H"]
            assert HS.same_bytes(H, H.T), sc["name"]
            if not np.isnan(H).any() and ref["n_terms"] >= 6:
                assert np.all(np.linalg.eigvalsh(H) > -1e-9 * np.abs(H).max()), sc["name"]


def test_term_counts_and_poses_of_the_edge_scenes(oracle):
    chunk = capi.Frontend._test_place_hessian_chunk_terms()
    totals = (chunk - 1, chunk, chunk + 1, 600)
    refs = HS.reference(oracle, True, HS.term_count_scene(oracle, totals))
    assert [r["n_terms"] for r in refs] == list(totals)
    refs = HS.reference(oracle, True, HS.block_size_scene(oracle))
    assert [r["n_terms"] for r in refs] == [1 + HS.K, HS.K + 1, 1 + HS.K, 0, 3] and not refs[3]["H"].any()
    true, scaled, zero, nan_t, nan_q = HS.reference(oracle, True, HS.pose_scene(oracle))
    # normalize() takes the scale out up to rounding; a zero quaternion is left alone and gives another matrix
    assert np.allclose(true["H"], scaled["H"], rtol=1e-9) and not np.allclose(true["H"], zero["H"], rtol=1e-3)
    assert not np.isnan(zero["H"]).any() and np.isnan(nan_q["H"]).all() and np.isnan(nan_t["H"]).any()
    assert nan_q["n_singular"] == 0 and nan_q["n_terms"] == true["n_terms"] >= FLOOR
