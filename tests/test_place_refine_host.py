"""CPU: okvis2_amd/csrc/place_refine_dev.h compiled into a stand-alone host program (tests/cpp/place_refine_step_main.cpp,
-ffp-contract=off as the library) against the numpy restatement tests/place_refine_ref.py, byte for byte and under both
orders of the FP64 sums.  The program is the solver alone: it is fed the evaluation records (cost, g, A, n_terms) the
restatement computed, in the order it asked for them, and after every call its whole per-multiframe record must equal
the restatement's state at that point: the pose, the cost, g, A, the scaling, the radius, nu, the function-tolerance
flag, both counters, the candidate and its model change; after the last call the status, pose, counts and costs.
Scenes: noisy, far, wild, directed, no-term and conversion (the census of test_place_refine_ref.py holds every reachable
branch to at least 16 occurrences in them).  The same program built with -fsanitize=address,undefined ends clean.
And the boundary of okvfe_place_refine_blocks_device: exported, declared, bound, its argument errors that need no device,
and the pipelined-lanes audit classifies it as joining."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import place_hessian_scenes as HS
import place_refine_ref as PR
import place_refine_scenes as RS
from okvis2_amd import capi
from test_capi_join_audit import classify

NAME = "okvfe_place_refine_blocks_device"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "place_refine_step_main.cpp")
EVAL = np.dtype([("cost", "<f8"), ("g", "<f8", 6), ("a", "<f8", 21), ("n_terms", "<i4"), ("n_singular", "<i4")])
RECORD = np.dtype([("x", "<f8", 7), ("cost", "<f8"), ("cost0", "<f8"), ("g", "<f8", 6), ("a", "<f8", 21), ("S", "<f8", 6),
                   ("radius", "<f8"), ("nu", "<f8"), ("xc", "<f8", 7), ("model_change", "<f8"), ("start", "<f8", 7),
                   ("function_tolerance", "<i4"), ("it", "<i4"), ("n_acc", "<i4"), ("status", "<i4"), ("pending", "<i4"),
                   ("n_terms", "<i4"), ("bad_best", "<i4"), ("pad", "<i4")])
assert EVAL.itemsize == 232 and RECORD.itemsize == 504
RUNNING = -1
SCENES = ("noisy", "far", "wild", "directed", "no_term", "conversion")


def _build(d, name, extra):
    exe = d / name
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + ROOT, *extra, "-o", str(exe), SOURCE]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("place_refine_host")
    return d, _build(d, "place_refine_step_main", []), _build(
        d, "place_refine_step_main_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _upper(A):
    return np.array([A[i, j] for i, j in PR.UPPER])


def _traced(oracle, tree, sc):
    """the restatement over the verified multiframes of a scene with a hook around refine's `evaluate` (through
    place_refine_ref.accumulate, which only it calls): per multiframe the reference and, per evaluation, its result and
    the locals of refine at the moment it asked"""
    keep = ("x", "cost", "cost0", "g", "A", "S", "radius", "nu", "function_tolerance", "it", "n_acc", "model_change", "xc")
    original = PR.accumulate
    out = []
    for mf in sc["mfs"]:
        if mf["verdict"] != 3:
            continue
        trace = []

        def hooked(res, jac):
            got = original(res, jac)
            ev = sys._getframe(1)                                   # refine's evaluate(pose)
            loc = ev.f_back.f_locals                                # refine
            trace.append(dict(cost=got[0], g=got[1].copy(), a=_upper(got[2]), n_terms=ev.f_locals["ev"]["n_terms"],
                              pose=np.array(ev.f_locals["pose"], dtype=np.float64),
                              state={k: np.array(loc[k], dtype=np.float64) for k in keep if loc.get(k) is not None}))
            return got

        PR.accumulate = hooked
        try:
            ref = PR.refine(oracle, tree, sc["hp"], mf["frames"], mf["ml"], mf["state"], sc["cams"], sc["T_SC_params"],
                            mf["hyp"], mf["best"], None, sc["max_iterations"], True)
        finally:
            PR.accumulate = original
        out.append((mf, ref, trace))
    return out


_TRACES = {}


def _scene_traces(oracle, tree, kind):
    key = (kind, tree)
    if key not in _TRACES:
        sc = getattr(RS, kind + "_scene")(oracle)
        _TRACES[key] = (sc, _traced(oracle, tree, sc))
    return _TRACES[key]


def _request(path, tree, sc, traced, initial=False):
    with open(path, "wb") as f:
        f.write(struct.pack("<iii", int(tree), len(traced), sc["max_iterations"]))
        for mf, ref, trace in traced:
            bad = not 0 <= int(mf["best"]) < len(mf["hyp"])
            if bad:
                f.write(struct.pack("<ii", 2, len(trace)))
            elif initial:
                f.write(struct.pack("<ii", 1, len(trace)))
                f.write(np.asarray(ref["start_pose"], dtype="<f8").tobytes())
            else:
                f.write(struct.pack("<ii", 0, len(trace)))
                f.write(np.asarray(mf["hyp"][mf["best"]], dtype="<f8").tobytes())
            ev = np.zeros(len(trace), EVAL)
            for k, t in enumerate(trace):
                ev[k]["cost"], ev[k]["g"], ev[k]["a"], ev[k]["n_terms"] = t["cost"], t["g"], t["a"], t["n_terms"]
            f.write(ev.tobytes())


def _check(records, traced, what):
    o = 0
    n_pending = 0
    for mi, (mf, ref, trace) in enumerate(traced):
        recs = records[o:o + len(trace)]
        o += len(trace)
        w = what + (mi,)
        assert HS.same_bytes(recs[0]["start"], ref["start_pose"]) and HS.same_bytes(trace[0]["pose"], ref["start_pose"]), w
        for k, rec in enumerate(recs[:-1]):
            # the record after call k waits for the evaluation of call k + 1: the restatement's state when it asked for it
            st, wk = trace[k + 1]["state"], w + (k,)
            assert rec["status"] == RUNNING and rec["pending"] == 1, wk
            assert HS.same_bytes(rec["xc"], trace[k + 1]["pose"]) and HS.same_bytes(rec["xc"], st["xc"]), wk
            for name in ("x", "cost", "cost0", "g", "S", "radius", "nu", "model_change"):
                assert HS.same_bytes(rec[name], st[name]), wk + (name, rec[name], st[name])
            assert HS.same_bytes(rec["a"], _upper(st["A"])), wk
            assert (int(rec["function_tolerance"]), int(rec["it"]), int(rec["n_acc"])) == (
                int(st["function_tolerance"]), int(st["it"]), int(st["n_acc"])), wk
            n_pending += 1
        last = recs[-1]
        assert last["pending"] == 0 and int(last["status"]) == ref["status"], (w, int(last["status"]), ref["status"])
        assert HS.same_bytes(last["x"], ref["pose"]), (w, last["x"], ref["pose"])
        assert HS.same_bytes(np.array([last["cost0"], last["cost"]]), ref["cost"]), w
        assert (int(last["it"]), int(last["n_acc"]), int(last["n_terms"])) == (ref["n_iterations"], ref["n_accepted"],
                                                                               ref["n_terms"]), w
    assert o == len(records)
    return n_pending


def _run(d, exe, oracle, tree, kind, initial=False):
    sc, traced = _scene_traces(oracle, tree, kind)
    req, resp = d / "req.bin", d / "resp.bin"
    _request(req, tree, sc, traced, initial)
    r = subprocess.run([str(exe), str(req), str(resp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (kind, r.returncode, r.stdout, r.stderr)
    records = np.fromfile(resp, RECORD)
    assert len(records) == sum(len(t) for _, _, t in traced), kind
    return traced, _check(records, traced, (kind, tree, initial))


@pytest.mark.parametrize("kind", SCENES)
def test_program_equals_the_restatement_after_every_call(programs, oracle, fp64_order, kind):
    d, exe, _ = programs
    tree = fp64_order == "eigen_tree"
    traced, n_pending = _run(d, exe, oracle, tree, kind)
    statuses = [ref["status"] for _, ref, _ in traced]
    if kind in ("noisy", "far", "wild"):
        assert n_pending >= 16 and set(statuses) <= {1, 2}
    if kind == "far":
        assert any(ref["n_accepted"] < ref["n_iterations"] for _, ref, _ in traced)        # rejected or invalid steps
    if kind == "directed":
        assert statuses == [4, 4] + [4] * RS.BAD_BEST
    if kind == "no_term":
        assert statuses == [3] * 16
    if kind == "noisy":                                             # the start given as a pose instead of a hypothesis
        _run(d, exe, oracle, tree, kind, initial=True)


def test_program_ends_clean_under_the_sanitizers(programs, oracle):
    """AddressSanitizer and UndefinedBehaviorSanitizer on the host program itself (its own main), every scene"""
    d, _, san = programs
    oracle.set_reduction(True)
    for kind in SCENES:
        _run(d, san, oracle, True, kind)


def test_program_refuses_a_request_that_ends_early(programs, oracle, tmp_path):
    """a multiframe whose solver still waits for an evaluation: exit status 3, not a made-up answer"""
    d, exe, _ = programs
    oracle.set_reduction(True)
    sc, traced = _scene_traces(oracle, True, "noisy")
    cut = [(mf, ref, trace[:1]) for mf, ref, trace in traced if len(trace) > 1][:1]
    assert cut
    req = tmp_path / "req.bin"
    _request(req, True, sc, cut)
    r = subprocess.run([str(exe), str(req), str(tmp_path / "resp.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3, (r.returncode, r.stderr)


def test_symbol_exported_declared_and_bound():
    lib = C.CDLL(capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "okvfe.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert hasattr(lib, NAME) and re.search(r"\b%s\s*\(" % NAME, code) and NAME in capi.EXPORTS
    assert "#define OKVFE_ABI_VERSION 8" in header and capi.ABI_VERSION == 8
    assert "typedef struct okvfe_place_refine_device" in code
    assert len(getattr(capi.lib(), NAME).argtypes) == 17
    assert C.sizeof(capi.PlaceRefineDevice) == 9 * C.sizeof(C.c_void_p)
    assert [n for n, _ in capi.PlaceRefineDevice._fields_] == ["poses", "status", "n_iterations", "n_accepted", "n_terms", "cost",
                                                               "start_poses", "H", "n_singular"]
    fields = re.search(r"typedef struct okvfe_place_refine_device \{(.*?)\}", code, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", fields) == [n for n, _ in capi.PlaceRefineDevice._fields_]
    # the header states the deviations, what is unpinned, the launch count and where H is taken
    for text in ("DEFINED DEVIATIONS from ceres", "DENSE_QR", "max |g_j|", "PARITY UNPINNED: ceres' loop",
                 "2 max_iterations", "at result->poses", "it >= max_iterations", "no tree over the"):
        assert text in header, text
    mirror = open(os.path.join(ROOT, "okvis2_amd", "host", "okvfe_frontend.hpp")).read()
    assert NAME + "(" in mirror and "verifyPlaceRefineBlocks(" in mirror
    assert "place_refine_cli.cpp" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "k_place_refine.hip" in open(os.path.join(ROOT, "okvis2_amd", "csrc", "Makefile")).read()


def test_a_null_context_is_invalid_before_any_device_work():
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    pset = capi.Frontend.make_place_set_device(0, None)
    res = capi.Frontend.make_place_refine_device(a, a)
    cams = (C.c_int32 * 1)(0)
    f = getattr(capi.lib(), NAME)
    assert f(None, C.byref(pset), buf, 1, 1, cams, buf, buf, 1, buf, None, buf, buf, None, 10, C.byref(res),
             None) == capi.ERR_INVALID_ARGUMENT
    assert f(None, None, None, -1, 0, None, None, None, 0, None, None, None, None, None, -1, None, None) == capi.ERR_INVALID_ARGUMENT


def test_the_entry_point_joins_the_pipelined_lanes():
    joins, missing, unclassified = classify()
    assert NAME in joins and not missing and not unclassified
