"""CPU: okvis2_amd/csrc/ransac_hyp_dev.h compiled into a stand-alone host program (tests/cpp/ransac_hyp_main.cpp,
-ffp-contract=off as the library) against the numpy restatement tests/ransac_hyp_ref.py, byte for byte and under both
orders of the FP64 sums, on every census scene of ransac_hyp_scenes.py: the program is fed the correspondence lists the
restatement built and must return its hypotheses, samples, solution counts and validity.  The same program built with
-fsanitize=address,undefined ends clean.  okvfe_p3p_hypothesis (the library's host entry point) equals the restatement
on the same samples.  And the boundary of the three entry points: exported, declared, bound, their argument errors that
need no device, and the pipelined-lanes audit classifies both device calls as joining."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import ransac_hyp_ref as RH
import ransac_hyp_scenes as HS
from okvis2_amd import capi
from test_capi_join_audit import classify

NAMES = ("okvfe_p3p_hypothesis", "okvfe_ransac3d2d_hypotheses_blocks_device", "okvfe_place_hypotheses_blocks_device")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "ransac_hyp_main.cpp")
RECORD = np.dtype([("p", "<f8", 3), ("b", "<f8", 3), ("sigma", "<f8"), ("cam", "<i4"), ("row", "<i4")])
ANSWER = np.dtype([("H", "<f8", 12), ("samples", "<i4", 4), ("n_solutions", "<i4"), ("valid", "<i4")])
assert RECORD.itemsize == 64 and ANSWER.itemsize == 120


def _build(d, name, extra):
    exe = d / name
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + ROOT, *extra, "-o", str(exe), SOURCE]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("ransac_hyp_host")
    return d, _build(d, "ransac_hyp_main", []), _build(
        d, "ransac_hyp_main_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


_REFS = {}


def _references(oracle, tree):
    """[(scene, n_hyp, gates, refs)]: every census scene, and the first general scene once more with gates 0, 1, 2"""
    if tree not in _REFS:
        out = []
        for sc, n_hyp in HS.census_scenes(oracle):
            out.append((sc, n_hyp, None, HS.reference(tree, sc, n_hyp)))
        sc, n_hyp = HS.census_scenes(oracle)[2]
        gates = [0, 1, 2][:len(sc["mfs"])]
        out.append((sc, n_hyp, gates, HS.reference(tree, sc, n_hyp, gates=gates)))
        _REFS[tree] = out
    return _REFS[tree]


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return np.array_equal(a.view(np.uint64)[~np.isnan(a)], b.view(np.uint64)[~np.isnan(b)]) and \
            np.array_equal(np.isnan(a), np.isnan(b))
    return np.array_equal(a, b)


def _run(d, exe, tree, sc, n_hyp, gates, refs):
    req, resp = d / "req.bin", d / "resp.bin"
    keys = HS.keys_of(sc)
    with open(req, "wb") as f:
        f.write(struct.pack("<iiQ", int(tree), len(sc["mfs"]), HS.SEED))
        for i, ref in enumerate(refs):
            corr = ref["corr"]
            n = len(corr["cam"])
            f.write(struct.pack("<Qiiiii", keys[i], n_hyp, len(sc["cams"]), HS.K, -1 if gates is None else gates[i], n))
            for Cm, r in sc["T_SC"]:
                f.write(np.asarray(Cm, "<f8").reshape(-1).tobytes() + np.asarray(r, "<f8").tobytes())
            rec = np.zeros(n, RECORD)
            rec["p"], rec["b"], rec["sigma"], rec["cam"], rec["row"] = corr["p"], corr["b"], corr["sigma"], corr["cam"], corr["row"]
            f.write(rec.tobytes())
    r = subprocess.run([str(exe), str(req), str(resp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = np.fromfile(resp, ANSWER).reshape(len(refs), n_hyp)
    for i, ref in enumerate(refs):
        w = (sc["name"], tree, gates, i)
        assert _same(got["H"][i], ref["H"]), (w, "H")
        assert np.array_equal(got["valid"][i], ref["valid"]), (w, "valid")
        assert np.array_equal(got["samples"][i], ref["samples"]), (w, "samples")
        assert np.array_equal(got["n_solutions"][i], ref["n_solutions"]), (w, "n_solutions")
    return got


@pytest.mark.parametrize("tree", (True, False), ids=("eigen_tree", "left_to_right"))
def test_program_equals_the_restatement(programs, oracle, tree):
    d, exe, _ = programs
    valid = 0
    for sc, n_hyp, gates, refs in _references(oracle, tree):
        valid += int(_run(d, exe, tree, sc, n_hyp, gates, refs)["valid"].sum())
    assert valid >= 1000


def test_program_ends_clean_under_the_sanitizers(programs, oracle):
    """AddressSanitizer and UndefinedBehaviorSanitizer on the host program itself (its own main), every scene"""
    d, _, san = programs
    for sc, n_hyp, gates, refs in _references(oracle, True):
        _run(d, san, True, sc, n_hyp, gates, refs)


def test_program_refuses_a_malformed_request(programs, tmp_path):
    d, exe, _ = programs
    req = tmp_path / "req.bin"
    req.write_bytes(struct.pack("<iiQ", 1, 1, 5) + struct.pack("<Qiiiii", 0, 4, 1, 256, -1, 3))  # the records are missing
    r = subprocess.run([str(exe), str(req), str(tmp_path / "resp.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2


@pytest.mark.parametrize("tree", (True, False), ids=("eigen_tree", "left_to_right"))
def test_library_p3p_equals_the_restatement(oracle, tree):
    """okvfe_p3p_hypothesis on the samples of the directed scene and of one general scene"""
    scenes = HS.census_scenes(oracle)
    n = 0
    for sc, n_hyp in (scenes[-1], scenes[3]):
        for ref in HS.reference(tree, sc, n_hyp):
            corr = ref["corr"]
            slot = corr["cam"] * HS.K + corr["row"]
            for h in range(n_hyp):
                if ref["samples"][h, 3] < 0:
                    continue
                idx = [int(np.flatnonzero(slot == s)[0]) for s in ref["samples"][h]]
                c = int(corr["cam"][idx[0]])
                H, valid, n_sol = capi.p3p_hypothesis(corr["p"][idx], corr["b"][idx], corr["sigma"][idx[3]], sc["T_SC"][c], tree)
                assert _same(H, ref["H"][h]) and valid == ref["valid"][h] and n_sol == ref["n_solutions"][h], (sc["name"], h)
                n += 1
    assert n >= 500


def test_symbols_exported_declared_and_bound():
    lib = C.CDLL(capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "okvfe.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, code) and name in capi.EXPORTS, name
    assert "#define OKVFE_ABI_VERSION 8" in header and capi.ABI_VERSION == 8
    assert [len(getattr(capi.lib(), n).argtypes) for n in NAMES] == [8, 13, 14]
    fields = re.search(r"typedef struct okvfe_ransac_hypotheses_device \{(.*?)\}", code, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", fields) == [n for n, _ in capi.RansacHypothesesDevice._fields_]
    assert C.sizeof(capi.RansacHypothesesDevice) == 5 * C.sizeof(C.c_void_p)
    # the header states the algorithm, what is unpinned and the deviation
    for text in ("A DEFINED ALGORITHM, PARITY UNPINNED", "0x9E3779B97F4A7C15", "DEVIATION from gp3p", "ROOT ORDER IS SOLUTION ORDER",
                 "at most 64 times", "at most 128 steps", "exactly 3 Newton steps", "the first on ties"):
        assert text in header, text
    assert "k_ransac_hyp.hip" in open(os.path.join(ROOT, "okvis2_amd", "csrc", "Makefile")).read()
    # the functions shared with the consensus exist once, in k_ransac.hip, whose translation unit holds the new kernel
    csrc = os.path.join(ROOT, "okvis2_amd", "csrc")
    assert '#include "k_ransac_hyp.hip"' in open(os.path.join(csrc, "k_ransac.hip")).read()
    for fn in ("bool make_correspondence(", "void invert_hypothesis(", "double ransac_distance("):
        holders = [f for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip", ".cpp")) and fn in open(os.path.join(csrc, f)).read()]
        assert holders == ["k_ransac.hip"], (fn, holders)


def test_argument_errors_that_need_no_device():
    P = np.arange(12, dtype=np.float64)
    pose = capi.make_pose(np.eye(3), np.zeros(3))
    H = np.zeros(12)
    valid, n_sol = C.c_uint8(7), C.c_int32(7)
    f = capi.lib().okvfe_p3p_hypothesis
    ptr = lambda a: a.ctypes.data
    good = [ptr(P), ptr(P), C.c_double(1.0), C.byref(pose), 1, ptr(H), C.byref(valid), C.byref(n_sol)]
    for i, bad in ((0, None), (1, None), (3, None), (4, 2), (4, -1), (5, None), (6, None)):
        args = list(good)
        args[i] = bad
        assert f(*args) == capi.ERR_INVALID_ARGUMENT, i
    assert valid.value == 7 and n_sol.value == 7
    args = list(good)
    args[7] = None                                            # n_solutions is optional
    assert f(*args) == capi.OK
    # collinear points: no valid hypothesis, 12 zeros
    H[:] = 5.0
    assert f(*good) == capi.OK and valid.value == 0 and not H.any()
    # the device calls without a context
    buf = (C.c_double * 64)()
    res = capi.Frontend.make_ransac_hypotheses_device(C.addressof(buf), C.addressof(buf))
    cams = (C.c_int32 * 1)(0)
    tab = capi.LandmarkTableDevice()
    pset = capi.Frontend.make_place_set_device(0, None)
    L = capi.lib()
    assert L.okvfe_ransac3d2d_hypotheses_blocks_device(None, C.byref(tab), buf, 1, 1, cams, C.byref(pose), buf, None, 1, 50,
                                                       C.byref(res), None) == capi.ERR_INVALID_ARGUMENT
    assert L.okvfe_place_hypotheses_blocks_device(None, C.byref(pset), buf, 1, 1, cams, C.byref(pose), buf, None, None, 1, 50,
                                                  C.byref(res), None) == capi.ERR_INVALID_ARGUMENT


def test_the_device_calls_join_the_pipelined_lanes():
    joins, missing, unclassified = classify()
    assert set(NAMES[1:]) <= set(joins) and not missing and not unclassified
