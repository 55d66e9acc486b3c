"""CPU: okvis2_amd/csrc/ransac2d2d_hyp_dev.h compiled into a stand-alone host program
(tests/cpp/ransac2d2d_hyp_main.cpp, -ffp-contract=off as the library) against the restatement
tests/ransac2d2d_hyp_ref.py, byte for byte and under both orders of the FP64 sums, on the directed, the count and one
general scene of the device tests: the program is fed the correspondence lists the restatement built and must return
its hypotheses, samples, root counts and validity.  The same program built with -fsanitize=address,undefined ends clean.
okvfe_twopt_rotation_hypothesis and okvfe_fivept_hypothesis (the library's host entry points) equal the restatement on the
same samples.  And the boundary of the three entry points: exported, declared, bound, their argument errors that need
no device, and the pipelined-lanes audit classifies the device call as joining."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import ransac2d2d_hyp_ref as H2
import ransac2d2d_hyp_scenes as HS
import ransac2d2d_scenes as S2
from okvis2_amd import capi
from test_capi_join_audit import classify

NAMES = ("okvfe_twopt_rotation_hypothesis", "okvfe_fivept_hypothesis", "okvfe_ransac2d2d_hypotheses_blocks_device")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "ransac2d2d_hyp_main.cpp")
RECORD = np.dtype([("b1", "<f8", 3), ("b2", "<f8", 3), ("s1", "<f8"), ("s2", "<f8"), ("kA", "<i4"), ("pad", "<i4")])
ANSWER = np.dtype([("M", "<f8", 9), ("H", "<f8", 12), ("rot_samples", "<i4", 2), ("rel_samples", "<i4", 8),
                   ("n_roots", "<i4"), ("rot_valid", "<i4"), ("rel_valid", "<i4"), ("pad", "<i4")])
assert RECORD.itemsize == 72 and ANSWER.itemsize == 224
N_HYP = 64   # all of them: the directed pairs reach their branches over the 64 of the census


def _build(d, name, extra):
    exe = d / name
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + ROOT, *extra, "-o", str(exe), SOURCE]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("ransac2d2d_hyp_host")
    return d, _build(d, "ransac2d2d_hyp_main", []), _build(
        d, "ransac2d2d_hyp_main_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _scenes(oracle):
    return HS.directed_scene(oracle), HS.count_scene(oracle), S2.general_scene(oracle, ("euroc", "euroc1"))


def _same(a, b):
    return np.array_equal(HS.bits(a), HS.bits(np.asarray(b, dtype=np.asarray(a).dtype)))


def _run(d, exe, tree, sc, refs):
    req, resp = d / "req.bin", d / "resp.bin"
    lists = [(pi, c, rc) for pi, ref in enumerate(refs) for c, rc in enumerate(ref)]
    with open(req, "wb") as f:
        f.write(struct.pack("<iiQ", int(tree), len(lists), HS.SEED))
        for pi, c, rc in lists:
            corr = rc["corr"]
            n = len(corr["kA"])
            f.write(struct.pack("<Qiiii", pi, c, N_HYP, n, 0))
            rec = np.zeros(n, RECORD)
            rec["b1"], rec["b2"], rec["s1"], rec["s2"], rec["kA"] = corr["b1"], corr["b2"], corr["s1"], corr["s2"], corr["kA"]
            f.write(rec.tobytes())
    r = subprocess.run([str(exe), str(req), str(resp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = np.fromfile(resp, ANSWER).reshape(len(lists), N_HYP)
    for i, (pi, c, rc) in enumerate(lists):
        w = (sc["name"], tree, pi, c)
        for key, ref_key in (("M", "rot_H"), ("H", "rel_H"), ("rot_samples", "rot_samples"), ("rel_samples", "rel_samples"),
                             ("n_roots", "n_roots"), ("rot_valid", "rot_valid"), ("rel_valid", "rel_valid")):
            assert _same(got[key][i], rc[ref_key][:N_HYP]), (w, key)
    return got


@pytest.mark.parametrize("tree", (True, False), ids=("eigen_tree", "left_to_right"))
def test_program_equals_the_restatement(programs, oracle, tree):
    d, exe, _ = programs
    valid = 0
    for sc in _scenes(oracle):
        if sc["name"] == "hyp-directed":   # every directed branch, the polynomial without a real root among them
            refs, census = HS.directed_reference(tree, sc)
            HS.assert_directed_branches(refs, census)
        else:
            refs = HS.reference(tree, sc)
        got = _run(d, exe, tree, sc, refs)
        valid += int(got["rel_valid"].sum())
    assert valid >= 300


def test_program_ends_clean_under_the_sanitizers(programs, oracle):
    """AddressSanitizer and UndefinedBehaviorSanitizer on the host program itself (its own main), every scene"""
    d, _, san = programs
    for sc in _scenes(oracle):
        _run(d, san, True, sc, HS.reference(True, sc))


def test_program_refuses_a_malformed_request(programs, tmp_path):
    d, exe, _ = programs
    req = tmp_path / "req.bin"
    req.write_bytes(struct.pack("<iiQ", 1, 1, 5) + struct.pack("<Qiiii", 0, 0, 4, 12, 0))  # the records are missing
    r = subprocess.run([str(exe), str(req), str(tmp_path / "resp.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2


@pytest.mark.parametrize("tree", (True, False), ids=("eigen_tree", "left_to_right"))
def test_library_entry_points_equal_the_restatement(oracle, tree):
    """okvfe_twopt_rotation_hypothesis and okvfe_fivept_hypothesis on the samples of the directed and a general scene"""
    n = 0
    for sc in (HS.directed_scene(oracle), S2.general_scene(oracle, ("euroc", "euroc1"))):
        for ref in HS.reference(tree, sc):
            for rc in ref:
                corr = rc["corr"]
                if rc["n_corr"] < 10:
                    continue
                row = {int(k): i for i, k in enumerate(corr["kA"])}
                for h in range(N_HYP):
                    idx = [row[int(k)] for k in rc["rot_samples"][h]]
                    M, valid = capi.twopt_rotation_hypothesis(corr["b1"][idx], corr["b2"][idx])
                    assert _same(M, rc["rot_H"][h]) and valid == rc["rot_valid"][h], (sc["name"], h, "two-point")
                    idx = [row[int(k)] for k in rc["rel_samples"][h]]
                    Hm, valid, n_roots = capi.fivept_hypothesis(corr["b1"][idx], corr["b2"][idx], corr["s1"][idx[5:]],
                                                                corr["s2"][idx[5:]], tree)
                    assert _same(Hm, rc["rel_H"][h]) and valid == rc["rel_valid"][h] and n_roots == rc["n_roots"][h], \
                        (sc["name"], h, "five-point")
                    n += 1
    assert n >= 200


def test_symbols_exported_declared_and_bound():
    lib = C.CDLL(capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "okvfe.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, code) and name in capi.EXPORTS, name
    assert "#define OKVFE_ABI_VERSION 8" in header and capi.ABI_VERSION == 8
    assert [len(getattr(capi.lib(), n).argtypes) for n in NAMES] == [4, 8, 19]
    fields = re.search(r"typedef struct okvfe_ransac2d2d_hypotheses_device \{(.*?)\}", code, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", fields) == [n for n, _ in capi.Ransac2d2dHypothesesDevice._fields_]
    assert C.sizeof(capi.Ransac2d2dHypothesesDevice) == 8 * C.sizeof(C.c_void_p)
    # the header states the algorithm, what is unpinned and the deviation, and no longer leaves the hypotheses out
    for text in ("DEVIATION from Stewenius", "pair_key 128 + c 2 + problem", "FULL pivoting", "at most 128 steps",
                 "even multiplicity is NOT found", "Horn's closed form", "(R-, +b^)", "the first on ties"):
        assert text in header, text
    assert "stay with the caller; opengv's adaptive stop" not in header
    assert "k_ransac2d2d_hyp.hip" in open(os.path.join(ROOT, "okvis2_amd", "csrc", "Makefile")).read()
    # the functions shared with the consensus exist once, in k_ransac2d2d.hip, whose translation unit holds the new kernel
    csrc = os.path.join(ROOT, "okvis2_amd", "csrc")
    assert '#include "k_ransac2d2d_hyp.hip"' in open(os.path.join(csrc, "k_ransac2d2d.hip")).read()
    for fn in ("void make_correspondence2(", "int id_lookup(", "void id_insert(", "double rotation_only_distance(",
               "void inverse_translation(", "double relative_pose_distance("):
        holders = [f for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip", ".cpp")) and fn in open(os.path.join(csrc, f)).read()]
        assert holders == ["k_ransac2d2d.hip"], (fn, holders)


def test_argument_errors_that_need_no_device():
    b = np.array([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8]] * 4)
    s = np.ones(3)
    M, Hm = np.full(9, 5.0), np.full(12, 5.0)
    valid, n_roots = C.c_uint8(7), C.c_int32(7)
    ptr = lambda a: a.ctypes.data
    two = capi.lib().okvfe_twopt_rotation_hypothesis
    good = [ptr(b), ptr(b), ptr(M), C.byref(valid)]
    for i in range(4):
        args = list(good)
        args[i] = None
        assert two(*args) == capi.ERR_INVALID_ARGUMENT, i
    assert valid.value == 7
    assert two(*good) == capi.OK and valid.value == 1 and np.array_equal(M, np.eye(3).reshape(-1))
    same = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0]])      # a cross product of norm 0: invalid, 9 zeros
    assert two(ptr(same), ptr(same), ptr(M), C.byref(valid)) == capi.OK and valid.value == 0 and not M.any()
    five = capi.lib().okvfe_fivept_hypothesis
    good = [ptr(b), ptr(b), ptr(s), ptr(s), 1, ptr(Hm), C.byref(valid), C.byref(n_roots)]
    valid.value = 7
    for i, bad in ((0, None), (1, None), (2, None), (3, None), (4, 2), (4, -1), (5, None), (6, None)):
        args = list(good)
        args[i] = bad
        assert five(*args) == capi.ERR_INVALID_ARGUMENT, i
    assert valid.value == 7 and n_roots.value == 7
    args = list(good)
    args[7] = None                                            # n_roots is optional
    assert five(*args) == capi.OK
    assert five(*good) == capi.OK and valid.value == 0 and not Hm.any()   # two distinct bearings only: a failed pivot
    # the device call without a context
    buf = (C.c_double * 64)()
    res = capi.Frontend.make_ransac2d2d_hypotheses_device(*[C.addressof(buf)] * 4)
    cams = (C.c_int32 * 1)(0)
    assert capi.lib().okvfe_ransac2d2d_hypotheses_blocks_device(
        None, buf, 1, buf, 1, 1, cams, cams, 1, cams, buf, buf, None, 0, None, 1, 50, C.byref(res), None) == capi.ERR_INVALID_ARGUMENT


def test_the_device_call_joins_the_pipelined_lanes():
    joins, missing, unclassified = classify()
    assert NAMES[2] in joins and not missing and not unclassified
