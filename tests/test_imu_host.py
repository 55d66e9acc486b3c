"""CPU: okvis2_amd/csrc/imu_dev.h compiled into a stand-alone host program (tests/cpp/imu_propagation_main.cpp,
-ffp-contract=off as the library) against the numpy restatement tests/imu_ref.py: byte for byte on every scene of
tests/imu_scenes.py, a NaN standing for any NaN, under both orders of the FP64 sums and in all three forms, no row
exempt; the same program built with -fsanitize=address,undefined ends clean; and the library's host entry
okvfe_imu_propagation gives the same bytes."""
import os
import subprocess

import numpy as np
import pytest

import imu_scenes as SC
from okvis2_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "imu_propagation_main.cpp")
FORMS = dict(mean=(False, False), jacobian=(True, False), covariance=(True, True))


def _build(d, name, extra):
    exe = d / name
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + ROOT, *extra, "-o", str(exe), SOURCE]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("imu_host")
    return d, _build(d, "imu_propagation_main", []), _build(
        d, "imu_propagation_main_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _compare(got, refs, n_cams, form, what):
    jacobian, covariance = FORMS[form]
    want = SC.expected(refs, n_cams, jacobian=jacobian, covariance=covariance)
    for k, w in want.items():
        if not SC.same_bytes(got[k], w):
            bad = [m for m in range(len(refs)) if not SC.same_bytes(got[k][m], w[m])]
            raise AssertionError((what, form, k, "multiframes", bad[:8], len(bad)))


def _run(d, exe, sc, refs, tree, form, what):
    jacobian, covariance = FORMS[form]
    req, resp = d / "req.bin", d / "resp.bin"
    SC.write_request(req, sc["mfs"], sc["T_SC_params"], tree, jacobian, covariance)
    r = subprocess.run([str(exe), str(req), str(resp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (what, r.returncode, r.stdout, r.stderr)
    _compare(SC.read_response(resp, len(sc["mfs"]), len(sc["T_SC_params"])), refs, len(sc["T_SC_params"]), form, what)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("tree", [True, False], ids=["eigen_tree", "left_to_right"])
def test_program_equals_the_restatement_byte_for_byte(programs, tree, form):
    d, exe, _ = programs
    refs, _ = SC.references(tree)
    for sc, rf in zip(SC.scenes(), refs):
        _run(d, exe, sc, rf, tree, form, sc["name"])
    mixed = SC.mixed_batch()
    _run(d, exe, mixed, [SC.reference_one(tree, mf, mixed["T_SC_params"]) for mf in mixed["mfs"]], tree, form, "mixed")


def test_program_ends_clean_under_the_sanitizers(programs):
    """AddressSanitizer and UndefinedBehaviorSanitizer on the host program itself (its own main), every scene"""
    d, _, san = programs
    refs, _ = SC.references(True)
    for sc, rf in zip(SC.scenes(), refs):
        for form in FORMS:
            _run(d, san, sc, rf, True, form, ("sanitizers", sc["name"]))


@pytest.mark.parametrize("tree", [True, False], ids=["eigen_tree", "left_to_right"])
def test_library_host_entry_equals_the_restatement(tree):
    """okvfe_imu_propagation of libokvfe.so (no context, no device work): the seam of ViFrontendInterface::propagation"""
    refs, _ = SC.references(tree)
    for sc, rf in zip(SC.scenes(), refs):
        samples, begin, states = SC.pack(sc["mfs"])
        n_cams = len(sc["T_SC_params"])
        for form, (jacobian, covariance) in FORMS.items():
            got = capi.imu_propagation(SC.PARAMS, samples, begin, states, sc["T_SC_params"], eigen_tree=tree,
                                       jacobian=jacobian, covariance=covariance)
            want = SC.expected(rf, n_cams, jacobian=jacobian, covariance=covariance)
            for k, w in want.items():
                if got[k] is None:
                    assert bool((w == SC.SENTINEL).all()), (form, k)
                    continue
                g = got[k].reshape(w.shape)
                untouched = w == SC.SENTINEL                        # the wrapper's own fill there: NaN, or -1
                fill = np.isnan(g) if g.dtype.kind == "f" else g == -1
                assert bool(fill[untouched].all()), (sc["name"], form, k)
                assert SC.same_bytes(np.where(untouched, w, g), w), (sc["name"], form, k)
    # B = 1 with one multiframe's samples alone, and the argument checks
    mf, r = SC.scenes()[1]["mfs"][0], refs[1][0]
    samples, begin, states = SC.pack([mf])
    one = capi.imu_propagation(SC.PARAMS, samples, begin, states, SC.scenes()[1]["T_SC_params"], eigen_tree=tree)
    assert SC.same_bytes(one["pose"][0], r["pose"]) and SC.same_bytes(one["covariance"][0], r["covariance"].reshape(-1))
    assert SC.same_bytes(one["gravity_C"][0], r["gravity_C"])
    with pytest.raises(capi.OkvfeError):
        capi.imu_propagation(SC.PARAMS, samples, np.array([3, 0], np.int32), states)
    empty = capi.imu_propagation(SC.PARAMS, np.zeros((0, 8)), np.zeros(1, np.int32), np.zeros((0, 18)))
    assert empty["pose"].shape == (0, 7)
