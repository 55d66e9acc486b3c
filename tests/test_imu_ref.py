"""CPU: the numpy restatement of ImuError::propagation (tests/imu_ref.py) on the scenes of tests/imu_scenes.py: the census
of its branches, F against central differences of its own outputs, P symmetric and positive semi-definite to rounding, and
a record of what libm's sin and cos would change."""
import numpy as np
import pytest

import elementary_ref as E
import imu_ref as R
import imu_scenes as SC

FLOOR = 16
# Central differences (h = 1e-5, oplus on the pose, plain differences on speed and biases) agree with F to 5.8e-5 of
# max(1, max |F|) over the 108 finite multiframes below, whatever h between 1e-6 and 1e-4: F is the reference's
# linearisation, which drops terms of that size, not the exact derivative.  The bound is ten times the measured figure
# (DESIGN.md).
F_AGREEMENT_MEASURED = 5.8e-5
F_BOUND = 10 * F_AGREEMENT_MEASURED
FD_KINDS = ("general", "start_on_sample", "forty_samples", "two_samples", "duplicate_timestamp", "zero_rate")
EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("tree", [True, False], ids=["eigen_tree", "left_to_right"])
def test_census_floors(tree):
    _, census = SC.references(tree)
    for key in R.CENSUS:
        if key in R.UNREACHABLE:
            assert census[key] == 0, key
        else:
            assert census[key] >= FLOOR, (key, census[key])
    kinds = [mf["kind"] for sc in SC.scenes() for mf in sc["mfs"]]
    assert all(kinds.count(k) >= FLOOR for k in SC.KINDS)
    assert sorted({len(mf["ts"]) for sc in SC.scenes() for mf in sc["mfs"]})[:2] == [0, 2]
    assert max(len(mf["ts"]) for sc in SC.scenes() for mf in sc["mfs"]) == 40
    assert [len(sc["T_SC_params"]) for sc in SC.scenes()] == [1, 2, 5]


def _interval_values(mf):
    """theta_half and Phi of an edge multiframe's intervals (rates (s, 0, 0), zero bias, 5 ms apart)"""
    dt = R.time_diff(mf["ts"][1], mf["ts"][0])
    s = mf["gyro"][0, 0]
    return SC._theta_half(s, dt), SC._phi(s, dt)


def test_both_sides_of_every_knife_edge():
    """adjacent doubles on either side of each edge, at least eight multiframes a side"""
    sides = {k: [0, 0] for k in SC.EDGE_KINDS}
    for sc in SC.scenes():
        for mf in sc["mfs"]:
            if mf["kind"] not in SC.EDGE_KINDS:
                continue
            sides[mf["kind"]][mf["side"]] += 1
            lo, hi = SC.edges()[mf["kind"]]
            assert np.nextafter(lo, np.inf) == hi
            if mf["kind"] in ("gyro_at_g_max", "acc_at_a_max"):
                v = np.abs(mf["gyro"] if mf["kind"] == "gyro_at_g_max" else mf["acc"])
                limit = SC.PARAMS["g_max" if mf["kind"] == "gyro_at_g_max" else "a_max"]
                assert (v > limit).any() == bool(mf["side"]) and v.max() == (lo, hi)[mf["side"]]
                continue
            theta_half, Phi = _interval_values(mf)
            above = {"theta_half_at_1e-6": theta_half > E.SINC_EDGE, "phi_at_1e-4": not Phi < 1.0e-4,
                     "theta_half_at_pi_4": not theta_half <= E.PI_4, "phi_at_pi_4": not Phi <= E.PI_4}[mf["kind"]]
            assert above == bool(mf["side"]), (mf["kind"], mf["side"])
    assert all(min(v) >= 8 for v in sides.values()), sides
    refs, _ = SC.references(True)
    for sc, rf in zip(SC.scenes(), refs):
        for mf, r in zip(sc["mfs"], rf):
            if mf["kind"] == "theta_half_at_pi_4":                 # the pose is finite on the near side only; F never is
                assert np.isnan(r["pose"]).any() == bool(mf["side"]) and np.isnan(r["jacobian"]).any()
                assert r["n_out_of_range"] == r["n_propagated"] > 0
            if mf["kind"] == "phi_at_pi_4":
                assert not np.isnan(r["pose"]).any() and np.isnan(r["jacobian"]).any() == bool(mf["side"])
                assert r["n_out_of_range"] == (r["n_propagated"] if mf["side"] else 0)


def test_defined_cases():
    refs, _ = SC.references(True)
    seen = set()
    for sc, rf in zip(SC.scenes(), refs):
        for mf, r in zip(sc["mfs"], rf):
            if mf["kind"] == "front_after_start":
                assert r["status"] == R.STATUS_FRONT_AFTER_START and r["pose"] is None and r["n_propagated"] is None
            elif mf["kind"] == "empty":
                assert r["status"] == R.STATUS_EMPTY and r["pose"] is None
            elif mf["kind"] == "end_past_last":
                assert r["n_propagated"] == -1 and np.array_equal(r["pose"], mf["T_WS"]) and r["jacobian"] is None
                assert np.array_equal(r["speed_and_bias"], mf["sb"]) and r["covariance"] is None
            elif mf["kind"] in ("end_equals_start", "end_before_start"):
                assert r["n_propagated"] == 0 and np.array_equal(r["pose"][:3], mf["T_WS"][:3])
                assert np.array_equal(r["speed_and_bias"], mf["sb"]) and not r["covariance"].any()
                assert np.array_equal(r["jacobian"], np.eye(15))
            elif mf["kind"] == "nan_sample":
                assert np.isnan(r["pose"]).any() or np.isnan(r["speed_and_bias"]).any()
            else:
                continue
            seen.add(mf["kind"])
    assert len(seen) == 6


def test_a_callers_dt_comes_out_bit_equal():
    """Time - Time through Duration's normalising constructor, and toSec()"""
    t = lambda s, n: np.array([s, n], np.uint32)
    assert R.time_diff(t(10, 5000000), t(10, 0)) == np.float64(0.0) + np.float64(1e-9) * np.float64(5000000)
    assert R.time_diff(t(11, 2), t(10, 999999999)) == np.float64(0.0) + np.float64(1e-9) * np.float64(3)
    assert R.time_diff(t(10, 0), t(10, 1)) == np.float64(-1.0) + np.float64(1e-9) * np.float64(999999999)
    assert R.time_diff(t(12, 7), t(10, 7)) == 2.0
    assert R.time_lt(t(1, 5), t(2, 0)) and R.time_lt(t(1, 5), t(1, 6)) and not R.time_lt(t(1, 5), t(1, 5))


def _central_differences(tree, mf, h=1.0e-5):
    F = np.zeros((15, 15))
    for j in range(15):
        outs = []
        for s in (1.0, -1.0):
            d = np.zeros(15)
            d[j] = s * h
            outs.append(R.propagation(tree, SC.PARAMS, mf["ts"], mf["gyro"], mf["acc"], mf["t_start"], mf["t_end"],
                                      R.oplus(mf["T_WS"], d[:6]), mf["sb"] + d[6:], want_jacobian=False,
                                      want_covariance=False))
        F[:6, j] = R.ominus(outs[0]["pose"], outs[1]["pose"]) / (2.0 * h)
        F[6:, j] = (outs[0]["speed_and_bias"] - outs[1]["speed_and_bias"]) / (2.0 * h)
    return F


def test_jacobian_agrees_with_central_differences():
    refs, _ = SC.references(True)
    worst, n = 0.0, 0
    for sc, rf in zip(SC.scenes(), refs):
        for mf, r in zip(sc["mfs"], rf):
            if mf["kind"] not in FD_KINDS or r["jacobian"] is None or not np.isfinite(r["jacobian"]).all():
                continue
            F = _central_differences(True, mf)
            worst = max(worst, float(np.abs(F - r["jacobian"]).max() / max(1.0, np.abs(r["jacobian"]).max())))
            n += 1
    print("F against central differences over %d multiframes: %.3g of max(1, max |F|)" % (n, worst))
    assert n >= 100 and worst <= F_BOUND, (n, worst)


def test_covariance_is_symmetric_and_positive_semidefinite_to_rounding():
    """measured: asymmetry 1.7 eps of max |P|, no negative eigenvalue at all; held at 16 eps"""
    refs, _ = SC.references(True)
    n, asym, low = 0, 0.0, 0.0
    for rf in refs:
        for r in rf:
            P = r["covariance"]
            if P is None or not np.isfinite(P).all() or not P.any():
                continue
            scale = np.abs(P).max()
            asym = max(asym, float(np.abs(P - P.T).max() / scale))
            ev = np.linalg.eigvalsh(0.5 * (P + P.T))
            low = min(low, float(ev.min() / ev.max()))
            n += 1
    print("P over %d multiframes: asymmetry %.3g eps, lowest eigenvalue %.3g eps of the largest" % (n, asym / EPS, low / EPS))
    assert n >= 200 and asym <= 16 * EPS and low >= -16 * EPS


def test_record_what_libm_would_change():
    """libm=True: numpy's sin and cos in place of the three fixed functions.  A record, no bound on the code
    under test: measured 0 in the pose, 1.9e-14 relative in F and 6.2e-13 relative in P over 243 finite multiframes."""
    refs, _ = SC.references(True)
    keys = ("pose", "jacobian", "covariance")
    worst, n = dict.fromkeys(keys, 0.0), 0
    for sc, rf in zip(SC.scenes(), refs):
        for mf, r in zip(sc["mfs"], rf):
            if r["covariance"] is None or not all(np.isfinite(r[k]).all() for k in keys):
                continue
            o = SC.reference_one(True, mf, libm=True)
            n += 1
            for k in keys:
                nz = r[k] != 0
                if nz.any():
                    worst[k] = max(worst[k], float((np.abs(o[k] - r[k])[nz] / np.abs(r[k][nz])).max()))
    print("largest relative differences with libm over %d multiframes: %r" % (n, worst))
    assert n >= 200 and all(np.isfinite(v) for v in worst.values())
