"""CPU: okvis2_amd/csrc/elementary_fixed.h (log_fixed, sin_fixed, cos_fixed, sinc_fixed) compiled into a host program
(tests/cpp/elementary_fixed_main.cpp, -ffp-contract=off as the library) against the numpy restatement
tests/elementary_ref.py, byte for byte, on a dense sample that covers both sides of every branch; and the distance of
both to libm in ulp, held at what the header states."""
import math
import os
import subprocess

import numpy as np
import pytest

import elementary_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The largest distances measured on the sample below (glibc's sin, cos and log, which are correctly rounded in nearly all
# cases): sin_fixed 1 ulp, cos_fixed 1 ulp, log_fixed 2 ulp.  The header states them; they are the bounds.
ULP_BOUND = dict(sin=1, cos=1, log=2)


def _neighbours(v, n=3):
    out = [v]
    lo = hi = np.float64(v)
    for _ in range(n):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return out


def sample():
    rng = np.random.default_rng(20)
    trig = np.concatenate([
        np.linspace(-E.PI_4, E.PI_4, 20001), rng.uniform(-E.PI_4, E.PI_4, 20000),
        10.0 ** rng.uniform(-12, -0.2, 4000) * rng.choice([-1.0, 1.0], 4000),
        np.array(_neighbours(E.PI_4) + _neighbours(-E.PI_4) + _neighbours(E.SINC_EDGE) + _neighbours(-E.SINC_EDGE)
                 + [0.0, -0.0, 5e-324, 1e-300, 0.8, -0.8, 1.0, 2.0, -3.0, 1e300, np.inf, -np.inf, np.nan])])
    logs = np.concatenate([
        np.linspace(1.0, 4.0, 20001), 1.0 + 10.0 ** rng.uniform(-16, 0, 8000), 2.0 ** rng.uniform(0, 1023.9, 8000),
        np.array(_neighbours(1.0) + _neighbours(E.SQRT2) + _neighbours(2.0) + _neighbours(2.0 * E.SQRT2)
                 + _neighbours(0.5 * E.SQRT2) + [np.finfo(np.float64).max, 0.999, 0.5, 0.0, -1.0, np.inf, -np.inf, np.nan])])
    return np.concatenate([trig, logs]).astype(np.float64), len(trig)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the header's four functions on the sample, from a program g++ builds here"""
    d = tmp_path_factory.mktemp("elementary")
    exe = d / "elementary_fixed_main"
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + ROOT, "-o", str(exe),
           os.path.join(ROOT, "tests", "cpp", "elementary_fixed_main.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    x, n_trig = sample()
    (d / "req.bin").write_bytes(x.tobytes())
    out = subprocess.run([str(exe), str(d / "req.bin"), str(d / "resp.bin")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.frombuffer((d / "resp.bin").read_bytes(), np.float64).reshape(4, len(x))
    return x, n_trig, dict(sin=got[0], cos=got[1], sinc=got[2], log=got[3])


def _same(a, b):
    canon = lambda v: np.where(np.isnan(v), np.float64(np.nan), v).view(np.uint64)
    return np.array_equal(canon(np.asarray(a, np.float64)), canon(np.asarray(b, np.float64)))


def test_header_equals_the_restatement_byte_for_byte(host):
    x, n_trig, got = host
    assert _same(got["sin"], E.sin_fixed(x)) and _same(got["cos"], E.cos_fixed(x))
    sinc, big = E.sinc_fixed(x)
    assert _same(got["sinc"], sinc) and _same(got["log"], E.log_fixed(x))
    # both sides of every branch are in the sample
    t = x[:n_trig]
    inside = np.abs(t) <= E.PI_4
    assert inside.sum() > 40000 and (~inside & ~np.isnan(t)).sum() >= 8 and np.isnan(t).sum() == 1
    assert E.PI_4 in t and np.nextafter(E.PI_4, 1.0) in t and (t < 0).sum() > 1000
    assert (big[:n_trig] & inside).sum() > 1000 and (~big[:n_trig] & (t != 0)).sum() > 100
    assert E.SINC_EDGE in t and np.nextafter(E.SINC_EDGE, 1.0) in t
    l = x[n_trig:]
    m = np.frexp(l[(l >= 1.0) & np.isfinite(l)])[0] * 2.0
    assert (m >= E.SQRT2).sum() > 1000 and (m < E.SQRT2).sum() > 1000 and E.SQRT2 in l and np.nextafter(E.SQRT2, 1.0) in l
    assert (l < 1.0).sum() >= 6 and np.inf in l and np.isnan(l).sum() == 1 and 1.0 in l


def test_defined_values_outside_the_domains(host):
    x, n_trig, got = host
    t = x[:n_trig]
    out = ~(np.abs(t) <= E.PI_4)
    assert np.isnan(got["sin"][:n_trig][out]).all() and np.isnan(got["cos"][:n_trig][out]).all()
    assert np.isnan(got["sinc"][:n_trig][out]).all()
    assert not np.isnan(got["sin"][:n_trig][~out]).any() and not np.isnan(got["cos"][:n_trig][~out]).any()
    l, gl = x[n_trig:], got["log"][n_trig:]
    assert np.isnan(gl[~(l >= 1.0)]).all() and np.all(gl[l == np.inf] == np.inf)
    assert np.isfinite(gl[(l >= 1.0) & np.isfinite(l)]).all() and np.all(gl[l == 1.0] == 0.0)
    # sinc at 0 is 1, and its two branches meet at the edge to the last bits
    assert np.all(got["sinc"][:n_trig][t == 0] == 1.0)
    lo, hi = E.sinc_fixed(E.SINC_EDGE)[0], E.sinc_fixed(np.nextafter(E.SINC_EDGE, 1.0))[0]
    assert abs(float(lo) - float(hi)) <= 2 * np.spacing(1.0)


def _ulps(got, want):
    want = np.asarray(want, np.float64)
    return np.abs(got - want) / np.spacing(np.abs(want))


def test_within_the_stated_ulp_of_libm(host):
    x, n_trig, got = host
    t = x[:n_trig]
    inside = np.abs(t) <= E.PI_4
    worst = {}
    for name, f in (("sin", math.sin), ("cos", math.cos)):
        want = np.array([f(v) for v in t[inside]])
        nz = want != 0
        worst[name] = float(_ulps(got[name][:n_trig][inside][nz], want[nz]).max())
        assert np.all(got[name][:n_trig][inside][~nz] == 0.0)
    l = x[n_trig:]
    dom = (l > 1.0) & np.isfinite(l)
    want = np.array([math.log(v) for v in l[dom]])
    worst["log"] = float(_ulps(got["log"][n_trig:][dom], want).max())
    print("largest distance to libm in ulp:", worst)
    header = open(os.path.join(ROOT, "okvis2_amd", "csrc", "elementary_fixed.h")).read()
    assert "differ from libm by at most 1 ulp, log_fixed by at most 2 ulp" in header
    for name, bound in ULP_BOUND.items():
        assert worst[name] <= bound, (name, worst[name])
