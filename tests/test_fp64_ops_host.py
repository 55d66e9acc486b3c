"""CPU: okvis2_amd/csrc/fp64_ops.h on its own, compiled into a stand-alone host program (tests/cpp/fp64_ops_main.cpp,
-ffp-contract=off as the library), plain and with -fsanitize=address,undefined.  The template sums sum3<kTree> /
sum4<kTree> against tests/ransac_ref.py's sum3 / sum4, the runtime form sum3_select against the template form, and
quat_normalized<kTree> / quat_product against tests/place_refine_ref.py's normalized / product: bit for bit (every NaN
counts as the same value: which operand's payload an addition hands on is the compiler's choice), under both orders.
Inputs: cancellation, signed zeros, infinities of both signs, a NaN in each position and seeded random values over the
whole exponent range, subnormals included.  The two orders differ on cancellation inputs, so a header with the orders
swapped cannot pass."""
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

import place_refine_ref as PR
from ransac_ref import sum3, sum4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "fp64_ops_main.cpp")
INF, NAN = np.inf, np.nan
# 1 + 1e16 is 1e16 (a tie, to even) and 1e16 - 1e16 is 0: where the small terms meet the large ones decides what is left
CANCEL3 = [(1.0, 1e16, -1e16), (1e16, -1e16, 1.0), (1e16, 1.0, -1e16), (-1e16, 1e16, 1.0), (3.0, 1e16, -1e16),
           (0.1, 0.2, 0.3), (1e-300, 1e300, -1e300), (1e308, 1e308, -1e308)]
CANCEL4 = [(1.0, 1e16, -1e16, 1.0), (1e16, 1.0, 1.0, -1e16), (1e16, -1e16, 1.0, 1.0), (1.0, 1.0, 1e16, -1e16),
           (0.1, 0.2, 0.3, 0.4), (1e308, 1e308, -1e308, -1e308), (1e308, -1e308, 1e308, -1e308)]


def _random(rng, shape):
    """every finite double equally likely per exponent: sign, an exponent field in [0, 2046], 52 random mantissa bits"""
    n = int(np.prod(shape))
    bits = (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63)) | (rng.integers(0, 2047, n, dtype=np.uint64) << np.uint64(52)) \
        | rng.integers(0, 1 << 52, n, dtype=np.uint64)
    return bits.view(np.float64).reshape(shape)


def _with_nan_in_each_position(row):
    return [tuple(NAN if j == i else v for j, v in enumerate(row)) for i in range(len(row))]


def sample():
    rng = np.random.default_rng(64)
    near = rng.uniform(-1.0, 1.0, (1000, 4)) * 10.0 ** rng.integers(-3, 4, (1000, 1))   # (like the products of a dot product)
    t = list(CANCEL3) + list(itertools.product((0.0, -0.0), repeat=3)) + list(itertools.product((INF, -INF, 1.0), repeat=3))
    t += _with_nan_in_each_position((1.0, 2.0, 3.0)) + _with_nan_in_each_position((INF, -INF, 0.0)) + [(NAN, NAN, NAN)]
    t += [(-1.0, 2.0, 0.0), (4.0, 0.0, 0.0), (5e-324, 5e-324, -5e-324)]     # (and the first terms sqrt and finite see)
    triples = np.concatenate([np.array(t, np.float64), _random(rng, (3000, 3)), near[:, :3]])
    q = list(CANCEL4) + list(itertools.product((0.0, -0.0), repeat=4)) + list(itertools.product((INF, -INF, 1.0), repeat=4))
    q += _with_nan_in_each_position((1.0, 2.0, 3.0, 4.0)) + _with_nan_in_each_position((INF, -INF, 0.0, -0.0))
    quads = np.concatenate([np.array(q, np.float64), _random(rng, (3000, 4)), near])
    unit = rng.normal(size=(500, 8))
    special = [(0.0, 0.0, 0.0, 0.0), (-0.0, 0.0, -0.0, 0.0), (NAN, NAN, NAN, NAN), (0.0, 0.0, 0.0, 1.0), (3.0, 0.0, 0.0, 4.0),
               (INF, 0.0, 0.0, 1.0), (1.0, -INF, 0.0, 1.0), (1e-200, 1e-200, 0.0, 0.0), (5e-324, 0.0, 0.0, 0.0),
               (1e200, 1.0, 1.0, 1.0), (1.0, 1e8, -1e8, 1.0)] + _with_nan_in_each_position((0.5, -0.5, 0.5, 0.5))
    pairs = [a + b for a in special for b in ((0.0, 0.0, 0.0, 1.0), (0.5, -0.5, 0.5, 0.5))] + [b + a for a in special for b in special[:3]]
    quats = np.concatenate([np.array(pairs, np.float64), unit, _random(rng, (500, 8)),
                            np.concatenate([unit[:200, :4], _random(rng, (200, 4))], axis=1)])
    return triples, quads, quats


def _build(d, name, extra):
    exe = d / name
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + ROOT, *extra, "-o", str(exe), SOURCE]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(d, exe, triples, quads, quats):
    req, resp = d / "req.bin", d / (exe.name + ".resp.bin")
    req.write_bytes(struct.pack("<iiii", len(triples), len(quads), len(quats), 0) + triples.tobytes() + quads.tobytes()
                    + quats.tobytes())
    r = subprocess.run([str(exe), str(req), str(resp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout, r.stderr)
    out = np.frombuffer(resp.read_bytes(), np.float64)
    a, b = 6 * len(triples), 6 * len(triples) + 2 * len(quads)
    assert len(out) == b + 12 * len(quats)
    return out[:a].reshape(-1, 6), out[a:b].reshape(-1, 2), out[b:].reshape(-1, 12)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("fp64_ops")
    triples, quads, quats = sample()
    plain = _run(d, _build(d, "fp64_ops_main", []), triples, quads, quats)
    san = _run(d, _build(d, "fp64_ops_main_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]),
               triples, quads, quats)
    return triples, quads, quats, plain, san


def _same(a, b):
    canon = lambda v: np.where(np.isnan(v), np.float64(np.nan), v).view(np.uint64)
    return np.array_equal(canon(np.ascontiguousarray(a, np.float64)), canon(np.ascontiguousarray(b, np.float64)))


def _reference_sums(triples, quads):
    with np.errstate(all="ignore"):
        s3 = {tree: sum3(tree, triples[:, 0], triples[:, 1], triples[:, 2]) for tree in (True, False)}
        s4 = {tree: sum4(tree, quads[:, 0], quads[:, 1], quads[:, 2], quads[:, 3]) for tree in (True, False)}
    return s3, s4


def test_template_sums_equal_the_restatement_under_both_orders(host):
    triples, quads, _, (g3, g4, _), _ = host
    s3, s4 = _reference_sums(triples, quads)
    assert _same(g3[:, 0], s3[True]) and _same(g3[:, 1], s3[False])
    assert _same(g4[:, 0], s4[True]) and _same(g4[:, 1], s4[False])
    # the orders differ where terms cancel (and on the random rows): a header with the orders swapped fails the lines above
    c3, c4 = len(CANCEL3), len(CANCEL4)
    assert np.array_equal(triples[:c3], np.array(CANCEL3)) and np.array_equal(quads[:c4], np.array(CANCEL4))
    assert (g3[:c3, 0] != g3[:c3, 1]).any() and (g4[:c4, 0] != g4[:c4, 1]).any()
    # 1 + (1e16 - 1e16) against (1 + 1e16) - 1e16, and (1 + 1e16) + (-1e16 + 1) against ((1 + 1e16) - 1e16) + 1
    assert g3[0, 0] == 1.0 and g3[0, 1] == 0.0 and g4[0, 0] == 0.0 and g4[0, 1] == 1.0
    assert not _same(g3[c3:, 0], g3[c3:, 1]) and not _same(g4[c4:, 0], g4[c4:, 1])
    # the sample holds what it claims: zeros of both signs, both infinities, a NaN in each position, every exponent range
    for rows in (triples, quads):
        assert np.signbit(rows[rows == 0]).any() and (~np.signbit(rows[rows == 0])).any()
        assert (rows == INF).any() and (rows == -INF).any() and all(np.isnan(rows[:, j]).any() for j in range(rows.shape[1]))
        e = np.frexp(rows[np.isfinite(rows) & (rows != 0)])[1]
        assert e.min() < -1000 and e.max() > 1000 and len(rows) > 3000
    assert np.isnan(g3[:, 0]).sum() > 10 and np.isinf(g3[:, 0]).sum() > 10


def test_signed_zeros_and_infinities_follow_ieee(host):
    triples, _, _, (g3, _, _), _ = host
    for tree in (0, 1):
        z = {tuple(np.signbit(r)): g for r, g in zip(triples, g3[:, tree]) if np.all(r == 0)}
        assert len(z) == 8 and all(v == 0 for v in z.values())
        assert [s for s, v in z.items() if np.signbit(v)] == [(True, True, True)]   # -0 only from three -0
    rows = np.isinf(triples).any(axis=1) & ~np.isnan(triples).any(axis=1)
    both = rows & (triples == INF).any(axis=1) & (triples == -INF).any(axis=1)
    assert both.sum() >= 12 and np.isnan(g3[both][:, :2]).all()                      # inf - inf
    assert rows.sum() > both.sum() and np.isinf(g3[rows & ~both][:, :2]).all()


def test_runtime_form_equals_the_template_form_under_both_orders(host):
    _, _, _, (g3, _, _), _ = host
    assert _same(g3[:, 2], g3[:, 0]) and _same(g3[:, 3], g3[:, 1])
    assert not _same(g3[:, 2], g3[:, 3])


def test_finite_and_sqrt(host):
    triples, _, _, (g3, _, _), _ = host
    x = triples[:, 0]
    assert np.array_equal(g3[:, 4] == 1.0, np.isfinite(x)) and set(g3[:, 4]) == {0.0, 1.0}
    with np.errstate(all="ignore"):
        assert _same(g3[:, 5], np.sqrt(x))
    assert np.isnan(x).any() and (x == INF).any() and (x == -INF).any() and (x < 0).any() and (x == 5e-324).any()


def test_quaternion_product_and_normalized_equal_the_restatement(host):
    _, _, quats, (_, _, gq), _ = host
    for tree, cols in ((True, slice(0, 4)), (False, slice(4, 8))):
        want = np.array([PR.normalized(tree, q[:4]) for q in quats])
        assert _same(gq[:, cols], want), tree
    assert _same(gq[:, 8:12], np.array([PR.product(q[:4], q[4:]) for q in quats]))
    assert not _same(gq[:, 0:4], gq[:, 4:8])                                         # the order reaches squaredNorm()
    # a zero quaternion and a NaN quaternion go through as given; so does one whose squared norm underflows to zero
    for given in ((0.0, 0.0, 0.0, 0.0), (-0.0, 0.0, -0.0, 0.0), (NAN, NAN, NAN, NAN), (1e-200, 1e-200, 0.0, 0.0),
                  (5e-324, 0.0, 0.0, 0.0), (NAN, -0.5, 0.5, 0.5), (0.5, -0.5, 0.5, NAN)):
        rows = [i for i, q in enumerate(quats) if _same(q[:4], np.array(given))]
        assert rows, given
        for i in rows:
            assert _same(gq[i, 0:4], np.array(given)) and _same(gq[i, 4:8], np.array(given)), given
    three_four = [i for i, q in enumerate(quats) if tuple(q[:4]) == (3.0, 0.0, 0.0, 4.0)]
    assert three_four and np.array_equal(gq[three_four[0], 0:4], np.array([0.6, 0.0, 0.0, 0.8]))


def test_program_ends_clean_under_the_sanitizers_with_the_same_bytes(host):
    """AddressSanitizer and UndefinedBehaviorSanitizer on the host program itself (its own main)"""
    _, _, _, plain, san = host
    for a, b in zip(plain, san):
        assert _same(a, b)


def test_one_copy_of_each_shared_operation():
    csrc = os.path.join(ROOT, "okvis2_amd", "csrc")
    text = {n: open(os.path.join(csrc, n)).read() for n in sorted(os.listdir(csrc)) if n.endswith((".h", ".hip", ".cpp"))}
    for needle in ("if constexpr (kTree) return", "tree ? w + s : s + w", "((aw * bx + ax * bw) + ay * bz) - az * by",
                   "0x7FF0000000000000ull) != 0x7FF0000000000000ull", "__host__ __device__ inline __attribute__((always_inline))",
                   "int current_device_slot() {"):
        where = [n for n, s in text.items() if needle in s]
        assert where == ["capi_context.cpp" if "current_device_slot" in needle else "fp64_ops.h"], (needle, where)
    assert text["fp64_ops.h"].count("if constexpr (kTree) return") == 2 and "#include" not in text["fp64_ops.h"]
