"""CPU: the restatement tests/ransac2d2d_hyp_ref.py held to evidence that does not come from itself -- the epipolar
constraints, numpy.roots, the scenes' ground truth -- and the directed cases of the solver, each asserted to reach its
branch.  The library, the stand-alone program and the kernel are held to the restatement byte for byte elsewhere
(test_ransac2d2d_hyp_host.py, test_gpu_ransac2d2d_hyp*.py).  This file runs no library code: it checks the restatement,
which is itself new, against independent evidence, so unlike the host and GPU files it does not depend on the
library's new symbols."""
import numpy as np
import pytest

import ransac2d2d_hyp_ref as H2
import ransac2d2d_hyp_scenes as HS
from ransac_hyp_ref import draw

SIGMA = np.full(3, 2.0e-6)
N_SCENES = 2400
# The near-degenerate set: a sample whose 10 x 10 elimination meets a pivot below this (a criterion on the input: the
# pivots are a function of the eight bearing pairs alone).
MIN_PIVOT = 1.0e-3
# Measured on the N_SCENES seeded noise-free general scenes of ransac2d2d_hyp_scenes.solver_scene, worst entry of
# [R | t / |t|] against the truth: median 1.9e-14; 0.9 % of all scenes beyond 1e-6; 4.2 % of the scenes excluded by
# MIN_PIVOT; worst error outside the excluded set 1.18e-3 (a scene with six real roots, its smallest pivot 1.45e-3).
# The bound is ten times that worst.
MEASURED_WORST = 1.18e-3
POSE_BOUND = 10.0 * MEASURED_WORST
MAX_EXCLUDED = 0.05

_MEASURED = {}


def _solve(seed, **kw):
    Rm, t, b1, b2 = HS.solver_scene(seed, **kw)
    d = {}
    Hm, valid, n_roots = H2.fivept(True, b1, b2, SIGMA, SIGMA, details=d)
    return Rm, t, b1, b2, Hm, valid, n_roots, d


def _min_pivot(d):
    return min(abs(p) for p in d["pivots"]) if len(d["pivots"]) == 10 else 0.0


def _measurement():
    if not _MEASURED:
        rows = []
        for seed in range(N_SCENES):
            Rm, t, b1, b2, Hm, valid, n_roots, d = _solve(seed)
            rows.append((HS.pose_error(Hm, Rm, t) if valid else np.inf, _min_pivot(d), n_roots))
        _MEASURED["rows"] = np.array(rows)
    return _MEASURED["rows"]


def test_chosen_hypothesis_is_the_true_pose_on_general_scenes():
    """Noise-free general scenes: the hypothesis is the true [R | t / |t|] within POSE_BOUND = 1.18e-2, ten times the
    measured worst 1.18e-3, outside the near-degenerate set (smallest elimination pivot below 1e-3: 4.2 % of the
    scenes, at most 5 % allowed).  Median 1.9e-14, 0.9 % of all scenes beyond 1e-6."""
    rows = _measurement()
    err, piv = rows[:, 0], rows[:, 1]
    keep = piv >= MIN_PIVOT
    excluded = 1.0 - keep.mean()
    worst = float(err[keep].max())
    print("scenes", len(err), "median", float(np.median(err)), "beyond 1e-6", float((err > 1e-6).mean()), "excluded", excluded,
          "worst outside the excluded set", worst, "bound", POSE_BOUND)
    assert excluded <= MAX_EXCLUDED, excluded
    assert worst <= POSE_BOUND, worst


def test_every_essential_matrix_satisfies_the_five_epipolar_constraints():
    """|b1^T E b2| of the five solved pairs, E scaled to unit Frobenius norm, for every real root of 200 scenes.  The
    basis of the null space comes out of a fully pivoted elimination of products of unit vectors: residuals of a few
    ulp; 1e-10 leaves five decimal orders."""
    worst, n = 0.0, 0
    for seed in range(200):
        Rm, t, b1, b2, Hm, valid, n_roots, d = _solve(seed)
        for E in d["Es"]:
            E = np.array(E).reshape(3, 3)
            if not np.all(np.isfinite(E)):
                continue
            E = E / np.linalg.norm(E)
            worst = max(worst, max(abs(b1[i] @ E @ b2[i]) for i in range(5)))
            n += 1
    print("essential matrices", n, "worst residual", worst)
    assert n >= 600 and worst <= 1.0e-10


def test_real_root_count_equals_numpy_roots_where_the_roots_are_separated():
    """separated: every non-real root of numpy.roots lies more than 1e-3 (relative to max(1, |z|)) off the real axis
    and the real ones lie more than 1e-3 apart"""
    compared = 0
    for seed in range(400):
        d = _solve(seed)[7]
        z = np.roots(d["P"][::-1])
        off = np.abs(z.imag) / np.maximum(1.0, np.abs(z))
        real = np.sort(z[off <= 1.0e-6].real)
        rest = off[off > 1.0e-6]
        if (len(rest) and rest.min() <= 1.0e-3) or (len(real) > 1 and np.diff(real).min() <= 1.0e-3):
            continue
        compared += 1
        assert len(real) == len(d["roots"]), (seed, real, d["roots"])
        assert np.allclose(real, d["roots"], rtol=1e-6, atol=1e-9), (seed, real, d["roots"])
        assert d["roots"] == sorted(d["roots"]) and len(d["roots"]) <= 10
    assert compared >= 350


def test_two_point_rotation_is_the_true_rotation_on_pure_rotations():
    """b1 = R b2 exactly up to rounding of the scene: M is R to 1e-12 (two triads of unit vectors, no cancellation
    beyond the cross product of bearings at least 0.01 rad apart in these scenes)"""
    worst = 0.0
    for seed in range(300):
        Rm, t, b1, b2 = HS.solver_scene(seed, rotation_only=True)
        M, valid = H2.twopt(b1[:2], b2[:2])
        assert valid == 1
        worst = max(worst, float(np.abs(M.reshape(3, 3) - Rm).max()))
        assert np.allclose(M.reshape(3, 3) @ b2[5], b1[5], atol=1e-12)
    print("two-point worst error", worst)
    assert worst <= 1.0e-12


def test_sampler_draws_distinct_positions_from_the_shared_stream():
    for n in (10, 11, 64, 700):
        for h in range(64):
            for count, problem in ((2, 0), (8, 1)):
                key = H2.fold_key(12345, 3, problem)
                pos = H2.sample(HS.SEED, key, h, n, count)
                assert len(set(pos)) == count and min(pos) >= 0 and max(pos) < n
                assert pos[0] == draw(HS.SEED, key, h, 0, n)          # the first draw is the shared draw itself
    # the key separates pair, camera and problem, and does not know the batch
    assert len({H2.fold_key(p, c, q) for p in range(5) for c in range(64) for q in (0, 1)}) == 5 * 64 * 2
    assert H2.sample(1, H2.fold_key(7, 1, 1), 3, 50, 8) != H2.sample(1, H2.fold_key(7, 1, 0), 3, 50, 8)


# ---- directed cases ------------------------------------------------------------------------------------------------
def test_pure_rotation_fed_to_the_five_point():
    """t = 0: E = [t]x R vanishes, every [t']x R fits the five pairs.  The solver ends on every scene, either invalid
    (the polynomial degenerates: its leading coefficient, a pivot) or with a finite [R | t]; both are reached."""
    census = H2.new_census()
    for seed in range(60):
        Rm, t, b1, b2 = HS.solver_scene(seed, rotation_only=True)
        Hm, valid, n_roots = H2.fivept(True, b1, b2, SIGMA, SIGMA, census=census)
        assert np.all(np.isfinite(Hm)) and (valid == 1 or not Hm.any())
    print(census)
    assert census["rel_valid"] >= 10 and census["bad_lead"] + census["elim_pivot"] + census["no_finite_sum"] >= 5


def test_planar_scene_the_extra_samples_pick_the_physical_solution():
    """five points on a plane have two physical solutions; samples 5 .. 7 lie off the plane and pick the true one.
    Bound and excluded set of the general scenes (planar samples are excluded far more often: their pivots are small)."""
    kept, worst = 0, 0.0
    for seed in range(120):
        Rm, t, b1, b2, Hm, valid, n_roots, d = _solve(seed, planar=True)
        assert valid == 1 and n_roots >= 2 and len([s for s in d["sums"] if np.isfinite(s)]) >= 8
        if _min_pivot(d) >= MIN_PIVOT:
            kept += 1
            worst = max(worst, HS.pose_error(Hm, Rm, t))
    print("planar scenes kept", kept, "worst", worst)
    assert kept >= 60 and worst <= POSE_BOUND


def test_duplicate_and_collinear_bearings_fail_a_pivot():
    Rm, t, b1, b2 = HS.solver_scene(3)
    census = H2.new_census()
    d1, d2 = b1.copy(), b2.copy()
    d1[1], d2[1] = d1[0], d2[0]                                  # a pair listed twice: Q has rank 4
    Hm, valid, n_roots = H2.fivept(True, d1, d2, SIGMA, SIGMA, census=census)
    assert valid == 0 and not Hm.any() and n_roots == 0
    a = np.linspace(-0.4, 0.4, 8)
    c1 = np.stack([np.sin(a), np.zeros(8), np.cos(a)], axis=1)   # all bearings on the great circle y = 0, in both
    c2 = np.stack([np.sin(a + 0.1), np.zeros(8), np.cos(a + 0.1)], axis=1)   # frames: Q lives in four columns
    Hm, valid, n_roots = H2.fivept(True, c1, c2, SIGMA, SIGMA, census=census)
    assert valid == 0 and not Hm.any()
    assert census["null_pivot"] + census["elim_pivot"] == 2, census
    M, valid = H2.twopt(np.stack([b1[0], b1[0]]), b2[:2], census=census)
    assert valid == 0 and not M.any() and census["rot_zero_cross"] == 1


def test_a_nan_bearing_is_invalid():
    Rm, t, b1, b2 = HS.solver_scene(4)
    for row in (0, 4, 6):
        census = H2.new_census()
        n1 = b1.copy()
        n1[row, 1] = np.nan
        Hm, valid, n_roots = H2.fivept(True, n1, b2, SIGMA, SIGMA, census=census)
        assert valid == 0 and not Hm.any(), row
        assert census["null_pivot"] + census["elim_pivot"] + census["no_finite_sum"] + census["bad_lead"] + census["no_root"] == 1
    M, valid = H2.twopt(n1[[6, 1]], b2[[6, 1]])
    assert valid == 0 and not M.any()


def test_the_adapters_fallback_bearing():
    """(1, 0, 0) in the older frame where a back-projection failed: four of them among the five solved pairs leave Q
    with rank 4 (their rows live in three columns); one of them is a wrong but solvable sample"""
    Rm, t, b1, b2 = HS.solver_scene(6)
    census = H2.new_census()
    f1 = b1.copy()
    f1[:4] = (1.0, 0.0, 0.0)
    Hm, valid, n_roots = H2.fivept(True, f1, b2, SIGMA, SIGMA, census=census)
    assert valid == 0 and census["null_pivot"] == 1
    f1 = b1.copy()
    f1[2] = (1.0, 0.0, 0.0)
    Hm, valid, n_roots = H2.fivept(True, f1, b2, SIGMA, SIGMA, census=census)
    assert np.all(np.isfinite(Hm)) and census["null_pivot"] == 1
    M, valid = H2.twopt(np.array([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]]), b2[:2])
    assert valid == 0


def test_a_polynomial_without_a_real_root():
    """bearings that no motion relates: seed 254 of this family has a degree-10 polynomial that numpy.roots, too,
    finds without a real root"""
    rng = np.random.default_rng([254, 5])
    b1 = rng.normal(size=(8, 3))
    b1 /= np.linalg.norm(b1, axis=1, keepdims=True)
    b2 = rng.normal(size=(8, 3))
    b2 /= np.linalg.norm(b2, axis=1, keepdims=True)
    census, d = H2.new_census(), {}
    Hm, valid, n_roots = H2.fivept(True, b1, b2, np.ones(3), np.ones(3), census=census, details=d)
    assert valid == 0 and n_roots == 0 and not Hm.any() and census["no_root"] == 1
    z = np.roots(d["P"][::-1])
    assert np.abs(z.imag).min() > 1.0e-3


def test_the_order_of_the_sums_reaches_the_choice_only():
    """both orders of the FP64 sums solve the same roots; only the distance follows the switch"""
    differ = 0
    for seed in range(40):
        Rm, t, b1, b2 = HS.solver_scene(seed)
        da, db = {}, {}
        Ha, va, na = H2.fivept(True, b1, b2, SIGMA, SIGMA, details=da)
        Hb, vb, nb = H2.fivept(False, b1, b2, SIGMA, SIGMA, details=db)
        assert da["roots"] == db["roots"] and da["P"] == db["P"] and na == nb
        differ += int(da["sums"] != db["sums"])
    assert differ >= 1
