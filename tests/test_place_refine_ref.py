"""CPU: the numpy definition of the refinement of Frontend::verifyRecognisedPlace's pose (place_refine_ref.py: ceres'
Levenberg-Marquardt restated over the terms of okvfe_place_hessian_blocks_device) on its own, before a kernel is held to
it: the census floors of the scenes (place_refine_scenes.py), the cost over accepted steps, both orders of the FP64
sums, the start and iteration-limit rules, H at the pose out, and its minimiser against
scipy.optimize.least_squares(loss='cauchy') over the same residuals."""
import numpy as np
import pytest

import place_hessian_ref as PH
import place_refine_ref as PR
import place_refine_scenes as RS
import ransac_scenes as S
from okvis2_amd import capi

FLOOR = 16


def _chunk():
    """terms the Hessian kernel evaluates at a time: the term counts of the edge scene straddle it"""
    return capi.Frontend._test_place_hessian_chunk_terms()


# ---- the restatement on its own -------------------------------------------------------------------------------------------
_CACHE = {}


def _scenes(oracle):
    """every scene with its reference under Eigen's order of the sums, built once"""
    if "all" not in _CACHE:
        census = PR.new_census()
        chunk = _chunk()
        scenes = [RS.general_scene(oracle, spec) for spec in S.GENERAL_SPECS]
        scenes += [RS.truth_scene(oracle), RS.wild_scene(oracle), RS.no_term_scene(oracle), RS.far_scene(oracle),
                   RS.noisy_scene(oracle), RS.term_count_scene(oracle, (chunk - 1, chunk, chunk + 1, 600)),
                   RS.block_size_scene(oracle), RS.directed_scene(oracle), RS.conversion_scene(oracle)]
        _CACHE["all"] = ({sc["name"]: (sc, RS.reference(oracle, True, sc, census=census)) for sc in scenes}, census)
    return _CACHE["all"]


def test_scenes_reach_every_reachable_branch(oracle):
    scenes, census = _scenes(oracle)
    print(census)
    assert set(PR.UNREACHABLE) < set(PR.CENSUS)
    for key in PR.CENSUS:
        if key in PR.UNREACHABLE:
            assert census[key] == 0, (key, census)
        else:
            assert census[key] >= FLOOR, (key, census)
    # what the scenes are for
    statuses = lambda name: [r["status"] for r in scenes[name][1]]
    chunk = _chunk()
    assert [r["n_terms"] for r in scenes["terms-%d-%d-%d-600" % (chunk - 1, chunk, chunk + 1)][1]] == [chunk - 1, chunk, chunk + 1, 600]
    assert [r["n_terms"] for r in scenes["block-sizes"][1]] == [1 + RS.K, RS.K + 1, 1 + RS.K, 0, 3]
    assert statuses("block-sizes")[3] == 3 and statuses("no-term") == [3] * 16 + [0] * 8
    assert statuses("directed") == [4, 0, 0, 4] + [4] * RS.BAD_BEST
    directed = scenes["directed"][1]
    assert np.isnan(directed[0]["cost"]).all() and not np.isnan(directed[0]["pose"]).any()   # singular terms: the start stays
    assert all(np.isnan(r["pose"]).all() and np.isnan(r["start_pose"]).all() for r in directed[-RS.BAD_BEST:])
    assert sorted(len(scenes["general-" + S.spec_id(s)][1]) for s in S.GENERAL_SPECS) == [1, 3, 3, 17]
    assert all(1 in statuses(n) or 2 in statuses(n) for n in scenes if n.startswith("general"))
    # started at the truth without noise the loop ends within a step or two, converged
    assert all(r["status"] == 1 and r["n_accepted"] <= 1 for r in scenes["truth-euroc+euroc1"][1])
    # far starts: the first step of some multiframe is rejected
    assert any(r["n_accepted"] < r["n_iterations"] for r in scenes["far-euroc+euroc1"][1])


def test_cost_never_increases_over_accepted_steps(oracle):
    scenes, _ = _scenes(oracle)
    n = 0
    for name, (sc, refs) in scenes.items():
        for r in refs:
            costs = np.array(r["costs"])
            if r["status"] in (1, 2) and len(costs) > 1:
                assert np.all(np.diff(costs) < 0.0), (name, costs)
                assert costs[0] == r["cost"][0] and costs[-1] == r["cost"][1] and len(costs) == 1 + r["n_accepted"]
                n += 1
    assert n >= 100


def test_both_orders_of_the_sums_take_the_same_branches(oracle):
    scenes, _ = _scenes(oracle)
    sc, refs = scenes["general-euroc+euroc1"]
    other = RS.reference(oracle, False, sc)
    assert [r["status"] for r in other] == [r["status"] for r in refs]
    assert any(r["pose"] is not None and not np.array_equal(r["pose"], o["pose"]) for r, o in zip(refs, other))


def test_initial_pose_and_max_iterations(oracle):
    scenes, _ = _scenes(oracle)
    sc, refs = scenes["noisy-euroc+euroc1"]
    mf = sc["mfs"][0]
    args = (oracle, True, sc["hp"], mf["frames"], mf["ml"], mf["state"], sc["cams"], sc["T_SC_params"])
    start = PR.start_pose(mf["hyp"][mf["best"]])
    again = PR.refine(*args, initial=start)
    assert np.array_equal(again["pose"], refs[0]["pose"]) and np.array_equal(again["start_pose"], start)
    none = PR.refine(*args, hypotheses=mf["hyp"], best=mf["best"], max_iterations=0)
    assert none["status"] == 2 and none["n_iterations"] == 0 and np.array_equal(none["pose"], start)
    assert none["cost"][0] == none["cost"][1] == refs[0]["cost"][0]
    one = PR.refine(*args, hypotheses=mf["hyp"], best=mf["best"], max_iterations=1)
    assert one["n_iterations"] == 1 and one["status"] == 2
    # H out is the Hessian call's H at the pose out
    H = PH.evaluate(*args, refs[0]["pose"])["H"]
    assert np.array_equal(H, refs[0]["H"])


# The largest distance measured between the restatement's pose and scipy's minimiser, in the tangent space at the start
# (|delta| over 3 translations in metres and 3 rotations in radians), over the 16 multiframes of the noisy scene (all of
# them end converged within the 10 iterations of the shipped configurations): 1.06e-4; the two costs then agree to 1e-5
# of 700.  Both solvers stop on tolerances, the restatement on ceres' function tolerance of 1e-6 of the cost.  The bound
# is ten times the measured maximum.
SCIPY_BOUND = 1.06e-3


def test_minimiser_against_scipy_least_squares(oracle):
    """the defined algorithm minimises the right function: scipy's trust-region reflective solver with loss='cauchy',
    f_scale=3 (rho(z) = 9 log(1 + z / 9), ceres' CauchyLoss(3)) over the same residual function, parameterised by
    pose_plus from the start pose, run to tight tolerances.  scipy applies its loss to every scalar residual and ceres to
    the squared norm of a term's two, so scipy is handed the norm of each term's residual: the cost is then the same
    0.5 sum(9 log(1 + (r0 r0 + r1 r1) / 9))."""
    scipy_optimize = pytest.importorskip("scipy.optimize")
    sc, refs = _scenes(oracle)[0]["noisy-euroc+euroc1"]
    worst, used = 0.0, 0
    for mf, ref in zip(sc["mfs"], refs):
        if ref["status"] != 1:
            continue                                                # the iteration limit: excluded from this check only
        start = ref["start_pose"]
        args = (oracle, True, sc["hp"], mf["frames"], mf["ml"], mf["state"], sc["cams"], sc["T_SC_params"])

        def residuals(delta):
            r = np.concatenate(PH.evaluate(*args, PH.pose_plus(start, delta))["residual"])
            return np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1])  # (one residual per term: see the docstring)

        def inverse_plus(pose):
            """delta with pose_plus(start, delta) == pose up to rounding"""
            q0 = start[3:] / np.linalg.norm(start[3:])
            dq = PH._qmul(pose[3:] / np.linalg.norm(pose[3:]), np.array([-q0[0], -q0[1], -q0[2], q0[3]]))
            dq = dq if dq[3] >= 0 else -dq
            n = np.linalg.norm(dq[:3])
            angle = 2.0 * np.arctan2(n, dq[3])
            return np.concatenate([pose[:3] - start[:3], dq[:3] * (angle / n if n > 0 else 2.0)])

        mine = inverse_plus(ref["pose"])
        assert np.allclose(PH.pose_plus(start, mine), ref["pose"], atol=1e-12)
        sol = scipy_optimize.least_squares(residuals, mine, loss="cauchy", f_scale=3.0, xtol=1e-14, ftol=1e-14, gtol=1e-14,
                                           max_nfev=300)
        worst = max(worst, float(np.linalg.norm(sol.x - mine)))
        used += 1
    print("largest tangent-space distance to scipy's minimiser: %.3e over %d multiframes" % (worst, used))
    assert used >= (3 * len(refs) + 3) // 4, used
    assert worst < SCIPY_BOUND, worst
