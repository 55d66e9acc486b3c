"""CPU: the restatement tests/ransac_hyp_ref.py against ground truth, and the census of its branches.

Ground truth: on the noise-free scenes ransac_hyp_scenes.truth_scene (the four rigs of ransac_scenes.GENERAL_SPECS) the
chosen hypothesis of every valid sample equals the scene's T_WS within ransac_hyp_scenes.TRUTH_BOUND, the measured worst
error of the restatement times 8 (the figures stand in that module's docstring and in DESIGN.md).  Excluded, counted and
held to at most 2 %: the samples ransac_hyp_scenes.near_degenerate names (a sliver triangle or two nearly equal
bearings among the three solver samples).
Census: every case of ransac_hyp_scenes.CENSUS_CASES occurs at least CENSUS_FLOOR times across the census scenes."""
import numpy as np
import pytest

import ransac_hyp_ref as RH
import ransac_hyp_scenes as HS
import ransac_scenes as S


@pytest.mark.parametrize("tree", (True, False), ids=("eigen_tree", "left_to_right"))
def test_ground_truth(oracle, tree):
    worst, excluded, total, invalid = 0.0, 0, 0, 0
    for spec in S.GENERAL_SPECS:
        sc = HS.truth_scene(oracle, spec)
        for mf, ref in zip(sc["mfs"], HS.reference(tree, sc, HS.N_HYP)):
            truth = S.pose_matrix(mf["T_WS"])
            slot = ref["corr"]["cam"] * HS.K + ref["corr"]["row"]
            for h in range(HS.N_HYP):
                if not ref["valid"][h]:
                    invalid += 1
                    continue
                total += 1
                idx = [int(np.flatnonzero(slot == s)[0]) for s in ref["samples"][h]]
                assert len(set(idx)) == 4 and len(set(ref["corr"]["cam"][idx])) == 1   # four distinct samples, one camera
                if HS.near_degenerate(ref["corr"]["p"][idx[:3]], ref["corr"]["b"][idx[:3]]):
                    excluded += 1
                    continue
                err = float(np.abs(ref["H"][h] - truth).max())
                worst = max(worst, err)
                assert err <= HS.TRUTH_BOUND, (sc["name"], h, err, int(ref["n_solutions"][h]))
    print("ground truth: worst", worst, "bound", HS.TRUTH_BOUND, "excluded", excluded, "of", total, "invalid", invalid)
    assert total >= 500 and invalid == 0
    assert excluded <= 0.02 * total, (excluded, total)
    assert worst <= HS.TRUTH_WORST, "the measured figure in ransac_hyp_scenes.py is out of date"


@pytest.mark.parametrize("tree", (True, False), ids=("eigen_tree", "left_to_right"))
def test_census(oracle, tree):
    census = RH.new_census()
    for sc, n_hyp in HS.census_scenes(oracle):
        HS.reference(tree, sc, n_hyp, census=census)
    print(census)
    short = {k: census[k] for k in HS.CENSUS_CASES if census[k] < HS.CENSUS_FLOOR}
    assert not short, short


def test_sampler_draws_distinct_positions_of_one_camera():
    """every (n, camera split): four distinct positions inside the camera of the first, whatever the key"""
    for n_c in ((4,), (5,), (7, 4), (3, 40), (4, 3, 9), (1, 1, 1, 1)):
        cam_of = np.repeat(np.arange(len(n_c)), n_c)
        for key in (0, 1, 2**40 + 7, 2**64 - 1):
            for h in range(64):
                pos = RH.sample(HS.SEED, key, h, cam_of)
                assert 0 <= pos[0] < len(cam_of)
                own = n_c[cam_of[pos[0]]]
                if own < 4:
                    assert pos[1:] == [-1, -1, -1]
                else:
                    assert len(set(pos)) == 4 and len(set(cam_of[pos])) == 1, (n_c, key, h, pos)
    assert RH.sample(HS.SEED, 3, 0, np.zeros(0, np.int64)) == [-1, -1, -1, -1]
    # every position of a list of five is drawn by someone, in every draw
    seen = np.zeros((4, 5), bool)
    for h in range(64):
        for j, i in enumerate(RH.sample(HS.SEED, 9, h, np.zeros(5, np.int64))):
            seen[j, i] = True
    assert seen.all()
