"""CPU: the scenes of stereo_insert_scenes.py on the restatement alone (stereo_insert_ref.py).  Together they reach every
branch label of the census at least FLOOR times, so the GPU test, which compares the device call with the restatement
on these scenes, cannot pass by leaving a branch out; the directed scenes do what their names say."""
import numpy as np
import pytest

import stereo_insert_ref as SR
import stereo_insert_scenes as S


def _tree(fp64_order):
    return fp64_order == "eigen_tree"


def test_every_census_label_is_reached(oracle, fp64_order):
    tree = _tree(fp64_order)
    total = SR.new_census()
    for sc in S.all_scenes(oracle, tree):
        _, census = S.reference(oracle, tree, sc["name"])
        for k, v in census.items():
            total[k] += v
    print(total)
    short = {k: v for k, v in total.items() if v < S.FLOOR}
    assert not short, short


def test_scene_shapes(oracle, fp64_order):
    """what the kernel's paths depend on: the block sizes, both keyframe values in one call, 2 / 3 / 5 cameras, nine
    pairs, every camera model, the table size"""
    scenes = S.all_scenes(oracle, _tree(fp64_order))
    counts = {len(k) for sc in scenes for mf in sc["mfs"] for k in mf["kps"]}
    assert {0, 1, 255, 256, 257, S.K} <= counts, sorted(counts)
    assert {len(sc["cams"]) for sc in scenes} == {2, 3, 5}
    assert {1, 3, 9, 10} <= {len(sc["pairs"]) for sc in scenes}  # Hilti's nine; ten <= OKVFE_STEREO_MAX_PAIRS
    assert {c.dist_type for sc in scenes for c in sc["cams"]} == {0, 1, 2, 3}
    assert any([mf["keyframe"] for mf in sc["mfs"]] == [True, False, True] for sc in scenes)
    for sc in scenes:
        assert len(sc["hp"]) == S.L == len(sc["initialised"]) and len(sc["mfs"]) <= 8, sc["name"]
        for c0, c1 in sc["pairs"]:
            assert 0 <= c0 < c1 < len(sc["cams"])
        assert sc["pairs"] == sorted(sc["pairs"])  # im0 ascending, then im1


def _scene(oracle, tree, name):
    return {s["name"]: s for s in S.all_scenes(oracle, tree)}[name]


@pytest.mark.parametrize("first", ["succeeds", "fails", "creates"])
def test_chains(oracle, fp64_order, first):
    tree = _tree(fp64_order)
    name = "chains-first-" + first
    sc = _scene(oracle, tree, name)
    refs, _ = S.reference(oracle, tree, name)
    for mf, ref, n in zip(sc["mfs"], refs, (2, 3, 65)):
        k1, cnt = np.unique(mf["matches"][0]["k1"], return_counts=True)
        assert np.all(cnt == n), (n, cnt)
        a, lm = ref["action"][0].reshape(-1, n), ref["lm"][0].reshape(-1, n)
        if first == "succeeds":    # the head adds the observation to image 1, the followers read that id
            assert np.all(a[:, 0] == SR.OBS1) and np.all(lm == lm[:, :1]) and np.all(lm[:, 0] < S.L)
            assert np.all((a[:, 1:] == SR.OBS0) == (np.arange(1, n) % 4 != 3))
        elif first == "fails":     # the head's landmark is 32 px off: the second row creates
            assert np.all(a[:, 0] == 0) and np.all(a[:, 1] == (SR.CREATE | SR.OBS0 | SR.OBS1))
            assert np.all(lm[:, 1:] == lm[:, 1:2]) and np.all(lm[:, 1] >= S.L)
        else:
            assert np.all(a[:, 0] == (SR.CREATE | SR.OBS0 | SR.OBS1)) and np.all(lm == lm[:, :1])
    if first == "creates":         # a full block on k1 = 0: one landmark, every fifth row 5 px off
        ref = refs[3]
        assert ref["counts"][0] == S.K and ref["counts"][1] == 1 and len(set(ref["lm"][0].tolist())) == 1
        assert np.all((ref["action"][0][1:] == SR.OBS0) == (np.arange(1, S.K) % 5 != 0))


def test_shared_landmarks_and_pairs(oracle, fp64_order):
    tree = _tree(fp64_order)
    refs, census = S.reference(oracle, tree, "shared-bad-failed-edge")
    a = refs[0]["action"][0].reshape(-1, 6)
    # (a) the first of two keypoints with one landmark re-initialises it, the second finds it initialised;
    # (b) the chain of the k1 that also carries it reads the re-set point: accepted at 0.0 px, rejected at 4.4 px
    assert np.all(a[:, 0] == SR.REINIT) and np.all(a[:, 1] == 0) and np.all(a[:, 2] == SR.OBS0) and np.all(a[:, 3] == 0)
    assert np.all(a[:, 4] == SR.OBS1) and np.all(a[:, 5] == SR.OBS1)  # (c)
    assert census["both_reinit"] >= 18 and census["read_point_reset"] >= 36
    refs, census = S.reference(oracle, tree, "across-pairs")
    for ref, kf in zip(refs, (True, False, True)):
        a0, a1, a2 = ref["action"]
        if not kf:
            assert ref["counts"][1] == 0 and not np.any(a0) and not np.any(a2)
            continue
        assert np.all(a0 == (SR.CREATE | SR.OBS0 | SR.OBS1)) and ref["counts"][1] == 18
        reinit = np.arange(18) % 6 != 0
        assert np.all((a1 == SR.REINIT) == reinit) and np.all((a2 == SR.OBS1) == reinit)
        assert np.all(ref["lm"][2] == ref["lm"][0]) and np.all(ref["lm"][0] >= S.L)  # pair (1,2) acts on the creation
    assert census["read_id_earlier_pair"] >= 36 and census["read_point_created"] >= 15


def test_bad_k1_ids_and_failed_projections(oracle, fp64_order):
    tree = _tree(fp64_order)
    sc = _scene(oracle, tree, "shared-bad-failed-edge")
    refs, census = S.reference(oracle, tree, "shared-bad-failed-edge")
    mf, ref = sc["mfs"][1], refs[1]
    n1 = len(mf["kps"][1])
    k1 = mf["matches"][0]["k1"]
    assert {n1 - 1, n1, S.K - 1, S.K, -2} <= set(k1.tolist())
    bad = (k1 < 0) | (k1 >= n1)
    assert not np.any(ref["action"][0][bad]) and np.all(ref["lm"][0][bad] == -1) and ref["counts"][0] == int((~bad).sum())
    assert {-1, -2, S.L - 1, S.L} <= set(mf["ids"][0].tolist()) and {-1, -2, S.L - 1, S.L} <= set(mf["ids"][1].tolist())
    assert np.all(ref["ids"][0][mf["ids"][0] == S.L] != S.L) and np.all(ref["ids"][0][mf["ids"][0] == -2] != -2)
    for side in ("add0", "add1"):
        assert census[side + "_nan"] >= S.FLOOR and census[side + "_status"] >= S.FLOOR, census
    # the 4 px edge: exactly 4.0 adds nothing; the bisected pair of adjacent doubles has one verdict each
    mf, ref = sc["mfs"][3], refs[3]
    verdicts = [(bool(ref["action"][0][k0] & SR.OBS0), expect) for k0, expect in mf["expect_obs0"]]
    assert all(g == e for g, e in verdicts), verdicts
    assert [e for _, e in mf["expect_obs0"]][:4] == [False, False, True, True]
    assert mf["expect_obs0"][4][1] != mf["expect_obs0"][5][1]
