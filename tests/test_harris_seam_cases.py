"""CPU: the scenes of tests/harris_seam_cases.py really put maxima on both sides of every lane and strip hand-over of
the fused score + NMS kernel, in its outermost columns and in its first and last tested rows -- by the oracle alone."""
import numpy as np
import pytest

import harris_seam_cases as S


def test_the_widths_take_the_forms_they_are_meant_for():
    nd = {n: w // 4 for n, (w, h) in S.CASES.items()}
    assert S.strips(200) == 1 and nd["part_strip"] < 64           # lanes past the row end repeat the last dword
    assert S.strips(256) == 1 and nd["full_strip"] == 64          # lane 0 and lane 63 are image border
    assert S.strips(504) == 2 and nd["two_strips"] == S.STRIP + 64  # the second strip is exactly full: no packing
    assert S.strips(752) == 3 and S.seams(752) == [252, 500]
    # packed: the last strip holds at most half a wave (halo lane + store lanes), several images share one
    last = nd["packed"] - S.STRIP * (S.strips(272) - 1)
    assert S.strips(272) == 2 and last <= 32 and 64 // last == S.PACK_IMAGES
    assert S.batch_for_tile_61("packed") % S.PACK_IMAGES == 9      # the last packed wave of the batch holds nine of ten
    assert S.PACK_IMAGES > 1                                       # ... and the one of a single image one of ten
    for n, (w, h) in S.CASES.items():
        assert 64 <= h <= 130 and w % 4 == 0
        assert S.batch_for_tile_61(n) * S.strips(w) * ((h + 60) // 61) > 512  # more than 128 blocks of four waves
    assert S.CASES["three_strips"][1] > 2 * 61                     # three 61-row tiles, six 25-row tiles
    lw, lh = S.LAYER
    assert ((S.LAYER_IMAGE[0] // 3) * 2, (S.LAYER_IMAGE[1] // 3) * 2) == (lw, lh) == S.CASES["packed"]
    nd0 = S.LAYER_IMAGE[0] // 4
    assert S.strips(S.LAYER_IMAGE[0]) == 2 and nd0 - S.STRIP > 32  # layer 0: two plain strips beside the packed layer


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_planted_maxima_are_maxima(oracle, name):
    w, h = S.CASES[name]
    plan = S.planted(w, h)
    for c in S.seams(w):  # both sides of every hand-over, in the first and the last tested row, and a pair across it
        assert {("dot", c - 1, 2), ("dot", c, h - 3), ("pair", c - 1, 12)} <= set(plan)
    for seed in range(S.DISTINCT):
        score, cand, kps = S.reference(name, seed)
        have = set(zip(cand["x"].tolist(), cand["y"].tolist()))
        confirmed = 0
        for kind, x, y in plan:
            if kind == "dot" and 2 <= x <= w - 3:
                assert (x, y) in have, (name, seed, x, y)
                confirmed += 1
            elif kind == "dot":  # columns 1 and w - 2 carry scores and never maxima
                assert score[y, x] > S.THR and (x, y) not in have, (name, seed, x, y)
            else:
                # equal scores in adjacent pixels, both at least every other neighbour and the threshold: both pass the
                # kernel's test (>=), the row is flagged, and the raster-scan rule keeps the left one alone
                a, b = int(score[y, x]), int(score[y, x + 1])
                nb = score[y - 1:y + 2, x - 1:x + 3].astype(np.int64)
                nb[1, 1:3] = -1 << 40
                assert a == b and a >= S.THR and a >= nb.max(), (name, seed, x, y, a, b)
                assert (x, y) in have and (x + 1, y) not in have, (name, seed, x, y)
                confirmed += 1
        assert confirmed >= 2
        assert not any(x < 2 or x > w - 3 or y < 2 or y > h - 3 for x, y in have)
        assert min(cand["y"]) == 2 and max(cand["y"]) == h - 3  # the first and the last tested row
        assert not (score[0].any() or score[h - 1].any() or score[:, 0].any() or score[:, w - 1].any())  # the rim is zero
        assert score[1].any() and score[h - 2].any() and score[:, 1].any() and score[:, w - 2].any()
        assert 100 < len(kps) < S.MAX_KPTS and len(cand) < S.MAX_CAND


def test_the_packed_layer_keeps_keypoints_at_its_seam(oracle):
    """layer 1 of the one-octave scale space is 272 px wide: keypoints of that layer on both sides of column 252"""
    for seed in range(S.DISTINCT):
        k = S.layer_reference(seed)
        x1 = k[k["octave"] == 1]["x"] / 1.5  # layer-1 columns
        assert (k["octave"] == 0).sum() > 300 and len(x1) > 50
        assert ((x1 >= 240) & (x1 < 252)).any() and (x1 >= 252).any(), (seed, np.sort(x1)[-8:])
