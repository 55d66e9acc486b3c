"""CPU: the scenes of tests/harris_tile_cases.py really put maxima where the last row tile of the fused score + NMS
kernel can lose or invent them -- by the oracle alone."""
import numpy as np
import pytest

import harris_tile_cases as H


@pytest.mark.parametrize("w,h", list(H.DIRECT) + [H.PACKED])
def test_planted_rows_carry_maxima(oracle, w, h):
    rows = H.planted_rows(h)
    assert {h - 3, h - 4, h - 1} <= set(rows)
    for seed in range(H.DISTINCT):
        score, cand, kps = H.reference(w, h, seed)
        have = set(int(y) for y in cand["y"])
        for r in H.testable(h, rows):
            assert r in have, (w, h, seed, r)
        assert not (score[0].any() or score[h - 1].any())  # rim rows are zero by definition
        assert score[h - 2].any() and score[1].any()
        assert 20 < len(kps) < H.MAX_KPTS and len(cand) < H.MAX_CAND
        # kept keypoints sit on the last rows that may carry maxima as well
        ys = np.floor(kps["y"] + 0.5).astype(int)
        assert (ys >= h - 5).any()


def test_partial_tiles_cover_the_group_boundaries():
    """rows in the last 61-row tile: 1, 5, 6, 7, 60, 61 and 1 again (one group of six more or less at 6 | 7)"""
    assert [h - ((h - 1) // 61) * 61 for h in H.HEIGHTS] == [1, 5, 6, 7, 60, 61, 1]
    assert all(H.batch_for_tile_61(w, h) * (2 if w > 248 else 1) * ((h + 60) // 61) > 512 for w in H.WIDTHS for h in H.HEIGHTS)


def test_the_62_row_case_is_a_scale_space_layer(oracle):
    """heights below the context's minimum run as the 2/3-sampled layer of a scale space, and that layer keeps keypoints on
    its last rows that may carry maxima"""
    assert sorted(H.AS_LAYER) == [(248, 62), (500, 62)] and len(H.DIRECT) + len(H.AS_LAYER) == len(H.WIDTHS) * len(H.HEIGHTS)
    for (lw, lh), (w, h) in H.AS_LAYER.items():
        assert ((w // 3) * 2, (h // 3) * 2) == (lw, lh) and h >= H.MIN_ROWS
        low = 0
        for seed in range(H.DISTINCT):
            k = H.layer_reference(w, h, seed)
            on_layer = k[k["octave"] == 1]
            assert len(on_layer) >= 5 and (k["octave"] == 0).sum() > 50
            low += int((on_layer["y"] / 1.5 >= lh - 5).sum())
        assert low >= 1, (lw, lh)
