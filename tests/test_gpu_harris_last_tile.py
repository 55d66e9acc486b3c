"""GPU: the partial last row tile of the fused score + NMS kernel (harris_kernel, csrc/k_harris.hip): rows past the image
are not stored, rows h - 2 and h - 1 are not tested, everything above is.  Heights that leave 1, 5, 6, 7, 60 and 61 rows to the last 61-row tile (and 12 ..
23 to the last 25-row tile), maxima planted around the tile's first and last rows (tests/harris_tile_cases.py), the
map-free and the map-writing form, one image per call (25-row tiles) and a batch large enough for 61-row tiles: score
rows, candidate counts and kept keypoints against the oracle.  A context takes 64 rows and more: the 62-row case is the
2/3-sampled layer of a 93-row scale space (one image per call; its structure under 61-row tiles -- one row in the last
tile -- is the 123-row case of the batch test)."""
import ctypes as C

import numpy as np
import pytest

from okvis2_amd import capi

import gpu_common as G
import harris_tile_cases as H

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _counts(fe, n, which):
    host = np.zeros(n, dtype=np.int32)
    st = capi.lib().okvfe_copy_to_host(C.c_void_p(host.ctypes.data), C.c_void_p(getattr(fe.device_outputs(), which)),
                                       C.c_size_t(host.nbytes), None)
    assert st == 0
    return host


def _score_maps(fe, n, w, h):
    """the score maps of the last call, columns in image order"""
    out = fe.device_outputs()
    assert out.scores is not None
    host = np.empty(n * h * out.score_pitch, dtype=np.int32)
    st = capi.lib().okvfe_copy_to_host(C.c_void_p(host.ctypes.data), C.c_void_p(out.scores), C.c_size_t(host.nbytes), None)
    assert st == 0
    cols = np.array([capi.lib().okvfe_score_column(fe._h, int(x)) for x in range(w)])
    return host.reshape(n, h, out.score_pitch)[:, :, cols]


def _check_counts(fe, n, w, h):
    cand, kept = _counts(fe, n, "candidate_counts"), _counts(fe, n, "detect_counts")
    for i in range(n):
        _, rc, rk = H.reference(w, h, i % H.DISTINCT)
        assert cand[i] == len(rc) and kept[i] == len(rk), (i, cand[i], len(rc), kept[i], len(rk))


@pytest.mark.parametrize("w,h", list(H.DIRECT) + [H.PACKED])
def test_one_image_per_call(oracle, w, h):
    """25-row tiles (a call that cannot fill the GPU): keypoints byte for byte, both forms, and the map's rows"""
    fe = capi.Frontend(w, h, H.RADIUS, 0, H.THR, H.MAX_KPTS, max_candidates=H.MAX_CAND)
    for seed in range(H.DISTINCT):
        img = H.scene(w, h, seed)
        score, cand, kps = H.reference(w, h, seed)
        G.assert_keypoints_equal(fe.detect(img), kps)  # map-free
        assert _counts(fe, 1, "candidate_counts")[0] == len(cand)
        fe.set_keep_score_map(True)
        G.assert_keypoints_equal(fe.detect(img), kps)  # map-writing
        assert _counts(fe, 1, "candidate_counts")[0] == len(cand)
        got = _score_maps(fe, 1, w, h)[0]
        assert np.array_equal(got, score), np.argwhere(got != score)[:8]
        fe.set_keep_score_map(False)


@pytest.mark.parametrize("lw,lh", sorted(H.AS_LAYER))
def test_rows_below_the_minimum_as_a_scale_space_layer(oracle, lw, lh):
    """62 rows: layer 1 of a one-octave scale space over 93 rows (the layers take the map-writing form)"""
    w, h = H.AS_LAYER[(lw, lh)]
    fe = capi.Frontend(w, h, H.RADIUS, 1, H.THR, H.MAX_KPTS, max_candidates=H.MAX_CAND)
    for seed in range(H.DISTINCT):
        ref = H.layer_reference(w, h, seed)
        assert (ref["octave"] == 1).sum() > 50
        G.assert_keypoints_equal(fe.detect(H.layer_scene(w, h, seed)), ref)


@pytest.mark.parametrize("w,h", list(H.DIRECT) + [H.PACKED])
def test_batch_with_61_row_tiles(oracle, w, h):
    """a batch that takes the 61-row tiles: candidate and kept counts of every image in both forms, every score row of
    the map-writing form"""
    n = H.batch_for_tile_61(w, h)
    fe = capi.Frontend(w, h, H.RADIUS, 0, H.THR, H.MAX_KPTS, max_batch=n, max_candidates=H.MAX_CAND)
    fe.set_internal_lanes(1)  # one launch for the whole batch: the tile height follows the launch's size
    imgs = np.stack([H.scene(w, h, i % H.DISTINCT) for i in range(n)])
    d_img = torch.from_numpy(imgs).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    fe.detect_batch_device(d_img.data_ptr(), n, stream)
    torch.cuda.synchronize()
    assert fe.device_outputs().scores is None
    _check_counts(fe, n, w, h)
    fe.set_keep_score_map(True)
    fe.detect_batch_device(d_img.data_ptr(), n, stream)
    torch.cuda.synchronize()
    _check_counts(fe, n, w, h)
    maps = _score_maps(fe, n, w, h)
    for i in range(n):
        want = H.reference(w, h, i % H.DISTINCT)[0]
        assert np.array_equal(maps[i], want), (i, np.argwhere(maps[i] != want)[:8])
