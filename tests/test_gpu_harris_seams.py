"""GPU: the lane and strip hand-overs of the fused score + NMS kernel (harris_kernel, csrc/k_harris.hip).  A lane takes
the pixels, covariance products and scores next to its own four columns from its neighbour lanes; lane 0 and lane 63 of a
wave have one neighbour only, and strips meet at seams.  The scenes of tests/harris_seam_cases.py plant maxima on both
sides of every hand-over (equal-score pairs across it included: the fix-up flag), in the outermost columns and in the
first and last tested rows, on one strip (partly and exactly full), two and three strips and a packed last strip whose
wave is partly filled.  The map-free and the map-writing form, one image per call (25-row tiles) and a batch large
enough for 61-row tiles: kept keypoints, candidate counts and every score row against the oracle; and one scale-space
call of one octave whose second layer runs the packed form beside the first layer's kernel."""
import ctypes as C

import numpy as np
import pytest

from okvis2_amd import capi

import gpu_common as G
import harris_seam_cases as S

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


def _check_counts(fe, name, n):
    cand, kept = _counts(fe, n, "candidate_counts"), _counts(fe, n, "detect_counts")
    for i in range(n):
        _, rc, rk = S.reference(name, i % S.DISTINCT)
        assert cand[i] == len(rc) and kept[i] == len(rk), (i, cand[i], len(rc), kept[i], len(rk))


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_one_image_per_call(oracle, name):
    """25-row tiles (a call that cannot fill the GPU): keypoints byte for byte, both forms, and every row of the map"""
    w, h = S.CASES[name]
    fe = capi.Frontend(w, h, S.RADIUS, 0, S.THR, S.MAX_KPTS, max_candidates=S.MAX_CAND)
    for seed in range(S.DISTINCT):
        img = S.scene(name, seed)
        score, cand, kps = S.reference(name, seed)
        G.assert_keypoints_equal(fe.detect(img), kps)  # map-free
        assert _counts(fe, 1, "candidate_counts")[0] == len(cand)
        fe.set_keep_score_map(True)
        G.assert_keypoints_equal(fe.detect(img), kps)  # map-writing
        assert _counts(fe, 1, "candidate_counts")[0] == len(cand)
        got = _score_maps(fe, 1, w, h)[0]
        assert np.array_equal(got, score), np.argwhere(got != score)[:8]
        fe.set_keep_score_map(False)


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_batch_with_61_row_tiles(oracle, name):
    """a batch that takes the 61-row tiles (the packed width: twelve full waves of ten images and one of nine): candidate
    and kept counts of every image in both forms, every score row of the map-writing form"""
    w, h = S.CASES[name]
    n = S.batch_for_tile_61(name)
    fe = capi.Frontend(w, h, S.RADIUS, 0, S.THR, S.MAX_KPTS, max_batch=n, max_candidates=S.MAX_CAND)
    fe.set_internal_lanes(1)  # one launch for the whole batch: the tile height follows the launch's size
    imgs = np.stack([S.scene(name, i % S.DISTINCT) for i in range(n)])
    d_img = torch.from_numpy(imgs).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    fe.detect_batch_device(d_img.data_ptr(), n, stream)
    torch.cuda.synchronize()
    assert fe.device_outputs().scores is None
    _check_counts(fe, name, n)
    fe.set_keep_score_map(True)
    fe.detect_batch_device(d_img.data_ptr(), n, stream)
    torch.cuda.synchronize()
    _check_counts(fe, name, n)
    maps = _score_maps(fe, n, w, h)
    for i in range(n):
        want = S.reference(name, i % S.DISTINCT)[0]
        assert np.array_equal(maps[i], want), (i, np.argwhere(maps[i] != want)[:8])


def test_packed_layer_beside_another_layers_kernel(oracle):
    """a scale space of one octave: layer 0 (408 px, two plain strips) and layer 1 (272 px, packed) take the map-writing
    form on streams of their own"""
    w, h = S.LAYER_IMAGE
    fe = capi.Frontend(w, h, S.RADIUS, 1, S.THR, S.MAX_KPTS, max_candidates=S.MAX_CAND)
    for seed in range(S.DISTINCT):
        G.assert_keypoints_equal(fe.detect(S.layer_scene(seed)), S.layer_reference(seed))
