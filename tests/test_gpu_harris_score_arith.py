"""GPU: the score arithmetic of harris_kernel (csrc/k_harris.hip, score_row) on the scenes of tests/harris_score_cases.py
-- 0/255 edges of every direction, stripes and checkers of 1 .. 3 px, half-amplitude noise, a flat image -- which put
A, B and C at the parities, signs and sizes the census of that file counts.  Every form that computes a score: the fused
kernel writing its map (set_keep_score_map(True): every score byte-equal to the oracle), the map-free form (candidate
counts and the kept keypoints, which are the candidate records after selection, byte for byte; the C ABI hands out no
candidate records as such) and okvfe_harris_score_device (the score-only kernel, byte-equal to the oracle).  One image
per call (25-row tiles) and a batch sized for 61-row tiles, on one strip, two strips and a packed last strip."""
import ctypes as C

import numpy as np
import pytest

from okvis2_amd import capi

import gpu_common as G
import harris_score_cases as H

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


def _check_counts(fe, shape, n):
    cand, kept = _counts(fe, n, "candidate_counts"), _counts(fe, n, "detect_counts")
    for i in range(n):
        name = H.NAMES[i % len(H.NAMES)]
        _, rc, rk = H.reference(shape, name)
        assert cand[i] == len(rc) and kept[i] == len(rk), (i, name, cand[i], len(rc), kept[i], len(rk))


@pytest.mark.parametrize("shape", sorted(H.SHAPES))
def test_one_image_per_call(oracle, shape):
    """25-row tiles: map-free candidates and keypoints, then the map-writing form and every score of its map"""
    w, h = H.SHAPES[shape]
    fe = capi.Frontend(w, h, H.RADIUS, 0, H.THR, H.MAX_KPTS)
    for name in H.NAMES:
        img = H.scene(shape, name)
        score, cand, kps = H.reference(shape, name)
        G.assert_keypoints_equal(fe.detect(img), kps)  # map-free
        assert _counts(fe, 1, "candidate_counts")[0] == len(cand), name
        fe.set_keep_score_map(True)
        G.assert_keypoints_equal(fe.detect(img), kps)  # map-writing
        assert _counts(fe, 1, "candidate_counts")[0] == len(cand), name
        got = _score_maps(fe, 1, w, h)[0]
        assert np.array_equal(got, score), (name, np.argwhere(got != score)[:8])
        fe.set_keep_score_map(False)


@pytest.mark.parametrize("shape", sorted(H.SHAPES))
def test_batch_with_61_row_tiles(oracle, shape):
    """a batch that takes the 61-row tiles, the scenes in turn: candidate and kept counts of every image in both forms,
    every score of the map-writing form"""
    w, h = H.SHAPES[shape]
    n = H.batch_for_tile_61(shape)
    assert n >= len(H.NAMES)
    fe = capi.Frontend(w, h, H.RADIUS, 0, H.THR, H.MAX_KPTS, max_batch=n)
    fe.set_internal_lanes(1)  # one launch for the whole batch: the tile height follows the launch's size
    imgs = np.stack([H.scene(shape, H.NAMES[i % len(H.NAMES)]) for i in range(n)])
    d_img = torch.from_numpy(imgs).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    fe.detect_batch_device(d_img.data_ptr(), n, stream)
    torch.cuda.synchronize()
    assert fe.device_outputs().scores is None
    _check_counts(fe, shape, n)
    fe.set_keep_score_map(True)
    fe.detect_batch_device(d_img.data_ptr(), n, stream)
    torch.cuda.synchronize()
    _check_counts(fe, shape, n)
    maps = _score_maps(fe, n, w, h)
    for i in range(n):
        name = H.NAMES[i % len(H.NAMES)]
        want = H.reference(shape, name)[0]
        assert np.array_equal(maps[i], want), (i, name, np.argwhere(maps[i] != want)[:8])


@pytest.mark.parametrize("shape", sorted(H.SHAPES))
def test_score_only_kernel(oracle, shape):
    """okvfe_harris_score_device: the dense map of every scene, one call for all of them"""
    w, h = H.SHAPES[shape]
    n = len(H.NAMES)
    fe = capi.Frontend(w, h, H.RADIUS, 0, H.THR, H.MAX_KPTS, max_batch=n)
    imgs = np.stack([H.scene(shape, name) for name in H.NAMES])
    d_img = torch.from_numpy(imgs).cuda()
    d_sc = torch.full((n, h, w), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    fe.harris_score_device(d_img.data_ptr(), n, d_sc.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_sc.cpu().numpy()
    for i, name in enumerate(H.NAMES):
        want = H.reference(shape, name)[0]
        assert np.array_equal(got[i], want), (name, np.argwhere(got[i] != want)[:8])
