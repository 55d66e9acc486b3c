"""GPU: the self-ordering selection kernel (select_lazy_kernel<true>) against the oracle, byte for byte, on the
edges of its chunk loop and its tail: the cap reached inside a chunk, empty / tiny / overflowing candidate sets,
thousands of tied scores through the key-range split, keypoints on the image rim, a batch of mixed content in one
call -- with and without a score map."""
import numpy as np
import pytest

from okvis2_amd import capi, synth

import gpu_common as G

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
W, H = 752, 480


def _checker(cell=9):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where(((xx // cell) + (yy // cell)) % 2 == 0, 40, 215).astype(np.uint8)


def _rim(seed):
    img = synth.noise_image(W, H, seed).copy()
    img[2:4, :] = np.where((np.arange(W) // 3) % 2 == 0, 250, 5)
    img[-4:-2, :] = img[2:4, :]
    img[:, 2:4] = np.where((np.arange(H) // 3) % 2 == 0, 250, 5)[:, None]
    img[:, -4:-2] = img[:, 2:4]
    return img


def _both_paths(fe, img, ref):
    G.assert_keypoints_equal(fe.detect(img), ref)  # map-free
    fe.set_keep_score_map(True)
    G.assert_keypoints_equal(fe.detect(img), ref)  # okvfe_set_keep_score_map: through the score map
    fe.set_keep_score_map(False)


@pytest.mark.parametrize("maxk", [1, 7, 64])
def test_cap_inside_a_chunk(oracle, maxk):
    img = synth.corners_image(W, H, 11)
    fe = capi.Frontend(W, H, 38.0, 0, 40, maxk, max_candidates=1 << 15)
    ref = oracle.detect(img, 38.0, 0, 40, maxk)
    assert len(ref) == maxk
    _both_paths(fe, img, ref)


def test_zero_one_and_capacity_candidates(oracle):
    fe = capi.Frontend(W, H, 38.0, 0, 150, 700, max_candidates=1 << 15)
    flat = np.full((H, W), 128, np.uint8)
    _both_paths(fe, flat, oracle.detect(flat, 38.0, 0, 150, 700))
    one = np.full((H, W), 20, np.uint8)
    one[200:210, 300:310] = 220
    ref = oracle.detect(one, 38.0, 0, 150, 700)
    assert len(ref) >= 1
    _both_paths(fe, one, ref)
    # a candidate list of exactly its capacity is selected; one more overflows (no keypoints, reported)
    img = synth.noise_image(W, H, 21)
    n = len(oracle.nms(oracle.harris_score(img), 40))
    exact = capi.Frontend(W, H, 38.0, 0, 40, 700, max_candidates=n)
    _both_paths(exact, img, oracle.detect(img, 38.0, 0, 40, 700))
    over = capi.Frontend(W, H, 38.0, 0, 40, 700, max_candidates=n - 1)
    with pytest.raises(capi.OkvfeError) as e:
        over.detect(img)
    assert e.value.status == capi.ERR_CAPACITY


@pytest.mark.parametrize("maxk,radius", [(700, 38.0), (150, 38.0), (700, 17.0)])
def test_tied_scores_through_the_key_range_split(oracle, maxk, radius):
    img = _checker()
    fe = capi.Frontend(W, H, radius, 0, 100, maxk, max_candidates=1 << 15)
    ref = oracle.detect(img, radius, 0, 100, maxk)
    assert len(ref) > 50
    _both_paths(fe, img, ref)


def test_rim_keypoints(oracle):
    fe = capi.Frontend(W, H, 38.0, 0, 40, 700, max_candidates=1 << 16)
    for seed in (300, 301):
        img = _rim(seed)
        ref = oracle.detect(img, 38.0, 0, 40, 700)
        assert len(ref) > 100
        _both_paths(fe, img, ref)


@pytest.mark.parametrize("n_images", [1, 6])
def test_mixed_batch_with_description(oracle, n_images):
    """B = 1 and a batch that mixes empty, corner, checker and rim content in one call, with the camera-aware
    extractor's set-up in the selection's tail (the keypoints AND the descriptors against the oracle)."""
    cfg = synth.euroc_config()
    fb = G.make_frontend(cfg, max_batch=n_images)
    for ci, cam in enumerate(cfg.cams):
        fb.set_camera(ci, cam)
    pool = [G.image_for(cfg, 5), np.zeros((H, W), np.uint8), _checker(12), _rim(7), G.image_for(cfg, 6),
            synth.noise_image(W, H, 8)]
    imgs = np.stack(pool[:n_images])
    d = torch.from_numpy(imgs).cuda()
    cams = np.array([i % 2 for i in range(n_images)], np.int32)
    fb.detect_describe_batch_device(d.data_ptr(), n_images, cams, np.tile(np.array([0, 1, 0], np.float32),
                                                                            (n_images, 1)), None)
    torch.cuda.synchronize()
    for i in range(n_images):
        cam = cfg.cams[cams[i]]
        rays, jac = oracle.awareness_maps(cam)
        rk, rd = oracle.detect_describe(imgs[i], cfg.uniformity_radius, 0, cfg.abs_threshold, cfg.max_kpts,
                                        oracle.MODE_CAMERA_AWARE, rays, jac, np.float32(cam.fu), (0.0, 1.0, 0.0))
        k, dd, _, _ = fb.download(i)
        G.assert_keypoints_equal(k, rk)
        assert np.array_equal(dd, rd)
