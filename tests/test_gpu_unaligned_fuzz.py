"""GPU: the two generators of test_gpu_fuzz.py on widths that are NOT a multiple of 4 (64 .. 920, redrawn until
w % 4 != 0) and at a device pointer 0 .. 3 bytes past an aligned address, through okvfe_detect_describe_batch_device on
a batch of 1 .. 5 images -- the dense fallback chain (unaligned_cases.py) on shapes no hand-written case names.  Seed
bases of their own: no configuration of test_gpu_fuzz.py moves."""
import numpy as np
import pytest

from okvis2_amd import capi, synth

import gpu_common as G

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _image(rng, w, h, kind):
    if kind == "noise":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "corners":
        return synth.corners_image(w, h, int(rng.integers(1, 10000)), cell=int(rng.choice([8, 12, 20])))
    # blocks: every pixel doubled -> equal-score neighbours (fix-up pass), plus a flat band
    small = synth.corners_image((w + 1) // 2, (h + 1) // 2, int(rng.integers(1, 10000)), cell=6)
    img = np.repeat(np.repeat(small, 2, axis=0), 2, axis=1)[:h, :w].copy()
    img[h // 3:h // 3 + 9, :] = 77
    return img


def _odd_width(rng):
    w = int(rng.integers(64, 921))
    while w % 4 == 0:
        w = int(rng.integers(64, 921))
    return w


def _batch_on_device(imgs, offset):
    flat = np.ascontiguousarray(imgs).reshape(-1)
    buf = torch.zeros(flat.size + 8, dtype=torch.uint8, device="cuda")
    buf[offset:offset + flat.size] = torch.from_numpy(flat).cuda()
    return buf, buf.data_ptr() + offset


@pytest.mark.parametrize("seed", list(range(16)))
def test_random_configuration_at_an_odd_width(oracle, seed):
    rng = np.random.default_rng(21000 + seed)
    w = _odd_width(rng)
    h = int(rng.integers(70, 420))
    kind = ["noise", "corners", "blocks"][seed % 3]
    radius = float(rng.choice([6.0, 10.0, 17.5, 26.0, 38.0]))
    thr = int(rng.choice([1, 5, 40, 150, 400]))
    maxk = int(rng.choice([50, 300, 700, 2000]))
    mode = ["upright", "gradient", "upright", "gradient"][seed % 4]
    si = bool(seed % 5 == 0)
    offset = int(rng.integers(0, 4))
    n = int(rng.integers(1, 6))
    imgs = np.stack([_image(rng, w, h, kind) for _ in range(n)])
    fe = capi.Frontend(w, h, radius, 0, thr, maxk, rotation_invariant=(mode == "gradient"), scale_invariant=si,
                       max_candidates=1 << 16, max_batch=n)
    omode = oracle.MODE_GRADIENT if mode == "gradient" else oracle.MODE_UPRIGHT
    rk, rd = oracle.detect_describe(imgs[0], radius, 0, thr, maxk, omode, scale_invariant=si)
    kps, desc, _, _ = fe.detect_describe(imgs[0])
    G.assert_keypoints_equal(kps, rk)
    assert np.array_equal(desc, rd), (w, h, kind, radius, thr, maxk, mode, si)
    det = fe.detect(imgs[0])
    ref = oracle.detect(imgs[0], radius, 0, thr, maxk)
    G.assert_keypoints_equal(det, ref)
    buf, ptr = _batch_on_device(imgs, offset)
    fe.detect_describe_batch_device(ptr, n, None, None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    fe.check_capacity(n)
    for i in range(n):
        rk, rd = oracle.detect_describe(imgs[i], radius, 0, thr, maxk, omode, scale_invariant=si)
        k, d, _, _ = fe.download(i)
        G.assert_keypoints_equal(k, rk)
        assert np.array_equal(d, rd), (w, h, kind, radius, thr, maxk, mode, si, offset, n, i)


@pytest.mark.parametrize("seed", list(range(16)))
def test_random_camera_aware_configuration_at_an_odd_width(oracle, seed):
    """The production extraction mode on random cameras (radial-tangential / equidistant, focal length 0.45 .. 1.3
    image widths, off-centre principal point), random extraction directions, sizes, content, thresholds, radii and
    caps, where the camera-aware-only descriptor kernel, map-free detection and the self-ordering selection's fused
    set-up do NOT apply: describe_kernel<4, generic> behind the dense score map."""
    rng = np.random.default_rng(25000 + seed)
    w = _odd_width(rng)
    h = int(rng.integers(80, 500))
    kind = ["noise", "corners", "blocks"][seed % 3]
    radius = float(rng.choice([10.0, 17.5, 26.0, 38.0, 50.0]))
    thr = int(rng.choice([5, 40, 150, 400]))
    maxk = int(rng.choice([50, 300, 700, 1500]))
    offset = int(rng.integers(0, 4))
    n = int(rng.integers(1, 6))
    imgs = np.stack([_image(rng, w, h, kind) for _ in range(n)])
    dist = int(rng.choice([1, 2]))
    f = float(rng.uniform(0.45, 1.3)) * w
    d = (tuple(rng.uniform(-0.3, 0.1, 1)) + tuple(rng.uniform(-0.05, 0.1, 1)) + tuple(rng.uniform(-2e-3, 2e-3, 2))) \
        if dist == 1 else tuple(rng.uniform(-0.02, 0.02, 4))
    cam = synth.Camera(w, h, f, f * float(rng.uniform(0.97, 1.03)), w / 2 + float(rng.uniform(-8, 8)),
                       h / 2 + float(rng.uniform(-8, 8)), dist, tuple(float(x) for x in d))
    g = rng.normal(0, 1, 3)
    g[1] += 2.0
    g = tuple(float(x) for x in (g / np.linalg.norm(g)).astype(np.float32))
    fe = capi.Frontend(w, h, radius, 0, thr, maxk, max_candidates=1 << 16, max_batch=n)
    fe.set_camera(0, cam)
    rays, jac = oracle.awareness_maps(cam)
    rk, rd = oracle.detect_describe(imgs[0], radius, 0, thr, maxk, oracle.MODE_CAMERA_AWARE, rays, jac, np.float32(cam.fu), g)
    kps, desc, _, _ = fe.detect_describe(imgs[0], cam=0, gravity=g)
    G.assert_keypoints_equal(kps, rk)
    assert np.array_equal(desc, rd), (w, h, kind, radius, thr, maxk, dist)
    buf, ptr = _batch_on_device(imgs, offset)
    fe.detect_describe_batch_device(ptr, n, np.zeros(n, np.int32), np.tile(np.float32(g), (n, 1)),
                                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    fe.check_capacity(n)
    for i in range(n):
        rk, rd = oracle.detect_describe(imgs[i], radius, 0, thr, maxk, oracle.MODE_CAMERA_AWARE, rays, jac,
                                        np.float32(cam.fu), g)
        rbp, rv = oracle.backproject_keypoints(cam, rk)
        k, dd, bp, bv = fe.download(i)
        G.assert_keypoints_equal(k, rk)
        assert np.array_equal(dd, rd), (w, h, kind, radius, thr, maxk, dist, offset, n, i)
        assert np.array_equal(bv, rv) and np.array_equal(bp.view(np.uint64), rbp.view(np.uint64)), i
