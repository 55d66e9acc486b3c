"""Scenes of tests/test_gpu_final_slots.py, and what makes each worth running -- predicates over the CPU oracle's
keypoints that tests/test_final_slots_cases_host.py asserts without a GPU.

On the batched camera-aware route of a fused call the selection tail (k_select.hip) decides a keypoint's validity
completely -- border, ray, extra samples and the sample boxes of describe_aware_kernel's 64 lanes (describe_setup_dev.h:
first_pass_boxes_inside, skipped where the conservative patch bound lies strictly inside the image) -- counts the
survivors per pass of 256 and writes them to their final slots; the descriptor kernel works in place and a
back-projection kernel stands in for the compaction pass.  The scenes put keypoints on both sides of every one of these
decisions: on the border line of all four rims, in the band where the border test passes and a sample box leaves the
image, where the quick test fails and the exact one passes, in images that keep nothing, and at kept counts around the
pass length.

Images are dots on a bright ground (a 3 x 3 dark dot is one Harris maximum at its centre) or noise; maps are hand-built
(ray (0, 0, 1) and gravity (0, 1, 0): M = [[J0, J1], [J3, J4]] / fu), the same M on every pixel off the every-8th-pixel
grid that the library's camera statistics sample (describe_scenes.py: _Maps)."""
import functools

import numpy as np

import describe_scenes as S
from okvis2_amd import synth

F = np.float32
GRAV = (0.0, 1.0, 0.0)
W, H = 256, 128
RADIUS, THR, MAX_KPTS = 6.5, 50, 600
PATTERNS = ("default", "box1.73")  # both widths of the extra boxes (5 x 5 and 10 x 10)
BAND_M = S.similarity(1.22, 0.4)   # row norms 1.22: boxes reach beyond the border line, patches stay in the LDS classes


def camera(w=W, h=H, radtan8=False):
    """intrinsics of the back-projection (the hand-built maps replace the camera's own)"""
    if radtan8:
        return synth.Camera(w, h, 150.0, 148.0, w / 2.0 - 0.6, h / 2.0 + 0.2, 3,
                            (-0.12, 0.02, 2.0e-4, -1.0e-4, 0.003, 0.01, -0.002, 0.0005))
    return synth.Camera(w, h, 150.0, 148.0, w / 2.0 - 0.6, h / 2.0 + 0.2, 1, (-0.12, 0.02, 2.0e-4, -1.0e-4))


@functools.lru_cache(maxsize=None)
def maps(M=None, w=W, h=H):
    """(rays, jac, fu): M on every pixel but the statistics grid (identity there and where M is None)"""
    m = S._Maps(w, h, GRAV)
    if M is not None:
        jac = np.array([M[0], M[1], 0.0, M[2], M[3], 0.0], dtype=F)
        on_grid = (np.arange(h)[:, None] % 8 == 0) & (np.arange(w)[None, :] % 8 == 0)
        m.jac[~on_grid] = jac
    m.rays.setflags(write=False)
    m.jac.setflags(write=False)
    return m.rays, m.jac, 1.0


def dots(centres, w=W, h=H):
    img = np.full((h, w), 250, dtype=np.uint8)
    for x, y in centres:
        img[y - 1:y + 2, x - 1:x + 2] = 10
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def rim_scene(pat_key):
    """dots at border - 3 .. border + 3 pixels from each of the four rims (a dot's maxima sit a pixel off its centre),
    one of each distance along every rim"""
    b = int(S.pattern(pat_key).border)
    c = []
    for i, d in enumerate(range(b - 3, b + 4)):
        c += [(d, 34 + 9 * i), (W - 1 - d, 38 + 9 * i), (44 + 13 * i, d), (140 + 13 * i, H - 1 - d)]
    return dots(c)


@functools.lru_cache(maxsize=None)
def band_scene():
    """a sheared lattice of dots, nine pixels apart, row j shifted by j pixels: every distance from every rim occurs"""
    c = [(6 + 9 * i + (j % 9), 6 + 9 * j) for j in range((H - 12) // 9 + 1) for i in range((W - 21) // 9 + 1)]
    return dots([(x, y) for x, y in c if 4 <= x < W - 4 and 4 <= y < H - 4])


@functools.lru_cache(maxsize=None)
def all_dropped_scene(pat_key):
    """dots closer to a rim than the border: detected, none described"""
    b = int(S.pattern(pat_key).border)
    c = [(6 + 10 * i, 5 + (i % 3) * 4) for i in range(24)] + [(6 + 10 * i, H - 6 - (i % 3) * 4) for i in range(24)]
    c += [(5 + (j % 3) * 4, 30 + 10 * j) for j in range(7)] + [(W - 6 - (j % 3) * 4, 30 + 10 * j) for j in range(7)]
    assert all(min(x, y, W - 1 - x, H - 1 - y) < b - 3 for x, y in c)
    return dots(c)


def flat_scene():
    img = np.full((H, W), 128, dtype=np.uint8)
    img.setflags(write=False)
    return img


# ---- kept counts around the pass length: noise, the cap decides ------------------------------------------------------
PASS_COUNTS = (255, 256, 257, 513)
PASS_RADIUS, PASS_THR = 6.5, 30


@functools.lru_cache(maxsize=None)
def pass_scene():
    img = synth.noise_image(W, H, 12)
    img.setflags(write=False)
    return img


# ---- the predicates --------------------------------------------------------------------------------------------------
def reference(oracle, img, M, radius=RADIUS, thr=THR, max_kpts=MAX_KPTS, w=W, h=H):
    """(detected, described keypoints, descriptors) by the oracle under maps(M)"""
    rays, jac, fu = maps(M, w, h)
    det = oracle.detect(img, radius, 0, thr, max_kpts)
    k, d = oracle.describe(img, det, oracle.MODE_CAMERA_AWARE, rays, jac, F(fu), GRAV)
    return det, k, d


def m_at(M, x, y):
    u, v = int(F(x) + F(0.5)), int(F(y) + F(0.5))
    return (1.0, 0.0, 0.0, 1.0) if (M is None or (u % 8 == 0 and v % 8 == 0)) else M


def passes_border(p, x, y, w=W, h=H):
    b = F(int(p.border))
    return not (F(x) < b or F(x) >= F(w - int(p.border)) or F(y) < b or F(y) >= F(h - int(p.border)))


def quick_inside(p, M, x, y, w=W, h=H):
    """the tail's quick test in float32: the conservative patch bound strictly inside the image"""
    M = [F(v) for v in M]
    reach = S.pattern_reach(p)
    nx = F(np.sqrt(F(F(M[0] * M[0]) + F(M[1] * M[1]))) * F(1.001))
    ny = F(np.sqrt(F(F(M[2] * M[2]) + F(M[3] * M[3]))) * F(1.001))
    ex = F(F(max(nx, F(1.0)) * reach) + F(0.75))
    ey = F(F(max(ny, F(1.0)) * reach) + F(0.75))
    x, y = F(x), F(y)
    return bool(F(x - ex) >= 0 and F(x + ex) < F(w - 1) and F(y - ey) >= 0 and F(y + ey) < F(h - 1))


def census(p, det, kept, M, w=W, h=H):
    """-> dict of counts over the detected keypoints: dropped by the border test, dropped by a sample box although the
    border test passes, kept although the quick test fails, kept with the quick test"""
    kept_xy = {(float(k["x"]), float(k["y"])) for k in kept}
    out = dict(border=0, box=0, kept_exact=0, kept_quick=0)
    for q in det:
        x, y = q["x"], q["y"]
        Mq = m_at(M, x, y)
        is_kept = (float(x), float(y)) in kept_xy
        if not passes_border(p, x, y, w, h):
            assert not is_kept
            out["border"] += 1
        elif not is_kept:
            assert not S.boxes_inside(p, Mq, x, y, w, h)
            out["box"] += 1
        elif quick_inside(p, Mq, x, y, w, h):
            assert S.boxes_inside(p, Mq, x, y, w, h)  # the quick test is a subset of the exact one
            out["kept_quick"] += 1
        else:
            out["kept_exact"] += 1
    return out
