"""Scenes of tests/test_gpu_select_tail_loads.py, and what makes each of them worth running -- stated as predicates over
the CPU oracle's keypoints, which tests/test_select_tail_loads_cases.py asserts without a GPU.

The selection tail (refine_emit, k_select.hip) reads the 7 x 7 window of a kept keypoint as one 12-byte run per row from
a base clamped into the row, and ray and Jacobian as three loads.  The pattern's centre sample lies in that window for
most keypoints (a form of the tail that takes it from there has to pass the centre-sample scenes; today every lane
loads it), and the record the tail leaves travels on through every descriptor route.  The scenes put keypoints where
each of these can go wrong: on all four rims of the first and the last image of a batch whose tensor holds nothing
else, on refinements of exactly +-1 pixel, on both sides of the "box inside window and image" test, next to keypoints
the ray test drops, and on every descriptor route behind the tail."""
import functools

import numpy as np

from okvis2_amd import synth

F = np.float32
GRAV = (0.05, 0.99, -0.1)

# ---- window rim: 64 x 64 and 76 x 64 (a row whose last 12-byte run is not 16-byte aligned) -------------------------
RIM_RADIUS, RIM_THRESHOLD, RIM_KPTS = 4.0, 20, 400
RIM_H = 64
RIM_SEED = {64: 3, 76: 46}  # seeds whose mirrored scenes put at least two keypoints on every rim (searched with the oracle)


@functools.lru_cache(maxsize=None)
def rim_scenes(w):
    """plain / mirrored in x / mirrored in y"""
    base = synth.corners_image(w, RIM_H, RIM_SEED[w], cell=7, jitter=2)
    out = {"plain": base, "mx": base[:, ::-1].copy(), "my": base[::-1].copy()}
    for a in out.values():
        a.setflags(write=False)
    return out


RIM_ORDER = ("mx", "my", "plain")  # image 0: the left-rim scene; last image: a bottom-rim scene


def rim_batch(w):
    s = rim_scenes(w)
    return np.stack([s[k] for k in RIM_ORDER])


def rim_camera(w, h=RIM_H):
    return synth.Camera(w, h, 80.0, 81.0, w / 2 - 0.7, h / 2 + 0.4, 1, (-0.05, 0.004, 0.0002, -0.0001))


def rim_counts(det, w, h):
    """keypoints with x < 2, x > w - 3, y < 2, y > h - 3"""
    x, y = det["x"], det["y"]
    return int((x < 2).sum()), int((x > w - 3).sum()), int((y < 2).sum()), int((y > h - 3).sum())


def integer_coordinates(det):
    """keypoints with a coordinate on the pixel grid: refinements of 0 or exactly +-1, which reach the window's edge"""
    x, y = det["x"], det["y"]
    return int(((x == np.floor(x)) | (y == np.floor(y))).sum())


# ---- centre sample: the "box inside window and image" test, restated -------------------------------------------------
def integer_maxima(det, score, w, h):
    """(u, v) of the integer maximum each keypoint was refined from -- the one pixel within a pixel of it that carries
    its score -- or None where that is ambiguous"""
    out = []
    for p in det:
        found = [(u, v) for v in range(int(p["y"]) - 1, int(p["y"]) + 3) for u in range(int(p["x"]) - 1, int(p["x"]) + 3)
                 if 0 <= u < w and 0 <= v < h and abs(p["x"] - u) <= 1 and abs(p["y"] - v) <= 1 and
                 F(score[v, u]) == p["response"]]
        out.append(found[0] if len(found) == 1 else None)
    return out


def centre_box_in_window(x, y, u, v, sigma_half, w, h):
    """the box of a sample AT the keypoint (pattern offset 0, 0) lies inside the image and inside the 7 x 7 window
    around (u, v): float32 arithmetic of the published box sum (x -+ sigma_half, rounded to the nearest pixel)"""
    x, y, s = F(x), F(y), F(sigma_half)
    x_1, x1, y_1, y1 = F(x - s), F(x + s), F(y - s), F(y + s)
    if not (x_1 >= 0 and y_1 >= 0 and x1 < F(w - 1) and y1 < F(h - 1)):
        return False
    x_left, x_right = int(F(x_1 + F(0.5))), int(F(x1 + F(0.5)))
    y_top, y_bottom = int(F(y_1 + F(0.5))), int(F(y1 + F(0.5)))
    if x_right - x_left > 4 or y_bottom - y_top > 4:
        return False
    return x_left >= u - 3 and x_right <= u + 3 and y_top >= v - 3 and y_bottom <= v + 3


def centre_census(det, score, w, h, sigma_half):
    """-> (keypoints whose centre box fits window and image, keypoints whose box does not, unresolved maxima)"""
    inside = outside = unknown = 0
    for p, uv in zip(det, integer_maxima(det, score, w, h)):
        if uv is None:
            unknown += 1
        elif centre_box_in_window(p["x"], p["y"], uv[0], uv[1], sigma_half, w, h):
            inside += 1
        else:
            outside += 1
    return inside, outside, unknown


CENTRE_SEED = 61
WIDE_BOX_SCALE = 1.73  # box class 1: the extra boxes take the 10 x 10 form, no sample comes from the window


@functools.lru_cache(maxsize=None)
def centre_scene():
    cfg = synth.euroc_config()
    img = synth.corners_image(cfg.w, cfg.h, CENTRE_SEED)
    img.setflags(write=False)
    return cfg, img


# ---- dropped keypoints: a camera whose rays are zero on part of the image -------------------------------------------
DROP_W, DROP_H, DROP_SEED = 128, 96, 5
DROP_FROM_X = 70  # rays of columns >= this are zero


def drop_camera():
    return rim_camera(DROP_W, DROP_H)


def drop_maps(oracle):
    rays, jac = oracle.awareness_maps(drop_camera())
    rays = np.array(rays, dtype=np.float32).reshape(DROP_H, DROP_W, 3).copy()
    rays[:, DROP_FROM_X:, :] = 0.0
    return rays, np.array(jac, dtype=np.float32).reshape(DROP_H, DROP_W, 6).copy()


@functools.lru_cache(maxsize=None)
def drop_scene():
    img = synth.corners_image(DROP_W, DROP_H, DROP_SEED, cell=7, jitter=2)
    img.setflags(write=False)
    return img


# ---- descriptor routes: a batch of three whose middle image is flat ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def flat_middle_batch():
    cfg = synth.euroc_config()
    imgs = np.stack([synth.corners_image(cfg.w, cfg.h, 43), np.full((cfg.h, cfg.w), 128, np.uint8),
                     synth.corners_image(cfg.w, cfg.h, 44)])
    imgs.setflags(write=False)
    return cfg, imgs


LANES_IMAGES = 128  # two internal lanes need 64 images each
