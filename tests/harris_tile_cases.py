"""Scenes and references shared by tests/test_harris_tile_scenes_host.py and tests/test_gpu_harris_last_tile.py: images
whose heights leave the fused score + NMS kernel (harris_kernel, csrc/k_harris.hip) a partial last row tile.

A wave of that kernel owns one strip x TH rows (TH = 61; calls too small to fill the GPU take 25) and walks them in
groups of six row steps; in the last tile of an image the rows past the image are computed, never stored and never
tested, and rows h - 2 and h - 1 are stored and not tested.  The heights below leave a last tile of 1, 5, 6 (one full
group), 7 (one row into the second group), 60 and 61 rows under TH = 61 and of 12 .. 23 under TH = 25.  A context takes
images of 64 rows and more, so the 62-row case runs as the 2/3-sampled layer of a 93-row scale space (372 x 93 ->
248 x 62, 750 x 93 -> 500 x 62: layer_size, csrc/capi_context.cpp).  Noise carries maxima on (almost) every row; dots
are planted on the rows where a row loop that stops a group early or stores a row too many would show: rows h - 3 and
h - 4 (the last two that may carry maxima), the first and last row of the last tile and the last row of the tile before
it.  (A form of the kernel that ends the last tile at the group of six that reaches the image's last row passed these
scenes and was not kept, for want of a measurable gain: LAB_NOTES.md, "Final slots assigned in the selection tail".)"""
import functools

import numpy as np

from okvis2_amd import synth

HEIGHTS = (62, 66, 67, 68, 121, 122, 123)
WIDTHS = (248, 500)
MIN_ROWS = 64  # okvfe_create refuses smaller images; smaller layers exist inside a scale space only
DIRECT = tuple((w, h) for w in WIDTHS for h in HEIGHTS if h >= MIN_ROWS)
AS_LAYER = {(w, h): ((w // 2) * 3, (h // 2) * 3) for w in WIDTHS for h in HEIGHTS if h < MIN_ROWS}  # layer -> image size
PACKED = (1032, 68)  # five strips, the narrow last one shared by six images per wave
TILE_ROWS = (25, 61)
RADIUS, THR, MAX_KPTS, MAX_CAND = 8.0, 60, 1500, 1 << 13
DISTINCT = 3


def planted_rows(h):
    """rows that get dots, for both tile heights"""
    rows = {h - 3, h - 4}
    for th in TILE_ROWS:
        first = ((h - 1) // th) * th  # first row of the last tile
        rows |= {first, h - 1, first - 1}
    return sorted(r for r in rows if 0 <= r < h)


def testable(h, rows):
    """the rows of `rows` that may carry maxima (2 <= y < h - 2)"""
    return [r for r in rows if 2 <= r < h - 2]


@functools.lru_cache(maxsize=None)
def scene(w, h, seed):
    """noise at half contrast with one bright dot per planted row in a dark pad of its own (columns differ per row so
    that pads of neighbouring rows do not overlap)"""
    img = (synth.noise_image(w, h, seed) // 2 + 40).astype(np.uint8)
    for i, y in enumerate(planted_rows(h)):
        x = 12 + 17 * i + 5 * seed
        img[max(y - 3, 0):y + 4, x - 3:x + 4] = 10
        img[y, x] = 255
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def reference(w, h, seed):
    """(score map, candidates, kept keypoints) of scene(w, h, seed) by the oracle: computed once, never changed"""
    import oracle_lib as O
    img = scene(w, h, seed)
    score = O.harris_score(img)
    cand = O.nms(score, THR)
    kps = O.detect(img, RADIUS, 0, THR, MAX_KPTS)
    for a in (score, cand, kps):
        a.setflags(write=False)
    return score, cand, kps


def batch_for_tile_61(w, h):
    """images a call needs so that the library picks 61-row tiles (k_harris.hip: more than 128 blocks of four waves)"""
    nd = w // 4
    strips = 1
    while (strips - 1) * 62 + 64 < nd:
        strips += 1
    tiles = strips * ((h + 60) // 61)
    return 512 // tiles + 1


@functools.lru_cache(maxsize=None)
def layer_scene(w, h, seed):
    """jittered cells of ten pixels: structure that survives the 2/3 sampling, down to the last rows"""
    img = synth.corners_image(w, h, 40 + seed, cell=10)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def layer_reference(w, h, seed):
    """keypoints of layer_scene(w, h, seed) through a scale space of one octave (layers w x h and (w / 3) * 2 x
    (h / 3) * 2) by the oracle"""
    import oracle_lib as O
    k = O.detect(layer_scene(w, h, seed), RADIUS, 1, THR, MAX_KPTS)
    k.setflags(write=False)
    return k
