"""Scenes and references shared by tests/test_harris_seam_cases.py and tests/test_gpu_harris_seams.py: images whose
maxima sit where the fused score + NMS kernel (harris_kernel, csrc/k_harris.hip) hands values from lane to lane and
from strip to strip.

A wave of that kernel owns one strip of a row tile: lane l of strip s holds dword 62 s + l (four pixels) of every row
and takes the pixels, the covariance products and the scores of the columns next to its own from lanes l - 1 and
l + 1.  Lane 0 has no left and lane 63 no right neighbour (they read zero): inside the image they are halo lanes whose
results are dropped (strips overlap by two dwords), at the image border the rim is zero by definition, and lanes past
the row end repeat the last dword.  So what can go wrong sits at lane 0 and lane 63 of a wave and at the strip seams,
between columns 248 k + 3 and 248 k + 4.  Where two horizontally adjacent pixels both pass the test (equal scores) the
row is flagged for nms_fixup_kernel, which needs both sides of a seam to agree on the hit.

Widths: one strip that is not full (200 px = 50 dwords: the lanes behind repeat the last dword), one strip exactly
full (256 px: lane 0 and lane 63 are both image border), two strips with the second exactly full (504 px), three
strips (752 px: 63 + 62 + 63 store lanes) and a width whose short last strip is packed, ten images to a wave (272 px: 6
dwords per image); batches of that width leave the last packed wave partly filled.  On the widths of one strip the
"seams" are the borders lane 0 | lane 1 and the last two dwords of the row.

Planted on noise at half contrast, each in a dark pad of its own: single bright pixels (a maximum of the score at the
pixel itself) on both sides of every seam in the first and the last tested row (2 and h - 3) and in rows between, in
columns 2 and w - 3 (the outermost that may carry maxima) and in columns 1 and w - 2 (which may not); and pairs of
bright pixels across every seam, whose two scores are equal by symmetry."""
import functools

import numpy as np

from okvis2_amd import synth

#        name          w    h
CASES = {"part_strip": (200, 64),
         "full_strip": (256, 66),
         "two_strips": (504, 64),
         "three_strips": (752, 130),
         "packed": (272, 64)}
PACK_IMAGES = 10  # images per packed wave at 272 px (64 lanes / (1 halo + 5 store lanes))
LAYER_IMAGE = (408, 96)  # scale space of one octave: layer 0 = 408 x 96 (two plain strips), layer 1 = 272 x 64 (packed)
LAYER = (272, 64)
RADIUS, THR, MAX_KPTS, MAX_CAND = 8.0, 60, 2500, 1 << 13
DISTINCT = 3
STRIP = 62  # dwords a strip advances by


def strips(w):
    nd = w // 4
    n = 1
    while (n - 1) * STRIP + 64 < nd:
        n += 1
    return n


def seams(w):
    """first column right of every hand-over: the strip seams, or on one strip the borders of its outer lanes"""
    n = strips(w)
    if n > 1:
        return [4 * (STRIP * k + 1) for k in range(1, n)]
    return [4, w - 4]


def planted(w, h):
    """[(kind, x, y)]: kind "dot" = one bright pixel at (x, y); "pair" = bright pixels at (x, y) and (x + 1, y)"""
    out = []
    for c in seams(w):
        out += [("dot", c - 1, 2), ("dot", c, h - 3), ("pair", c - 1, 12), ("dot", c, 42), ("dot", c - 1, 52)]
    out += [("dot", 1, 22), ("dot", w - 2, 22), ("dot", 2, 32), ("dot", w - 3, 32)]
    return out


@functools.lru_cache(maxsize=None)
def scene(name, seed):
    w, h = CASES[name]
    img = (synth.noise_image(w, h, 7 + seed) // 2 + 40).astype(np.uint8)
    for kind, x, y in planted(w, h):
        x1 = x + 1 if kind == "pair" else x
        img[max(y - 3, 0):y + 4, max(x - 3, 0):x1 + 4] = 10
        img[y, x:x1 + 1] = 255
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def reference(name, seed):
    """(score map, candidates, kept keypoints) of scene(name, seed) by the oracle: computed once, never changed"""
    import oracle_lib as O
    img = scene(name, seed)
    score = O.harris_score(img)
    cand = O.nms(score, THR)
    kps = O.detect(img, RADIUS, 0, THR, MAX_KPTS)
    for a in (score, cand, kps):
        a.setflags(write=False)
    return score, cand, kps


def batch_for_tile_61(name):
    """images a call needs so that the library picks 61-row tiles (k_harris.hip: more than 128 blocks of four waves)"""
    w, h = CASES[name]
    return 512 // (strips(w) * ((h + 60) // 61)) + 1


@functools.lru_cache(maxsize=None)
def layer_scene(seed):
    """jittered cells of ten pixels: structure that survives the 2/3 sampling"""
    img = synth.corners_image(LAYER_IMAGE[0], LAYER_IMAGE[1], 60 + seed, cell=10)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def layer_reference(seed):
    """keypoints of layer_scene(seed) through a scale space of one octave, by the oracle"""
    import oracle_lib as O
    k = O.detect(layer_scene(seed), RADIUS, 1, THR, MAX_KPTS)
    k.setflags(write=False)
    return k
