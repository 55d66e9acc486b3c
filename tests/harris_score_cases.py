"""Scenes, census and references shared by tests/test_harris_score_cases_host.py and tests/test_gpu_harris_score_arith.py:
images that drive the score arithmetic of harris_kernel (csrc/k_harris.hip, score_row) to the ends of its ranges.

Per pixel the kernel holds A = smoothed gx^2 >> 14, B = smoothed gy^2 >> 14 (both 0 .. 16256, packed A | B << 16) and
C = smoothed gx gy >> 14 (-16256 .. 16256) and computes

    tq = ((A >> 1) + (B >> 1)) >> 1         as  v_sad_u16(AB & 0xFFFEFFFE, 0, 0) >> 2
    score = A B - C^2 - tq^2                with 24-bit multiplies (a form on v_dot2_i32_i16 with C << 16 | tq as operand
                                            was measured and not kept: LAB_NOTES.md "K1: score on SAD and dot2")

What can go wrong: the parity of A and B (the mask exists for A and B both odd with (A + B) % 4 == 0, where (A + B) >> 2
is one too large), the sign and the size of C (the upper i16 of the dot product's operand in the measured form), A B near
its upper end,
and the columns next to the rim, whose A, B and C sum a zero column.  The census below counts, per scene, the pixels of
each such class from the definition in numpy; FLOORS records what the scenes together must reach, per shape.

Scenes (every one reaches all four image borders, so the rim-adjacent columns see the same content):
0/255 step edges, vertical, horizontal and both diagonals (both signs of C); stripes and checkers of 1, 2 and 3 px;
half-amplitude noise; one flat image (all-zero scores: ties everywhere, no candidate)."""
import functools

import numpy as np

import harris_seam_cases as S

#         name          w    h     the shapes of tests/harris_seam_cases.py
SHAPES = {"full_strip": S.CASES["full_strip"],   # 256 x 66: one strip
          "two_strips": S.CASES["two_strips"],   # 504 x 64
          "packed": S.CASES["packed"]}           # 272 x 64: a packed last strip
RADIUS, THR, MAX_KPTS = S.RADIUS, S.THR, S.MAX_KPTS


def _edge_v(w, h):
    img = np.zeros((h, w), np.uint8)
    img[:, w // 2 + 1:] = 255
    return img


def _edge_h(w, h):
    img = np.zeros((h, w), np.uint8)
    img[h // 2 + 1:, :] = 255
    return img


def _diag(w, h, sign):
    y, x = np.mgrid[0:h, 0:w]
    # a saw of diagonal 0/255 edges, period 24 px, so that both rim columns are crossed at several rows
    return np.where(((x + sign * y) % 24) < 12, 255, 0).astype(np.uint8)


def _stripes(w, h, k):
    x = np.arange(w)
    return np.repeat((((x // k) & 1) * 255).astype(np.uint8)[None, :], h, axis=0)


def _checker(w, h, k):
    y, x = np.mgrid[0:h, 0:w]
    return ((((x // k) + (y // k)) & 1) * 255).astype(np.uint8)


def _noise(w, h):
    rng = np.random.default_rng(20 + w)
    return (rng.integers(0, 256, size=(h, w)) // 2 + 64).astype(np.uint8)


def _flat(w, h):
    return np.full((h, w), 128, np.uint8)


SCENES = {"edge_v": _edge_v, "edge_h": _edge_h,
          "diag_pos": lambda w, h: _diag(w, h, 1), "diag_neg": lambda w, h: _diag(w, h, -1),
          "stripes_1": lambda w, h: _stripes(w, h, 1), "stripes_2": lambda w, h: _stripes(w, h, 2),
          "stripes_3": lambda w, h: _stripes(w, h, 3),
          "checker_1": lambda w, h: _checker(w, h, 1), "checker_2": lambda w, h: _checker(w, h, 2),
          "checker_3": lambda w, h: _checker(w, h, 3),
          "noise_half": _noise, "flat": _flat}
NAMES = sorted(SCENES)


@functools.lru_cache(maxsize=None)
def scene(shape, name):
    w, h = SHAPES[shape]
    img = np.ascontiguousarray(SCENES[name](w, h))
    assert img.shape == (h, w) and img.dtype == np.uint8
    img.setflags(write=False)
    return img


def abc(img):
    """A, B, C of every pixel from the definition (int64, floor shifts; rim entries zero)"""
    p = img.astype(np.int64)
    h, w = p.shape
    gx = np.zeros((h, w), np.int64)
    gy = np.zeros((h, w), np.int64)
    gx[1:-1, 1:-1] = (3 * (p[:-2, 2:] - p[:-2, :-2]) + 10 * (p[1:-1, 2:] - p[1:-1, :-2]) + 3 * (p[2:, 2:] - p[2:, :-2]))
    gy[1:-1, 1:-1] = (3 * (p[2:, :-2] - p[:-2, :-2]) + 10 * (p[2:, 1:-1] - p[:-2, 1:-1]) + 3 * (p[2:, 2:] - p[:-2, 2:]))
    out = []
    for e in ((gx * gx) >> 14, (gy * gy) >> 14, (gx * gy) >> 14):
        s = np.zeros_like(e)
        for dy, ky in enumerate((1, 2, 1)):
            for dx, kx in enumerate((1, 2, 1)):
                s[1:-1, 1:-1] += ky * kx * e[dy:h - 2 + dy, dx:w - 2 + dx]
        out.append(s)
    return out


def score_from_abc(A, B, Cc):
    tq = ((A >> 1) + (B >> 1)) >> 1
    sc = A * B - Cc * Cc - tq * tq
    sc[0, :] = sc[-1, :] = 0
    sc[:, 0] = sc[:, -1] = 0
    return sc


CLASSES = ("parity_00", "parity_01", "parity_10", "parity_11", "odd_odd_sum_mod4_0", "C_ge_2p12", "C_le_m2p12",
           "AB_ge_2p25", "score_neg", "score_pos")


def census(img):
    """{class: (pixels inside the rim, of them in the rim-adjacent columns 1 and w - 2)}"""
    A, B, Cc = abc(img)
    sc = score_from_abc(A, B, Cc)
    inner = np.zeros(img.shape, bool)
    inner[1:-1, 1:-1] = True
    rimcol = np.zeros(img.shape, bool)
    rimcol[1:-1, 1] = rimcol[1:-1, -2] = True
    pa, pb = A & 1, B & 1
    masks = {"parity_00": (pa == 0) & (pb == 0), "parity_01": (pa == 0) & (pb == 1),
             "parity_10": (pa == 1) & (pb == 0), "parity_11": (pa == 1) & (pb == 1),
             "odd_odd_sum_mod4_0": (pa == 1) & (pb == 1) & ((A + B) % 4 == 0),
             "C_ge_2p12": Cc >= 1 << 12, "C_le_m2p12": Cc <= -(1 << 12),
             "AB_ge_2p25": A * B >= 1 << 25, "score_neg": sc < 0, "score_pos": sc > 0}
    return {k: (int((m & inner).sum()), int((m & rimcol).sum())) for k, m in masks.items()}


@functools.lru_cache(maxsize=None)
def census_of_shape(shape):
    """the scenes of one shape together: {class: (pixels, pixels in columns 1 and w - 2)}"""
    tot = {k: [0, 0] for k in CLASSES}
    for name in NAMES:
        for k, (a, b) in census(scene(shape, name)).items():
            tot[k][0] += a
            tot[k][1] += b
    return {k: tuple(v) for k, v in tot.items()}


# The sizes.  The registers allow |C| <= 16256 and A B <= 16256^2, but no image gets there: gx and gy of a pixel are
# taken from the same 3 x 3 pixels and |gx| + |gy| <= (6 + 20) * 255 = 6630 (the corner taps of the two filters cancel
# in pairs), so |gx gy| >> 14 <= 670 and |C| <= 10720, and with s = |gx| / 6630 in [0.385, 0.615] (|g| <= 4080)
# A B <= (16 * 2683)^2 * max E[s^2] E[(1 - s)^2] = 1.28e8 < 2^27.  Over ALL 2^25 patches of 5 x 5 pixels of 0 / 255 the
# centre pixel reaches |C| = 7417 and A B = 6.94e7 (exhaustive search); the diagonal edges here reach |C| = 6875 and
# A B = 4.7e7.  So the classes of size are |C| >= 2^12 (both signs) and
# A B >= 2^25; the reaches above them -- C to +-16256, A B >= 2^27 -- exist in the arithmetic only, and the host test
# checks them there (a numpy restatement of the kernel's operations against the definition, over the register ranges).
#
# What the scenes of a shape together must contain, (anywhere inside the rim, in columns 1 and w - 2): half of the
# census of the scenes as they were written (census_of_shape), rounded down -- the noise scene is the only one that
# depends on a generator.
FLOORS = {
    "full_strip": {"parity_00": (86026, 677),
                   "parity_01": (1999, 16),
                   "parity_10": (2064, 17),
                   "parity_11": (7446, 57),
                   "odd_odd_sum_mod4_0": (1032, 6),
                   "C_ge_2p12": (1354, 10),
                   "C_le_m2p12": (1356, 12),
                   "AB_ge_2p25": (17441, 11),
                   "score_neg": (27862, 209),
                   "score_pos": (24198, 188)},
    "two_strips": {"parity_00": (164728, 655),
                   "parity_01": (3967, 15),
                   "parity_10": (3807, 18),
                   "parity_11": (14242, 55),
                   "odd_odd_sum_mod4_0": (1925, 7),
                   "C_ge_2p12": (2593, 11),
                   "C_le_m2p12": (2593, 11),
                   "AB_ge_2p25": (33432, 10),
                   "score_neg": (53252, 208),
                   "score_pos": (46338, 177)},
    "packed": {"parity_00": (88614, 657),
                   "parity_01": (2138, 13),
                   "parity_10": (2071, 15),
                   "parity_11": (7616, 58),
                   "odd_odd_sum_mod4_0": (1042, 8),
                   "C_ge_2p12": (1394, 10),
                   "C_le_m2p12": (1395, 11),
                   "AB_ge_2p25": (17924, 10),
                   "score_neg": (28677, 205),
                   "score_pos": (24939, 179)},
}


@functools.lru_cache(maxsize=None)
def reference(shape, name):
    """(score map, candidates, kept keypoints) of a scene by the oracle: computed once, never changed"""
    import oracle_lib as O
    img = scene(shape, name)
    score = O.harris_score(img)
    cand = O.nms(score, THR)
    kps = O.detect(img, RADIUS, 0, THR, MAX_KPTS)
    for a in (score, cand, kps):
        a.setflags(write=False)
    return score, cand, kps


def batch_for_tile_61(shape):
    """images a call needs so that the library picks 61-row tiles"""
    return S.batch_for_tile_61(shape)
