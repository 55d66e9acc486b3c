"""Shapes, scenes and references shared by tests/test_unaligned_cases_host.py and tests/test_gpu_unaligned_chain.py
(tests/test_gpu_unaligned_fuzz.py draws its own): images whose WIDTH is not a multiple of 4, or whose device pointer is
not dword aligned.  Such a call never sees the fused score + NMS kernel, the map-free selection, describe_aware_kernel,
describe_rot_kernel or the buffer_load ... lds patch staging; it runs the dense fallback chain instead:

    harris_generic_kernel<false>   (csrc/k_harris.hip)  byte loads, clamped columns, per-column store guards
    nms_generic_kernel             (csrc/k_nms.hip)     needs w % 4 != 0 (or a score pointer off 16 bytes); a pointer
                                                        offset at an aligned width takes nms_kernel on the dense map
    launch_sort                                         where the selection form does not order its candidates itself
    the selection forms on ScoreLayout{w, 0}, refine_emit reading the map
    describe_kernel<4, generic>    (csrc/k_describe.hip) routes kAllModes / kWideBoxes, byte-wise stage_patch
    compact_kernel

Widths (the smallest at which each piece of the generic kernels' index arithmetic differs): one lane = 4 pixels, one
x-block = 64 lanes = 256 pixels.

    65, 66, 67             one x-block, the last lane holds 1, 2, 3 columns
    253, 254, 255          the last lane group of block 0 is partial: nms_generic_kernel settles equal neighbours of
                           block 0 in registers (raster_accept_wave)
    257, 258, 259, 261     block 1 holds one lane with 1, 2, 3 columns, or two lanes (4 + 1); for w % 4 == 3 the column
                           x = w - 3, the only candidate column inside a partial quad, lies at x >= 256
    513, 515               a third x-block

Heights lie on both sides of the row tilings: nms_generic_kernel walks K_GEN_ITERS * 4 = 32 rows per block,
harris_generic_kernel K_TH = 32 rows per wave and K_TH * K_WAVES_PER_BLOCK = 128 per block (64 .. 67, 95, 97, 127, 129).
65 x 65, 66 x 65 and 67 x 65 have w * h % 4 = 1, 2, 3: in a batch of nine every image starts at another residue.

Selection forms (lazy_plan, csrc/k_select.hip, asked through the lab build's okvfe_lab_select_plan): array bins at
radius 10 (12 at 1032 px), linked lists at radius 2, and the grid kernels where neither fits the LDS -- at these sizes
that takes a radius of 0.3 .. 1.25 pixels (GRID_RADIUS: the largest of 0.3, 0.4, 0.5, 0.6, 0.75, 1, 1.25 that reaches
them at 300 keypoints), i.e. an occupancy grid of some 10 MB per image.  All three forms are reached at every shape.

No plateau scenes: Harris maps of doubled pixels, blocks and checkerboards carry no horizontally adjacent equal scores
>= 1 at these sizes, so the raster tie rule across x = 255|256 is exercised on the AGAST score (agast_tie_scene).

    python tests/unaligned_cases.py        the census
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:  # (run as a script: the package lives one level up)
    sys.path.insert(0, _ROOT)

import oracle_lib as O
from okvis2_amd import synth

# csrc/k_harris.hip (kTH, kWavesPerBlock) and csrc/k_nms.hip (kGenIters); test_unaligned_cases_host.py reads them back
K_TH, K_WAVES_PER_BLOCK, K_GEN_ITERS = 32, 4, 8
HARRIS_BLOCK_ROWS = K_TH * K_WAVES_PER_BLOCK
NMS_BLOCK_ROWS = 4 * K_GEN_ITERS
X_BLOCK = 256  # pixels per x-block of both generic kernels

WIDTH_CLASSES = {"one_block": (65, 66, 67), "partial_block0": (253, 254, 255), "block1": (257, 258, 259, 261),
                 "three_blocks": (513, 515)}
ODD_SHAPES = ((65, 65), (66, 65), (67, 65), (253, 64), (254, 66), (255, 67), (257, 95), (258, 97), (259, 67),
              (261, 127), (513, 129), (515, 97))
RESIDUE_SHAPES = ((65, 65), (66, 65), (67, 65))  # w * h % 4 = 1, 2, 3
MODE_SHAPES = ((255, 95), (259, 97))             # every extraction mode; the second has keypoints at x >= 256
HEIGHTS = tuple(sorted({h for _, h in ODD_SHAPES}))
BATCH = 9
FLAT = 3  # index of the flat image of a batch

FORMS = ("array", "list", "grid")
GRID_RADIUS = {(65, 65): 0.3, (66, 65): 0.3, (67, 65): 0.3, (253, 64): 0.6, (254, 66): 0.6, (255, 67): 0.6,
               (257, 95): 0.75, (258, 97): 0.75, (259, 67): 0.6, (261, 127): 0.75, (513, 129): 1.25, (515, 97): 1.0}
MAX_KPTS = 300
THRESHOLDS = (1, 3000000)  # every maximum of the map / about a sixth of them on noise
MAX_CAND = 1 << 13         # above the densest image's count (test_unaligned_cases_host.py)

# aligned widths for the pointer-offset cases: (w, h, form) -- one strip, two strips, harris_tile_cases.PACKED (the
# last strips share a wave), and a shape under the linked-list selection
ALIGNED_CASES = ((256, 64, "array"), (260, 121, "array"), (1032, 68, "array"), (264, 66, "list"))
ALIGNED_CAMERA = "equidistant"  # its aligned calls take kAwareBatched, the production route
SCORE_WIDTHS = ((256, 64), (259, 67))  # okvfe_harris_score_device at image and score pointer offsets

# the overflow case: fewer candidate slots than the oracle counts maxima
CAPACITY_CASE = dict(w=259, h=67, form="array", thr=1, max_candidates=256)

# scale space: (w, h, octaves); layer widths by layer_size's rule cover w % 4 = 1, 2, 3 (and one aligned layer)
SCALE_SPACE = ((519, 139, 2), (517, 140, 1))
SCALE_SPACE_PARAMS = dict(radius=12.0, thr=100000, max_kpts=200, agast_thr=20)


def form_params(form, w, h):
    """(uniformity radius, max keypoints) that make a w x h context take selection form `form`"""
    if form == "array":
        return (12.0 if w > 1024 else 10.0), MAX_KPTS
    if form == "list":
        return 2.0, MAX_KPTS
    return GRID_RADIUS[(w, h)], MAX_KPTS


def frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def rim_image(w, h, seed):
    """noise with period-3 bars two pixels inside each rim (the content of
    test_keypoints_on_the_image_rim_without_a_score_map): maxima on columns 2, 3, w - 4, w - 3 and the same rows"""
    img = synth.noise_image(w, h, seed).copy()
    img[2:4, :] = np.where((np.arange(w) // 3) % 2 == 0, 250, 5)
    img[-4:-2, :] = img[2:4, :]
    img[:, 2:4] = np.where((np.arange(h) // 3) % 2 == 0, 250, 5)[:, None]
    img[:, -4:-2] = img[:, 2:4]
    return img


@functools.lru_cache(maxsize=None)
def batch(w, h):
    """nine images [9, h, w]: noise, rim structure and jittered cells in turn, image FLAT without any structure"""
    s = 1000 + 7 * w + 13 * h
    imgs = [synth.noise_image(w, h, s), rim_image(w, h, s + 1), synth.corners_image(w, h, s + 2, cell=12),
            np.full((h, w), 77, np.uint8), synth.noise_image(w, h, s + 4), rim_image(w, h, s + 5),
            synth.corners_image(w, h, s + 6, cell=8), synth.noise_image(w, h, s + 7), rim_image(w, h, s + 8)]
    return frozen(np.stack(imgs).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def score_reference(w, h):
    """oracle.harris_score of every image of batch(w, h)"""
    return frozen(np.stack([O.harris_score(img) for img in batch(w, h)]))


@functools.lru_cache(maxsize=None)
def candidates(w, h, thr):
    return tuple(frozen(O.nms(np.ascontiguousarray(sc), thr)) for sc in score_reference(w, h))


@functools.lru_cache(maxsize=None)
def detect_reference(w, h, radius, thr, max_kpts):
    return tuple(frozen(O.detect(img, radius, 0, thr, max_kpts)) for img in batch(w, h))


# ---- extraction modes ----------------------------------------------------------------------------------------------
MODES = ("upright", "gradient", "scale_invariant", "radtan", "equidistant", "radtan8")
GRAVITY = (0.12, 0.98, -0.09)


def camera(w, h, model):
    """a distorted pinhole camera for an image of any size (built like camera_for of select_keys_cases.py); the RADTAN8
    coefficients are those of the reference's test object at its field of view (synth.radtan8_config)"""
    if model == "radtan":
        return synth.Camera(w, h, 0.62 * w, 0.63 * w, w / 2 - 0.7, h / 2 + 0.4, 1, (-0.05, 0.004, 0.0002, -0.0001))
    if model == "equidistant":
        return synth.Camera(w, h, 0.55 * w, 0.56 * w, w / 2 + 1.3, h / 2 - 0.6, 2, (-0.01, 0.015, -0.004, 0.001))
    if model == "radtan8":
        f = 350.0 / 752.0 * w
        return synth.Camera(w, h, f, f * 360.0 / 350.0, w / 2 + 0.9, h / 2 - 1.1, 3,
                            (0.6261, 0.001, -0.0002, 0.0001, 0.0001, 0.9541, 0.1151, -0.0075))
    raise KeyError(model)


@functools.lru_cache(maxsize=None)
def camera_maps(w, h, model):
    cam = camera(w, h, model)
    if model == "radtan8":
        import radtan8_ref as R8
        rays, jac = R8.awareness_maps(cam)
    else:
        rays, jac = O.awareness_maps(cam)
    return frozen(rays), frozen(jac)


def backproject(w, h, model, kps):
    cam = camera(w, h, model)
    if model == "radtan8":
        import radtan8_ref as R8
        return R8.backproject_keypoints(cam, kps)
    return O.backproject_keypoints(cam, kps)


def frontend_kwargs(mode):
    """capi.Frontend arguments of an extraction mode"""
    return dict(rotation_invariant=(mode != "upright"), scale_invariant=(mode == "scale_invariant"))


@functools.lru_cache(maxsize=None)
def describe_reference(w, h, radius, thr, max_kpts, mode):
    """per image of batch(w, h): (keypoints, descriptors, back-projections or None, validity or None) by the oracle"""
    out = []
    for img, kps in zip(batch(w, h), detect_reference(w, h, radius, thr, max_kpts)):
        if mode in ("radtan", "equidistant", "radtan8"):
            rays, jac = camera_maps(w, h, mode)
            k, d = O.describe(img, kps, O.MODE_CAMERA_AWARE, rays, jac, np.float32(camera(w, h, mode).fu), GRAVITY)
            bp, bv = backproject(w, h, mode, k)
            out.append((frozen(k), frozen(d), frozen(bp), frozen(bv)))
        else:
            omode = O.MODE_UPRIGHT if mode == "upright" else O.MODE_GRADIENT
            k, d = O.describe(img, kps, omode, scale_invariant=(mode == "scale_invariant"))
            out.append((frozen(k), frozen(d), None, None))
    return tuple(out)


# ---- the AGAST tie scene (raster rule across x = 255|256) ----------------------------------------------------------
AGAST_TIE_WIDTHS = (259, 261, 333)
AGAST_TIE_HEIGHT, AGAST_TIE_THR = 136, 20
AGAST_TIE_RADIUS, AGAST_TIE_MAX_KPTS = 0.75, 4096  # accepted pixels of a run lie two apart: every candidate is kept


@functools.lru_cache(maxsize=None)
def agast_tie_scene(w):
    """Bright horizontal dashes of 2, 3 and 4 pixels on a dark ground, four rows apart.  No dash pixel lies on the
    radius-3 ring of another, so all pixels of a dash score the same (the 16 ring pixels are darker by the same amount):
    a run of equal maxima, of which the raster scan keeps every second one starting with the leftmost.  One dash per
    row crosses x = 255|256 (nms_generic_kernel settles x < 256 in registers and walks memory beyond), the others start
    at x >= 256 where the width leaves room, and fill block 0.  The AGAST score is zero within three pixels of the rim,
    so the last passing column is w - 4: at w = 259 that is x = 255, the last pixel the register path owns (the runs end
    there and block 1 has none), at w = 261 the crossing runs end at x = 257 in the second lane of block 1."""
    h = AGAST_TIE_HEIGHT
    img = np.full((h, w), 20, np.uint8)
    for k, y in enumerate(range(4, h - 3, 4)):
        length = 2 + k % 3
        start = 255 - (k // 3) % (length - 1) if w > 264 else w - 3 - length
        img[y, start:start + length] = 180 + k
        x = start + length + 7
        j = k
        while x + 4 < w - 2:
            length = 2 + j % 3
            img[y, x:x + length] = 150 + (j % 50)
            x += length + 7 + j % 2
            j += 1
        x = start - 9
        while x - 4 >= 2:
            length = 2 + j % 3
            img[y, x - length + 1:x + 1] = 150 + (j % 50)
            x -= length + 7 + j % 2
            j += 1
    return frozen(img)


def passing_mask(score, thr):
    """numpy restatement of passes() (csrc/k_nms.hip): >= thr, no strictly greater neighbour, 2 <= x < w - 2 and
    2 <= y < h - 2.  Coverage claim only: no result is compared through it."""
    h, w = score.shape
    s = score.astype(np.int64)
    p = s >= thr
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                nb = np.full_like(s, np.iinfo(np.int64).min)
                ys, yd = slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0))
                xs, xd = slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0))
                nb[yd, xd] = s[ys, xs]
                p &= ~(nb > s)
    p[:2] = p[-2:] = False
    p[:, :2] = p[:, -2:] = False
    return p


def tie_run_census(score, thr):
    """horizontal runs of two or more passing pixels: {"crossing_255_256", "starting_at_256_or_beyond", "length_3_or_more"}"""
    p = passing_mask(score, thr)
    out = dict(crossing_255_256=0, starting_at_256_or_beyond=0, length_3_or_more=0, runs=0)
    for row in p:
        x = 0
        w = len(row)
        while x < w:
            if not row[x]:
                x += 1
                continue
            e = x
            while e + 1 < w and row[e + 1]:
                e += 1
            if e > x:
                out["runs"] += 1
                out["crossing_255_256"] += int(x <= 255 and e >= 256)
                out["starting_at_256_or_beyond"] += int(x >= 256)
                out["length_3_or_more"] += int(e - x + 1 >= 3)
            x = e + 1
    return out


@functools.lru_cache(maxsize=None)
def agast_tie_reference(w):
    """(score map, NMS candidates, keypoints kept at a radius that suppresses nothing) by the oracle"""
    img = agast_tie_scene(w)
    score = O.agast_score(img)
    cand = O.nms(score, AGAST_TIE_THR)
    kps = O.detect(img, AGAST_TIE_RADIUS, 0, AGAST_TIE_THR, AGAST_TIE_MAX_KPTS, score_type=O.SCORE_AGAST)
    return frozen(score), frozen(cand), frozen(kps)


# ---- census (from the oracle alone) --------------------------------------------------------------------------------
CENSUS_FLOOR = 16


def kept_rounded(kps):
    return np.floor(kps["x"] + 0.5).astype(np.int64), np.floor(kps["y"] + 0.5).astype(np.int64)


def census():
    """counts over every odd-width scene of the module: where the oracle's candidates (threshold 1) and kept keypoints
    (every form, both thresholds) lie relative to the generic kernels' index arithmetic"""
    c = dict(col_2=0, col_w_minus_3=0, row_2=0, row_h_minus_3=0, col_w_minus_3_in_partial_quad=0, x_ge_256=0, x_ge_512=0,
             nms_block_first_row=0, nms_block_last_row=0, nms_partial_block_first_row=0, nms_partial_block_last_row=0,
             harris_wave_first_row=0, harris_wave_last_row=0, kept_within_3_of_rim=0, dropped_at_right_rim=0,
             dropped_at_bottom_rim=0)
    border = O.pattern().border
    for w, h in ODD_SHAPES:
        last_block = ((h - 1) // NMS_BLOCK_ROWS) * NMS_BLOCK_ROWS
        for cand in candidates(w, h, THRESHOLDS[0]):
            x, y = cand["x"], cand["y"]
            c["col_2"] += int((x == 2).sum())
            c["col_w_minus_3"] += int((x == w - 3).sum())
            c["row_2"] += int((y == 2).sum())
            c["row_h_minus_3"] += int((y == h - 3).sum())
            if w % 4 == 3:
                c["col_w_minus_3_in_partial_quad"] += int((x == w - 3).sum())
            c["x_ge_256"] += int((x >= 256).sum())
            c["x_ge_512"] += int((x >= 512).sum())
            full = y < last_block
            c["nms_block_first_row"] += int((full & (y % NMS_BLOCK_ROWS == 0)).sum())
            c["nms_block_last_row"] += int((full & (y % NMS_BLOCK_ROWS == NMS_BLOCK_ROWS - 1)).sum())
            if h % NMS_BLOCK_ROWS:
                c["nms_partial_block_first_row"] += int((y == last_block).sum())
                c["nms_partial_block_last_row"] += int((~full & (y == h - 3)).sum())
            c["harris_wave_first_row"] += int(((y > 0) & (y % K_TH == 0)).sum())
            c["harris_wave_last_row"] += int((y % K_TH == K_TH - 1).sum())
        for form in FORMS:
            radius, maxk = form_params(form, w, h)
            for thr in THRESHOLDS:
                for img, kps in zip(batch(w, h), detect_reference(w, h, radius, thr, maxk)):
                    xs, ys = kept_rounded(kps)
                    c["kept_within_3_of_rim"] += int(((xs <= 3) | (xs >= w - 4) | (ys <= 3) | (ys >= h - 4)).sum())
                    if form == "array" and len(kps):
                        k, _ = O.describe(img, kps, O.MODE_GRADIENT)
                        gone = ~np.isin(kps["x"].view(np.uint32).astype(np.uint64) << 32 | kps["y"].view(np.uint32),
                                        k["x"].view(np.uint32).astype(np.uint64) << 32 | k["y"].view(np.uint32))
                        c["dropped_at_right_rim"] += int((gone & (kps["x"] >= w - border)).sum())
                        c["dropped_at_bottom_rim"] += int((gone & (kps["y"] >= h - border)).sum())
    return c


def stride_residues(w, h, n=BATCH):
    """residue mod 4 of the first byte of each image of a batch at an aligned base pointer"""
    return [(i * w * h) % 4 for i in range(n)]


if __name__ == "__main__":
    for k, v in census().items():
        print("%-34s %6d" % (k, v))
    for w, h in RESIDUE_SHAPES:
        print("stride residues %d x %d: %s" % (w, h, stride_residues(w, h)))
    for w in AGAST_TIE_WIDTHS:
        sc, cand, kps = agast_tie_reference(w)
        print("agast ties w = %d: %s, %d candidates, %d kept" % (w, tie_run_census(sc, AGAST_TIE_THR), len(cand), len(kps)))
    for w, h in ODD_SHAPES:
        print("%d x %d: candidates at threshold 1 / %d: %s / %s" % (
            w, h, THRESHOLDS[1], [len(c) for c in candidates(w, h, THRESHOLDS[0])],
            [len(c) for c in candidates(w, h, THRESHOLDS[1])]))
