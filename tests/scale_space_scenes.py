"""Scenes for the cross-layer stage of the scale-space detector (octaves > 0), and the detector configurations they run
under.  Every scene is a small uint8 image with the octave count it is run at; tests/test_scale_space_scenes_host.py
asserts, on the census of tests/scale_space_ref.py, what the scenes reach, and tests/test_gpu_scale_space_census.py runs
them on the device.

Sizes: four octaves need a top layer of 16 x 16, i.e. an image of 192 x 192 at least; okvfe_create takes no image side
below 64.  The sizes cover w % 3 and h % 3 in
{0, 1, 2}, odd and even layer-1 / layer-2 sizes, and layer widths that are and are not multiples of 4 (the layers then
take different score / NMS kernels)."""
import numpy as np

import oracle_lib as O

MAX_KPTS = 80
# name -> (uniformity radius, absolute threshold, score type)
CONFIGS = {
    "harris": (5.0, 30, O.SCORE_HARRIS),
    "agast": (5.0, 15, O.SCORE_AGAST),
    "brisk": (0.0, 15, O.SCORE_BRISK_SCALESPACE),
}


def _noise(w, h, seed, amp):
    return np.random.default_rng(seed).integers(-amp, amp + 1, size=(h, w))


def multiscale_checker(w, h, seed, amp=6):
    """horizontal bands of checker cells 5 / 9 / 17 / 33 / 65 px, levels 40 / 210, +-amp noise: every layer of four
    octaves finds cells of its own size"""
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w), dtype=np.int64)
    cells = (5, 9, 17, 33, 65)
    edges = np.linspace(0, h, len(cells) + 1).astype(int)
    for cell, y0, y1 in zip(cells, edges[:-1], edges[1:]):
        band = np.where(((xx // cell) + (yy // cell)) % 2 == 0, 40, 210)
        img[y0:y1] = band[y0:y1]
    return np.clip(img + _noise(w, h, seed, amp), 0, 255).astype(np.uint8)


def squares(w, h, pitch=48, lo=60, hi=200):
    """exact two-level pattern without noise: bright squares of `pitch` px on a grid of 2 * pitch.  With pitch = 48 all
    their edges sit on multiples of 3 * 2^4, so every sampler reproduces the two levels exactly in all eight layers: the
    corners score the same in every layer (ties across layers: sb == s == sa) and among themselves (ties across the cut)"""
    yy, xx = np.mgrid[0:h, 0:w]
    on = ((xx // pitch) % 2 == 1) & ((yy // pitch) % 2 == 1)
    return np.where(on, hi, lo).astype(np.uint8)


def small_squares(w, h):
    """the same two-level idea at pitch 12 (exact in layers 0 .. 3) -- many equal corners per layer"""
    return squares(w, h, pitch=12, lo=50, hi=220)


def rim(w, h, seed):
    """noise with two-level structure two pixels inside all four rims: maxima in the last columns / rows that the
    NMS admits, whose windows in the layer above are clipped at its right / bottom border"""
    img = np.random.default_rng(seed).integers(0, 256, size=(h, w)).astype(np.uint8)
    img[2:4, :] = np.where((np.arange(w) // 3) % 2 == 0, 250, 5)
    img[-4:-2, :] = img[2:4, :]
    img[:, 2:4] = np.where((np.arange(h) // 3) % 2 == 0, 250, 5)[:, None]
    img[:, -4:-2] = img[:, 2:4]
    return img


def rim_blocks(w, h, seed):
    """coarse blocks of random level that run into the right and bottom rims: the UPPER layers also get maxima in their
    last admitted columns / rows"""
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w), dtype=np.uint8)
    for cell in (7, 13, 25):
        lv = rng.integers(0, 256, size=(h // cell + 1, w // cell + 1)).astype(np.uint8)
        blk = np.kron(lv, np.ones((cell, cell), dtype=np.uint8))[:h, :w]
        # anchor the block grid at the bottom-right corner
        blk = blk[::-1, ::-1]
        y0 = {7: 0, 13: h // 3, 25: 2 * h // 3}[cell]
        y1 = {7: h // 3, 13: 2 * h // 3, 25: h}[cell]
        img[y0:y1] = blk[y0:y1]
    return img


def flat(w, h):
    return np.full((h, w), 128, dtype=np.uint8)


def dots(w, h, seed, contrast=50):
    """single pixels of low contrast on a flat background, on columns / rows that are 0 or 2 modulo 3: two-thirds sampling
    keeps 4/9 of the contrast there and half sampling 1/4, so layers 0 and 1 have candidates and no layer above has any"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 60, dtype=np.uint8)
    for y in range(9, h - 9, 9):
        for x in range(9, w - 9, 9):
            img[y + 2 * int(rng.integers(0, 2)), x + 2 * int(rng.integers(0, 2))] = 60 + contrast
    return img


def blobs(w, h, period=16, amplitude=20):
    """a smooth egg-crate pattern: too gentle for layer 0 to score above the thresholds of CONFIGS, strong once it is
    sampled down -- the upper layers have thousands of 2-D maxima and layer 0 has none"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.round(128 + amplitude * np.sin(2 * np.pi * xx / period) * np.sin(2 * np.pi * yy / period)).astype(np.uint8)


def squares_over_blobs(w, h):
    """squares() in the upper half, blobs() in the lower: layer 0 has the few corners of the squares, the layers above
    it also the thousands of maxima of the blobs"""
    img = blobs(w, h)
    img[:h // 2] = squares(w, h)[:h // 2]
    return img


# (name, image, octaves)
def _build():
    s = []
    s.append(("checker-400x392", multiscale_checker(400, 392, 1), 4))
    s.append(("checker-394x389", multiscale_checker(394, 389, 2), 4))
    s.append(("checker-296x293", multiscale_checker(296, 293, 3), 4))
    s.append(("squares-400x392", squares(400, 392), 4))
    s.append(("squares-296x293", squares(296, 293), 4))
    s.append(("rim-394x389", rim(394, 389, 4), 4))
    s.append(("rimblocks-200x196", rim_blocks(200, 196, 5), 4))
    s.append(("rimblocks-296x293", rim_blocks(296, 293, 6), 4))
    s.append(("flat-400x392", flat(400, 392), 4))
    s.append(("dots-400x392", dots(400, 392, 7), 4))
    s.append(("smallsquares-200x196", small_squares(200, 196), 4))
    s.append(("rim-296x293", rim(296, 293, 11), 4))
    s.append(("rim-200x196", rim(200, 196, 12), 4))
    s.append(("smallsquares-296x293", small_squares(296, 293), 4))
    s.append(("squares24-400x392", squares(400, 392, pitch=24, lo=30, hi=180), 4))
    s.append(("blobs-400x392", blobs(400, 392), 4))
    s.append(("rim-127x101", rim(127, 101, 8), 2))
    s.append(("smallsquares-100x64", small_squares(100, 64), 2))
    s.append(("checker-96x72", multiscale_checker(96, 72, 9), 2))
    s.append(("rim-65x68", rim(65, 68, 10), 1))
    return s


_SCENES = None


def scenes():
    global _SCENES
    if _SCENES is None:
        _SCENES = _build()
    return _SCENES


def scene(name):
    for n, img, octaves in scenes():
        if n == name:
            return img, octaves
    raise KeyError(name)


def octave_counts(w, h):
    """the octave counts 1 .. 4 whose top layer is at least 16 x 16"""
    return [o for o in (1, 2, 3, 4) if min(O.layer_size(w, h, 2 * o - 1)) >= 16]


def sizes():
    """(w, h, octaves) of the scenes, in order of first appearance"""
    out = []
    for _, img, octaves in scenes():
        key = (img.shape[1], img.shape[0], octaves)
        if key not in out:
            out.append(key)
    return out


def batch_for(w, h, octaves):
    """the scenes of one size with the flat and the "layers 0-1 only" image of that size, in batches of 5 for the
    device-resident call: [(name, image)] * 5 per batch, every batch holding both special images"""
    own = [(n, img) for n, img, o in scenes() if img.shape == (h, w) and o == octaves and not n.startswith(("flat", "dots"))]
    special = [("flat-%dx%d" % (w, h), flat(w, h)), ("dots-%dx%d" % (w, h), dots(w, h, 7))]
    batches = []
    for i in range(0, len(own), 3):
        part = own[i:i + 3]
        while len(part) < 3:
            part.append(own[0])
        batches.append([part[0], special[0], part[1], special[1], part[2]])
    return batches
