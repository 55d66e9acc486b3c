"""Directed scenes for the descriptor kernels: flat content under hand-built camera maps.

Every other descriptor test takes its keypoints from the detector, on textured images, under the shipped camera
models.  Here the test dictates all three inputs of the extractor:

* CONTENT on which a box mean that is off by one unit flips bits.  A descriptor bit is value[i] > value[j] with values
  1024 x mean intensity; on noise 0.03 % of the short pairs lie within one unit of each other, on a flat 255 image
  84 %, on flat 128 98 %, on flat 250 with dark 3 x 3 dots 73 % (test_describe_scenes_host.py asserts the floors).
  There the integer truncations of the rim weights alone decide the bits.
* M PER PIXEL.  okvfe_set_camera_maps takes arbitrary ray / Jacobian maps.  With fu = 1, ray (0, 0, 1) and extraction
  direction (0, 1, 0) the set-up (describe_setup_dev.h, camera_aware_matrix) yields M = [[J0, J1], [J3, J4]] exactly;
  J2 / J5 do not enter M but do enter the per-camera statistics that pick the kernel (capi_context.cpp), so the ROUTE
  is steered through J2 on the every-8th-pixel grid without touching any M (`steer`).  A keypoint's M is stamped on
  the ONE pixel its position rounds to, (int)(kx + 0.5f): a ray lookup one pixel off reads the background identity.
* KEYPOINT POSITIONS: okvfe_compute takes arbitrary keypoints, so rims, float knife edges and binade crossings are
  hit on purpose.

CPU only and deterministic (numpy + the CPU oracle's pattern).  `census` restates the float32 geometry of
describe_setup_one; it is a coverage claim only -- no result is compared through it.

    python tests/describe_scenes.py        the census of every scene
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:  # (run as a script: the package lives one level up)
    sys.path.insert(0, _ROOT)

import oracle_lib as O
from okvis2_amd import synth

F = np.float32
W, H = 256, 128
CONTENTS = ("flat255", "flat128", "dots250", "dither", "noise")
DOT_LATTICE, DOT_VALUE = 40, 20


def nextafter(x, towards):
    return F(np.nextafter(F(x), F(towards)))


def content(name, w, h):
    """the image of a content family"""
    if name == "flat255":
        return np.full((h, w), 255, dtype=np.uint8)
    if name == "flat128":
        return np.full((h, w), 128, dtype=np.uint8)
    if name == "dots250":  # dark 3 x 3 dots on a 40 px lattice
        img = np.full((h, w), 250, dtype=np.uint8)
        for cy in range(DOT_LATTICE // 2, h - 1, DOT_LATTICE):
            for cx in range(DOT_LATTICE // 2, w - 1, DOT_LATTICE):
                img[cy - 1:cy + 2, cx - 1:cx + 2] = DOT_VALUE
        return img
    if name == "dither":  # 200 / 201, iid
        return (200 + np.random.default_rng(77).integers(0, 2, size=(h, w))).astype(np.uint8)
    if name == "noise":
        return synth.noise_image(w, h, 78)
    raise KeyError(name)


# ---- patterns ------------------------------------------------------------------------------------------------------
def _set_border(p):
    reach = max(math.hypot(float(p.px[i]), float(p.py[i])) + float(p.sigma_half[i]) for i in range(p.n_points))
    p.border = int(math.ceil(reach)) + 1


# half-widths installed through okvfe_set_pattern: sample index -> exact float value.  Samples 0 and 1 of the 66-point
# pattern are the ones beyond the 64 lanes ("extras", small-box class: at most 2.0 / 4.25), 2.. are first-pass samples
# (at most 4.75 / 9.75); below 0.5 the published code takes a bilinear point sample, so 0.5 is the smallest box.
PATTERN_TWEAKS = {
    "extra2.0": {0: 2.0, 1: 2.0},
    "edges_narrow": {0: 0.5, 2: 4.75, 3: 0.5},
    "edges_wide": {0: 4.25, 1: 4.25, 2: 9.75},
}
BOX_SCALES = {"box1.73": 1.73, "box2.3": 2.3}


def pattern(key="default"):
    """the oracle's pattern struct of a variant: "default", a box_scale of BOX_SCALES (what okvfe_config.box_scale
    installs: half-side in double x the float factor, rounded once; the border follows) or a tweak of PATTERN_TWEAKS
    (installed through okvfe_set_pattern; the border stays, border >= reach + 1 holds)"""
    p = O.Pattern()
    O.lib().orc_pattern_build(C.byref(p))  # (not O.pattern(): the tests replace that one with a variant)
    if key == "default":
        return p
    if key in BOX_SCALES:
        f = float(F(BOX_SCALES[key]))
        for i in range(p.n_points):
            p.sigma_half[i] = F(float(p.sigma_half[i]) * f)
        _set_border(p)
        return p
    for i, s in PATTERN_TWEAKS[key].items():
        p.sigma_half[i] = F(s)
    reach = max(F(math.hypot(float(p.px[i]), float(p.py[i]))) + F(p.sigma_half[i]) for i in range(p.n_points))
    assert float(p.border) >= reach + 1.0  # the rule of okvfe_set_pattern
    return p


def pattern_reach(p):
    """Pattern::reach (host_tables.cpp, pattern_reach)"""
    reach = max(math.sqrt(float(p.px[i]) * float(p.px[i]) + float(p.py[i]) * float(p.py[i])) + float(p.sigma_half[i])
                for i in range(p.n_points))
    return F(reach * 1.0001 + 1.0e-3)


def pattern_extent(p):
    """farthest |offset| + half-width of a sample (pixels a box may reach from the keypoint under |M| = 1)"""
    return max(math.hypot(float(p.px[i]), float(p.py[i])) + float(p.sigma_half[i]) for i in range(p.n_points))


# ---- scenes --------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Field:
    """camera maps + keypoints: everything of a scene but the image"""
    name: str
    w: int
    h: int
    rays: np.ndarray
    jac: np.ndarray
    fu: float
    gravity: tuple
    keypoints: np.ndarray
    pattern: str = "default"
    intent: list = None  # field_classes: what each stamp is there for


@dataclasses.dataclass
class Scene:
    name: str
    image: np.ndarray
    rays: np.ndarray
    jac: np.ndarray
    fu: float
    gravity: tuple
    keypoints: np.ndarray
    pattern: str   # key of `pattern`; "default" = no tweak
    route: str     # key of ROUTES the scene is built for
    content: str = ""
    field: Field = None  # the maps before steering: what every route of the pattern shares


SIZES = (7.2, 12.0, 17.4, 12.0, 20.0, 9.0, 26.0, 12.0)  # keypoint diameters: rungs 0 .. 23 of the scale ladder


def make_keypoints(xy):
    """records that must travel through unchanged: every field distinct per keypoint"""
    k = np.zeros(len(xy), dtype=O.KEYPOINT_DTYPE)
    for i, (x, y) in enumerate(xy):
        k[i] = (F(x), F(y), F(SIZES[i % len(SIZES)]), F(-1.0), F(0.5 * i + 1.0), i % 3, i)
    return k


class _Maps:
    def __init__(self, w, h, gravity=(0.0, 1.0, 0.0)):
        self.w, self.h, self.gravity = w, h, gravity
        self.rays = np.zeros((h, w, 3), dtype=F)
        self.rays[..., 2] = 1.0
        self.jac = np.zeros((h, w, 6), dtype=F)
        self.jac[..., 0] = 1.0
        self.jac[..., 4] = 1.0
        self.xy = []
        self.stamped = {}

    def pixel(self, kx, ky):
        return int(F(kx) + F(0.5)), int(F(ky) + F(0.5))

    def free(self, kx, ky):
        u, v = self.pixel(kx, ky)
        return (u % 8 or v % 8) and (u, v) not in self.stamped  # off the grid of the camera statistics

    def add(self, kx, ky, M=None, ray=None, J=None):
        """keypoint at (kx, ky); M (4 floats) is stamped on the pixel it rounds to (None: the background stays).
        ray (0, 1, 0): the pixel whose e_y falls through to the third candidate, M = [[J2, J0], [J5, J3]]"""
        u, v = self.pixel(kx, ky)
        plain = M is None and ray is None and J is None
        key = "plain" if plain else (None if M is None else tuple(np.asarray(M, dtype=F).tolist()), ray, J)
        assert plain or u % 8 or v % 8, (u, v)
        assert self.stamped.setdefault((u, v), key) == key, ("two Ms on one pixel", u, v)
        if ray is not None:
            self.rays[v, u] = ray
        if J is not None:
            self.jac[v, u] = J
        elif M is not None:
            m = np.asarray(M, dtype=F)
            if ray is not None and tuple(ray) == (0.0, 1.0, 0.0):
                self.jac[v, u] = (m[1], 0.0, m[0], m[3], 0.0, m[2])
            else:
                self.jac[v, u] = (m[0], m[1], 0.0, m[2], m[3], 0.0)
        self.xy.append((F(kx), F(ky)))

    def field(self, name, pat_key):
        return Field(name, self.w, self.h, self.rays, self.jac, 1.0, self.gravity, make_keypoints(self.xy), pat_key)


def similarity(s, theta):
    c, sn = math.cos(theta), math.sin(theta)
    return (F(s * c), F(-s * sn), F(s * sn), F(s * c))


def _spot(rng, m, lo_x, lo_y):
    """a free sub-pixel position at least (lo_x, lo_y) from the rims"""
    for _ in range(1000):
        kx = F(rng.uniform(lo_x, m.w - 1 - lo_x))
        ky = F(rng.uniform(lo_y, m.h - 1 - lo_y))
        if m.free(kx, ky):
            return kx, ky
    raise RuntimeError("no free pixel")


def field_similarity(pat_key, w=W, h=H, n=120, seed=1, gravity=(0.0, 1.0, 0.0), scales=(0.5, 1.6)):
    """random rotations x isotropic scales, every box inside the image"""
    p = pattern(pat_key)
    ext, rng = pattern_extent(p), np.random.default_rng(seed)
    m = _Maps(w, h, gravity)
    smax = min(scales[1], ((min(w, h) - 1) / 2.0 - 2.0) / ext)
    for _ in range(n):
        s = rng.uniform(scales[0], smax)
        lo = max(p.border + 0.01, s * ext + 1.0)
        kx, ky = _spot(rng, m, lo, lo)
        m.add(kx, ky, similarity(s, rng.uniform(0.0, 2.0 * math.pi)))
    return m.field("similarity", pat_key)


AFFINE = ((1.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0, 0.0), (0.0, -1.0, 1.0, 0.0), (-1.0, 0.0, 0.0, -1.0),
          similarity(1.0, math.pi / 4), similarity(1.0, math.pi / 6), (1.0, 0.5, 0.0, 1.0), (1.0, 0.0, 0.4, 1.0),
          (1.5, 0.0, 0.0, 0.6), (0.6, 0.0, 0.0, 1.4), (-1.0, 0.0, 0.0, 1.0), (0.0, 1.0, 1.0, 0.0),
          (1.0e-3, 0.0, 0.0, 1.0e-3), (1.2, 0.3, -0.2, 0.9))


def field_affine(pat_key, w=W, h=H, seed=2):
    """identity, the zero matrix, rotations, shear, anisotropic and mirrored M"""
    p = pattern(pat_key)
    ext, rng = pattern_extent(p), np.random.default_rng(seed)
    m = _Maps(w, h)
    for M in AFFINE:
        nx, ny = math.hypot(M[0], M[1]), math.hypot(M[2], M[3])
        for _ in range(5):
            kx, ky = _spot(rng, m, max(p.border + 0.01, nx * ext + 1.0), max(p.border + 0.01, ny * ext + 1.0))
            m.add(kx, ky, M)
    return m.field("affine", pat_key)


def subpixel_positions(x0):
    """x0 and the positions around x0 + 0.5, where (int)(kx + 0.5f) goes over to the next pixel: the float neighbours
    of x0 + 0.5 itself (a sub-pixel part of nextafter(0.5) added to x0 would round away) and 1e-5 either side"""
    half = F(x0 + 0.5)
    return (F(x0), half, nextafter(half, 0.0), nextafter(half, 1.0e9), F(x0 + 0.49999), F(x0 + 0.50001))


def field_checker(pat_key, w=W, h=H, seed=3):
    """two-M checkerboard over the whole image: pixels of even x + y carry the identity, the others a 1.2 x rotation,
    so a ray lookup one pixel off changes M; keypoints on every sub-pixel part around the rounding threshold"""
    p = pattern(pat_key)
    ext, rng = pattern_extent(p), np.random.default_rng(seed)
    m = _Maps(w, h)
    odd = (np.add.outer(np.arange(h), np.arange(w)) & 1) == 1
    m.jac[odd] = np.array([similarity(1.2, 0.7)[0], similarity(1.2, 0.7)[1], 0.0, similarity(1.2, 0.7)[2],
                           similarity(1.2, 0.7)[3], 0.0], dtype=F)
    lo = int(math.ceil(max(p.border, 1.2 * ext + 1.0))) + 1
    for ix in range(6):
        for iy in range(6):
            for parity in (0, 1):
                x0 = int(rng.integers(lo, w - 1 - lo))
                y0 = int(rng.integers(lo, h - 2 - lo))
                y0 += (x0 + y0 + parity) & 1
                m.xy.append((subpixel_positions(x0)[ix], subpixel_positions(y0)[iy]))
    return m.field("checker", pat_key)


def patch_geometry(M, kx, ky, reach, w, h):
    """(pw, ph, class, px0, by0, clipped to the image?) of describe_setup_one in float32, None where the set-up leaves
    class 3 without a patch"""
    M = [F(v) for v in M]
    with np.errstate(all="ignore"):
        nx = np.sqrt(F(M[0] * M[0]) + F(M[1] * M[1])) * F(1.001)
        ny = np.sqrt(F(M[2] * M[2]) + F(M[3] * M[3])) * F(1.001)
        ex = F(F(max(nx, F(1.0))) * reach) + F(0.75)
        ey = F(F(max(ny, F(1.0))) * reach) + F(0.75)
    if not (ex < 1024.0 and ey < 1024.0):
        return None
    bx0, bx1 = int(math.floor(F(kx - ex))), int(math.ceil(F(kx + ex)))
    by0, by1 = int(math.floor(F(ky - ey))), int(math.ceil(F(ky + ey)))
    clipped = bx0 < 0 or by0 < 0 or bx1 > w - 1 or by1 > h - 1
    bx0, by0, bx1, by1 = max(bx0, 0), max(by0, 0), min(bx1, w - 1), min(by1, h - 1)
    px0 = bx0 & ~3
    pw, ph = bx1 - px0 + 1, by1 - by0 + 1
    cls = 0 if (pw <= 64 and ph <= 64) else (1 if (pw <= 80 and ph <= 72) else 3)
    return pw, ph, cls, px0, by0, clipped


def boxes_inside(p, M, kx, ky, w, h):
    """sample_positions (orc_describe.c) in float32: every box inside the image?"""
    n = p.n_points
    px, py = np.array(p.px[:n], dtype=F), np.array(p.py[:n], dtype=F)
    sg = np.array(p.sigma_half[:n], dtype=F)
    M = [F(v) for v in M]
    with np.errstate(all="ignore"):
        xf = F(kx) + (M[0] * px + M[1] * py)
        yf = F(ky) + (M[2] * px + M[3] * py)
        ok = (xf - sg >= 0) & (yf - sg >= 0) & (xf + sg < F(w - 1)) & (yf + sg < F(h - 1))
    return bool(np.all(ok))


CLASS_TARGETS = ((0, 64, 0), (0, 65, 1), (0, 80, 1), (0, 81, 3), (1, 64, 0), (1, 65, 1), (1, 72, 1), (1, 73, 3))
CLASS_PLACES = ("centre", "left", "right", "top", "bottom")


def field_classes(pat_key, w=W, h=H):
    """stamps whose row norms put the patch width on each side of 64 and 80 and its height on each side of 64 and 72
    (ex = max(nx 1.001, 1) reach + 0.75, px0 aligned down to 4, clipped to the image) while the other side stays
    within 64, so the class is the one the boundary decides: (axis, pixels, class) of CLASS_TARGETS.  Each target is
    searched where it is used -- at the centre and next to each rim, where the clip takes part in the size -- over
    the stretch (steps of 5e-4) and the pixel the keypoint sits on.  `intent` lists (keypoint, axis, pixels, class,
    place); a target no stretch reaches (wide-box patterns start above the small ones) is absent from it."""
    p = pattern(pat_key)
    reach = pattern_reach(p)
    R = max(math.hypot(float(p.px[i]), float(p.py[i])) for i in range(p.n_points))
    sg = max(float(p.sigma_half[i]) for i in range(p.n_points))
    m = _Maps(w, h)
    intent = []
    for i, (axis, target, cls) in enumerate(CLASS_TARGETS):
        for place in CLASS_PLACES:
            found = None
            for j in range(8):  # (outer: the position closest to the rim, where the clip acts, is taken first)
                for s in np.arange(1.0, 1.6, 0.0005):
                    M = tuple(F(v) for v in ((s, 0.0, 0.0, 1.0) if axis == 0 else (1.0, 0.0, 0.0, s)))
                    near_x = max(p.border + 0.3, float(M[0]) * R + sg + 0.05)
                    near_y = max(p.border + 0.3, float(M[3]) * R + sg + 0.05)
                    kx, ky = {"centre": (w // 2 - 20.7 + 5 * i + j, h // 2 + 1.2),
                              "left": (near_x + j, h // 2 - 11.8 + 3 * i),
                              "right": (w - 1 - near_x - j, h // 2 - 11.3 + 3 * i),
                              "top": (w // 2 - 59.4 + 7 * i + j, near_y + j % 2),
                              "bottom": (w // 2 + 20.1 + 7 * i + j, h - 1 - near_y - j % 2)}[place]
                    g = patch_geometry(M, kx, ky, reach, w, h)
                    if (g[axis] == target and (g[1 - axis] <= 64 and g[2] == cls or pat_key != "default")
                            and m.free(kx, ky) and boxes_inside(p, M, kx, ky, w, h)):
                        found = (kx, ky, M)
                        break
                if found:
                    break
            if found:
                intent.append((len(m.xy), axis, target, patch_geometry(found[2], found[0], found[1], reach, w, h)[2], place))
                m.add(*found)
    f = m.field("classes", pat_key)
    f.intent = intent
    return f


def field_unusable(pat_key, w=W, h=H, seed=4):
    """pixels without a usable ray or Jacobian between usable ones: both sides must drop exactly these keypoints"""
    p = pattern(pat_key)
    ext, rng = pattern_extent(p), np.random.default_rng(seed)
    m = _Maps(w, h)
    nan, inf = float("nan"), float("inf")
    bad = (dict(ray=(0.0, 0.0, 0.0)), dict(J=(nan, 0.0, 0.0, 0.0, 1.0, 0.0)), dict(J=(1.0, 0.0, 0.0, nan, 1.0, 0.0)),
           dict(J=(1.0, 0.0, 0.0, 0.0, inf, 0.0)), dict(J=(-inf, 0.0, 0.0, 0.0, 1.0, 0.0)),
           dict(J=(1.0e6, 0.0, 0.0, 0.0, 1.0e6, 0.0)), dict(J=(1.0, 1.0e6, 0.0, 0.0, 1.0, 0.0)))
    lo = max(p.border + 0.01, 1.3 * ext + 1.0)
    for rep in range(5):
        for b in bad:
            kx, ky = _spot(rng, m, lo, lo)
            m.add(kx, ky, **b)
            kx, ky = _spot(rng, m, lo, lo)
            m.add(kx, ky, similarity(rng.uniform(0.6, 1.3), rng.uniform(0.0, 6.28)))
    return m.field("unusable", pat_key)


def field_fallback2(pat_key, w=W, h=H):
    """extraction direction (0, 0, 1) on rays (0, 0, 1): e_y falls through to the second candidate, camera +y"""
    f = field_similarity(pat_key, w, h, n=40, seed=5, gravity=(0.0, 0.0, 1.0), scales=(0.6, 1.3))
    f.name = "fallback2"
    return f


def field_fallback3(pat_key, w=W, h=H, seed=6):
    """some pixels with ray (0, 1, 0) under direction (0, 1, 0): first and second candidate vanish, the third (camera
    +x) gives e_y = (1, 0, 0), e_x = (0, 0, 1) and M = [[J2, J0], [J5, J3]]"""
    p = pattern(pat_key)
    ext, rng = pattern_extent(p), np.random.default_rng(seed)
    m = _Maps(w, h)
    lo = max(p.border + 0.01, 1.3 * ext + 1.0)
    for i in range(32):
        kx, ky = _spot(rng, m, lo, lo)
        M = similarity(rng.uniform(0.6, 1.3), rng.uniform(0.0, 6.28)) if i % 4 else (1.0, 0.0, 0.0, 1.0)
        m.add(kx, ky, M, ray=(0.0, 1.0, 0.0) if i % 2 == 0 else None)
    return m.field("fallback3", pat_key)


def knife_positions(limit, fractions=(0.0, 0.25, 0.5, 0.75, 1.0)):
    """float positions at which a box of half-width s lands on another pixel count, with their float neighbours:
    (int)(x + s + 0.5f) or (int)(x - s + 0.5f) steps where x + s + 0.5 or x - s + 0.5 is whole -- at fraction 0.5 for
    s = 2.0, at 0.25 and 0.75 for 4.25, 4.75 and 9.75, at 0 for 0.5 (k + 1 is the binade's end) -- from 63 and one binade up (127, then 255 ...
    below `limit`).  Just below such a position the float sum x + s may tie up to it: the 2.0 case of pattern_facts."""
    out, k = [], 63
    while k + 1 < limit:
        for fr in fractions:
            out += [nextafter(k + fr, 0.0), F(k + fr), nextafter(k + fr, 1.0e9)]
        k = 2 * k + 1
    return out


def crossing_positions(p, limit, lo, hi):
    """keypoint coordinates that put sample i's x - sigma or x + sigma on each side of a binade boundary B"""
    out = []
    idx = (0, 1, 7, max(range(p.n_points), key=lambda i: float(p.px[i])))
    B = 64
    while B < limit:
        for i in idx:
            for sign in (-1.0, 1.0):
                k = F(F(B + sign * float(p.sigma_half[i])) - F(p.px[i]))
                out += [v for v in (nextafter(k, 0.0), k, nextafter(k, 1.0e9)) if lo <= v < hi]
        B *= 2
    return out


def field_positions(pat_key, w=W, h=H):
    """rims, knife edges and binade crossings; identity M except one row of zero-matrix stamps (every box at the
    keypoint itself) and the stretches that put a box on the last kept column / row"""
    p = pattern(pat_key)
    b = p.border
    m = _Maps(w, h)
    xs = [F(b), nextafter(b, 0.0), F(w - b), nextafter(w - b, 0.0)]
    ys = [F(b), nextafter(b, 0.0), F(h - b), nextafter(h - b, 0.0)]
    my, mx = F(h // 2 + 0.5), F(w // 2 + 3.5)
    for x in xs:
        m.add(x, my)
        for y in ys:
            m.add(x, y)
    for y in ys:
        m.add(mx, y)
    row_a, row_b = F(h // 2 - 9.75), F(h // 2 + 11.5)
    for x in knife_positions(w - b) + crossing_positions(p, w, b, w - b):
        m.add(x, row_a)
        if (int(x + F(0.5)) % 8 or int(row_b + F(0.5)) % 8) and m.free(x, row_b):
            m.add(x, row_b, (0.0, 0.0, 0.0, 0.0))
    col_a, col_b = F(w // 2 - 30.25), F(w // 2 + 41.5)
    for y in knife_positions(h - b) + crossing_positions(p, h, b, h - b):
        m.add(col_a, y)
        if m.free(col_b, y):
            m.add(col_b, y, (0.0, 0.0, 0.0, 0.0))
    # the last kept column / row: the largest stretch (steps of 1e-4) that keeps every box inside, and the next one
    kx, ky = nextafter(w - b, 0.0), nextafter(h - b, 0.0)
    for axis in (0, 1):
        s = 1.0
        pos = (kx, F(h // 2 - 3.25 + axis)) if axis == 0 else (F(w // 2 - 11.25), ky)
        mk = (lambda v: (v, 0.0, 0.0, 1.0)) if axis == 0 else (lambda v: (1.0, 0.0, 0.0, v))
        while boxes_inside(p, mk(s + 1.0e-4), pos[0], pos[1], w, h):
            s += 1.0e-4
        m.add(pos[0], pos[1], mk(s))
        other = (pos[0], pos[1] + F(9.0)) if axis == 0 else (pos[0] + F(9.0), pos[1])
        m.add(other[0], other[1], mk(s + 1.0e-4))
    return m.field("positions", pat_key)


def field_extent(pat_key, w, h):
    """a 4092-pixel side: keypoints at the far end push px0 >> 2 / by0 of the geometry word, the first-byte offset and
    the w * h range of the image buffer to their highest values; the binade crossings beyond 256 ride along"""
    p = pattern(pat_key)
    b, ext = p.border, pattern_extent(p)
    m = _Maps(w, h)
    # (a far-end keypoint cannot be stretched along the long side: its boxes would leave the image)
    wide = w > h
    Ms = ((1.0, 0.0, 0.0, 1.0), (1.0, 0.0, 0.0, 1.2) if wide else (1.2, 0.0, 0.0, 1.0),
          (1.0, 0.0, 0.0, 1.5) if wide else (1.5, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0, 0.0), similarity(0.7, 4.0))
    long_, short = max(w, h), min(w, h)
    far = [nextafter(long_ - b, 0.0), F(long_ - b - 1.5), F(long_ - b - 9.25), F(long_ - 44.7), F(long_ - 60.5),
           F(long_ - 75.25), F(long_ - 33.5), F(long_ - 38.75), F(long_ - 52.25), F(long_ - 57.0), F(b), F(b + 13.5)]
    mid = F(short // 2 + 0.25)
    assert 1.5 * ext + 1.0 < short / 2.0 - 2.0
    for i, a in enumerate(far):
        c = mid + F(i % 3)
        m.add(*((a, c) if wide else (c, a)), Ms[i % len(Ms)])
    knives = [v for v in knife_positions(long_ - b) + crossing_positions(p, long_, b, long_ - b) if v > 200.0]
    for i, a in enumerate(knives):
        c = mid + F(3.0 + i % 4)
        if m.free(*((a, c) if wide else (c, a))):
            m.add(*((a, c) if wide else (c, a)), Ms[i % len(Ms)] if i % len(Ms) else None)
    return m.field("extent%dx%d" % (w, h), pat_key)


def field_pattern_edges(pat_key, w=W, h=H):
    """the knife-edge positions under the identity (the centre sample sits at the keypoint) and under the zero matrix
    (every sample does), for patterns whose half-widths sit exactly on a threshold of pattern_facts"""
    p = pattern(pat_key)
    b = p.border
    m = _Maps(w, h)
    rows = (F(h // 2 - 13.75), F(h // 2 + 3.5), F(h // 2 + 17.25))
    for x in knife_positions(w - b):
        m.add(x, rows[0])
        m.add(x, rows[1], (0.0, 0.0, 0.0, 0.0))
        m.add(x, rows[2], similarity(1.0, math.pi / 2))
    cols = (F(w // 2 - 50.25), F(w // 2 + 21.5), F(w // 2 + 60.75))
    for y in knife_positions(h - b):
        m.add(cols[0], y)
        m.add(cols[1], y, (0.0, 0.0, 0.0, 0.0))
        m.add(cols[2], y, similarity(1.0, math.pi / 2))
    for x in knife_positions(w - b, (0.5,))[:3]:      # both coordinates on the edge
        for y in knife_positions(h - b, (0.5,))[:3]:
            m.add(x, y, (0.0, 0.0, 0.0, 0.0) if sum(m.pixel(x, y)) % 2 else None)  # (one M per pixel)
    return m.field("pattern_edges", pat_key)


_FIELDS = {}


def fields(pat_key="default", w=W, h=H):
    """the content-independent half of the scenes of one pattern variant and image size (cached: read-only)"""
    key = (pat_key, w, h)
    if key not in _FIELDS:
        if max(w, h) > 1024:
            _FIELDS[key] = [field_extent(pat_key, w, h)]
        elif pat_key in PATTERN_TWEAKS:
            _FIELDS[key] = [field_pattern_edges(pat_key, w, h), field_affine(pat_key, w, h)]
        else:
            _FIELDS[key] = [field_similarity(pat_key, w, h), field_affine(pat_key, w, h), field_checker(pat_key, w, h),
                            field_classes(pat_key, w, h), field_unusable(pat_key, w, h), field_fallback2(pat_key, w, h),
                            field_fallback3(pat_key, w, h), field_positions(pat_key, w, h)]
    return _FIELDS[key]


# ---- routes --------------------------------------------------------------------------------------------------------
# How each descriptor kernel is reached (describe_route, capi_detect.cpp; the camera statistics of
# okvfe_set_camera_maps, capi_context.cpp).  steer: share of the every-8th-pixel grid whose J2 is stretched.
ROUTES = {
    "aware_batched":        dict(pattern="default", aware=True, steer=0.0, expect="kAwareBatched"),
    "aware_batched_wide":   dict(pattern="box1.73", aware=True, steer=0.0, expect="kAwareBatched"),
    "aware6":               dict(pattern="default", aware=True, steer=0.2, expect="kAware6"),
    "aware5":               dict(pattern="default", aware=True, steer=0.6, expect="kAware5"),
    "aware_wide_boxes":     dict(pattern="box1.73", aware=True, steer=0.2, expect="kAwareWideBoxes"),
    "rot_upright":          dict(pattern="default", aware=False, rotation_invariant=False, expect="kRot"),
    "rot_gradient":         dict(pattern="default", aware=False, rotation_invariant=True, expect="kRot"),
    "wide_boxes_upright":   dict(pattern="box1.73", aware=False, rotation_invariant=False, expect="kWideBoxes"),
    "wide_boxes_gradient":  dict(pattern="box1.73", aware=False, rotation_invariant=True, expect="kWideBoxes"),
    "all_modes_box_aware":  dict(pattern="box2.3", aware=True, steer=0.0, expect="kAllModes"),
    "all_modes_box_gradient": dict(pattern="box2.3", aware=False, rotation_invariant=True, expect="kAllModes"),
    "all_modes_scale_aware": dict(pattern="default", aware=True, steer=0.0, scale_invariant=True, expect="kAllModes"),
    "all_modes_scale_gradient": dict(pattern="default", aware=False, rotation_invariant=True, scale_invariant=True,
                                     expect="kAllModes"),
    "all_modes_w254":       dict(pattern="default", aware=True, steer=0.0, w=254, expect="kAllModes"),
}
KERNEL_CLASS = {"default": 0, "box1.73": 1, "box2.3": 2, "extra2.0": 1, "edges_narrow": 0, "edges_wide": 1}
STRETCHED_J2 = 3.0


def steer(jac, share):
    """J2 = 3 on `share` of the every-8th-pixel grid: the row norm sqrt(J0^2 + J1^2 + J2^2) / fu the camera statistics
    read there says "patch of neither LDS class" and "does not fit one buffer", while M, which does not see J2 under
    ray (0, 0, 1), stays what it was (no keypoint of a scene rounds to a grid pixel)"""
    if share <= 0.0:
        return jac
    out = jac.copy()
    i = 0
    for y in range(0, jac.shape[0], 8):
        for x in range(0, jac.shape[1], 8):
            if (7 * i) % 10 < round(share * 10):
                out[y, x, 2] = STRETCHED_J2
            i += 1
    return out


def aware_patch_class(nx, ny, reach):
    """describe_aware_patch_class (k_describe_aware.hip)"""
    ex = F(F(max(F(nx * F(1.001)), F(1.0))) * reach) + F(0.75)
    ey = F(F(max(F(ny * F(1.001)), F(1.0))) * reach) + F(0.75)
    pw, ph = 2 * int(math.ceil(ex)) + 4, 2 * int(math.ceil(ey)) + 1
    return 0 if (pw <= 64 and ph <= 64) else (1 if (pw <= 80 and ph <= 72) else 3)


def patch_fits(nx, ny, border):
    """describe_patch_fits (k_describe.hip): one piece of the 6-wave form's LDS buffer"""
    ex = F(F(max(F(nx * F(1.001)), F(1.0))) * F(border - 1)) + F(1.5)
    ey = F(F(max(F(ny * F(1.001)), F(1.0))) * F(border - 1)) + F(1.5)
    pw, ph = 2 * int(math.ceil(ex)) + 5, 2 * int(math.ceil(ey)) + 2
    nq = (pw + 15) >> 4
    if nq * 16 > 152:
        return False
    R = 64 // nq
    return ((ph + R - 1) // R) * R * nq * 16 <= 6032 - 160 - 16


def camera_stats(jac, fu, p):
    """(share of grid pixels of neither LDS class, share that does not fit) -- refresh_camera_patch_stats"""
    g = jac[::8, ::8].reshape(-1, 6).astype(F)
    with np.errstate(all="ignore"):
        nx = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2]) / F(fu)
        ny = np.sqrt(g[:, 3] * g[:, 3] + g[:, 4] * g[:, 4] + g[:, 5] * g[:, 5]) / F(fu)
    keep = ~(np.isnan(nx) | np.isnan(ny))
    reach = pattern_reach(p)
    seen = int(keep.sum())
    slow = sum(aware_patch_class(a, b, reach) > 1 for a, b in zip(nx[keep], ny[keep]))
    large = sum(not patch_fits(a, b, p.border) for a, b in zip(nx[keep], ny[keep]))
    return slow / max(seen, 1), large / max(seen, 1)


def box_class(p):
    """pattern_facts (host_tables.cpp): 0 = boxes of at most 11 x 11 (extras 5 x 5), 1 = 21 x 21 (10 x 10), 2 = beyond.
    An extra of half-width exactly 2.0 can span 6 pixels in float32, so it belongs to class 1."""
    extra = max(p.n_points - 64, 0)
    cls = 0
    for i in range(p.n_points):
        s = F(p.sigma_half[i])
        if not (s < F(2.0) if i < extra else s <= F(4.75)):
            cls = max(cls, 1)
        if not (s <= F(4.25 if i < extra else 9.75)) or not (s >= F(0.5)):
            cls = 2
    return cls


ROUTE_NAMES = ("kAwareBatched", "kRot", "kAwareWideBoxes", "kWideBoxes", "kAllModes", "kAware5", "kAware6")  # DescribeRoute


def predicted_route(route, jac, w, h, pat_key=None):
    """the DescribeRoute a call of ROUTES[route] takes on maps `jac`: the library's own describe_route (the lab build
    exports it on plain integers, tests/test_describe_route.py) on the facts a context would derive -- the pattern's
    box class and the camera statistics, restated above"""
    r = ROUTES[route]
    p = pattern(pat_key or r["pattern"])
    slow, large = camera_stats(steer(jac, r.get("steer", 0.0)), 1.0, p) if r["aware"] else (0.0, 0.0)
    facts = dict(all_aware=r["aware"], none_aware=not r["aware"], aware_fast=slow * 10 <= 1, wide_patches=large * 5 > 2,
                 box_class=box_class(p), rot_ok=p.border <= 29 and p.n_points - 64 <= 6, extra=max(p.n_points - 64, 0),
                 scale_invariant=r.get("scale_invariant", False), n_layers=1, w=w, h=h, aligned=True)
    lab = C.CDLL(os.path.join(_ROOT, "okvis2_amd", "libokvfe_lab.so"))  # (loads without a GPU)
    lab.okvfe_lab_describe_route.restype = C.c_int32
    box = C.c_int32()
    return ROUTE_NAMES[lab.okvfe_lab_describe_route((C.c_int32 * 12)(*[int(v) for v in facts.values()]), C.byref(box))]


def scenes(route, contents=CONTENTS, w=None, h=None, pat_key=None):
    """every field of the route's pattern variant x every content"""
    r = ROUTES[route]
    w, h = w or r.get("w", W), h or H
    pat_key = pat_key or r["pattern"]
    out = []
    for f in fields(pat_key, w, h):
        for c in contents:
            out.append(Scene("%s/%s/%s" % (route, f.name, c), content(c, w, h), f.rays, steer(f.jac, r.get("steer", 0.0)),
                             f.fu, f.gravity, f.keypoints, pat_key, route, c, f))
    return out


# ---- census (coverage claim only) ----------------------------------------------------------------------------------
def census(f: Field):
    """per keypoint of a camera-aware call: (fate, direction candidate, patch class, pw, ph, M); fate is "kept" or the
    drop reason "border" / "ray" / "nan" / "box".  numpy float32 restatement of describe_setup_one + the oracle's box
    test; an ulp of disagreement at an edge may move a count by one."""
    p = pattern(f.pattern)
    reach = pattern_reach(p)
    out = []
    g = [F(v) for v in f.gravity]
    cands = (g, [F(0), F(1), F(0)], [F(1), F(0), F(0)])
    for k in f.keypoints:
        kx, ky = F(k["x"]), F(k["y"])
        b = p.border
        if kx < F(b) or kx >= F(f.w - b) or ky < F(b) or ky >= F(f.h - b):
            out.append(("border", -1, -1, 0, 0, None))
            continue
        u, v = int(kx + F(0.5)), int(ky + F(0.5))
        r, J = f.rays[v, u], f.jac[v, u]
        if r[0] == 0 and r[1] == 0 and r[2] == 0:
            out.append(("ray", -1, -1, 0, 0, None))
            continue
        with np.errstate(all="ignore"):
            for c, gc in enumerate(cands):
                gr = F(F(gc[0] * r[0]) + F(gc[1] * r[1])) + F(gc[2] * r[2])
                ey = [gc[i] - F(gr * r[i]) for i in range(3)]
                n2 = F(F(ey[0] * ey[0]) + F(ey[1] * ey[1])) + F(ey[2] * ey[2])
                if n2 >= F(1.0e-12):
                    break
            if not n2 >= F(1.0e-12):
                out.append(("ray", -1, -1, 0, 0, None))
                continue
            n = np.sqrt(n2)
            ey = [e / n for e in ey]
            ex = [F(ey[1] * r[2]) - F(ey[2] * r[1]), F(ey[2] * r[0]) - F(ey[0] * r[2]), F(ey[0] * r[1]) - F(ey[1] * r[0])]
            M = [(F(F(J[o] * a[0]) + F(J[o + 1] * a[1])) + F(J[o + 2] * a[2])) / F(f.fu) for o in (0, 3) for a in (ex, ey)]
        geo = patch_geometry(M, kx, ky, reach, f.w, f.h)
        pw, ph, cls = (geo[0], geo[1], geo[2]) if geo else (0, 0, 3)
        if any(np.isnan(M)):
            out.append(("nan", c, cls, pw, ph, M))
        elif not boxes_inside(p, M, kx, ky, f.w, f.h):
            out.append(("box", c, cls, pw, ph, M))
        else:
            out.append(("kept", c, cls, pw, ph, M))
    return out


# ---- the batched case: detection + fused set-up ----------------------------------------------------------------------
BATCH_W, BATCH_H, BATCH_N = 256, 256, 9
BATCH_PARAMS = dict(uniformity_radius=12.0, abs_threshold=50, max_kpts=200)
BATCH_MS = ((1.0, 0.0, 0.0, 1.0), similarity(1.2, 0.5), similarity(1.5, 1.1), similarity(0.7, 2.0), (1.0, 0.3, 0.0, 1.0),
            similarity(1.3, 4.0), similarity(1.45, 5.0))


def batched_case():
    """(images [9, h, w], rays, jac, fu, gravity): dots-250 images that differ in the darkness of their dots and in a
    few dots moved off the lattice, under maps that carry one M per dot on the 7 x 7 pixels around it -- whichever
    pixel a sub-pixel detection at the dot rounds to carries the intended M.  Lattice dots sit at 20 + 40 i: their
    neighbourhoods never touch the every-8th-pixel grid."""
    w, h = BATCH_W, BATCH_H
    m = _Maps(w, h)
    rng = np.random.default_rng(9)
    imgs = np.full((BATCH_N, h, w), 250, dtype=np.uint8)
    d = 0
    for cy in range(DOT_LATTICE // 2, h - 1, DOT_LATTICE):
        for cx in range(DOT_LATTICE // 2, w - 1, DOT_LATTICE):
            M = BATCH_MS[d % len(BATCH_MS)]
            m.jac[cy - 3:cy + 4, cx - 3:cx + 4] = np.array([M[0], M[1], 0.0, M[2], M[3], 0.0], dtype=F)
            for b in range(BATCH_N):
                ox, oy = (0, 0) if (d + b) % 5 else (int(rng.integers(-2, 3)), int(rng.integers(-2, 3)))
                imgs[b, cy + oy - 1:cy + oy + 2, cx + ox - 1:cx + ox + 2] = 10 + 12 * ((d + 3 * b) % 9)
            d += 1
    return imgs, m.rays, m.jac, 1.0, (0.0, 1.0, 0.0)


if __name__ == "__main__":
    want = sys.argv[1] if len(sys.argv) > 1 else ""
    for key, (w, h) in (("default", (W, H)), ("box1.73", (W, H)), ("box2.3", (W, H)), ("default", (254, H)),
                        ("default", (4092, 96)), ("default", (96, 4092)), ("extra2.0", (W, H)),
                        ("edges_narrow", (W, H)), ("edges_wide", (W, H))):
        for f in fields(key, w, h):
            if want not in f.name:
                continue
            cs = census(f)
            fate, cand, cls = {}, {}, {}
            for c in cs:
                fate[c[0]] = fate.get(c[0], 0) + 1
                if c[0] == "kept":
                    cand[c[1]] = cand.get(c[1], 0) + 1
                    cls[c[2]] = cls.get(c[2], 0) + 1
            print("%-12s %4dx%-4d %-14s n=%3d %s candidates %s classes %s" % (key, w, h, f.name, len(cs), fate, cand, cls))
