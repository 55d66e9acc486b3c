"""The cross-layer stage of the scale-space detector (octaves > 0), restated independently, with a census.

What happens BETWEEN the per-layer stages is written here from the definitions in the comments of
oracle/orc_detect.c ("scale space (octaves > 0)" and "score_type 2 = the published BRISK scale-space detector"),
in numpy integers and fractions.Fraction, not from the C code:

  layer scale / size   Fractions; layer 1 = (w // 3) * 2, layer l >= 2 = half of layer l - 2
  samplers             (a + b + c + d + 2) >> 2 and the separable (2,1,0) / (0,1,2) weights with (sum + 4) // 9
  neighbour window     a pixel centre x of layer l lies at x' = (s_l / s_m)(x + 1/2) - 1/2 in layer m; the window is
                       {u integer : |u - x'| <= 1} intersected with the layer -- no floor_div, no numerators
  maximum test         rejects only on a STRICTLY greater neighbour; neighbour maximum floored at 0, empty window = 0
  parabola             through (rb, sb), (1, s), (ra, sa) in exact rationals; vertex clamped to [lo, ra]; vertex and
                       value each rounded ONCE to float32

The per-layer stages come from the oracle's building blocks, which other tests pin (harris_score, agast_score,
fast58_score, nms, uniformity_select, subpixel2d).  detect() also counts what an image reaches: the census."""
from fractions import Fraction
import math

import numpy as np

import oracle_lib as O

CENSUS_KEYS = ("candidates", "rejected_below", "rejected_above", "rejected_virtual", "survivor_equal_neighbour",
               "clip_left", "clip_right", "clip_top", "clip_bottom", "empty_window", "kept", "cut", "cut_between_equal",
               "delivers_zero", "par_top_layer", "par_a_nonneg", "par_interior", "par_clamp_lo", "par_clamp_hi")


def layer_scale(l) -> Fraction:
    return Fraction(2 ** (l // 2)) if l % 2 == 0 else Fraction(3 * 2 ** ((l - 1) // 2), 2)


def layer_size(w, h, l):
    if l == 0:
        return w, h
    if l == 1:
        return (w // 3) * 2, (h // 3) * 2
    pw, ph = layer_size(w, h, l - 2)
    return pw // 2, ph // 2


def halfsample(img):
    a = img.astype(np.int64)
    h2, w2 = a.shape[0] // 2, a.shape[1] // 2
    a = a[:2 * h2, :2 * w2]
    return ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def twothirdsample(img):
    a = img.astype(np.int64)
    bh, bw = a.shape[0] // 3, a.shape[1] // 3
    a = a[:3 * bh, :3 * bw]
    # horizontally: the left output pixel of a block weighs its three source pixels (2,1,0), the right one (0,1,2)
    hz = np.empty((3 * bh, 2 * bw), dtype=np.int64)
    hz[:, 0::2] = 2 * a[:, 0::3] + a[:, 1::3]
    hz[:, 1::2] = a[:, 1::3] + 2 * a[:, 2::3]
    out = np.empty((2 * bh, 2 * bw), dtype=np.int64)
    out[0::2] = 2 * hz[0::3] + hz[1::3]
    out[1::2] = hz[1::3] + 2 * hz[2::3]
    return ((out + 4) // 9).astype(np.uint8)


def pyramid(img, n_layers):
    ims = [np.ascontiguousarray(img, dtype=np.uint8)]
    for l in range(1, n_layers):
        ims.append(twothirdsample(ims[0]) if l == 1 else halfsample(ims[l - 2]))
    return ims


def window(x, ratio, n):
    """integers u with |u - x'| <= 1, x' = ratio (x + 1/2) - 1/2, and its intersection with [0, n - 1]:
    (lo, hi) unclipped, (lo_c, hi_c) clipped -- empty when lo_c > hi_c"""
    xp = ratio * (Fraction(x) + Fraction(1, 2)) - Fraction(1, 2)
    lo, hi = math.ceil(xp - 1), math.floor(xp + 1)
    return lo, hi, max(lo, 0), min(hi, n - 1)


class Window2D:
    """the windows of every pixel coordinate of layer l in layer m (one Fraction evaluation per coordinate)"""

    def __init__(self, wl, hl, sl, wm, hm, sm):
        r = sl / sm
        self.wx = [window(x, r, wm) for x in range(wl)]
        self.wy = [window(y, r, hm) for y in range(hl)]

    def at(self, x, y):
        """(u0, u1, v0, v1) clipped, and the flags (left, right, top, bottom, empty)"""
        lx, hx, u0, u1 = self.wx[x]
        ly, hy, v0, v1 = self.wy[y]
        return (u0, u1, v0, v1), (lx < 0, hx > u1, ly < 0, hy > v1, u0 > u1 or v0 > v1)

    def max(self, score_map, x, y):
        """largest score in the window, None for an empty window"""
        (u0, u1, v0, v1), flags = self.at(x, y)
        if flags[4]:
            return None, flags
        return int(score_map[v0:v1 + 1, u0:u1 + 1].max()), flags

    def max_many(self, score_map, xs, ys):
        """max() for arrays of pixels: (maxima as int64, valid = window not empty, flags [n, 5])"""
        wx, wy = np.array(self.wx, dtype=np.int64).reshape(-1, 4), np.array(self.wy, dtype=np.int64).reshape(-1, 4)
        ax, ay = wx[xs], wy[ys]
        u0, u1, v0, v1 = ax[:, 2], ax[:, 3], ay[:, 2], ay[:, 3]
        flags = np.stack([ax[:, 0] < 0, ax[:, 1] > u1, ay[:, 0] < 0, ay[:, 1] > v1, (u0 > u1) | (v0 > v1)], axis=1)
        valid = ~flags[:, 4]
        best = np.full(len(xs), np.iinfo(np.int64).min, dtype=np.int64)
        span = int(max((u1 - u0).max(initial=0), (v1 - v0).max(initial=0))) + 1
        h, w = score_map.shape
        for dv in range(span):
            for du in range(span):
                u, v = u0 + du, v0 + dv
                inside = valid & (u <= u1) & (v <= v1)
                val = score_map[np.clip(v, 0, h - 1), np.clip(u, 0, w - 1)].astype(np.int64)
                best = np.where(inside & (val > best), val, best)
        return best, valid, flags


NODES = {"c0": (Fraction(2, 3), Fraction(3, 2), Fraction(7, 10)),
         "ci": (Fraction(3, 4), Fraction(3, 2), Fraction(3, 4)),
         "di": (Fraction(2, 3), Fraction(4, 3), Fraction(2, 3))}


def node_set(l):
    return "c0" if l == 0 else ("di" if l % 2 else "ci")


def parabola_exact(nodes, sb, s, sa):
    """-> (outcome, vertex, value) as exact rationals; outcome in a_nonneg / interior / clamp_lo / clamp_hi"""
    rb, ra, lo = NODES[nodes]
    d10 = Fraction(s - sb) / (1 - rb)
    d21 = Fraction(sa - s) / (ra - 1)
    a = (d21 - d10) / (ra - rb)
    if a >= 0:
        return "a_nonneg", Fraction(1), Fraction(s)
    # p(r) = s + (r - 1)(d10 + a (r - rb));  p'(r) = 0
    v = (a * (1 + rb) - d10) / (2 * a)
    outcome = "interior"
    if v < lo:
        v, outcome = lo, "clamp_lo"
    elif v > ra:
        v, outcome = ra, "clamp_hi"
    return outcome, v, s + (v - 1) * (d10 + a * (v - rb))


def near_f32_boundary(x: Fraction) -> bool:
    """x within relative 2^-40 of the midpoint of two adjacent float32 values (where a step-by-step FP64
    evaluation may round the other way)"""
    if x == 0:
        return False
    f = np.float32(float(x))
    for other in (np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))):
        mid = (Fraction(float(f)) + Fraction(float(other))) / 2
        if abs(x - mid) <= abs(x) * Fraction(1, 2 ** 40):
            return True
    return False


def parabola(nodes, sb, s, sa):
    """-> (outcome, relative scale f32, refined score f32, exempt)"""
    outcome, v, val = parabola_exact(nodes, sb, s, sa)
    return outcome, np.float32(float(v)), np.float32(float(val)), near_f32_boundary(v) or near_f32_boundary(val)


def score_map(img, score_type):
    return O.harris_score(img) if score_type == O.SCORE_HARRIS else O.agast_score(img)


class Prepared:
    """layer images, score maps, 2-D maxima and neighbour-window maxima of one image: shared by the octave counts of
    a scene, and by the AGAST and BRISK configurations (same score maps)"""

    def __init__(self, img, n_layers, thr, score_type):
        self.harris, self.thr = score_type == O.SCORE_HARRIS, thr
        self.images = pyramid(img, n_layers)
        self.scores = [score_map(im, score_type) for im in self.images]
        self.maxima = [O.nms(sc, thr) for sc in self.scores]
        self._virtual, self._windows, self._nb = None, {}, {}

    def serves(self, n_layers, thr, score_type):
        return len(self.images) >= n_layers and self.thr == thr and self.harris == (score_type == O.SCORE_HARRIS)

    @property
    def virtual(self):
        if self._virtual is None:
            self._virtual = O.fast58_score(self.images[0])
        return self._virtual

    def win(self, l, m):
        """windows of layer l's pixels in layer m; m = -1: the virtual layer below c0 (c0's own grid)"""
        if (l, m) not in self._windows:
            hl, wl = self.scores[l].shape
            hm, wm = self.scores[max(m, 0)].shape
            self._windows[(l, m)] = Window2D(wl, hl, layer_scale(l), wm, hm, layer_scale(max(m, 0)))
        return self._windows[(l, m)]

    def neighbour(self, l, m):
        """window maxima of ALL 2-D maxima of layer l in layer m: (maxima, valid, flags)"""
        if (l, m) not in self._nb:
            c = self.maxima[l]
            sm = self.virtual if m < 0 else self.scores[m]
            self._nb[(l, m)] = self.win(l, m).max_many(sm, c["x"].astype(np.int64), c["y"].astype(np.int64))
        return self._nb[(l, m)]


def _order(pts):
    """cmp_points' total order: score descending, then y, then x"""
    return pts[np.lexsort((pts["x"], pts["y"], -pts["score"].astype(np.int64)))]


def detect(img, radius, octaves, thr, max_kpts, score_type=O.SCORE_HARRIS, prep=None):
    """-> (keypoints in the oracle's dtype, census).  census["layers"][l] and census["total"] hold CENSUS_KEYS,
    census["per_layer_kept"] the keypoints per layer, census["ladder"] the distinct scale-ladder indices of the output
    and census["exempt_rows"] the output rows whose parabola lies on a float32 rounding boundary.

    The maximum test takes the neighbours in the order virtual layer (BRISK, layer 0), layer below, layer above and
    stops at the first that rejects: a rejection is counted for that neighbour, and the clip / empty counters count the
    windows the test looked at."""
    L = 2 * octaves
    p = prep if prep is not None else Prepared(img, L, thr, score_type)
    assert p.serves(L, thr, score_type)
    brisk = score_type == O.SCORE_BRISK_SCALESPACE
    rows, exempt_rows, layers = [], [], []
    for l in range(L):
        c = dict.fromkeys(CENSUS_KEYS, 0)
        hl, wl = p.scores[l].shape
        cand = p.maxima[l]
        s_all = cand["score"].astype(np.int64)
        c["candidates"] = len(cand)
        nbs = ([("virtual", -1)] if brisk and l == 0 else []) + ([("below", l - 1)] if l > 0 else []) + \
              ([("above", l + 1)] if l + 1 < L else [])
        ok = np.ones(len(cand), dtype=bool)
        equal = np.zeros(len(cand), dtype=bool)
        for name, m in nbs:
            best, valid, flags = p.neighbour(l, m)
            for j, key in enumerate(("clip_left", "clip_right", "clip_top", "clip_bottom", "empty_window")):
                c[key] += int((flags[:, j] & ok).sum())
            rejected = ok & valid & (best > s_all)  # strictly greater only
            c["rejected_" + name] = int(rejected.sum())
            equal |= ok & valid & (best == s_all)
            ok &= ~rejected
        c["survivor_equal_neighbour"] = int((ok & equal).sum())
        surv = cand[ok]
        if brisk:
            full = _order(surv)
            sel = full[:max_kpts]
        else:
            full = O.uniformity_select(surv, wl, hl, radius, 1 << 30) if len(surv) else surv
            sel = O.uniformity_select(surv, wl, hl, radius, max_kpts) if len(surv) else surv
            assert sel.tobytes() == full[:len(sel)].tobytes()  # the capped selection is a prefix of the uncapped one
        c["kept"], c["cut"] = len(sel), len(full) - len(sel)
        if c["cut"] > 0 and full["score"][len(sel) - 1] == full["score"][len(sel)]:
            c["cut_between_equal"] = 1
        c["delivers_zero"] = int(len(sel) == 0)
        scale = layer_scale(l)
        scale_f = np.float32(scale.numerator) / np.float32(scale.denominator)
        sc = p.scores[l]
        for i in range(len(sel)):
            u, v, s = int(sel["x"][i]), int(sel["y"][i]), int(sel["score"][i])
            ddx, ddy = O.subpixel2d(sc[v - 1:v + 2, u - 1:u + 2])
            xl, yl = np.float32(u) + np.float32(ddx), np.float32(v) + np.float32(ddy)
            X = scale_f * (xl + np.float32(0.5)) - np.float32(0.5)
            Y = scale_f * (yl + np.float32(0.5)) - np.float32(0.5)
            size, resp = np.float32(12.0) * scale_f, np.float32(s)
            if brisk and l + 1 >= L:
                c["par_top_layer"] += 1
            elif brisk:
                sb = p.win(l, l - 1).max(p.virtual if l == 0 else p.scores[l - 1], u, v)[0]
                sa = p.win(l, l + 1).max(p.scores[l + 1], u, v)[0]
                sb, sa = max(sb or 0, 0), max(sa or 0, 0)  # floor 0, empty window 0
                outcome, rel, resp, exempt = parabola(node_set(l), sb, s, sa)
                c["par_" + outcome] += 1
                size = (np.float32(12.0) * rel) * scale_f
                if exempt:
                    exempt_rows.append(len(rows))
            rows.append((X, Y, size, np.float32(-1.0), resp, l, -1))
        layers.append(c)
    kps = np.array(rows, dtype=O.KEYPOINT_DTYPE) if rows else np.zeros(0, dtype=O.KEYPOINT_DTYPE)
    census = {"layers": layers, "total": {k: sum(c[k] for c in layers) for k in CENSUS_KEYS},
              "per_layer_kept": [c["kept"] for c in layers],
              "ladder": sorted({O.scale_index(float(s)) for s in kps["size"]}), "exempt_rows": exempt_rows}
    return kps, census


# ---- the parabola for many triples at once, in int64 ------------------------------------------------------------------
# nodes over a common denominator q: rb = pb / q, ra = pa / q
_INT_NODES = {"c0": (6, 4, 9, (7, 10)), "ci": (4, 3, 6, (3, 4)), "di": (3, 2, 4, (2, 3))}


def parabola_many(nodes, sb, s, sa):
    """The closed form of parabola_exact for int arrays (|scores| <= 255), all products in int64:
       a's sign is that of Na = (sa - s)(q - pb) - (s - sb)(pa - q);
       vertex = P / Q with P = (q + pb) Na - (s - sb)(pa - q)(pa - pb), Q = 2 q Na;
       value  = s + (P - Q) q [(s - sb)(pa - q)(pa - pb) Q + Na (P q - pb Q)] / ((q - pb)(pa - q)(pa - pb) Q^2).
    -> dict: a_nonneg, below_lo, above_ra (bool), rel / resp (float32, rounded once from the exact quotient), exempt"""
    q, pb, pa, (lon, lod) = _INT_NODES[nodes]
    sb, s, sa = (np.asarray(v, dtype=np.int64) for v in (sb, s, sa))
    A, B, Cc = q - pb, pa - q, pa - pb
    e = s - sb
    Na = (sa - s) * A - e * B
    neg = Na < 0
    Na1 = np.where(neg, Na, -1)  # (placeholder where the parabola does not open downwards)
    P = (q + pb) * Na1 - e * B * Cc
    Q = 2 * q * Na1
    P, Q = -P, -Q  # Q > 0 (the value below is unchanged by flipping both)
    below_lo = neg & (P * lod < lon * Q)
    above_ra = neg & (P * q > pa * Q)
    num = (P - Q) * q * (e * B * Cc * Q + Na1 * (P * q - pb * Q))
    den = A * B * Cc * Q * Q
    vnum, vden = s * den + num, den
    rel64 = np.where(neg, P / Q, 1.0)
    resp64 = np.where(neg, vnum / vden, s.astype(np.float64))

    def boundary(x):
        f = x.astype(np.float32)
        out = np.zeros(x.shape, dtype=bool)
        for side in (np.float32(np.inf), np.float32(-np.inf)):
            mid = (f.astype(np.float64) + np.nextafter(f, side).astype(np.float64)) / 2
            out |= np.abs(x - mid) <= np.abs(x) * 2.0 ** -40
        return out & (x != 0)

    return {"a_nonneg": ~neg, "below_lo": below_lo, "above_ra": above_ra, "vertex_num": np.where(neg, P, 1),
            "vertex_den": np.where(neg, Q, 1), "rel": rel64.astype(np.float32), "resp": resp64.astype(np.float32),
            "exempt": neg & (boundary(rel64) | boundary(resp64))}
