"""CPU: the scenes of tests/scale_space_scenes.py against the census of tests/scale_space_ref.py, and that independent
restatement of the cross-layer stage against the oracle (oracle/orc_detect.c).

A mismatch between the restatement and the oracle is a finding about the oracle: it is reported, the restatement is not
tuned to it.

Labels proved unreachable (asserted below instead of given a floor):
  * windows clipped at the LEFT / TOP border, and EMPTY windows: 2-D maxima lie in columns 2 .. w - 3 (orc_nms), and for
    every layer pair of every image width 48 .. 1100 such a column's window starts at 0 or later and is not empty;
  * windows clipped at the RIGHT / BOTTOM border with the AGAST scores (AGAST 9-16 and the BRISK scale space): these
    score 0 within 3 px of the border, so maxima lie in columns 3 .. w - 4, and no such column's window is clipped.
    With the Harris score (columns up to w - 3) the right / bottom clip is reached, e.g. from layer 0 when w % 3 == 2;
  * the floor of 0 of the neighbour maximum (BRISK scale space): AGAST and FAST 5-8 scores are never negative and no
    window is empty, so a maximum over a window is never below 0;
  * the two clamps of the scale parabola: over all integer triples 0 <= sb, sa <= s <= 255 the vertex stays within
    [5/6, 5/4] (c0), [7/8, 5/4] (c_i), [5/6, 7/6] (d_i), inside [lo, ra] of each node set; and a >= 0 happens only for
    sb == s == sa."""
from fractions import Fraction

import numpy as np
import pytest

import scale_space_ref as R
import scale_space_scenes as S

FLOOR_LABELS = {
    "harris": ("rejected_below", "rejected_above", "survivor_equal_neighbour", "clip_right", "clip_bottom",
               "cut_between_equal", "delivers_zero"),
    "agast": ("rejected_below", "rejected_above", "survivor_equal_neighbour", "cut_between_equal", "delivers_zero"),
    "brisk": ("rejected_below", "rejected_above", "rejected_virtual", "survivor_equal_neighbour", "cut_between_equal",
              "par_a_nonneg", "delivers_zero"),
}
_PREP = {}


def _prepared(name, img, cfg, oracle):
    radius, thr, st = S.CONFIGS[cfg]
    key = (name, thr, st == oracle.SCORE_HARRIS)
    if key not in _PREP:
        _PREP[key] = R.Prepared(img, 8 if 4 in S.octave_counts(img.shape[1], img.shape[0]) else
                                2 * max(S.octave_counts(img.shape[1], img.shape[0])), thr, st)
    return _PREP[key]


def _run(name, img, octaves, cfg, oracle):
    radius, thr, st = S.CONFIGS[cfg]
    return R.detect(img, radius, octaves, thr, S.MAX_KPTS, st, prep=_prepared(name, img, cfg, oracle))


@pytest.mark.parametrize("cfg", sorted(S.CONFIGS))
def test_scenes_reach_the_floors(oracle, cfg):
    total = dict.fromkeys(R.CENSUS_KEYS, 0)
    best = [0] * 8
    ladder = set()
    for name, img, octaves in S.scenes():
        _, c = _run(name, img, octaves, cfg, oracle)
        for k in total:
            total[k] += c["total"][k]
        for l, n in enumerate(c["per_layer_kept"]):
            best[l] = max(best[l], n)
        ladder |= set(c["ladder"])
    print(cfg, "census:", total, "best per layer:", best, "ladder indices:", len(ladder))
    assert min(best) >= 5, best
    for label in FLOOR_LABELS[cfg]:
        assert total[label] >= 16, (label, total[label])
    # unreachable (module docstring); the properties behind it are asserted in the tests below
    assert total["clip_left"] == total["clip_top"] == total["empty_window"] == 0
    assert total["par_clamp_lo"] == total["par_clamp_hi"] == 0
    if cfg != "harris":
        assert total["clip_right"] == total["clip_bottom"] == 0
    if cfg == "brisk":
        assert len(ladder) >= 24, sorted(ladder)
        assert total["par_interior"] >= 16 and total["par_top_layer"] >= 16
    else:
        assert total["par_a_nonneg"] == total["par_interior"] == total["par_top_layer"] == 0


def test_special_scenes_are_what_they_claim(oracle):
    for cfg in S.CONFIGS:
        for w, h, octaves in S.sizes():
            radius, thr, st = S.CONFIGS[cfg]
            _, c = R.detect(S.flat(w, h), radius, octaves, thr, S.MAX_KPTS, st)
            assert c["total"]["candidates"] == 0 and c["total"]["delivers_zero"] == 2 * octaves
            _, c = R.detect(S.dots(w, h, 7), radius, octaves, thr, S.MAX_KPTS, st)
            cands = [l["candidates"] for l in c["layers"]]
            assert cands[0] > 0 and cands[1] > 0 and not any(cands[2:]), (cfg, w, h, cands)


@pytest.mark.parametrize("cfg", sorted(S.CONFIGS))
def test_reference_equals_the_oracle_on_every_scene_and_octave_count(oracle, cfg):
    radius, thr, st = S.CONFIGS[cfg]
    n_exempt = n_rows = 0
    for name, img, _ in S.scenes():
        for octaves in S.octave_counts(img.shape[1], img.shape[0]):
            got, c = _run(name, img, octaves, cfg, oracle)
            want = oracle.detect(img, radius, octaves, thr, S.MAX_KPTS, score_type=st)
            assert len(got) == len(want), (name, octaves, len(got), len(want))
            ex = np.zeros(len(got), dtype=bool)
            ex[c["exempt_rows"]] = True
            assert ex.sum() <= 0.001 * max(len(got), 1), (name, octaves, int(ex.sum()))
            for f in ("x", "y", "octave", "angle", "class_id"):
                assert got[f].tobytes() == want[f].tobytes(), (name, octaves, f)
            for f in ("size", "response"):
                a, b = got[f].view(np.uint32)[~ex], want[f].view(np.uint32)[~ex]
                assert np.array_equal(a, b), (name, octaves, f, np.flatnonzero(a != b)[:5])
            n_exempt += int(ex.sum())
            n_rows += len(got)
    print(cfg, "rows compared:", n_rows, "exempt rows:", n_exempt)
    assert n_rows > 5000


def test_layer_scales_and_sizes(oracle):
    for l in range(8):
        n, d = oracle.layer_scale(l)
        assert R.layer_scale(l) == Fraction(n, d)
    for w in range(16, 420):
        for l in range(8):
            assert R.layer_size(w, w + 5, l) == oracle.layer_size(w, w + 5, l)


def test_samplers_equal_the_oracle_on_every_layer_image(oracle):
    n = 0
    for name, img, octaves in S.scenes():
        ims = R.pyramid(img, 2 * octaves)
        for im in ims:
            if min(im.shape) >= 3:
                assert np.array_equal(R.halfsample(im), oracle.halfsample(im)), name
                assert np.array_equal(R.twothirdsample(im), oracle.twothirdsample(im)), name
                n += 1
        for l in range(2 * octaves):
            assert ims[l].shape[::-1] == oracle.layer_size(img.shape[1], img.shape[0], l)
    assert n > 100


def _ratio(l, m):
    r = R.layer_scale(l) / R.layer_scale(m)
    return r.numerator, r.denominator


@pytest.mark.parametrize("cfg", ["harris", "agast"])
def test_windows_equal_the_oracle_on_every_candidate(oracle, cfg):
    """orc_scale_neighbour_ok / orc_scale_neighbour_max per 2-D maximum of every scene, against the Fraction windows
    (agast: the score maps of the BRISK scale space too, with its virtual layer)"""
    import ctypes as C
    lib = oracle.lib()
    f_ok, f_max = lib.orc_scale_neighbour_ok, lib.orc_scale_neighbour_max
    f_max.restype = C.c_int32
    n = 0
    for name, img, octaves in S.scenes():
        p = _prepared(name, img, cfg, oracle)
        L = 2 * octaves
        for l in range(L):
            cand = p.maxima[l]
            for m in ([-1] if (cfg == "agast" and l == 0) else []) + [k for k in (l - 1, l + 1) if 0 <= k < L]:
                sm = np.ascontiguousarray(p.virtual if m < 0 else p.scores[m], dtype=np.int32)
                rn, rd = _ratio(l, max(m, 0))
                best, valid, _ = p.neighbour(l, m)
                ptr, (ho, wo) = C.c_void_p(sm.ctypes.data), sm.shape
                for i in range(len(cand)):
                    x, y, s = int(cand["x"][i]), int(cand["y"][i]), int(cand["score"][i])
                    want_ok = not (valid[i] and best[i] > s)
                    want_max = max(int(best[i]), 0) if valid[i] else 0
                    assert bool(f_ok(ptr, wo, ho, x, y, s, rn, rd)) == want_ok, (name, l, m, x, y)
                    assert f_max(ptr, wo, ho, x, y, rn, rd) == want_max, (name, l, m, x, y)
                n += len(cand)
    assert n > 50000


def test_windows_left_top_and_empty_are_unreachable(oracle):
    """Columns 2 .. w - 3 (what orc_nms admits): no window starts left of 0 or is empty, for every layer pair of every
    width.  Columns 3 .. w - 4 (AGAST scores are 0 within 3 px of the border): no window is clipped at all -- and
    with column w - 3 the right clip IS reached."""
    right_harris = 0
    for w in range(48, 1101):
        ws = [R.layer_size(w, w, l)[0] for l in range(8)]
        for l in range(8):
            if ws[l] < 8:
                break
            for m in (l - 1, l + 1):
                if not 0 <= m < 8 or ws[m] < 8:
                    continue
                r = R.layer_scale(l) / R.layer_scale(m)
                for x in (2, 3, ws[l] - 4, ws[l] - 3):
                    lo, hi, lo_c, hi_c = R.window(x, r, ws[m])
                    assert lo >= 0 and lo_c <= hi_c, (w, l, m, x)
                    if x in (3, ws[l] - 4):
                        assert hi <= ws[m] - 1, (w, l, m, x)
                    elif x == ws[l] - 3:
                        right_harris += int(hi > ws[m] - 1)
    assert right_harris > 100
    # the windows are monotonic in x, so the columns between the checked ones cannot do worse
    r = Fraction(2, 3)
    los = [R.window(x, r, 10 ** 6)[0] for x in range(50)]
    assert los == sorted(los)


def test_agast_scores_are_zero_within_three_pixels_of_the_border(oracle):
    """... and never negative, like the FAST 5-8 scores: with windows that are never empty, the floor of 0 of the
    neighbour maximum cannot show in an output of the BRISK scale space (a floor of -1 gives the same bytes)"""
    for name, img, _ in S.scenes()[:6]:
        sc = oracle.agast_score(img)
        assert sc.min() >= 0 and oracle.fast58_score(img).min() >= 0
        inner = np.zeros(sc.shape, dtype=bool)
        inner[3:-3, 3:-3] = True
        assert not sc[~inner].any()
        m = oracle.nms(oracle.harris_score(img), 1)
        assert m["x"].min() >= 2 and m["x"].max() <= img.shape[1] - 3 and m["y"].min() >= 2 and \
            m["y"].max() <= img.shape[0] - 3


_RANGES = {"c0": (Fraction(5, 6), Fraction(5, 4)), "ci": (Fraction(7, 8), Fraction(5, 4)),
           "di": (Fraction(5, 6), Fraction(7, 6))}


@pytest.mark.parametrize("nodes", ["c0", "ci", "di"])
def test_parabola_on_all_triples_no_clamp_fires_and_the_oracle_agrees(oracle, nodes):
    """every integer triple 0 <= sb, sa <= s <= 255: the closed form in int64 (parabola_many) finds no vertex outside
    [lo, ra], a >= 0 only for sb == s == sa, the vertex range of the table above, and orc_scale_refine's float32 results
    outside the exemption; the closed form itself equals the Fraction parabola on a sample"""
    rb, ra, lo = R.NODES[nodes]
    lo_f = 0.7 if nodes == "c0" else float(rb)
    vmin, vmax, n, n_exempt = None, None, 0, 0
    grid = np.arange(256)
    for s in range(256):
        sb, sa = (g.reshape(-1) for g in np.meshgrid(grid[:s + 1], grid[:s + 1], indexing="ij"))
        ss = np.full(len(sb), s)
        m = R.parabola_many(nodes, sb, ss, sa)
        assert not m["below_lo"].any() and not m["above_ra"].any()
        assert np.array_equal(m["a_nonneg"], (sb == s) & (sa == s))
        neg = ~m["a_nonneg"]
        if neg.any():
            v = m["vertex_num"][neg] / m["vertex_den"][neg]
            i, j = int(np.argmin(v)), int(np.argmax(v))
            fr = [Fraction(int(m["vertex_num"][neg][k]), int(m["vertex_den"][neg][k])) for k in (i, j)]
            vmin = fr[0] if vmin is None else min(vmin, fr[0])
            vmax = fr[1] if vmax is None else max(vmax, fr[1])
        rel, resp = oracle.scale_refine_many(float(rb), float(ra), lo_f, sb, ss, sa)
        keep = ~m["exempt"]
        assert np.array_equal(rel.view(np.uint32)[keep], m["rel"].view(np.uint32)[keep]), s
        assert np.array_equal(resp.view(np.uint32)[keep], m["resp"].view(np.uint32)[keep]), s
        n += len(sb)
        n_exempt += int(m["exempt"].sum())
    print(nodes, "triples:", n, "exempt:", n_exempt, "vertex range:", vmin, vmax)
    assert n == sum((s + 1) ** 2 for s in range(256))
    assert (vmin, vmax) == _RANGES[nodes] and lo <= vmin and vmax <= ra
    rng = np.random.default_rng(5)
    s = rng.integers(0, 256, size=1500)
    sb, sa = rng.integers(0, s + 1), rng.integers(0, s + 1)
    m = R.parabola_many(nodes, sb, s, sa)
    for i in range(len(s)):
        outcome, v, _ = R.parabola_exact(nodes, int(sb[i]), int(s[i]), int(sa[i]))
        _, rel, resp, exempt = R.parabola(nodes, int(sb[i]), int(s[i]), int(sa[i]))
        assert (outcome == "a_nonneg") == bool(m["a_nonneg"][i])
        assert v == Fraction(int(m["vertex_num"][i]), int(m["vertex_den"][i]))
        assert rel == m["rel"][i] and resp == m["resp"][i] and exempt == bool(m["exempt"][i])
