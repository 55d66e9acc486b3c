"""CPU: the directed descriptor scenes (tests/describe_scenes.py) satisfy, on the reference alone, the conditions that
make the GPU test on them (test_gpu_describe_directed.py) worth something.

Measured when this file was written (built-in 66-point pattern, the eight 256 x 128 fields, 32 to 163 keypoints each):

* near ties -- share of (kept keypoint, short pair) with |value[i] - value[j]| <= 1, lowest and highest field:
  flat255 80.5 - 89.3 %, flat128 97.1 - 98.9 %, dots250 70.2 - 75.6 %, dither (200 / 201) 1.2 - 7.3 %, noise
  0.00 - 0.01 % (0.03 % on the positions field without its zero-matrix keypoints).  ASSERTED per scene: at least 50 %
  on the flat and dotted contents, below 1 % on noise.  The dither is the in-between case and carries no floor.
* sensitivity -- descriptors of the 120-keypoint similarity field that change when one sample's value is off by +1 or
  -1, minimum over the 66 samples x 2 signs: flat255 0 (sample 0, +1, is unwatched there; the next is 30), dots250 8,
  their union 8.  ASSERTED: at least 1 in the union.
* kept counts -- ASSERTED: the oracle keeps exactly the keypoints the float32 census predicts, in every field under
  every pattern variant and image size (`python tests/describe_scenes.py` tabulates them: per default field 120, 70,
  72, 40, 35 of 70, 40, 32, 145 of 163; 128 on each 4092-pixel scene; 117 and 70 under the tweaked patterns).

The census is a coverage claim: no descriptor is compared through it."""
import ctypes as C

import numpy as np
import pytest

import describe_scenes as S
import oracle_lib as O

F = np.float32


def _use_pattern(monkeypatch, key):
    q = S.pattern(key)
    monkeypatch.setattr(O, "pattern", lambda: q)
    return q


def _smoothed():
    fn = O.lib().orc_smoothed_intensity
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float]
    return fn


def sample_values(img, p, M, kx, ky):
    """values of all samples of one keypoint: orc_smoothed_intensity at the float32 positions of sample_positions"""
    fn, (h, w) = _smoothed(), img.shape
    n = p.n_points
    px, py = np.array(p.px[:n], dtype=F), np.array(p.py[:n], dtype=F)
    M = [F(v) for v in M]
    xf = F(kx) + (M[0] * px + M[1] * py)
    yf = F(ky) + (M[2] * px + M[3] * py)
    return np.array([fn(img.ctypes.data, None, w, h, w, xf[i], yf[i], p.sigma_half[i]) for i in range(n)], dtype=np.int64)


def field_values(f, content):
    """[kept keypoints, samples] of a field on a content"""
    p = S.pattern(f.pattern)
    img = S.content(content, f.w, f.h)
    rows = [sample_values(img, p, c[5], k["x"], k["y"]) for c, k in zip(S.census(f), f.keypoints) if c[0] == "kept"]
    return np.array(rows), p


@pytest.mark.parametrize("key,size", [("default", (S.W, S.H)), ("box1.73", (S.W, S.H)), ("box2.3", (S.W, S.H)),
                                      ("default", (254, S.H)), ("default", (4092, 96)), ("default", (96, 4092)),
                                      ("extra2.0", (S.W, S.H)), ("edges_narrow", (S.W, S.H)), ("edges_wide", (S.W, S.H))])
def test_every_scene_runs_through_the_oracle(monkeypatch, key, size):
    """camera-aware, upright and gradient extraction of every field; the kept count of the camera-aware call is the
    one the census predicts, and the keypoints of the flat contents all take the same verdicts (a drop depends on
    geometry, never on content)"""
    _use_pattern(monkeypatch, key)
    contents = S.CONTENTS if max(size) <= 1024 else ("flat255", "dots250")
    for f in S.fields(key, *size):
        want = sum(c[0] == "kept" for c in S.census(f))
        for c in contents:
            img = S.content(c, f.w, f.h)
            k, d = O.describe(img, f.keypoints, O.MODE_CAMERA_AWARE, f.rays, f.jac, F(f.fu), f.gravity)
            assert len(k) == want, (f.name, c, len(k), want)
            assert len(d) == len(k)
            for mode in (O.MODE_UPRIGHT, O.MODE_GRADIENT):
                ku, du = O.describe(img, f.keypoints, mode)
                border = sum(c2[0] == "border" for c2 in S.census(f))
                assert len(ku) == len(f.keypoints) - border, (f.name, c, mode)


def test_near_tie_share_of_the_contents():
    """per scene (field x content): share of (kept keypoint, short pair) with |value[i] - value[j]| <= 1.  Noise is the
    contrast case, over all kept keypoints of every field that stamps no collapsed M (the affine and positions
    fields carry the zero matrix, under which every sample sits on the keypoint and ties on any content: 2 - 3 % on
    noise; they state no noise figure)."""
    shares = {}
    for f in S.fields("default"):
        collapsed = any(min(np.hypot(c[5][0], c[5][1]), np.hypot(c[5][2], c[5][3])) < 0.5
                        for c in S.census(f) if c[0] == "kept")
        for c in S.CONTENTS:
            V, p = field_values(f, c)
            si = np.array(p.short_i[:p.n_short])
            sj = np.array(p.short_j[:p.n_short])
            d = np.abs(V[:, si] - V[:, sj])
            if c == "noise" and collapsed:
                continue
            shares[(f.name, c)] = float((d <= 1).mean())
    for c in S.CONTENTS:
        print("near-tie share %-8s" % c, {f: round(100.0 * s, 2) for (f, cc), s in shares.items() if cc == c})
    assert sorted(f for f, c in shares if c == "noise") == ["checker", "classes", "fallback2", "fallback3", "similarity",
                                                            "unusable"]
    for (f, c), s in shares.items():
        if c in ("flat255", "flat128", "dots250"):
            assert s >= 0.5, (f, c, s)
        if c == "noise":
            assert s < 0.01, (f, c, s)


def test_an_error_of_one_on_any_sample_changes_a_descriptor():
    """+1 / -1 on the value of any one of the 66 samples changes at least one descriptor among the keypoints of the
    similarity field on flat 255 and dots-250"""
    f = S.fields("default")[0]
    assert f.name == "similarity" and len(f.keypoints) == 120
    changed = {}
    for c in ("flat255", "dots250"):
        V, p = field_values(f, c)
        si = np.array(p.short_i[:p.n_short])
        sj = np.array(p.short_j[:p.n_short])
        bits = V[:, si] > V[:, sj]
        for i in range(p.n_points):
            for e in (1, -1):
                V2 = V.copy()
                V2[:, i] += e
                changed[(c, i, e)] = int(((V2[:, si] > V2[:, sj]) != bits).any(axis=1).sum())
    per = {c: min(v for (cc, _, _), v in changed.items() if cc == c) for c in ("flat255", "dots250")}
    union = min(changed[("flat255", i, e)] + changed[("dots250", i, e)] for i in range(66) for e in (1, -1))
    print("sensitivity minima", per, "union", union)
    assert union >= 1, [(k, v) for k, v in changed.items() if v == 0][:8]


def test_class_census_of_the_default_scenes():
    cs = [c for f in S.fields("default") for c in S.census(f)]
    kept = [c for c in cs if c[0] == "kept"]
    for cls in (0, 1, 3):
        assert sum(c[2] == cls for c in kept) >= 16, cls
    pws, phs = {c[3] for c in kept}, {c[4] for c in kept}
    assert {64, 65, 80, 81} <= pws, sorted(pws)
    assert {64, 65, 72, 73} <= phs, sorted(phs)
    for cand in (0, 1, 2):
        assert sum(c[1] == cand for c in kept) >= 8, cand
    for reason in ("border", "ray", "box", "nan"):
        assert sum(c[0] == reason for c in cs) >= 4, reason


@pytest.mark.parametrize("w", [S.W, 254])
def test_every_patch_class_boundary_is_stamped_at_the_centre_and_at_each_rim(w):
    """pw 64 | 65 and 80 | 81 with ph <= 64, ph 64 | 65 and 72 | 73 with pw <= 64: the boundary alone decides the class
    (0 | 1 and 1 | 3), and each of the eight sizes is there, kept, at the centre and next to every rim"""
    f = next(f for f in S.fields("default", w, S.H) if f.name == "classes")
    cs = S.census(f)
    assert len(f.keypoints) == len(f.intent) == len(S.CLASS_TARGETS) * len(S.CLASS_PLACES) == 40
    assert {(a, t, c, pl) for _, a, t, c, pl in f.intent} == \
           {(a, t, c, pl) for a, t, c in S.CLASS_TARGETS for pl in S.CLASS_PLACES}
    for k, axis, target, cls, place in f.intent:
        fate, _, got_cls, pw, ph, _ = cs[k]
        assert fate == "kept" and got_cls == cls and (pw, ph)[axis] == target and (pw, ph)[1 - axis] <= 64, (k, cs[k])
    # next to a rim the clip to the image takes part in the size, for the stretched side
    reach = S.pattern_reach(S.pattern("default"))
    clipped = {(axis, place) for k, axis, target, cls, place in f.intent
               if S.patch_geometry(cs[k][5], f.keypoints[k]["x"], f.keypoints[k]["y"], reach, f.w, f.h)[5]}
    # (clipped at the right rim the width is w - px0 with px0 a multiple of 4: 64 and 80 exist only for w % 4 == 0)
    assert clipped >= {(0, "left"), (1, "top"), (1, "bottom")} | ({(0, "right")} if w % 4 == 0 else set()), clipped


def test_extreme_extents_reach_the_top_of_the_geometry_word():
    """px0 >> 2 (10 bits) and by0 (12 bits) of g1 close to their limits, every class present"""
    for (w, h) in ((4092, 96), (96, 4092)):
        (f,) = S.fields("default", w, h)
        reach = S.pattern_reach(S.pattern("default"))
        geo = [S.patch_geometry(c[5], k["x"], k["y"], reach, w, h) for c, k in zip(S.census(f), f.keypoints)]
        assert {g[2] for g in geo} == {0, 1, 3}
        if w > h:
            assert max(g[3] for g in geo) >> 2 >= 1000 and max(g[3] + g[0] for g in geo) == w
        else:
            assert max(g[4] for g in geo) >= 4000 and max(g[4] + g[1] for g in geo) == h


def test_routes_are_steered_as_intended():
    """describe_route (the lab build's export of it) sends every route's scenes where its name says, and the steering
    leaves every M alone"""
    for name, r in S.ROUTES.items():
        w = r.get("w", S.W)
        for f in S.fields(r["pattern"], w, S.H):
            assert S.predicted_route(name, f.jac, w, S.H) == r["expect"], (name, f.name)
            if r.get("steer"):
                a = S.census(f)
                b = S.census(S.Field(f.name, f.w, f.h, f.rays, S.steer(f.jac, r["steer"]), f.fu, f.gravity, f.keypoints,
                                     f.pattern))
                assert all(x[:5] == y[:5] for x, y in zip(a, b)) and _same_M(a, b), (name, f.name)
    for key, cls in S.KERNEL_CLASS.items():
        assert S.box_class(S.pattern(key)) == cls, key
    # the tweaked patterns under the four routes they run on: class 1 turns each into its wide-box form
    wide = {"aware_batched": "kAwareBatched", "aware6": "kAwareWideBoxes", "rot_upright": "kWideBoxes",
            "rot_gradient": "kWideBoxes"}
    for key in S.PATTERN_TWEAKS:
        for name, w_name in wide.items():
            for f in S.fields(key):
                want = w_name if S.KERNEL_CLASS[key] == 1 else S.ROUTES[name]["expect"]
                assert S.predicted_route(name, f.jac, S.W, S.H, key) == want, (key, name)
    for (w, h) in ((4092, 96), (96, 4092)):
        (f,) = S.fields("default", w, h)
        assert S.predicted_route("aware_batched", f.jac, w, h) == "kAwareBatched"


def _same_M(a, b):
    for x, y in zip(a, b):
        if (x[5] is None) != (y[5] is None):
            return False
        if x[5] is not None and not np.array_equal(np.array(x[5], dtype=F).view(np.uint32),
                                                   np.array(y[5], dtype=F).view(np.uint32)):
            return False
    return True


def test_half_width_two_can_span_six_pixels():
    """the float32 arithmetic behind the class of an extra sample: a box of half-width exactly 2.0 at
    xf = nextafter(63.5, 0) has x_right - x_left = 5, one more than the 5 x 5 form serves; 4.25, 4.75, 9.75 and 0.5
    stay inside their forms at every knife position of the scenes, and reach their largest size there"""
    def width(xf, s):
        xf, s = F(xf), F(s)
        return int(F(xf + s) + F(0.5)) - int(F(xf - s) + F(0.5))
    assert width(S.nextafter(63.5, 0.0), 2.0) == 5
    assert max(width(x, 2.0) for x in S.knife_positions(4092)) == 5
    for s, most in ((4.25, 9), (4.75, 10), (9.75, 20), (0.5, 2)):
        assert max(width(x, s) for x in S.knife_positions(4092)) == most, s
        assert min(width(x, s) for x in S.knife_positions(4092)) == most - 1, s


def test_batched_case_detects_on_every_class():
    """the nine dots-250 images of the batched GPU case: detections on class-1 and class-3 stamps in the oracle"""
    imgs, rays, jac, fu, grav = S.batched_case()
    p = S.pattern("default")
    reach = S.pattern_reach(p)
    classes, counts = set(), []
    for img in imgs:
        k = O.detect(img, S.BATCH_PARAMS["uniformity_radius"], 0, S.BATCH_PARAMS["abs_threshold"],
                     S.BATCH_PARAMS["max_kpts"])
        f = S.Field("batch", S.BATCH_W, S.BATCH_H, rays, jac, fu, grav, k)
        cs = S.census(f)
        classes |= {c[2] for c in cs if c[0] == "kept"}
        kk, _ = O.describe(img, k, O.MODE_CAMERA_AWARE, rays, jac, F(fu), grav)
        assert len(kk) == sum(c[0] == "kept" for c in cs)
        counts.append(len(kk))
    assert {0, 1, 3} <= classes, classes
    assert min(counts) >= 8 and len(set(map(bytes, imgs))) == len(imgs), counts
