"""GPU: the directed descriptor scenes of tests/describe_scenes.py through Frontend.compute (okvfe_compute), byte for
byte against the oracle: keypoint records, their order, the kept count, descriptors, back-projections and their
validity.  Flat content makes most descriptor bits near ties (test_describe_scenes_host.py), so a box mean that is off
by one unit -- a rim weight, a v_msad_u8 mask, a 24-bit multiply, the reciprocal division's correction -- shows.

Every content x M-field scene runs under every descriptor route.  How each route is steered (describe_route,
csrc/capi_detect.cpp; camera statistics of okvfe_set_camera_maps, csrc/capi_context.cpp):

    route                      how it is reached here
    kAwareBatched              default pattern, camera-aware, maps whose every-8th-pixel grid is mild
    kAwareBatched, WIDE        the same with box_scale = 1.73 (kernel class 1)
    kAware6                    J2 = 3 on 20 % of the every-8th-pixel grid: more than 10 % "neither LDS class", at
                               most 40 % "does not fit one buffer"
    kAware5                    J2 = 3 on 60 % of that grid: more than 40 % do not fit
    kAwareWideBoxes            box_scale = 1.73 on the 20 % camera
    kRot                       no camera-aware image: upright and gradient orientation, default pattern
    kWideBoxes                 box_scale = 1.73, upright and gradient
    kAllModes                  box_scale = 2.3 (class 2), camera-aware and gradient; scale_invariant = true,
                               camera-aware and gradient; a 254-pixel-wide image (rows not dword-aligned)

J2 does not enter M under ray (0, 0, 1), so the steering changes the kernel and nothing else: the routes of one pattern
share one oracle result.  Stamps sit off the every-8th-pixel grid, so they do not steer.  No ABI tells which kernel
ran; the route is what the library's own describe_route answers on the facts of the scene, asserted on the CPU
(test_routes_are_steered_as_intended), and pattern_kernel_class() is asserted here.  A kernel trace of
test_directed_scenes_under_every_route on an MI355X showed 40 launches per route variant, as the table says:
describe_aware_kernel<false> 40, <true> 40, describe_kernel<6, true, false> 40, <5, true, false> 40, <4, true, true>
40, <4, false, true> 80, <4, false, false> 200, describe_rot_kernel 80.

Teeth, observed on an MI355X with scratch builds: one rim weight of box_mean (k_describe_aware.hip) one lower
(r_x1_i - 1) fails 14 of the 33 cases here -- every case that runs that box sum -- with 90 of the 120 descriptors of
similarity / flat255 wrong; one corner weight one lower (A - 1) fails the same 14 with 83 of 120 wrong.  Both are also
caught by test_gpu_parity.py::test_describe_camera_aware_and_backprojection[euroc] (six textured images of some 700
keypoints); its mono640 case runs another kernel and passes.

One batched case covers the set-up fused into the selection kernel's tail (okvfe_detect_describe_batch_device, nine
images: the n_images & ~7 split of the block-to-image mapping).

What the scenes found: an extra sample (a pattern point beyond the 64 lanes) of half-width exactly 2.0 was classed with
the 5 x 5 boxes, but at xf = nextafter(63.5, 0) its box spans 6 pixels in float32; the set-up thread dropped the
keypoint the oracle keeps.  pattern_facts (csrc/host_tables.cpp) now sends exactly 2.0 to the 10 x 10 form."""
import numpy as np
import pytest

import describe_scenes as S
import gpu_common as G
from okvis2_amd import capi, synth

pytestmark = pytest.mark.gpu

MAX_KPTS = 400
_REF = {}


def camera(w, h):
    """intrinsics for the back-projection (the maps of the scenes replace the camera's own)"""
    return synth.Camera(w, h, 190.0, 185.0, w / 2.0 - 0.4, h / 2.0 + 0.3, 1, (-0.2, 0.05, 1.0e-4, -2.0e-4))


def reference(oracle, monkeypatch, pat_key, f, content, aware, rotation_invariant, scale_invariant):
    """oracle result of one scene, computed once per (pattern, field, content, mode) and shared by the routes"""
    mode = oracle.MODE_CAMERA_AWARE if aware else (oracle.MODE_GRADIENT if rotation_invariant else oracle.MODE_UPRIGHT)
    key = (pat_key, f.w, f.h, f.name, content, mode, scale_invariant)
    if key not in _REF:
        q = S.pattern(pat_key)
        monkeypatch.setattr(oracle, "pattern", lambda: q)
        img = S.content(content, f.w, f.h)
        rk, rd = oracle.describe(img, f.keypoints, mode, f.rays, f.jac, np.float32(f.fu), f.gravity,
                                 scale_invariant=scale_invariant)
        rbp, rv = oracle.backproject_keypoints(camera(f.w, f.h), rk)
        for a in (rk, rd, rbp, rv):
            a.setflags(write=False)
        _REF[key] = (rk, rd, rbp, rv)
    return _REF[key]


def check_scene(fe, ref, img, f, aware, label):
    rk, rd, rbp, rv = ref
    k, d, bp, bv = fe.compute(img, f.keypoints, cam=0, gravity=f.gravity if aware else None)
    assert len(k) == len(rk), (label, "kept", len(k), len(rk),
                               sorted(set(rk["class_id"].tolist()) ^ set(k["class_id"].tolist()))[:8])
    G.assert_keypoints_equal(k, rk)
    bad = np.flatnonzero((d != rd).any(axis=1))
    assert len(bad) == 0, (label, "descriptors", len(bad), "of", len(d), "first", k[bad[:3]])
    assert np.array_equal(bv, rv), label
    assert np.array_equal(bp.view(np.uint64), rbp.view(np.uint64)), label


def run_route(oracle, monkeypatch, route, w=None, h=None, contents=S.CONTENTS, pat_key=None, install=False):
    r = S.ROUTES[route]
    w, h = w or r.get("w", S.W), h or S.H
    pat_key = pat_key or r["pattern"]
    aware, rot, scale = r["aware"], r.get("rotation_invariant", True), r.get("scale_invariant", False)
    fe = capi.Frontend(w, h, 10.0, 0, 50, MAX_KPTS, rotation_invariant=rot, scale_invariant=scale,
                       box_scale=S.BOX_SCALES.get(pat_key, 1.0))
    fe.set_camera(0, camera(w, h))
    want = S.pattern(pat_key)
    if install:  # a tweak of the half-widths goes in through okvfe_set_pattern
        p = fe.get_pattern()
        for i in range(want.n_points):
            p.sigma_half[i] = want.sigma_half[i]
        fe.set_pattern(p)
    got = fe.get_pattern()
    assert bytes(got.sigma_half)[:4 * want.n_points] == bytes(want.sigma_half)[:4 * want.n_points]
    assert got.border == want.border and bytes(got.px) == bytes(want.px)
    assert fe.pattern_kernel_class() == S.KERNEL_CLASS[pat_key]
    n, maps_of = 0, None
    for sc in S.scenes(route, contents, w, h, pat_key):
        f = sc.field
        assert len(sc.keypoints) <= MAX_KPTS
        if maps_of is not f:
            fe.set_camera_maps(0, sc.rays, sc.jac, sc.fu)
            maps_of = f
        ref = reference(oracle, monkeypatch, pat_key, f, sc.content, aware, rot, scale)
        check_scene(fe, ref, sc.image, f, aware, sc.name)
        n += 1
    return n


@pytest.mark.parametrize("route", list(S.ROUTES))
def test_directed_scenes_under_every_route(oracle, monkeypatch, route):
    n = run_route(oracle, monkeypatch, route)
    assert n == 8 * len(S.CONTENTS)


@pytest.mark.parametrize("route", ["aware_batched", "aware6", "rot_gradient"])
@pytest.mark.parametrize("size", [(4092, 96), (96, 4092)])
def test_extreme_extents(oracle, monkeypatch, route, size):
    """keypoints at the far end of a 4092-pixel side: the highest px0 >> 2 / by0 of the packed geometry word, the
    highest first-byte offset and the end of the w * h buffer range"""
    assert run_route(oracle, monkeypatch, route, size[0], size[1], ("flat255", "dots250", "noise")) == 3


@pytest.mark.parametrize("route", ["aware_batched", "aware6", "rot_upright", "rot_gradient"])
@pytest.mark.parametrize("tweak", list(S.PATTERN_TWEAKS))
def test_half_widths_exactly_on_a_class_threshold(oracle, monkeypatch, tweak, route):
    """extras of half-width exactly 2.0 and 4.25, first-pass samples of exactly 4.75 and 9.75, boxes of exactly 0.5,
    at the float positions where such a box lands on one pixel more (k + 0.5 and its neighbours, two binades).
    Patterns of kernel class 1 turn the four routes into their wide-box forms."""
    assert run_route(oracle, monkeypatch, route, pat_key=tweak, install=True) == 2 * len(S.CONTENTS)


def test_fused_setup_of_a_batch_of_nine(oracle):
    """detection + description in one call: the per-keypoint set-up runs in the tail of the selection kernel"""
    import torch
    imgs, rays, jac, fu, grav = S.batched_case()
    n, prm = S.BATCH_N, S.BATCH_PARAMS
    cam = camera(S.BATCH_W, S.BATCH_H)
    fe = capi.Frontend(S.BATCH_W, S.BATCH_H, prm["uniformity_radius"], 0, prm["abs_threshold"], prm["max_kpts"],
                       max_batch=n)
    fe.set_camera(0, cam)
    fe.set_camera_maps(0, rays, jac, fu)
    d_img = torch.from_numpy(imgs).cuda()
    s = torch.cuda.current_stream().cuda_stream
    fe.detect_describe_batch_device(d_img.data_ptr(), n, np.zeros(n, dtype=np.int32), np.tile(np.float32(grav), (n, 1)), s)
    torch.cuda.synchronize()
    fe.check_capacity(n)
    classes = set()
    for i in range(n):
        k, d, bp, bv = fe.download(i)
        rk, rd = oracle.detect_describe(imgs[i], prm["uniformity_radius"], 0, prm["abs_threshold"], prm["max_kpts"],
                                        oracle.MODE_CAMERA_AWARE, rays, jac, np.float32(fu), grav)
        G.assert_keypoints_equal(k, rk)
        assert np.array_equal(d, rd), i
        rbp, rv = oracle.backproject_keypoints(cam, rk)
        assert np.array_equal(bv, rv) and np.array_equal(bp.view(np.uint64), rbp.view(np.uint64)), i
        assert len(k) >= 8
        cs = S.census(S.Field("batch", S.BATCH_W, S.BATCH_H, rays, jac, fu, grav, k))
        assert all(c[0] == "kept" for c in cs)
        classes |= {c[2] for c in cs}
    assert 1 in classes and 3 in classes, classes
