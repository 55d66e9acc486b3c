"""GPU: the dense fallback chain -- what a call runs when its width is not a multiple of 4 or its image pointer is not
dword aligned (harris_generic_kernel, nms_generic_kernel / nms_kernel on the dense map, launch_sort, the three selection
forms on ScoreLayout{w, 0}, refine_emit from the map, describe_kernel<4, generic> with the byte-wise stage_patch,
compact_kernel) -- against the oracle, byte for byte.  Shapes, scenes, references and their census: unaligned_cases.py
(held to its floors on the CPU by test_unaligned_cases_host.py, which also asserts the selection form and the
descriptor route of every case here).

    entry point                              odd width                          aligned width, pointer + 1 .. 3
    okvfe_detect (B = 1)                     every width x form x threshold     --  (host images are staged aligned)
    okvfe_detect_describe (B = 1)            every extraction mode              --
    okvfe_detect_ahead + okvfe_compute       every extraction mode              --
    okvfe_compute on given keypoints         describe_scenes.py at 253 and 255  --
    okvfe_detect_describe_batch_device       every width x form x threshold,    four shapes x upright / camera-aware x
                                             every mode, permuted batches       map kept or not, offsets 0 1 2 3 0
    okvfe_detect_batch_device +              --                                 every configuration of
      okvfe_describe_batch_device                                               describe_scenes.ROUTES, offsets 1 .. 3
    okvfe_harris_score_device                259 x 67                           256 x 64, image + 1 .. 3, score + 4 .. 12 B
    scale space (Harris and AGAST)           layer widths of every residue      --

okvfe_describe_batch_device describes the keypoints the detect half left in the context, it takes none from the caller:
the directed keypoints of describe_scenes.py cannot be fed to a device batch at a pointer offset, so each route's
configuration (pattern, mode, scale ladder, steered camera maps) runs here on the keypoints detected in textured
content.

Teeth, observed once on an MI355X with scratch builds that change values only (no address moves), against this file and
test_gpu_unaligned_fuzz.py:
  (a) nms_generic_kernel, `x < w - 2` -> `x < w - 3`: 36 cases fail -- every width of
      test_odd_width_through_every_selection_form, every case of test_odd_width_through_every_extraction_mode, both Harris
      scale spaces, the capacity test (its candidate counts), 9 fuzz seeds;
  (b) stage_patch's byte loop, `c < pw` -> `c < pw - 1` (the last patch column keeps what the previous keypoint left):
      test_directed_descriptor_scenes_at_odd_widths[253], [255], test_odd_width_through_every_extraction_mode[259-97-radtan]
      and test_batches_of_odd_stride_and_their_permutation[259-97-radtan] fail; the suite before this file stayed green
      (test_gpu_describe_directed.py's all_modes_w254 included);
  (c) harris_generic_kernel, cmask `col <= w - 2` -> `col <= w - 3`: 68 cases fail -- all of the above plus every case of
      test_aligned_width_at_pointer_offsets, test_score_map_at_image_and_score_pointer_offsets and
      test_describe_route_configurations_at_pointer_offsets (all_modes_w254 excepted)."""
import ctypes

import numpy as np
import pytest

import describe_scenes as DS
import gpu_common as G
import unaligned_cases as U
from okvis2_amd import capi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PERMUTATION = (4, 8, 1, 6, 0, 3, 7, 2, 5)


def to_host(ptr, dtype, count):
    host = np.empty(count, dtype=dtype)
    st = capi.lib().okvfe_copy_to_host(ctypes.c_void_p(host.ctypes.data), ctypes.c_void_p(ptr),
                                       ctypes.c_size_t(host.nbytes), None)
    assert st == capi.OK
    return host


def device_images(imgs, offset=0):
    """(tensor that owns the bytes, device pointer of the first image): the images at `offset` bytes past an
    allocation's start"""
    flat = np.ascontiguousarray(imgs).reshape(-1)
    buf = torch.zeros(flat.size + 8, dtype=torch.uint8, device="cuda")
    buf[offset:offset + flat.size] = torch.from_numpy(flat.copy()).cuda()
    assert buf.data_ptr() % 256 == 0
    return buf, buf.data_ptr() + offset


def run_batch(fe, ptr, n, cam_ids=None, gravity=None):
    fe.detect_describe_batch_device(ptr, n, cam_ids, gravity, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    fe.check_capacity(n)
    return [fe.download(i) for i in range(n)]


def assert_result(got, want, label):
    k, d, bp, bv = got
    G.assert_keypoints_equal(k, want[0])
    assert np.array_equal(d, want[1]), label
    if want[2] is not None:
        assert np.array_equal(bv, want[3]), label
        assert np.array_equal(bp.view(np.uint64), want[2].view(np.uint64)), label


def assert_dense_map_equals_oracle(fe, w, h, n, want):
    out = fe.device_outputs()
    assert out.scores is not None and out.score_strips == 0 and out.score_pitch == w
    got = to_host(out.scores, np.int32, n * h * w).reshape(n, h, w)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]  # every pixel, rim included


@pytest.mark.parametrize("w,h", U.ODD_SHAPES)
def test_odd_width_through_every_selection_form(oracle, w, h):
    """B = 1 detection and a batch of nine (noise, rim structure, jittered cells, one flat image) under each selection
    form at both thresholds; then once more with the score map kept, which must equal the oracle's on every pixel."""
    imgs = U.batch(w, h)
    buf, ptr = device_images(imgs)
    for form in U.FORMS:
        radius, maxk = U.form_params(form, w, h)
        for thr in U.THRESHOLDS:
            fe = capi.Frontend(w, h, radius, 0, thr, maxk, max_batch=U.BATCH, max_candidates=U.MAX_CAND)
            det = U.detect_reference(w, h, radius, thr, maxk)
            ref = U.describe_reference(w, h, radius, thr, maxk, "gradient")
            for i in (0, 1, 2, U.FLAT):
                G.assert_keypoints_equal(fe.detect(imgs[i]), det[i])
            for keep in (False, True):
                fe.set_keep_score_map(keep)
                got = run_batch(fe, ptr, U.BATCH)
                for i in range(U.BATCH):
                    assert_result(got[i], ref[i], (w, h, form, thr, keep, i))
                counts = to_host(fe.device_outputs().candidate_counts, np.int32, U.BATCH)
                assert counts.tolist() == [len(c) for c in U.candidates(w, h, thr)]
            assert_dense_map_equals_oracle(fe, w, h, U.BATCH, U.score_reference(w, h))
            assert len(got[U.FLAT][0]) == 0
            fe.close()


@pytest.mark.parametrize("mode", U.MODES)
@pytest.mark.parametrize("w,h", U.MODE_SHAPES)
def test_odd_width_through_every_extraction_mode(oracle, w, h, mode):
    """upright, gradient, the scale ladder, and camera-aware extraction under a radial-tangential, an equidistant and a
    RADTAN8 camera: B = 1 (okvfe_detect_describe), detect-ahead + compute, and the batch of nine, back-projections
    included"""
    radius, maxk = U.form_params("array", w, h)
    thr = U.THRESHOLDS[0]
    aware = mode in ("radtan", "equidistant", "radtan8")
    fe = capi.Frontend(w, h, radius, 0, thr, maxk, max_batch=U.BATCH, max_candidates=U.MAX_CAND, **U.frontend_kwargs(mode))
    kw = {}
    if aware:
        fe.set_camera(0, U.camera(w, h, mode))
        kw = dict(cam=0, gravity=U.GRAVITY)
    imgs = U.batch(w, h)
    det = U.detect_reference(w, h, radius, thr, maxk)
    ref = U.describe_reference(w, h, radius, thr, maxk, mode)
    for i in (0, 1, 2):
        assert_result(fe.detect_describe(imgs[i], **kw), ref[i], (mode, "b1", i))
        kd = fe.detect_ahead(imgs[i], **(kw or dict(cam=-1, gravity=None)))
        G.assert_keypoints_equal(kd, det[i])
        assert_result(fe.compute(fe._ahead_image, kd, **kw), ref[i], (mode, "ahead", i))
        assert_result(fe.compute(imgs[i].copy(), kd[::2].copy(), **kw),
                      _describe_subset(oracle, w, h, mode, imgs[i], kd[::2]), (mode, "compute", i))
    buf, ptr = device_images(imgs)
    cams = np.zeros(U.BATCH, np.int32) if aware else None
    grav = np.tile(np.float32(U.GRAVITY), (U.BATCH, 1)) if aware else None
    got = run_batch(fe, ptr, U.BATCH, cams, grav)
    for i in range(U.BATCH):
        assert_result(got[i], ref[i], (mode, "batch", i))
    assert sum(len(r[0]) for r in ref) >= 8 * 16  # (descriptors are compared on something)


def _describe_subset(oracle, w, h, mode, img, kps):
    if mode in ("radtan", "equidistant", "radtan8"):
        rays, jac = U.camera_maps(w, h, mode)
        k, d = oracle.describe(img, kps, oracle.MODE_CAMERA_AWARE, rays, jac, np.float32(U.camera(w, h, mode).fu), U.GRAVITY)
        bp, bv = U.backproject(w, h, mode, k)
        return k, d, bp, bv
    k, d = oracle.describe(img, kps, oracle.MODE_UPRIGHT if mode == "upright" else oracle.MODE_GRADIENT,
                           scale_invariant=(mode == "scale_invariant"))
    return k, d, None, None


@pytest.mark.parametrize("mode", ["gradient", "radtan"])
@pytest.mark.parametrize("w,h", U.RESIDUE_SHAPES + U.MODE_SHAPES)
def test_batches_of_odd_stride_and_their_permutation(oracle, w, h, mode):
    """w * h is odd (or 2 mod 4): the nine images of a batch start at different residues mod 4.  Image i equals the
    oracle's result for image i; the same images in another order give the same results in that order -- a descriptor
    that depended on the bytes the previous keypoint's patch left in the pad columns of the LDS rows would move."""
    radius, maxk = U.form_params("array", w, h)
    thr = U.THRESHOLDS[0]
    aware = mode == "radtan"
    fe = capi.Frontend(w, h, radius, 0, thr, maxk, max_batch=U.BATCH, max_candidates=U.MAX_CAND)
    if aware:
        fe.set_camera(0, U.camera(w, h, mode))
    cams = np.zeros(U.BATCH, np.int32) if aware else None
    grav = np.tile(np.float32(U.GRAVITY), (U.BATCH, 1)) if aware else None
    imgs = U.batch(w, h)
    ref = U.describe_reference(w, h, radius, thr, maxk, mode)
    assert w * h % 4 != 0
    for order in (tuple(range(U.BATCH)), PERMUTATION, tuple(range(U.BATCH))):
        buf, ptr = device_images(imgs[list(order)])
        got = run_batch(fe, ptr, U.BATCH, cams, grav)
        for i, src in enumerate(order):
            assert_result(got[i], ref[src], (mode, order, i))


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("mode", ["upright", U.ALIGNED_CAMERA])
@pytest.mark.parametrize("w,h,form", U.ALIGNED_CASES)
def test_aligned_width_at_pointer_offsets(oracle, w, h, form, mode, keep):
    """offsets 0, 1, 2, 3 and 0 again on one context: the fused chain, three times the dense fallback, and back; the
    layout okvfe_get_device_outputs reports follows what was written"""
    radius, maxk = U.form_params(form, w, h)
    thr = U.THRESHOLDS[1]
    aware = mode == U.ALIGNED_CAMERA
    fe = capi.Frontend(w, h, radius, 0, thr, maxk, max_batch=U.BATCH, max_candidates=U.MAX_CAND, **U.frontend_kwargs(mode))
    if aware:
        fe.set_camera(0, U.camera(w, h, mode))
    cams = np.zeros(U.BATCH, np.int32) if aware else None
    grav = np.tile(np.float32(U.GRAVITY), (U.BATCH, 1)) if aware else None
    fe.set_keep_score_map(keep)
    imgs = U.batch(w, h)
    ref = U.describe_reference(w, h, radius, thr, maxk, mode)
    for off in (0, 1, 2, 3, 0):
        buf, ptr = device_images(imgs, off)
        got = run_batch(fe, ptr, U.BATCH, cams, grav)
        for i in range(U.BATCH):
            assert_result(got[i], ref[i], (w, h, form, mode, keep, off, i))
        out = fe.device_outputs()
        if off:
            assert_dense_map_equals_oracle(fe, w, h, U.BATCH, U.score_reference(w, h))
        elif keep:
            assert out.scores is not None and out.score_strips >= 1 and out.score_pitch >= w
            m = to_host(out.scores, np.int32, U.BATCH * h * out.score_pitch).reshape(U.BATCH, h, out.score_pitch)
            cols = np.array([capi.lib().okvfe_score_column(fe._h, int(x)) for x in range(w)])
            inner = np.s_[:, 3:h - 3, 3:w - 3]
            assert np.array_equal(m[:, :, cols][inner], U.score_reference(w, h)[inner])
        else:
            assert out.scores is None


@pytest.mark.parametrize("w,h", U.SCORE_WIDTHS)
def test_score_map_at_image_and_score_pointer_offsets(oracle, w, h):
    """okvfe_harris_score_device: image pointer 0 .. 3 bytes and score pointer 0 .. 3 int32 past an aligned address (4-byte
    but not 16-byte aligned: the generic kernel); the map equals the oracle's and nothing around it is written"""
    n = 3
    imgs = U.batch(w, h)[:n]
    want = U.score_reference(w, h)[:n]
    fe = capi.Frontend(w, h, 10.0, 0, 1, 100, max_batch=n)
    front = (w + 3) // 4 * 4
    for img_off in range(4):
        buf, ptr = device_images(imgs, img_off)
        for sc_off in range(4):
            if w % 4 == 0 and img_off == 0 and sc_off == 0:
                continue  # the aligned kernel: test_gpu_parity.py
            d_sc = torch.full((front + sc_off + n * h * w + w + 4,), -7, dtype=torch.int32, device="cuda")
            first = front + sc_off
            assert (d_sc.data_ptr() + 4 * first) % 16 == 4 * sc_off
            fe.harris_score_device(ptr, n, d_sc.data_ptr() + 4 * first, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got = d_sc.cpu().numpy()
            assert np.array_equal(got[first:first + n * h * w].reshape(n, h, w), want), (img_off, sc_off)
            assert (got[:first] == -7).all() and (got[first + n * h * w:] == -7).all(), (img_off, sc_off)


@pytest.mark.parametrize("route", list(DS.ROUTES))
def test_describe_route_configurations_at_pointer_offsets(oracle, monkeypatch, route):
    """the configuration of every entry of describe_scenes.ROUTES (pattern variant, extraction mode, scale ladder,
    steered camera maps) through okvfe_detect_batch_device + okvfe_describe_batch_device with the image batch 1, 2 and 3
    bytes past an aligned address (all_modes_w254: 0 .. 3) -- kAllModes or kWideBoxes with aligned = false"""
    r = DS.ROUTES[route]
    w, h = r.get("w", DS.W), DS.H
    aware, rot, scale = r["aware"], r.get("rotation_invariant", True), r.get("scale_invariant", False)
    radius, thr, maxk, n = 10.0, 50, 300, 3
    pat = DS.pattern(r["pattern"])
    monkeypatch.setattr(oracle, "pattern", lambda: pat)
    fe = capi.Frontend(w, h, radius, 0, thr, maxk, rotation_invariant=rot, scale_invariant=scale, max_batch=n,
                       box_scale=DS.BOX_SCALES.get(r["pattern"], 1.0), max_candidates=U.MAX_CAND)
    assert fe.pattern_kernel_class() == DS.KERNEL_CLASS[r["pattern"]]
    f = DS.fields(r["pattern"], w, h)[0]
    jac = DS.steer(f.jac, r.get("steer", 0.0))
    cam = U.camera(w, h, "radtan")
    fe.set_camera(0, cam)
    fe.set_camera_maps(0, f.rays, jac, f.fu)
    imgs = np.stack([DS.content(c, w, h) for c in ("noise", "dots250", "dither")])
    mode = oracle.MODE_CAMERA_AWARE if aware else (oracle.MODE_GRADIENT if rot else oracle.MODE_UPRIGHT)
    want = []
    for img in imgs:
        k, d = oracle.detect_describe(img, radius, 0, thr, maxk, mode, f.rays, jac, np.float32(f.fu), f.gravity,
                                      scale_invariant=scale)
        bp, bv = oracle.backproject_keypoints(cam, k)
        want.append((k, d, bp, bv) if aware else (k, d, None, None))
    assert sum(len(x[0]) for x in want) >= 16
    cams = np.zeros(n, np.int32) if aware else None
    grav = np.tile(np.float32(f.gravity), (n, 1)) if aware else None
    stream = torch.cuda.current_stream().cuda_stream
    for off in ((0, 1, 2, 3) if w % 4 else (1, 2, 3)):
        buf, ptr = device_images(imgs, off)
        fe.detect_batch_device(ptr, n, stream)
        fe.describe_batch_device(ptr, n, cams, grav, stream)
        torch.cuda.synchronize()
        fe.check_capacity(n)
        for i in range(n):
            assert_result(fe.download(i), want[i], (route, off, i))


@pytest.mark.parametrize("w", [253, 255])
def test_directed_descriptor_scenes_at_odd_widths(oracle, monkeypatch, w):
    """the directed scenes of describe_scenes.py (flat content, hand-built M, keypoints on the rims and on the last
    column that keeps every box inside) at the two other residues of all_modes_w254, through okvfe_compute: the
    byte-wise patch staging with patch rows whose last columns are sampled"""
    import test_gpu_describe_directed as D
    assert D.run_route(oracle, monkeypatch, "all_modes_w254", w=w) == 8 * len(DS.CONTENTS)


@pytest.mark.parametrize("score", ["harris", "agast"])
@pytest.mark.parametrize("w,h,octaves", U.SCALE_SPACE)
def test_scale_space_with_unaligned_layers(oracle, w, h, octaves, score):
    """layer widths of every residue mod 4 (test_unaligned_cases_host.py) on noise, rim structure and jittered cells"""
    p = U.SCALE_SPACE_PARAMS
    imgs = U.batch(w, h)
    harris = score == "harris"
    thr = p["thr"] if harris else p["agast_thr"]
    fe = capi.Frontend(w, h, p["radius"], octaves, thr, p["max_kpts"], max_batch=U.BATCH, max_candidates=U.MAX_CAND,
                       score_type=capi.SCORE_HARRIS if harris else capi.SCORE_AGAST_9_16)
    st = oracle.SCORE_HARRIS if harris else oracle.SCORE_AGAST
    want = [oracle.detect_describe(img, p["radius"], octaves, thr, p["max_kpts"], oracle.MODE_GRADIENT, score_type=st)
            for img in imgs]
    G.assert_keypoints_equal(fe.detect(imgs[1]), oracle.detect(imgs[1], p["radius"], octaves, thr, p["max_kpts"],
                                                               score_type=st))
    buf, ptr = device_images(imgs)
    got = run_batch(fe, ptr, U.BATCH)
    layers = set()
    for i in range(U.BATCH):
        assert_result(got[i], (want[i][0], want[i][1], None, None), (score, i))
        layers |= set(want[i][0]["octave"].tolist())
    assert layers == set(range(2 * octaves)), layers
    assert len(got[U.FLAT][0]) == 0


def test_candidate_overflow_is_reported_and_leaves_the_context_usable(oracle):
    """fewer candidate slots than maxima: okvfe_check_capacity raises, the overflowing images keep no keypoints, the
    others are right; a fresh context with enough slots equals the oracle"""
    c = U.CAPACITY_CASE
    w, h, thr = c["w"], c["h"], c["thr"]
    radius, maxk = U.form_params(c["form"], w, h)
    imgs = U.batch(w, h)
    counts = [len(k) for k in U.candidates(w, h, thr)]
    ref = U.describe_reference(w, h, radius, thr, maxk, "gradient")
    buf, ptr = device_images(imgs)
    fe = capi.Frontend(w, h, radius, 0, thr, maxk, max_batch=U.BATCH, max_candidates=c["max_candidates"])
    fe.detect_describe_batch_device(ptr, U.BATCH, None, None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    with pytest.raises(capi.OkvfeError) as e:
        fe.check_capacity(U.BATCH)
    assert e.value.status == capi.ERR_CAPACITY
    got_counts = to_host(fe.device_outputs().candidate_counts, np.int32, U.BATCH)
    assert got_counts.tolist() == counts  # the count goes on past the capacity
    kept = to_host(fe.device_outputs().counts, np.int32, U.BATCH)
    for i in range(U.BATCH):
        if counts[i] > c["max_candidates"]:
            assert kept[i] == 0  # which maxima a full list drops depends on the order of the atomics: none is kept
            with pytest.raises(capi.OkvfeError) as e:
                fe.download(i)
            assert e.value.status == capi.ERR_CAPACITY
        else:
            assert_result(fe.download(i), ref[i], i)
    assert sum(n <= c["max_candidates"] for n in counts) >= 2
    fe.close()
    fe = capi.Frontend(w, h, radius, 0, thr, maxk, max_batch=U.BATCH, max_candidates=U.MAX_CAND)
    got = run_batch(fe, ptr, U.BATCH)
    for i in range(U.BATCH):
        assert_result(got[i], ref[i], i)


@pytest.mark.parametrize("w", U.AGAST_TIE_WIDTHS)
def test_agast_tie_runs_across_x_256(oracle, w):
    """Runs of equal AGAST maxima that cross x = 255|256, start beyond it, or are three and more long: block 0 of
    nms_generic_kernel settles them in registers, the blocks to its right walk the map.  Census of the scene by the
    oracle (test_unaligned_cases_host.py), runs of two or more passing pixels: w = 259: 792 runs, 528 of length >= 3,
    none reaches x = 256 (the AGAST score is zero from column w - 3 on: the runs end at x = 255, the last pixel of block
    0); w = 261: 803 runs, 22 cross 255|256, 11 start at x >= 256, 539 of length >= 3; w = 333: 996 runs, 33 cross, 198
    start at x >= 256, 666 of length >= 3.  The radius suppresses nothing: the kept keypoints are the accepted pixels."""
    h = U.AGAST_TIE_HEIGHT
    img = U.agast_tie_scene(w)
    score, cand, kps = U.agast_tie_reference(w)
    fe = capi.Frontend(w, h, U.AGAST_TIE_RADIUS, 0, U.AGAST_TIE_THR, U.AGAST_TIE_MAX_KPTS, rotation_invariant=False,
                       score_type=capi.SCORE_AGAST_9_16, max_batch=2, max_candidates=U.MAX_CAND)
    got = fe.detect(img)
    G.assert_keypoints_equal(got, kps)
    assert len(got) == len(cand)
    flipped = np.ascontiguousarray(img[::-1])
    buf, ptr = device_images(np.stack([img, flipped]))
    res = run_batch(fe, ptr, 2)
    counts = to_host(fe.device_outputs().candidate_counts, np.int32, 2)
    assert counts.tolist() == [len(cand), len(oracle.nms(oracle.agast_score(flipped), U.AGAST_TIE_THR))]
    for i, im in enumerate((img, flipped)):
        k, d = oracle.detect_describe(im, U.AGAST_TIE_RADIUS, 0, U.AGAST_TIE_THR, U.AGAST_TIE_MAX_KPTS, oracle.MODE_UPRIGHT,
                                      score_type=oracle.SCORE_AGAST)
        assert_result(res[i], (k, d, None, None), (w, i))
