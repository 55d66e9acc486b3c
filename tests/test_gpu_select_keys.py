"""GPU: the key scatter of the self-ordering selection kernel (select_lazy_kernel<true>, csrc/k_select.hip) and the
hand-over of kept records to its tail, against the oracle, byte for byte.

The kernel writes its sort keys per CHUNK (a cursor per chunk; keys are unordered inside a chunk, and which lane of a
wave arrives first at a cursor is not defined), so every case compares `detect` in both map modes and camera-aware
`detect_describe` with the oracle, and the batch cases also compare a call with its own repetition and with the same call
on another stream.  Each case names a regime of the scatter and asserts that its image reaches it: from
okvfe_device_outputs.candidate_counts (equal to the oracle's candidate count) and from the kernel's chunk schedule
restated on the oracle's scores (tests/select_keys_cases.py).  Images are as small as the regime's candidate count
allows; one to four images per call."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from okvis2_amd import capi, synth

import gpu_common as G
import select_keys_cases as K

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GRAV = (0.05, 0.99, -0.1)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device_counts(fe, n_images=1, which="candidate_counts"):
    """okvfe_device_outputs: candidate_counts (NMS maxima), detect_counts (kept keypoints), counts (described ones)"""
    out = fe.device_outputs()
    host = np.zeros(n_images, dtype=np.int32)
    st = capi.lib().okvfe_copy_to_host(C.c_void_p(host.ctypes.data), C.c_void_p(getattr(out, which)),
                                       C.c_size_t(host.nbytes), None)
    assert st == 0
    return host


def _download(fe, i):
    """(keypoints, descriptors) of image i of the last batch; None where its candidate list overflowed"""
    try:
        return fe.download(i)[:2]
    except capi.OkvfeError as e:
        assert e.status == capi.ERR_CAPACITY
        return None


def _serves(w, h, radius, max_kpts):
    """does select_lazy_kernel serve this configuration (launch_select's own plan, exported by the lab build)"""
    return bool(_plan(w, h, radius, max_kpts)[0])


def _lab():
    return C.CDLL(os.path.join(ROOT, "okvis2_amd", "libokvfe_lab.so"))


def _plan(w, h, radius, max_kpts):
    out = (C.c_int32 * 3)()
    _lab().okvfe_lab_select_plan(int(w), int(h), C.c_float(radius), int(max_kpts), int(max_kpts), out)
    return list(out)


@functools.lru_cache(maxsize=None)
def _maps(w, h):
    import oracle_lib as O
    return O.awareness_maps(K.camera_for(w, h))


def _check_image(oracle, img, radius, thr, max_kpts, max_candidates):
    """detect (map-free and through the score map) and camera-aware detect_describe of one image against the oracle;
    returns (candidates, chunk sizes, kept keypoints)"""
    h, w = img.shape
    assert _serves(w, h, radius, max_kpts)
    cand = K.candidates(oracle, img, thr)
    ref = oracle.detect(img, radius, 0, thr, max_kpts)
    fe = capi.Frontend(w, h, radius, 0, thr, max_kpts, max_candidates=max_candidates)
    cam = K.camera_for(w, h)
    fe.set_camera(0, cam)
    G.assert_keypoints_equal(fe.detect(img), ref)  # map-free
    assert _device_counts(fe)[0] == len(cand)
    fe.set_keep_score_map(True)
    G.assert_keypoints_equal(fe.detect(img), ref)  # through the score map
    assert _device_counts(fe)[0] == len(cand)
    fe.set_keep_score_map(False)
    rays, jac = _maps(w, h)
    rk, rd = oracle.detect_describe(img, radius, 0, thr, max_kpts, oracle.MODE_CAMERA_AWARE, rays, jac,
                                    np.float32(cam.fu), GRAV)
    k, d, _, _ = fe.detect_describe(img, cam=0, gravity=GRAV)
    G.assert_keypoints_equal(k, rk)
    assert np.array_equal(d, rd)
    assert _device_counts(fe)[0] == len(cand)
    sizes = K.chunk_sizes(cand["score"])
    print("candidates", len(cand), "chunks", sizes, "kept", len(ref), "described", len(rk))
    return len(cand), sizes, len(ref)


# ---- candidate-count regimes of the scatter ------------------------------------------------------------------------

def test_one_chunk(oracle):
    img = K.frozen(synth.corners_image(64, 64, 3, cell=8))
    n, sizes, kept = _check_image(oracle, img, 6.0, K.threshold_for(oracle, img, 40), 100, 1 << 12)
    assert n == 40 <= 64 and len(sizes) == 1 and kept > 3


@pytest.mark.parametrize("kind,chunks", [("corners", 2), ("noise", 3)])
def test_two_and_three_chunks(oracle, kind, chunks):
    img = K.frozen(synth.corners_image(96, 64, 3, cell=8) if kind == "corners" else synth.noise_image(96, 64, 3))
    n, sizes, kept = _check_image(oracle, img, 6.0, 40, 200, 1 << 12)
    assert len(sizes) == chunks and 64 < n <= 64 + 128 + 256 and kept > 10


def test_several_full_chunks(oracle):
    """chunks at the 1024-key target, each of several whole buckets"""
    img = K.frozen(synth.noise_image(320, 240, 3))
    n, sizes, kept = _check_image(oracle, img, 12.0, 40, 400, 1 << 13)
    assert n < K.FIRST_RECORDS and len([s for s in sizes if 512 < s <= K.ROUND_CAP]) >= 3 and kept > 50


@pytest.mark.parametrize("count", [K.FIRST_RECORDS - 1, K.FIRST_RECORDS, K.FIRST_RECORDS + 1, K.FIRST_RECORDS + 257])
def test_around_the_register_held_records(oracle, count):
    """5120 candidates are scattered from registers; one more starts the second scatter loop (one lane of it, then
    more than a wave of it)"""
    img = K.frozen(synth.noise_image(384, 288, 5))
    n, sizes, kept = _check_image(oracle, img, 14.0, K.threshold_for(oracle, img, count), 400, 1 << 13)
    assert n == count and len(sizes) >= 8 and kept > 50


def test_more_chunks_than_the_schedule_holds(oracle):
    """every tile's ~1000 tied corners are a bucket and a chunk of their own: more chunk ends than kFuseSched, so the
    rest is one last chunk, larger than a round and split by key range; max_candidates = 0 (the worst-case capacity)"""
    img = K.contrast_tiles()
    n, sizes, kept = _check_image(oracle, img, 38.0, 1, 700, 0)
    assert len(sizes) == K.FUSE_SCHED + 1 and sizes[-1] > K.ROUND_CAP and n > 40000 and kept > 100


def test_noisy_image_at_a_low_threshold_and_worst_case_capacity(oracle):
    """max_candidates = 0 and a noisy 752 x 480 image at a low threshold: 17.7 k candidates, both scatter loops, 24
    chunks (noise spreads over too few buckets to pass the schedule's 40 ends: the tiles above do that)"""
    img = K.frozen(synth.noise_image(752, 480, 8))
    n, sizes, kept = _check_image(oracle, img, 38.0, 1, 700, 0)
    assert n > 3 * K.FIRST_RECORDS and len(sizes) > 20 and kept > 100


@pytest.mark.parametrize("w,h,cell", [(160, 120, 4), (256, 192, 4)])
def test_bucket_of_equal_scores_through_the_key_range_split(oracle, w, h, cell):
    """exact checker content: thousands of candidates tie in ONE bucket = one oversized chunk (below and above the
    register-held 5120)"""
    img = K.checker(w, h, cell)
    n, sizes, kept = _check_image(oracle, img, 10.0, 100, 300, 1 << 13)
    assert sizes == [n] and n > K.ROUND_CAP and (n > K.FIRST_RECORDS) == (w == 256) and kept > 50


def test_overflowing_candidate_list_yields_no_keypoints(oracle):
    img = K.frozen(synth.noise_image(128, 96, 3))
    n = len(K.candidates(oracle, img, 40))
    assert n > 500
    fe = capi.Frontend(128, 96, 8.0, 0, 40, 200, max_candidates=n - 3)
    with pytest.raises(capi.OkvfeError) as e:
        fe.detect(img)
    assert e.value.status == capi.ERR_CAPACITY
    assert _device_counts(fe)[0] >= n - 3  # the count ran past the capacity
    d = torch.from_numpy(img.copy()[None]).cuda()
    fe.detect_describe_batch_device(d.data_ptr(), 1)
    torch.cuda.synchronize()
    assert _download(fe, 0) is None  # reported, and nothing kept on the device
    assert _device_counts(fe, 1, "detect_counts")[0] == 0 and _device_counts(fe, 1, "counts")[0] == 0
    # one candidate fewer than the capacity allows is selected as usual
    _check_image(oracle, img, 8.0, 40, 200, n)


def test_empty_image(oracle):
    img = K.frozen(np.full((64, 64), 128, np.uint8))
    n, sizes, kept = _check_image(oracle, img, 6.0, 40, 100, 1 << 12)
    assert n == 0 and sizes == [] and kept == 0


# ---- batches: the regimes side by side, determinism ----------------------------------------------------------------

BW, BH, BRADIUS, BTHR, BKPTS = 384, 288, 14.0, 1, 400


@functools.lru_cache(maxsize=None)
def _pool():
    """eight images of one size, one regime each; the capacity of the batch context lets all but the full noise image
    through"""
    full = synth.noise_image(BW, BH, 5)
    patched = full.copy()
    patched[:40, :60] = 128
    window = np.full((BH, BW), 128, np.uint8)
    window[100:164, 100:164] = synth.noise_image(64, 64, 9)
    return {
        "empty": K.frozen(np.full((BH, BW), 128, np.uint8)),
        "one chunk": K.blob(BW, BH),
        "two chunks": K.frozen(synth.corners_image(BW, BH, 3, cell=32, noise=0)),
        "second loop": K.frozen(patched),
        "equal scores": K.checker(BW, BH, 8),
        "overflow": K.frozen(full),
        "four chunks": K.frozen(synth.corners_image(BW, BH, 3, cell=16, noise=0)),
        "three chunks": K.frozen(window),
    }


GROUPS = {"a": ("empty", "one chunk", "two chunks", "second loop"),
          "b": ("equal scores", "overflow", "four chunks", "three chunks")}


@functools.lru_cache(maxsize=None)
def _pool_reference(name):
    """(candidates, chunk sizes, keypoints, descriptors) of a pool image: computed once, shared, never changed"""
    import oracle_lib as O
    img = _pool()[name]
    cand = K.candidates(O, img, BTHR)
    cam = K.camera_for(BW, BH)
    rays, jac = _maps(BW, BH)
    rk, rd = O.detect_describe(img, BRADIUS, 0, BTHR, BKPTS, O.MODE_CAMERA_AWARE, rays, jac, np.float32(cam.fu), GRAV)
    for a in (rk, rd):
        a.setflags(write=False)
    return len(cand), K.chunk_sizes(cand["score"]), rk, rd


def _batch_capacity():
    return _pool_reference("overflow")[0] - 2


def _batch_frontend():
    assert _serves(BW, BH, BRADIUS, BKPTS)
    fe = capi.Frontend(BW, BH, BRADIUS, 0, BTHR, BKPTS, max_batch=4, max_candidates=_batch_capacity())
    fe.set_camera(0, K.camera_for(BW, BH))
    return fe


def _run_batch(fe, names, stream=None):
    imgs = np.stack([_pool()[n] for n in names])
    d = torch.from_numpy(imgs).cuda()
    grav = np.tile(np.array(GRAV, dtype=np.float32), (len(names), 1))
    fe.detect_describe_batch_device(d.data_ptr(), len(names), np.zeros(len(names), np.int32), grav,
                                    stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    kept = _device_counts(fe, len(names), "detect_counts")
    got = [_download(fe, i) for i in range(len(names))]
    assert all((g is None and kept[i] == 0) or len(g[0]) <= kept[i] for i, g in enumerate(got))
    return got, _device_counts(fe, len(names))


def test_the_pool_reaches_its_regimes():
    cap = _batch_capacity()
    want = {"empty": 0, "one chunk": 1, "two chunks": 2, "three chunks": 3, "four chunks": 4}
    for name, chunks in want.items():
        assert len(_pool_reference(name)[1]) == chunks, name
    n, sizes, _, _ = _pool_reference("second loop")
    assert K.FIRST_RECORDS < n <= cap and len(sizes) >= 8
    n, sizes, _, _ = _pool_reference("equal scores")
    assert sizes == [n] and K.ROUND_CAP < n <= cap
    assert _pool_reference("overflow")[0] > cap


@pytest.mark.parametrize("group", ["a", "b"])
@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_regimes_mixed_in_one_batch(group, order):
    names = GROUPS[group] if order == "forward" else GROUPS[group][::-1]
    fe = _batch_frontend()
    got, counts = _run_batch(fe, names)
    for i, name in enumerate(names):
        n, _, rk, rd = _pool_reference(name)
        if name == "overflow":  # which maxima were dropped is not defined: the image keeps nothing, and says so
            assert counts[i] > _batch_capacity() and got[i] is None
            continue
        k, d = got[i]
        assert counts[i] == n, name
        G.assert_keypoints_equal(k, rk)
        assert np.array_equal(d, rd), name
    if "overflow" in names:
        with pytest.raises(capi.OkvfeError) as e:
            fe.check_capacity(len(names))
        assert e.value.status == capi.ERR_CAPACITY
    else:
        fe.check_capacity(len(names))


@pytest.mark.parametrize("group", ["a", "b"])
def test_same_call_twice_and_on_two_streams(group):
    """arrival order inside a chunk must not leak: identical bytes from a repetition and from another stream"""
    names = GROUPS[group]
    fe = _batch_frontend()
    first, c1 = _run_batch(fe, names)
    again, c2 = _run_batch(fe, names)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    on_s1, c3 = _run_batch(fe, names, s1.cuda_stream)
    other = _batch_frontend()
    on_s2, c4 = _run_batch(other, names, s2.cuda_stream)
    for run, c in ((again, c2), (on_s1, c3), (on_s2, c4)):
        assert np.array_equal(c, c1)
        for a, b in zip(first, run):
            assert (a is None) == (b is None)
            assert a is None or (a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes())
    assert sum(len(g[0]) for g in first if g is not None) > 300  # not vacuous


# ---- the tail's read-back of kept records (the caller of refine_emit reads the record, one lane per keypoint, 256 per
# pass): one keypoint short of a pass, a full pass, one and 44 into the second; a large image at radius 50 ----------------

@pytest.mark.parametrize("cap", [255, 256, 257, 300])
def test_kept_keypoints_around_256(oracle, cap):
    cfg = synth.euroc_config()
    img = K.frozen(synth.corners_image(cfg.w, cfg.h, 77, cell=12, levels=(0, 255), noise=0, jitter=0))
    n, sizes, kept = _check_image(oracle, img, cfg.uniformity_radius, cfg.abs_threshold, cap, 1 << 15)
    assert kept == cap  # supply exceeds the cap


def test_one_1024_square_image_at_radius_50(oracle):
    cfg = synth.tumvi1024_config()
    img = K.frozen(synth.corners_image(cfg.w, cfg.h, 5))
    n, sizes, kept = _check_image(oracle, img, cfg.uniformity_radius, cfg.abs_threshold, cfg.max_kpts, 1 << 14)
    assert n > K.FIRST_RECORDS and kept > 256


def test_six_euroc_images_per_cu():
    """select_lazy_kernel<true> at EuRoC's dynamic LDS: six workgroups per CU, as the runtime counts them (its six
    waves per SIMD and 6 x (26 560 + 240 B static) of the CU's 160 KiB); 512 bytes more would cost the sixth"""
    cfg = synth.euroc_config()
    array, _, lds = _plan(cfg.w, cfg.h, cfg.uniformity_radius, cfg.max_kpts)
    assert array and lds == 26560
    occ = _lab().okvfe_lab_select_occupancy
    occ.restype = C.c_int32
    assert occ(lds) == 6
    assert occ(lds + 512) == 5
