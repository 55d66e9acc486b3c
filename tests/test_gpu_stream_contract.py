"""GPU: the stream-ordering contract of a context (include/okvfe.h, okvfe_set_internal_lanes / okvfe_lanes_join).

A matrix of "call X is in flight on caller stream A, then consumer Y runs", at the size of the bench's pipelined-lanes
leg: EuRoC 752x480, 256 stereo frames (512 images), okvfe_set_internal_lanes(-4) (lane chunk 128 images).

* Expected bytes: the same inputs through the same context with lanes off, read after a device synchronisation;
  the 8 distinct stereo frames of the batch are anchored to the CPU oracle (keypoints, descriptors, FP64 back-
  projections as u64 patterns, match rows).  B = 1 rows compare with the oracle directly.
* Stale results look different: before each row the same call runs on other content (the images mirrored) and is
  host-joined, so a read that comes too early returns other bytes, not the right ones by luck.
* The lanes are held back: a bounded spin (matrix products, ~40 ms) on A just before the call under test.  The
  lanes start behind `lane_fork`, recorded on A behind the spin, so anything not ordered behind the lanes runs first
  and sees the old content -- a missing join fails every run instead of now and then.
* Caller streams are torch.cuda.Stream objects, not the legacy default stream (whose implicit ordering with
  synchronous copies would hide the camera rows).
* Separate hardware queues: under the runtime's default of 4 hardware queues per process, the dozen streams in play
  here share queues, and a queue runs its packets in submission order -- which orders by accident what the library
  forgot to order (the rows then pass without their joins).  test_matrix_on_separate_hardware_queues runs the whole
  matrix again in a fresh process with GPU_MAX_HW_QUEUES=16, where every stream has a queue of its own.
"""
import ctypes as C
import dataclasses
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import gpu_common as G
from okvis2_amd import capi, multigpu, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FRAMES, DISTINCT, LANES = 256, 8, -4
N = 2 * FRAMES
SPIN_MS = 40.0


def _copy_to_host(dst, ptr, stream):
    st = capi.lib().okvfe_copy_to_host(C.c_void_p(dst.ctypes.data), C.c_void_p(ptr), C.c_size_t(dst.nbytes),
                                       capi._s(stream))
    assert st == capi.OK


class Env:
    pass


@pytest.fixture(scope="module")
def env(oracle):
    import bench
    e = Env()
    cfg = e.cfg = synth.euroc_config()
    imgs, base = bench.make_inputs(cfg, FRAMES, DISTINCT, 5151)
    e.base = base
    fe = e.fe = G.make_frontend(cfg, max_batch=N, num_cameras=2)
    for ci, cam in enumerate(cfg.cams):
        fe.set_camera(ci, cam)
    K = e.K = fe.max_keypoints
    g16 = np.stack([[0.03 * ((i % 5) - 2), 1.0, 0.02 * ((i % 3) - 1)] for i in range(2 * DISTINCT)])
    e.g16 = g16 = (g16 / np.linalg.norm(g16, axis=1, keepdims=True)).astype(np.float32)
    e.grav = np.concatenate([g16] * (FRAMES // DISTINCT))
    e.cam_ids = np.array([0, 1] * FRAMES, dtype=np.int32)
    e.T0, e.T1 = synth.stereo_poses(cfg.baseline)
    e.f = [0.5 * (c.fu + c.fv) for c in cfg.cams]
    arr = []
    for i in range(FRAMES):
        sp = capi.StereoPair()
        sp.image0, sp.image1 = 2 * i, 2 * i + 1
        sp.T_WC0, sp.T_WC1 = capi.make_pose(*e.T0), capi.make_pose(*e.T1)
        sp.f0, sp.f1 = e.f[0], e.f[1]
        arr.append(sp)
    e.pairs = (capi.StereoPair * FRAMES)(*arr)
    e.d_img = torch.from_numpy(imgs).cuda()
    e.d_flip = torch.flip(e.d_img, dims=[2]).contiguous()  # the stale content of every row
    e.d_match = torch.zeros((FRAMES, K, capi.STEREO_MATCH_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    e.A, e.B, e.Cs = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    e.out = fe.device_outputs()  # (the pointers stay: rows read them on streams of their own)
    # the spin: a chain of 2048^2 matrix products on A, as many as take ~SPIN_MS (timed with events on A)
    e.spin_x = torch.randn((2048, 2048), device="cuda")
    e.spin_y = torch.empty_like(e.spin_x)
    e.spin_reps = 4
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(2):  # (the first round warms the BLAS up)
        t0.record(e.A)
        _spin(e, e.A)
        t1.record(e.A)
        e.A.synchronize()
    ms = max(t0.elapsed_time(t1), 1e-3)
    e.spin_reps = int(min(max(e.spin_reps * SPIN_MS / ms, 4), 4096))
    t0.record(e.A)
    _spin(e, e.A)
    t1.record(e.A)
    e.A.synchronize()
    e.spin_ms = t0.elapsed_time(t1)
    print(f"spin: {e.spin_reps} products, {e.spin_ms:.1f} ms")
    assert e.spin_ms > 0.5 * SPIN_MS

    # ---- expected bytes: lanes off, device-synchronised
    fe.set_internal_lanes(0)
    e.E, e.M = _unsplit(e, e.d_img)
    e.EF, e.MF = _unsplit(e, e.d_flip)
    maps = [oracle.awareness_maps(c) for c in cfg.cams]
    e.maps = maps
    for b in range(DISTINCT):
        side = []
        for c in range(2):
            i = 2 * b + c
            k, d = oracle.detect_describe(base[i], cfg.uniformity_radius, 0, cfg.abs_threshold, cfg.max_kpts,
                                          oracle.MODE_CAMERA_AWARE, maps[c][0], maps[c][1], np.float32(cfg.cams[c].fu),
                                          tuple(float(v) for v in g16[i]))
            bp, bv = oracle.backproject_keypoints(cfg.cams[c], k)
            gk, gd, gbp, gbv = _image(e.E, i)
            G.assert_keypoints_equal(gk, k)
            assert np.array_equal(gd, d)
            assert np.array_equal(gbp.view(np.uint64), bp.view(np.uint64)) and np.array_equal(gbv, bv)
            side.append((k, d, bp, bv))
        (k0, d0, b0, v0), (k1, d1, b1, v1) = side
        m = oracle.match_stereo(d0, k0, b0, v0, d1, k1, b1, v1, e.T0, e.T1, e.f[0], e.f[1], cfg.match_threshold)
        assert _rows(e.M, e.E, b).tobytes() == np.ascontiguousarray(m).tobytes(), b
    # replicas of the distinct frames are the distinct frames' bytes
    for i in range(2 * DISTINCT, N):
        assert _same_image(e.E, e.E, i, i % (2 * DISTINCT)), i
    # every image reads differently from its stale (mirrored) counterpart
    assert all(e.E["counts"][i] > 100 for i in range(N))
    assert not any(_same_image(e.E, e.EF, i) for i in range(N))
    fe.set_internal_lanes(LANES)
    yield e
    torch.cuda.synchronize()
    fe.close()


def _read(e, stream=None, n=N):
    """Raw results of images [0, n) through okvfe_get_device_outputs' pointers, copied on `stream`."""
    K, o = e.K, e.out
    r = {"counts": np.zeros(n, np.int32), "kps": np.zeros((n, K), capi.KEYPOINT_DTYPE),
         "desc": np.zeros((n, K, 48), np.uint8), "bp": np.zeros((n, K, 3), np.float64), "bpv": np.zeros((n, K), np.uint8)}
    for name, ptr in (("counts", o.counts), ("kps", o.keypoints), ("desc", o.descriptors), ("bp", o.backproj),
                      ("bpv", o.backproj_valid)):
        _copy_to_host(r[name], ptr, stream)
    if stream is None:
        torch.cuda.synchronize()
    else:
        stream.synchronize()
    return r


def _image(r, i):
    n = int(r["counts"][i])
    return r["kps"][i, :n], r["desc"][i, :n], r["bp"][i, :n], r["bpv"][i, :n]


def _same_image(r, q, i, j=None):
    j = i if j is None else j
    return all(np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
               for a, b in zip(_image(r, i), _image(q, j)))


def _diff(r, q, images):
    return [i for i in images if not _same_image(r, q, i)]


def _rows(m, r, f):
    return m[f, :int(r["counts"][2 * f])].copy()


def _match_rows(d_match):
    return d_match.cpu().numpy().view(capi.STEREO_MATCH_DTYPE).reshape(FRAMES, -1)


def _unsplit(e, img):
    e.fe.detect_describe_batch_device(img.data_ptr(), N, e.cam_ids, e.grav, e.A)
    e.fe.match_stereo_batch_device(e.pairs, e.d_match.data_ptr(), e.A)
    torch.cuda.synchronize()
    e.fe.check_capacity(N)
    return _read(e), _match_rows(e.d_match)


def _call(e, img, stream, n=N, match=True):
    e.fe.detect_describe_batch_device(img.data_ptr(), n, e.cam_ids[:n], e.grav[:n], stream)
    if match:
        e.fe.match_stereo_batch_device((capi.StereoPair * (n // 2))(*e.pairs[:n // 2]), e.d_match.data_ptr(), stream)


def _spin(e, stream, ms=SPIN_MS):
    """Bounded work on a caller stream (~ms, at most 8x SPIN_MS) that holds back everything queued behind it there."""
    reps = int(e.spin_reps * min(ms, 8 * SPIN_MS) / SPIN_MS)
    with torch.cuda.stream(stream):
        for _ in range(reps):
            torch.mm(e.spin_x, e.spin_x, out=e.spin_y)


def _host_join(e):
    e.fe.device_outputs()  # a host-side reader: synchronises the lanes
    torch.cuda.synchronize()


def _prime(e):
    """The same call on the mirrored content, host-joined: what a read that comes too early returns."""
    _call(e, e.d_flip, e.A)
    _host_join(e)


def _check_all(e, what):
    """After a host join: the call under test left the expected bytes everywhere."""
    _host_join(e)
    r = _read(e)
    bad = _diff(r, e.E, range(N))
    assert not bad, f"{what}: {len(bad)} images differ from the unsplit call after a host join, first {bad[:8]}"
    m = _match_rows(e.d_match)
    badm = [f for f in range(FRAMES) if _rows(m, e.E, f).tobytes() != _rows(e.M, e.E, f).tobytes()]
    assert not badm, f"{what}: match rows of {len(badm)} frames differ, first {badm[:8]}"


SAMPLE = [0, 1, 64, 127, 128, 129, 200, 255, 256, 300, 383, 384, 385, 450, 510, 511]  # every lane's slice


# ---- controls ------------------------------------------------------------------------------------------------------
def test_control_join_on_the_calls_stream(env):
    e = env
    _prime(e)
    _spin(e, e.A)
    _call(e, e.d_img, e.A)
    e.fe.lanes_join(e.A)
    e.A.synchronize()
    bad = [i for i in SAMPLE if not _same_image(_dl(e, i), e.E, 0, i)]
    assert not bad, bad
    _check_all(e, "control")


def test_control_event_to_another_stream(env):
    """lanes_join(A), an event on A, stream C waits for it and reads the outputs with copies of its own."""
    e = env
    _prime(e)
    _spin(e, e.A)
    _call(e, e.d_img, e.A)
    e.fe.lanes_join(e.A)
    ev = torch.cuda.Event()
    ev.record(e.A)
    e.Cs.wait_event(ev)
    r = _read(e, e.Cs)
    with torch.cuda.stream(e.Cs):
        m = e.d_match.clone()
    e.Cs.synchronize()
    assert not _diff(r, e.E, range(N))
    m = m.cpu().numpy().view(capi.STEREO_MATCH_DTYPE).reshape(FRAMES, -1)
    assert all(_rows(m, e.E, f).tobytes() == _rows(e.M, e.E, f).tobytes() for f in range(FRAMES))
    _host_join(e)


def _dl(e, i):
    """okvfe_download_image_result(i) as a one-image result record (counts / kps / desc / bp / bpv of image 0)."""
    k, d, bp, bv = e.fe.download(i)
    n = len(k)
    return {"counts": np.array([n], np.int32), "kps": k[None], "desc": d[None], "bp": bp[None], "bpv": bv[None]}


# ---- H: host readers after a join on another stream ----------------------------------------------------------------
@pytest.mark.parametrize("join_on", ["other_stream", "context_stream", "legacy_default"])
def test_h1_download_after_join_on_another_stream(env, join_on):
    """okvfe_lanes_join(ctx, B / NULL / the legacy default stream) orders that stream only; okvfe_download_image_result
    must still wait for the lanes (no device synchronisation in between)."""
    e = env
    _prime(e)
    _spin(e, e.A)
    _call(e, e.d_img, e.A)
    e.fe.lanes_join({"other_stream": e.B, "context_stream": None,
                     "legacy_default": torch.cuda.default_stream()}[join_on])
    bad = [i for i in SAMPLE if not _same_image(_dl(e, i), e.E, 0, i)]
    assert not bad, f"download read images {bad} before the lanes had written them"
    _check_all(e, "h1")


def test_h2_check_capacity_after_join_on_another_stream(env, oracle):
    """An NMS candidate list that overflows in a pipelined call is reported by okvfe_check_capacity after a join on
    another stream."""
    e = env
    cfg = e.cfg
    n = 256
    busy = synth.noise_image(cfg.w, cfg.h, 3)
    assert len(oracle.nms(oracle.harris_score(busy), cfg.abs_threshold)) > 8000
    fe = G.make_frontend(cfg, max_batch=n, num_cameras=2, max_candidates=8000)
    try:
        for ci, cam in enumerate(cfg.cams):
            fe.set_camera(ci, cam)
        fe.set_internal_lanes(LANES)
        calm = e.d_img[:n]
        hot = calm.clone()
        hot[150] = torch.from_numpy(busy).cuda()
        torch.cuda.synchronize()
        fe.detect_describe_batch_device(calm.data_ptr(), n, e.cam_ids[:n], e.grav[:n], e.A)
        fe.device_outputs()
        fe.check_capacity(n)  # the stale state has no overflow
        _spin(e, e.A)
        fe.detect_describe_batch_device(hot.data_ptr(), n, e.cam_ids[:n], e.grav[:n], e.A)
        fe.lanes_join(e.B)
        with pytest.raises(capi.OkvfeError) as err:
            fe.check_capacity(n)
        assert err.value.status == capi.ERR_CAPACITY and "image 150" in str(err.value)
        torch.cuda.synchronize()
    finally:
        torch.cuda.synchronize()
        fe.close()


def _swapped_pattern(p):
    q = capi.PatternData()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(p))
    for b in range(p.n_short):
        q.short_i[b], q.short_j[b] = p.short_j[b], p.short_i[b]
    return q


def test_h3_set_pattern_applies_to_later_calls(env):
    e = env
    fe = e.fe
    P1 = fe.get_pattern()
    P2 = _swapped_pattern(P1)
    try:
        _prime(e)
        _spin(e, e.A)
        _call(e, e.d_img, e.A)
        fe.lanes_join(e.B)
        fe.set_pattern(P2)
        torch.cuda.synchronize()
        r = _read(e)
        bad = _diff(r, e.E, range(N))
        assert not bad, f"the call in flight took the new pattern for {len(bad)} images, first {bad[:8]}"
        _call(e, e.d_img, e.A)
        _host_join(e)
        r2 = _read(e)
        assert np.array_equal(r2["counts"], e.E["counts"])
        assert all(_image(r2, i)[0].tobytes() == _image(e.E, i)[0].tobytes() for i in range(N))
        assert all(_image(r2, i)[1].tobytes() != _image(e.E, i)[1].tobytes() for i in range(N))
        fe.set_internal_lanes(0)  # the next call's bytes: the unsplit call under P2
        _call(e, e.d_img, e.A, match=False)
        torch.cuda.synchronize()
        assert not _diff(_read(e), r2, range(N))
    finally:
        torch.cuda.synchronize()
        fe.set_internal_lanes(LANES)
        fe.set_pattern(P1)


def test_h4_profile_read_after_join_on_another_stream(env):
    e = env
    fe = e.fe
    _prime(e)
    fe.profile_enable(True)
    try:
        _spin(e, e.A)
        _call(e, e.d_img, e.A)
        fe.lanes_join(e.B)
        prof = fe.profile_read()
        assert prof["match"][1] == 4 and prof["describe"][1] >= 4, prof  # (one matcher launch per lane)
        assert prof["describe"][0] > 0.0
    finally:
        torch.cuda.synchronize()
        fe.profile_enable(False)
    _check_all(e, "h4")


# ---- B: the B = 1 entry points while lanes are pending ------------------------------------------------------------
def _b1_reference(e, oracle, i=2, cam=0):
    cfg = e.cfg
    g = tuple(float(v) for v in e.g16[i])
    k, d = oracle.detect_describe(e.base[i], cfg.uniformity_radius, 0, cfg.abs_threshold, cfg.max_kpts,
                                  oracle.MODE_CAMERA_AWARE, e.maps[cam][0], e.maps[cam][1],
                                  np.float32(cfg.cams[cam].fu), g)
    bp, bv = oracle.backproject_keypoints(cfg.cams[cam], k)
    return e.base[i], g, (k, d, bp, bv)


def _assert_result(got, ref):
    G.assert_keypoints_equal(got[0], ref[0])
    assert np.array_equal(got[1], ref[1])
    assert np.array_equal(got[2].view(np.uint64), ref[2].view(np.uint64)) and np.array_equal(got[3], ref[3])


def test_b1_detect_while_lanes_run(env, oracle):
    """okvfe_detect (B = 1) while the lanes of a pipelined call run (no spin, no join): its keypoints equal the oracle,
    and the pipelined call's own results are intact afterwards.  A race, not held back: a guard, not a detector."""
    e = env
    img = e.base[2]
    ref = oracle.detect(img, e.cfg.uniformity_radius, 0, e.cfg.abs_threshold, e.cfg.max_kpts)
    _prime(e)
    _call(e, e.d_img, e.A)
    got = e.fe.detect(img)
    G.assert_keypoints_equal(got, ref)
    _check_all(e, "b1")


def test_b2_detect_ahead_compute_and_detect_describe(env, oracle):
    """After a join on another stream, the B = 1 extractor calls run behind the held-back lanes: what they leave in the
    context (the detect-ahead state, the result okvfe_download_image_result reads) is theirs, not lane 0's."""
    e = env
    fe = e.fe
    img, g, ref = _b1_reference(e, oracle)
    ref_det = oracle.detect(img, e.cfg.uniformity_radius, 0, e.cfg.abs_threshold, e.cfg.max_kpts)
    _prime(e)
    _spin(e, e.A)
    _call(e, e.d_img, e.A)
    fe.lanes_join(e.B)
    kps = fe.detect_ahead(img, 0, g)
    G.assert_keypoints_equal(kps, ref_det)
    torch.cuda.synchronize()
    _assert_result(fe.compute(img, kps, 0, g), ref)
    _prime(e)
    _spin(e, e.A)
    _call(e, e.d_img, e.A)
    fe.lanes_join(e.B)
    _assert_result(fe.detect_describe(img, 0, g), ref)
    torch.cuda.synchronize()
    _assert_result(fe.download(0), ref)
    _host_join(e)


# ---- S: stream-taking entry points on a stream the caller did not order ---------------------------------------------
def test_s1_gather_blocks_and_block_matcher_on_another_stream(env):
    e = env
    fe = e.fe
    nb = fe.gather_block_bytes()
    blocks = torch.zeros((N, nb), dtype=torch.uint8, device="cuda")
    d_m2 = torch.zeros_like(e.d_match)
    torch.cuda.synchronize()
    _prime(e)
    _spin(e, e.A)
    _call(e, e.d_img, e.A)
    fe.lanes_join(e.B)
    C_ = e.Cs
    fe.pack_gather_blocks_device(0, N, blocks.data_ptr(), C_)
    with torch.cuda.stream(C_):
        bl, br = blocks[0::2].contiguous(), blocks[1::2].contiguous()
    fe.match_stereo_blocks_batch_device(bl.data_ptr(), br.data_ptr(), FRAMES, e.T0, e.T1, e.f[0], e.f[1],
                                        d_m2.data_ptr(), C_)
    C_.synchronize()
    hb = blocks.cpu().numpy()
    bad = [i for i in range(N) if not all(a.tobytes() == b.tobytes() for a, b in
                                          zip(multigpu.unpack_block_host(hb[i], e.K), _image(e.E, i)))]
    assert not bad, f"gather blocks of {len(bad)} images are not the call's results, first {bad[:8]}"
    m = _match_rows(d_m2)
    badm = [f for f in range(FRAMES) if _rows(m, e.E, f).tobytes() != _rows(e.M, e.E, f).tobytes()]
    assert not badm, f"block matcher rows of {len(badm)} frames differ, first {badm[:8]}"
    _check_all(e, "s1")
    del bl, br


def test_s2_resliced_pipelined_call_on_another_stream(env):
    """A pipelined call of 512 images (dense mirrored content in lane 0's slice, blank images after it), a join on B,
    then a pipelined call of 384 images (chunk 96 instead of 128) on C: its lanes must not write the ranges the old
    lanes still work on."""
    e = env
    old = torch.zeros_like(e.d_img)
    old[:128] = e.d_flip[:128]
    torch.cuda.synchronize()
    _prime(e)
    _spin(e, e.A)
    _call(e, old, e.A, match=False)
    e.fe.lanes_join(e.B)
    _call(e, e.d_img, e.Cs, n=384, match=False)
    _host_join(e)
    r = _read(e)
    bad = _diff(r, e.E, range(384))
    assert not bad, f"{len(bad)} images of the re-sliced call differ, first {bad[:8]}"
    assert np.all(r["counts"][384:] == 0)
    del old


# ---- C: camera changes while a call is queued ----------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [0, LANES], ids=["unsplit", "pipelined"])
@pytest.mark.parametrize("how", ["set_camera_maps", "set_camera"])
def test_c_camera_change_applies_to_later_calls(env, oracle, how, lanes):
    """okvfe_set_camera_maps / okvfe_set_camera while a call of the old camera is queued on A: the queued call keeps the
    old maps (and intrinsics), the next call takes the new ones.  The hold-back outlasts the host work that runs before
    the first write to the device: set_camera_maps gets maps built beforehand (its writes follow within microseconds);
    set_camera builds the maps of 752x480 pixels on the host first, so its row spins for that time (measured by
    re-installing the current camera) plus SPIN_MS."""
    e = env
    fe = e.fe
    c0 = e.cfg.cams[0]
    new = dataclasses.replace(c0, fu=c0.fu * 1.04, fv=c0.fv * 1.04, cu=c0.cu + 5.0)
    rays, jac = oracle.awareness_maps(new)
    spin_ms = SPIN_MS
    if how == "set_camera":
        torch.cuda.synchronize()
        t = time.perf_counter()
        fe.set_camera(0, c0)  # (the same host work as the change below)
        spin_ms += 1e3 * (time.perf_counter() - t)
    try:
        fe.set_internal_lanes(lanes)
        _prime(e)
        _spin(e, e.A, spin_ms)
        _call(e, e.d_img, e.A, match=lanes != 0)
        if how == "set_camera":
            fe.set_camera(0, new)
        else:
            fe.set_camera_maps(0, rays, jac, new.fu)
        torch.cuda.synchronize()
        r = _read(e)
        bad = _diff(r, e.E, range(N))
        assert not bad, f"the call in flight took the new camera for {len(bad)} images, first {bad[:8]}"
        _call(e, e.d_img, e.A, match=False)
        _host_join(e)
        r2 = _read(e)
        assert not _diff(r2, e.E, range(1, N, 2))  # camera 1 did not change
        # the new maps change every camera-0 descriptor set; new intrinsics (set_camera) every back-projection
        assert all(_image(r2, i)[1].tobytes() != _image(e.E, i)[1].tobytes() for i in range(0, N, 2))
        if how == "set_camera":
            assert all(_image(r2, i)[2].tobytes() != _image(e.E, i)[2].tobytes() for i in range(0, N, 2))
        k, d = oracle.detect_describe(e.base[0], e.cfg.uniformity_radius, 0, e.cfg.abs_threshold, e.cfg.max_kpts,
                                      oracle.MODE_CAMERA_AWARE, rays, jac, np.float32(new.fu),
                                      tuple(float(v) for v in e.g16[0]))
        bp, bv = oracle.backproject_keypoints(new if how == "set_camera" else c0, k)
        _assert_result(_image(r2, 0), (k, d, bp, bv))
    finally:
        torch.cuda.synchronize()
        fe.set_camera(0, c0)
        fe.set_internal_lanes(LANES)


# ---- M: the per-stream workspace of the map matcher ----------------------------------------------------------------
def test_m1_map_blocks_across_ten_streams(oracle):
    """okvfe_match_to_map_blocks_device on 10 caller streams in turn (the 9th and 10th evict the oldest per-stream
    workspaces), the first two held back by a spin so that calls are in flight across the evictions, ragged n_frames:
    every call's rows equal the oracle."""
    cfg = synth.euroc_config()
    fe = G.make_frontend(cfg)
    K = fe.max_keypoints
    rng = np.random.default_rng(77)
    sizes = [650, 0, 333, K]
    cam = cfg.cams[0]
    frames = []
    for n in sizes:
        kps = np.zeros(n, dtype=oracle.KEYPOINT_DTYPE)
        kps["x"] = rng.uniform(30, 720, n)
        kps["y"] = rng.uniform(30, 450, n)
        desc = rng.integers(0, 256, (n, 48), dtype=np.uint8)
        bp, bv = oracle.backproject_keypoints(cam, kps) if n else (np.zeros((0, 3)), np.zeros(0, np.uint8))
        frames.append((kps, desc, bp, bv))
    nf, n_lm = len(frames), 1500
    counts = rng.integers(1, 4, n_lm)
    desc_begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    pool = rng.integers(0, 256, (desc_begin[-1], 48), dtype=np.uint8)
    proj = np.stack([np.stack([rng.uniform(0, 752, n_lm), rng.uniform(0, 480, n_lm)], 1) for _ in range(nf)])
    use = (rng.random((nf, K)) > 0.15).astype(np.uint8)
    for f, (kps, desc, _, _) in enumerate(frames):  # plant matches
        for l in range(0, min(len(kps), n_lm), 2):
            proj[f, l] = (kps["x"][l] + rng.normal(0, 3), kps["y"][l] + rng.normal(0, 3))
            pool[desc_begin[l]] = desc[l] ^ ((rng.random(48) < 0.05) * rng.integers(0, 256, 48)).astype(np.uint8)
    thr = 20.0
    ref = [oracle.match_to_map(desc, kps, use[f, :len(kps)], proj[f], desc_begin, pool, thr, cfg.match_threshold)
           for f, (kps, desc, _, _) in enumerate(frames)]
    assert sum(int((rl >= 0).sum()) for rl, _ in ref) > 150
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d_blocks = dev(np.stack([multigpu.pack_block_host(K, *fr) for fr in frames]))
    d_use, d_begin, d_pool, d_proj = dev(use), dev(desc_begin), dev(pool), dev(proj)
    md = fe.make_map_device(n_lm, d_begin.data_ptr(), d_pool.data_ptr(), d_proj.data_ptr())
    streams = [torch.cuda.Stream() for _ in range(10)]
    x = torch.randn((2048, 2048), device="cuda")
    y = torch.empty_like(x)
    outs = [(torch.full((nf, K), -7, dtype=torch.int32, device="cuda"),
             torch.full((nf, K), -7, dtype=torch.int32, device="cuda")) for _ in streams]
    torch.cuda.synchronize()
    try:
        for i, st in enumerate(streams):
            if i < 2:
                with torch.cuda.stream(st):
                    for _ in range(64):
                        torch.mm(x, x, out=y)
            n_frames = 1 + (i * 3) % nf  # ragged: 1, 4, 3, 2, 1, ...
            fe.match_to_map_blocks_device(d_blocks.data_ptr(), n_frames, d_use.data_ptr(), md, thr,
                                          outs[i][0].data_ptr(), outs[i][1].data_ptr(), st)
        torch.cuda.synchronize()
        for i in range(len(streams)):
            n_frames = 1 + (i * 3) % nf
            lm, bd = outs[i][0].cpu().numpy(), outs[i][1].cpu().numpy()
            for f in range(nf):
                n = len(frames[f][0])
                if f < n_frames:
                    assert np.array_equal(lm[f, :n], ref[f][0]) and np.array_equal(bd[f, :n], ref[f][1]), (i, f)
                assert np.all(lm[f, n if f < n_frames else 0:] == -7), (i, f)
    finally:
        torch.cuda.synchronize()
        fe.close()


# ---- the matrix with one hardware queue per stream ------------------------------------------------------------------
def test_matrix_on_separate_hardware_queues():
    """Every row above in a fresh process with GPU_MAX_HW_QUEUES=16: no two streams of the matrix share a hardware
    queue, so nothing but the library's own waits orders the lanes against the consumers."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "-m", "gpu",
                          "-k", "not separate_hardware_queues", os.path.abspath(__file__)],
                         cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and " passed" in out.stdout and "failed" not in out.stdout, \
        out.stdout[-4000:] + out.stderr[-2000:]
