"""GPU: the keypoint coverage masks of Frontend::doWeNeedANewKeyframe (okvfe_keyframe_coverage_blocks_device and its
B = 1 host seam okvfe_keyframe_coverage; Frontend.cpp:1074-1101, :1123-1149) against the numpy restatement in
keyframe_ref.py, which paints real u8 masks disc by disc.  All six fields of every record must be EQUAL: the
quantities are integers, nothing is tolerance-compared.

PARITY UNPINNED: cv::circle and the point rounding are restated from OpenCV's published source (OpenCV is neither in
the reference tree nor installed), so "equal" means equal to that restatement, not to a cv build.

Dense frames saturate the mask (700 random keypoints cover all 3600 pixels of the 48 x 75 EuRoC mask), so the sparse
frames (0, 1, 20, 226 keypoints) are the ones that discriminate; they are part of every batch."""
import numpy as np
import pytest

import gpu_common as G
import keyframe_ref as R
from okvis2_amd import capi, multigpu, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CONFIGS = {"euroc": (synth.euroc_config, 4), "tumvi1024": (synth.tumvi1024_config, 9),
           "hilti": (synth.hilti_config, 4), "mono640": (synth.mono640_config, 4)}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _frame(rng, w, h, n, frac):
    kps = np.zeros(n, dtype=capi.KEYPOINT_DTYPE)
    kps["x"] = rng.uniform(0, w - 0.5, n)
    kps["y"] = rng.uniform(0, h - 0.5, n)
    if n >= 20:  # the half-way values (cvRound: half to even), the far rim (centre outside the mask), the origin
        kps["x"][:8] = (5, 15, 25, 35, w - 0.5, 0, 45, w - 0.5)
        kps["y"][:8] = (5, 15, 35, 25, h - 0.5, 0, h - 0.5, 65)
    ids = rng.integers(1, 1 << 62, n).astype(np.uint64)
    ids[rng.random(n) >= frac] = 0
    if n > 40:
        ids[30:34] = ids[34]  # one landmark seen by several keypoints
    return kps, ids


def _batch(cfg, K, seed):
    rng = np.random.default_rng(seed)
    frames = [_frame(rng, cfg.w, cfg.h, n, frac) for frac in (0.0, 0.4, 1.0) for n in (0, 1, 20, 226, K)]
    blocks = np.stack([multigpu.pack_block_host(K, kps, np.zeros((len(kps), 48), np.uint8), np.zeros((len(kps), 3)),
                                                np.zeros(len(kps), np.uint8)) for kps, _ in frames])
    L = multigpu.block_layout(K)
    ids = rng.integers(1, 1 << 62, (len(frames), K)).astype(np.uint64)  # rows past a frame's count: never read
    for f, (kps, fid) in enumerate(frames):
        n = len(kps)
        ids[f, :n] = fid
        blocks[f, L["kps"] + n * 28:L["kps"] + K * 28] = 0xFF  # NaN coordinates past the count
    return frames, blocks, ids


def _expect(cfg, frames, id_set=None, kptrad=R.KPTRAD):
    out = np.zeros(len(frames), dtype=capi.COVERAGE_DTYPE)
    for f, (kps, ids) in enumerate(frames):
        c = R.coverage(cfg.w, cfg.h, kps, ids, id_set, kptrad)
        for name in R.COVERAGE_FIELDS:
            out[name][f] = c[name]
    return out


def _assert_records(got, want, what):
    for name in R.COVERAGE_FIELDS:
        assert np.array_equal(got[name], want[name]), (what, name, got[name], want[name])


def _run(fe, d_blocks, nf, d_ids, d_set, n_set, stream, extra=2, kptrad=R.KPTRAD):
    d_cov = torch.full((nf + extra, 6), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    fe.keyframe_coverage_blocks_device(d_blocks.data_ptr(), nf, d_ids.data_ptr(), d_cov.data_ptr(),
                                       None if d_set is None else d_set.data_ptr(), n_set, kptrad, stream)
    stream.synchronize()
    raw = d_cov.cpu().numpy()
    assert np.all(raw[nf:] == -7), "records past n_frames were written"
    return np.ascontiguousarray(raw[:nf]).view(capi.COVERAGE_DTYPE).reshape(-1)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_coverage_blocks_device_equals_the_restatement(name):
    make, radius = CONFIGS[name]
    cfg = make()
    assert R.radius_for(cfg.w, cfg.h) == radius
    fe = G.make_frontend(cfg)
    K = fe.max_keypoints
    frames, blocks, ids = _batch(cfg, K, 1074)
    nf = len(frames)
    assert blocks.shape[1] == fe.gather_block_bytes()
    d_blocks, d_ids = _dev(blocks), _dev(ids)
    st = torch.cuda.Stream()
    # the current frame: matched = id != 0
    got = _run(fe, d_blocks, nf, d_ids, None, 0, st)
    want = _expect(cfg, frames)
    _assert_records(got, want, "no set")
    one = [f for f in range(nf) if want["n_keypoints"][f] == 1]
    pixels = sum(2 * h + 1 for h in R.stencil(radius)) * 2 - (2 * radius + 1)
    assert len(one) == 3 and all(0 < want["detections_area"][f] <= pixels for f in one)
    assert np.array_equal(want["intersection_area"], want["matches_area"])
    assert np.array_equal(want["union_area"], want["detections_area"])
    sparse = [f for f in range(nf) if frames[f][1].size == 226 and 0 < np.count_nonzero(frames[f][1]) < 226]
    assert sparse and all(0 < want["matches_area"][f] < want["detections_area"][f] < (cfg.w // 10) * (cfg.h // 10)
                          for f in sparse)
    # the other frames: matched = id != 0 and id in S; S unsorted, with duplicates and zeros, some ids nobody carries
    rng = np.random.default_rng(7)
    carried = np.concatenate([fid[fid != 0] for _, fid in frames])
    s = np.concatenate([rng.choice(carried, len(carried) // 2, replace=False), np.zeros(5, np.uint64),
                        rng.integers(1, 1 << 62, 2500).astype(np.uint64), carried[:40]])
    rng.shuffle(s)
    assert len(s) > 2048  # more than one chunk of the kernel's id table
    d_set = _dev(s)
    got = _run(fe, d_blocks, nf, d_ids, d_set, len(s), st)
    want_set = _expect(cfg, frames, s)
    _assert_records(got, want_set, "set")
    assert 0 < want_set["n_matched"].sum() < want["n_matched"].sum()
    # the current frame's own rows as the set (zeros and rows past the counts included): frame 8 = 226 keypoints, 0.4
    cur = 8
    got = _run(fe, d_blocks, nf, d_ids, d_ids[cur], K, st)
    _assert_records(got, _expect(cfg, frames, ids[cur]), "own rows as the set")
    assert got[cur] == want[cur]
    # the empty set: nothing is matched; fewer frames than the buffer holds: the rest stays untouched
    got = _run(fe, d_blocks, nf - 4, d_ids, d_set, 0, st, extra=6)
    _assert_records(got, _expect(cfg, frames[:nf - 4], np.zeros(0, np.uint64)), "empty set")
    assert not got["n_matched"].any() and not got["matches_area"].any()
    # nothing else was written
    assert np.array_equal(d_blocks.cpu().numpy(), blocks) and np.array_equal(d_ids.cpu().numpy(), ids)
    assert np.array_equal(d_set.cpu().numpy(), s)
    # the host seam: the same kernel through host containers
    for f in (0, 1, 7, 8, 13, 14):
        kps, fid = frames[f]
        assert fe.keyframe_coverage(kps, fid) == want[f], f
        assert fe.keyframe_coverage(kps, fid, s) == want_set[f], f
    assert fe.keyframe_coverage(frames[8][0], frames[8][1], np.zeros(0, np.uint64))["n_matched"] == 0


def test_other_radii_and_many_keypoints_through_the_host_seam():
    """kptrad as ViSlamBackend uses it (0.09 * uniformityRadius / 36) and r = 0, 3, 5; more keypoints than one
    pass of the kernel's keypoint loop holds (8192), with a set of several chunks"""
    cfg = synth.euroc_config()
    fe = G.make_frontend(cfg)
    rng = np.random.default_rng(3)
    kps, ids = _frame(rng, cfg.w, cfg.h, 60, 0.5)
    for kptrad, r in ((0.0, 0), (0.07, 3), (0.09 * 38.0 / 36.0, 4), (0.105, 5), (0.2, 9)):
        assert R.radius_for(cfg.w, cfg.h, kptrad) == r
        got = fe.keyframe_coverage(kps, ids, None, kptrad)
        want = R.coverage(cfg.w, cfg.h, kps, ids, None, kptrad)
        assert {n: int(got[n]) for n in R.COVERAGE_FIELDS} == want, kptrad
    n = 9000
    kps = np.zeros(n, dtype=capi.KEYPOINT_DTYPE)
    kps["x"], kps["y"] = rng.uniform(0, 300, n), rng.uniform(0, 200, n)
    ids = rng.integers(1, 1 << 62, n).astype(np.uint64)
    ids[rng.random(n) < 0.5] = 0
    kps["x"][8500], kps["y"][8500] = 700.0, 440.0  # matched only if the second pass sees the set
    ids[8500] = 99
    s = np.concatenate([rng.integers(1, 1 << 62, 6000).astype(np.uint64), np.array([99], np.uint64), ids[:50]])
    got = fe.keyframe_coverage(kps, ids, s)
    want = R.coverage(cfg.w, cfg.h, kps, ids, s)
    assert {k: int(got[k]) for k in R.COVERAGE_FIELDS} == want
    assert want["n_matched"] >= 2


def test_coverage_of_detected_frames_and_the_decision():
    """straight from detect_describe_batch_device + pack_gather_blocks_device on synthetic stereo pairs: frame 0 is
    the current multiframe, its own landmark-id rows are the id set of the other two, and the verdict follows"""
    cfg = synth.euroc_config()
    nfr = 3
    fe = G.make_frontend(cfg, max_batch=2 * nfr, num_cameras=2)
    K = fe.max_keypoints
    for ci in range(2):
        fe.set_camera(ci, cfg.cams[ci])
    pairs = [synth.stereo_pair(cfg.w, cfg.h, 500 + i) for i in range(nfr)]
    imgs = np.stack([im for p in pairs for im in p[:2]])  # multiframe-major: frame f = images 2f, 2f + 1
    d_img = _dev(imgs)
    cam_ids = np.array([0, 1] * nfr, dtype=np.int32)
    grav = np.tile(np.array([0.0, 1.0, 0.0], dtype=np.float32), (2 * nfr, 1))
    d_blocks = torch.zeros((2 * nfr, fe.gather_block_bytes()), dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(11)
    ids = np.zeros((2 * nfr, K), dtype=np.uint64)
    ids[:2] = np.where(rng.random((2, K)) < 0.6, rng.integers(1, 5000, (2, K)), 0)
    pool = ids[:2][ids[:2] != 0]
    ids[2:4] = np.where(rng.random((2, K)) < 0.7, rng.choice(pool, (2, K)), rng.integers(6000, 7000, (2, K)))
    ids[4:6] = np.where(rng.random((2, K)) < 0.1, rng.choice(pool, (2, K)), 0)
    d_ids = _dev(ids)
    d_cov = torch.full((2 * nfr, 6), -7, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    fe.detect_describe_batch_device(d_img.data_ptr(), 2 * nfr, cam_ids, grav, st)
    fe.pack_gather_blocks_device(0, 2 * nfr, d_blocks.data_ptr(), st)
    fe.keyframe_coverage_blocks_device(d_blocks.data_ptr(), 2, d_ids.data_ptr(), d_cov.data_ptr(), stream=st)
    fe.keyframe_coverage_blocks_device(d_blocks[2:].data_ptr(), 2 * nfr - 2, d_ids[2:].data_ptr(),
                                       d_cov[2:].data_ptr(), d_ids.data_ptr(), 2 * K, stream=st)
    st.synchronize()
    got = d_cov.cpu().numpy().view(capi.COVERAGE_DTYPE).reshape(-1)
    host = d_blocks.cpu().numpy()
    recs = []
    for i in range(2 * nfr):
        kps = multigpu.unpack_block_host(host[i], K)[0]
        assert len(kps) > 50
        recs.append(R.coverage(cfg.w, cfg.h, kps, ids[i, :len(kps)], None if i < 2 else ids[:2].reshape(-1)))
        assert {n: int(got[n][i]) for n in R.COVERAGE_FIELDS} == recs[i], i
    want = R.decision(recs[:2], [recs[2:4], recs[4:6]])
    need, overlap = capi.keyframe_decision(got[:2], got[2:].reshape(nfr - 1, 2))
    assert (need, overlap) == want and 0.0 < overlap <= 1.0
    assert capi.keyframe_decision(got[:2]) == (True, 0.0)


def test_two_streams_in_flight():
    cfg = synth.euroc_config()
    fe = G.make_frontend(cfg)
    K = fe.max_keypoints
    fa, ba, ia = _batch(cfg, K, 21)
    fb, bb, ib = _batch(cfg, K, 22)
    d = [(_dev(ba), _dev(ia)), (_dev(bb), _dev(ib))]
    sa = np.concatenate([ia[7][:100], np.zeros(2, np.uint64)])
    d_sa = _dev(sa)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    covs = [torch.full((len(fa), 6), -7, dtype=torch.int32, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    for rep in range(2):  # four launches queued before anything is waited for
        for i in range(2):
            fe.keyframe_coverage_blocks_device(d[i][0].data_ptr(), len(fa), d[i][1].data_ptr(),
                                               covs[2 * rep + i].data_ptr(), d_sa.data_ptr() if rep else None,
                                               len(sa) if rep else 0, stream=streams[i])
    for s in streams:
        s.synchronize()
    for rep in range(2):
        for i, frames in enumerate((fa, fb)):
            got = covs[2 * rep + i].cpu().numpy().view(capi.COVERAGE_DTYPE).reshape(-1)
            _assert_records(got, _expect(cfg, frames, sa if rep else None), (rep, i))


def test_argument_validation_and_limits():
    cfg = synth.euroc_config()
    fe = G.make_frontend(cfg)
    K = fe.max_keypoints
    d_blocks = torch.zeros(fe.gather_block_bytes(), dtype=torch.uint8, device="cuda")
    d_ids = torch.zeros(K, dtype=torch.int64, device="cuda")
    d_cov = torch.full((2, 6), -7, dtype=torch.int32, device="cuda")
    b, i, c = d_blocks.data_ptr(), d_ids.data_ptr(), d_cov.data_ptr()
    bad = [dict(blocks_ptr=None), dict(n_frames=0), dict(n_frames=-1), dict(landmark_ids_ptr=None),
           dict(coverage_ptr=None), dict(n_id_set=-1, id_set_ptr=i), dict(n_id_set=3), dict(kptrad=-0.01),
           dict(kptrad=float("nan")), dict(kptrad=float("inf"))]
    for kw in bad:
        args = dict(blocks_ptr=b, n_frames=1, landmark_ids_ptr=i, coverage_ptr=c)
        args.update(kw)
        with pytest.raises(capi.OkvfeError) as e:
            fe.keyframe_coverage_blocks_device(**args)
        assert e.value.status == capi.ERR_INVALID_ARGUMENT and "okvfe_keyframe_coverage_blocks_device" in str(e.value), kw
    with pytest.raises(capi.OkvfeError) as e:  # radius 144 of a 48-row mask: beyond the stencil table
        fe.keyframe_coverage_blocks_device(b, 1, i, c, kptrad=3.0)
    assert e.value.status == capi.ERR_UNSUPPORTED
    kps = np.zeros(3, dtype=capi.KEYPOINT_DTYPE)
    for kptrad in (-1.0, float("nan")):
        with pytest.raises(capi.OkvfeError) as e:
            fe.keyframe_coverage(kps, np.zeros(3, np.uint64), None, kptrad)
        assert e.value.status == capi.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert np.all(d_cov.cpu().numpy() == -7)
    # an empty image through both doors
    zero = fe.keyframe_coverage(kps[:0], np.zeros(0, np.uint64))
    assert all(int(zero[n]) == 0 for n in R.COVERAGE_FIELDS)
    fe.keyframe_coverage_blocks_device(b, 1, i, c)
    torch.cuda.synchronize()
    assert np.all(d_cov.cpu().numpy()[0] == 0) and np.all(d_cov.cpu().numpy()[1] == -7)
