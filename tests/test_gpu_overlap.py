"""GPU: okvfe_overlap_pairs_blocks_device (ViSlamBackend::overlapFraction up to its counts, ViSlamBackend.cpp:2341-2427,
for a list of multiframe pairs in one launch) against the restatement in overlap_ref.py, which paints real u8 masks and
intersects real sets.  Every count must be EQUAL; the optional per-image records must be EQUAL to what the existing
okvfe_keyframe_coverage_blocks_device reports per pair and side with the other multiframe's ids, zero-padded by the test,
as the set.  The scenes (overlap_scenes.py) are sparse on purpose: dense frames saturate the mask.

PARITY UNPINNED for cv::circle and the point rounding, as in keyframe_ref.py."""
import numpy as np
import pytest

import gpu_common as G
import keyframe_ref as R
import overlap_ref as OR
import overlap_scenes as S
from okvis2_amd import capi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 3


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(fe, d_blocks, d_ids, stride_m, stride_c, M, C, pairs, stream, with_coverage=True):
    n = len(pairs)
    d_counts = torch.full((n + GUARD, 8), -7, dtype=torch.int32, device="cuda")
    d_cov = torch.full((n * 2 * C + GUARD, 6), -7, dtype=torch.int32, device="cuda") if with_coverage else None
    torch.cuda.synchronize()
    fe.overlap_pairs_blocks_device(d_blocks.data_ptr(), stride_m, stride_c, M, C, d_ids.data_ptr(),
                                   [p[0] for p in pairs], [p[1] for p in pairs], d_counts.data_ptr(),
                                   None if d_cov is None else d_cov.data_ptr(), S.KPTRAD, stream)
    stream.synchronize()
    raw = d_counts.cpu().numpy()
    assert np.all(raw[n:] == -7), "counts past n_pairs were written"
    counts = np.ascontiguousarray(raw[:n]).view(capi.OVERLAP_COUNTS_DTYPE).reshape(-1)
    cov = None
    if d_cov is not None:
        raw = d_cov.cpu().numpy()
        assert np.all(raw[n * 2 * C:] == -7), "coverage records past n_pairs x 2 x n_cams were written"
        cov = np.ascontiguousarray(raw[:n * 2 * C]).view(capi.COVERAGE_DTYPE).reshape(n, 2, C)
    return counts, cov


def _assert_counts(got, want, pairs, what):
    for field in OR.COUNT_FIELDS:
        bad = np.flatnonzero((got[field] != want[field]).any(axis=1))
        assert bad.size == 0, (what, field, [(pairs[i], got[field][i].tolist(), want[field][i].tolist()) for i in bad[:5]])


@pytest.mark.parametrize("name", sorted(S.CONFIGS))
def test_overlap_pairs_equal_the_restatement(name):
    cfg, K, mfs, ref = S.reference(name)
    S.check_floors(name)
    M, C = len(mfs), len(cfg.cams)
    assert R.radius_for(cfg.w, cfg.h, S.KPTRAD) == S.CONFIGS[name][1]
    if name == "hilti":
        assert C * K > 2048  # the id table's chunk edge is crossed (the counted rows of multiframe 0 alone: 2552)
        assert sum(len(k) for k, _ in mfs[0]) > 2048
    fe = G.make_frontend(cfg)
    assert fe.max_keypoints == K
    st = torch.cuda.Stream()
    pairs = [(a, b) for a in range(M) for b in range(M)]
    want = S.counts_array(ref, pairs)
    # layout (n_cams, 1): the cameras of a multiframe on consecutive blocks
    blocks, ids = S.pack(mfs, K, C, 1)
    assert blocks.shape[1] == fe.gather_block_bytes()
    d_blocks, d_ids = _dev(blocks), _dev(ids)
    counts, cov = _run(fe, d_blocks, d_ids, C, 1, M, C, pairs, st)
    _assert_counts(counts, want, pairs, "layout (n_cams, 1)")
    # the per-image records: the existing coverage call per pair and side, the other multiframe's rows zeroed past the counts
    padded = ids.reshape(M, C, K).copy()
    for m, mf in enumerate(mfs):
        for c, (kps, _) in enumerate(mf):
            padded[m, c, len(kps):] = 0
    d_padded = _dev(padded)
    d_one = torch.full((len(pairs), 2, C, 6), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(pairs):
        for f, (own, other) in enumerate(((a, b), (b, a))):
            fe.keyframe_coverage_blocks_device(d_blocks[own * C:].data_ptr(), C, d_ids[own * C:].data_ptr(),
                                               d_one[i, f].data_ptr(), d_padded[other].data_ptr(), C * K, S.KPTRAD, st)
    st.synchronize()
    one = d_one.cpu().numpy().reshape(-1, 6).view(capi.COVERAGE_DTYPE).reshape(len(pairs), 2, C)
    for field in R.COVERAGE_FIELDS:
        assert np.array_equal(cov[field], one[field]), field
        for i in (3, 17, 67, 89):  # ... and a few against the restatement directly
            for f in range(2):
                assert cov[field][i, f].tolist() == [r[field] for r in ref[pairs[i]]["per_image"][f]], (field, pairs[i], f)
    # layout (1, n_multiframes): camera-major; a pair list that names one multiframe many times; no per-image records
    blocks2, ids2 = S.pack(mfs, K, 1, M)
    d_blocks2, d_ids2 = _dev(blocks2), _dev(ids2)
    many = [(2, b) for b in range(M)] + [(2, 2)] * 3 + [(b, 2) for b in range(M)] + [(0, 0), (9, 8)]
    counts2, none = _run(fe, d_blocks2, d_ids2, 1, M, M, C, many, st, with_coverage=False)
    assert none is None
    _assert_counts(counts2, S.counts_array(ref, many), many, "layout (1, n_multiframes)")
    # nothing else was written
    assert np.array_equal(d_blocks.cpu().numpy(), blocks) and np.array_equal(d_ids.cpu().numpy(), ids)
    # the overlaps and the order of the sweep, from the device counts: previous = multiframe 1, multiframe 6 (NaN as
    # side B never shows: min keeps side A) included
    overlap = capi.overlap_fraction(counts)
    assert [float(v).hex() for v in overlap] == [float(ref[p]["overlap"]).hex() for p in pairs]
    frame_ids = np.array([40, 12, 77, 5, 63, 21, 90, 34, 58, 19], dtype=np.uint64)
    for previous in (1, 0, 8):
        row = overlap[previous * M:(previous + 1) * M]
        got = capi.motion_frame_order(row, frame_ids, previous).tolist()
        assert got == OR.motion_frame_order([ref[(previous, b)]["overlap"] for b in range(M)], frame_ids, previous)
        assert got[0] == previous and 3 <= len(got) < M


def test_behind_the_pack_call_and_behind_pipelined_lanes():
    """the join: the call on a side stream right behind okvfe_pack_gather_blocks_device, and with pipelined lanes
    (okvfe_set_internal_lanes(ctx, -4)) pending"""
    from okvis2_amd import multigpu, synth
    cfg = synth.euroc_config()
    scenes = [synth.stereo_pair(cfg.w, cfg.h, 900 + i)[:2] for i in range(4)]
    # 128 images is the least -4 cuts into lanes (64 images per lane: two of them)
    for lanes, nmf, pairs in ((None, 4, [(a, b) for a in range(4) for b in range(4)]),
                              (-4, 64, [(0, 33), (33, 0), (1, 62), (62, 31), (31, 31), (63, 2), (34, 35)])):
        fe = G.make_frontend(cfg, max_batch=2 * nmf, num_cameras=2)
        K = fe.max_keypoints
        for ci in range(2):
            fe.set_camera(ci, cfg.cams[ci])
        if lanes is not None:
            fe.set_internal_lanes(lanes)
        imgs = np.stack([im for i in range(nmf) for im in scenes[i % 4]])
        d_img = _dev(imgs)
        cam_ids = np.array([0, 1] * nmf, dtype=np.int32)
        grav = np.tile(np.array([0.0, 1.0, 0.0], dtype=np.float32), (2 * nmf, 1))
        d_blocks = torch.zeros((2 * nmf, fe.gather_block_bytes()), dtype=torch.uint8, device="cuda")
        rng = np.random.default_rng(5)
        ids = np.where(rng.random((2 * nmf, K)) < 0.5, rng.integers(1, 600, (2 * nmf, K)), 0).astype(np.uint64)
        d_ids = _dev(ids)
        d_counts = torch.full((len(pairs) + GUARD, 8), -7, dtype=torch.int32, device="cuda")
        # without lanes the caller's stream is what orders the three calls; with pipelined lanes the detect call's
        # work is on the lane streams whichever stream it was given, and the entry points that follow join it
        main, side = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        fe.detect_describe_batch_device(d_img.data_ptr(), 2 * nmf, cam_ids, grav, side if lanes is None else main)
        fe.pack_gather_blocks_device(0, 2 * nmf, d_blocks.data_ptr(), side)
        fe.overlap_pairs_blocks_device(d_blocks.data_ptr(), 2, 1, nmf, 2, d_ids.data_ptr(), [p[0] for p in pairs],
                                       [p[1] for p in pairs], d_counts.data_ptr(), None, S.KPTRAD, side)
        side.synchronize()
        raw = d_counts.cpu().numpy()
        assert np.all(raw[len(pairs):] == -7)
        counts = np.ascontiguousarray(raw[:len(pairs)]).view(capi.OVERLAP_COUNTS_DTYPE).reshape(-1)
        host = d_blocks.cpu().numpy()
        mfs = {}
        for m in sorted({m for p in pairs for m in p}):
            mfs[m] = []
            for c in range(2):
                kps = multigpu.unpack_block_host(host[2 * m + c], K)[0]
                assert len(kps) > 50
                mfs[m].append((kps, ids[2 * m + c, :len(kps)]))
        ref = {p: OR.overlap_counts(cfg.w, cfg.h, mfs[p[0]], mfs[p[1]], S.KPTRAD) for p in pairs}
        _assert_counts(counts, S.counts_array(ref, pairs), pairs, lanes)
        assert all(0.0 < v <= 1.0 for v in capi.overlap_fraction(counts))


def test_argument_validation_and_limits():
    cfg, K, mfs, _ = S.reference("euroc")
    fe = G.make_frontend(cfg)
    M, C = len(mfs), 2
    blocks, ids = S.pack(mfs, K, C, 1)
    d_blocks, d_ids = _dev(blocks), _dev(ids)
    d_counts = torch.full((4, 8), -7, dtype=torch.int32, device="cuda")
    b, i, c = d_blocks.data_ptr(), d_ids.data_ptr(), d_counts.data_ptr()
    good = dict(blocks_ptr=b, block_stride_m=C, block_stride_c=1, n_multiframes=M, n_cams=C, landmark_ids_ptr=i,
                pair_a=[0, 1], pair_b=[1, 1], counts_ptr=c, kptrad=S.KPTRAD)
    bad = [dict(blocks_ptr=None), dict(landmark_ids_ptr=None), dict(counts_ptr=None), dict(block_stride_m=-2),
           dict(block_stride_c=-1), dict(n_cams=0), dict(n_cams=33), dict(n_multiframes=-1), dict(kptrad=-0.1),
           dict(kptrad=float("nan")), dict(block_stride_m=1, block_stride_c=1),  # (0, 1) and (1, 0) on block 1
           dict(block_stride_m=0)]
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(capi.OkvfeError) as e:
            fe.overlap_pairs_blocks_device(**args)
        assert e.value.status == capi.ERR_INVALID_ARGUMENT and "okvfe_overlap_pairs_blocks_device" in str(e.value), kw
    for pa, pb, who in (([0, M], [1, 1], "pair 1"), ([0, 1, 2], [1, 1, -1], "pair 2")):
        with pytest.raises(capi.OkvfeError) as e:
            fe.overlap_pairs_blocks_device(**dict(good, pair_a=pa, pair_b=pb))
        assert e.value.status == capi.ERR_INVALID_ARGUMENT and who in str(e.value)
    with pytest.raises(capi.OkvfeError) as e:  # radius 144 of a 48-row mask: beyond the stencil table
        fe.overlap_pairs_blocks_device(**dict(good, kptrad=3.0))
    assert e.value.status == capi.ERR_UNSUPPORTED
    fe.overlap_pairs_blocks_device(**dict(good, pair_a=[], pair_b=[], counts_ptr=None))  # no pairs: OK, nothing launched
    torch.cuda.synchronize()
    assert np.all(d_counts.cpu().numpy() == -7)
    fe.overlap_pairs_blocks_device(**good)
    torch.cuda.synchronize()
    raw = d_counts.cpu().numpy()
    assert np.all(raw[2:] == -7) and np.all(raw[:2] >= 0)
