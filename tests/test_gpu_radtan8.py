"""GPU: the 8-coefficient radial-tangential camera (OKVFE_DIST_RADTAN8) through the device paths that
take a camera -- keypoint back-projection (compact_kernel), matchStereo on those back-projections,
matchMotionStereo's 4 px re-projection check and matchToMap's landmark projection.

The CPU oracle knows only the three older models, so the model itself comes from the test-side
restatement tests/radtan8_ref.py (bit-equal to the host tables: tests/test_radtan8_host.py): its
awareness maps, back-projections and projections are fed to the oracle's entry points, which take
them as arrays, and everything downstream is compared with the oracle bit for bit."""
import dataclasses

import numpy as np
import pytest

import gpu_common as G
import radtan8_ref as R8
from okvis2_amd import capi, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _gravity(n, seed):
    rng = np.random.default_rng(seed)
    g = np.stack([rng.uniform(-0.1, 0.1, n), np.ones(n), rng.uniform(-0.1, 0.1, n)], axis=1)
    return (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)


def _oracle_extract(oracle, cfg, cam, img, grav, maps=None):
    rays, jac = maps if maps is not None else R8.awareness_maps(cam)
    k, d = oracle.detect_describe(img, cfg.uniformity_radius, 0, cfg.abs_threshold, cfg.max_kpts,
                                  oracle.MODE_CAMERA_AWARE, rays, jac, np.float32(cam.fu),
                                  tuple(float(v) for v in grav))
    if cam.dist_type == capi.DIST_RADTAN8:
        bp, bv = R8.backproject_keypoints(cam, k)
    else:
        bp, bv = oracle.backproject_keypoints(cam, k)
    return k, d, bp, bv


def _assert_extraction_equal(got, ref):
    k, d, bp, bv = got
    rk, rd, rbp, rbv = ref
    G.assert_keypoints_equal(k, rk)
    assert np.array_equal(d, rd)
    assert np.array_equal(bv, rbv)
    assert np.array_equal(bp.view(np.uint64), rbp.view(np.uint64))


def _stereo_pairs(cfg, n):
    T0, T1 = synth.stereo_poses(cfg.baseline)
    f = [0.5 * (c.fu + c.fv) for c in cfg.cams]
    arr = []
    for i in range(n):
        sp = capi.StereoPair()
        sp.image0, sp.image1 = 2 * i, 2 * i + 1
        sp.T_WC0, sp.T_WC1 = capi.make_pose(*T0), capi.make_pose(*T1)
        sp.f0, sp.f1 = f[0], f[1]
        arr.append(sp)
    return (capi.StereoPair * n)(*arr), T0, T1, f


def _rig_end_to_end(oracle, cfg, n_frames, seed, check_b1=True):
    """detect + describe (B = 1 and batched) and matchStereo on a stereo rig against the oracle."""
    fe = G.make_frontend(cfg, max_batch=2 * n_frames, num_cameras=2)
    for ci, cam in enumerate(cfg.cams):
        fe.set_camera(ci, cam)
    imgs = np.stack([synth.corners_image(cfg.w, cfg.h, seed + i) for i in range(2 * n_frames)])
    grav = _gravity(2 * n_frames, seed)
    maps = [R8.awareness_maps(c) if c.dist_type == capi.DIST_RADTAN8 else oracle.awareness_maps(c)
            for c in cfg.cams]
    ref = [_oracle_extract(oracle, cfg, cfg.cams[i % 2], imgs[i], grav[i], maps[i % 2]) for i in range(2 * n_frames)]
    if check_b1:
        for i in range(2):
            _assert_extraction_equal(fe.detect_describe(imgs[i], cam=i % 2, gravity=grav[i]), ref[i])
    pairs, T0, T1, f = _stereo_pairs(cfg, n_frames)
    d_img = torch.from_numpy(imgs).cuda()
    d_match = torch.zeros((n_frames, cfg.max_kpts, capi.STEREO_MATCH_DTYPE.itemsize), dtype=torch.uint8,
                          device="cuda")
    cam_ids = np.array([0, 1] * n_frames, dtype=np.int32)
    fe.detect_describe_batch_device(d_img.data_ptr(), 2 * n_frames, cam_ids, grav)
    fe.match_stereo_batch_device(pairs, d_match.data_ptr())
    torch.cuda.synchronize()
    res = [fe.download(i) for i in range(2 * n_frames)]
    rows = d_match.cpu().numpy().view(capi.STEREO_MATCH_DTYPE).reshape(n_frames, -1)
    n_valid = 0
    for i in range(2 * n_frames):
        _assert_extraction_equal(res[i], ref[i])
        n_valid += int(res[i][3].sum())
    for fr in range(n_frames):
        k0, d0, bp0, bv0 = ref[2 * fr]
        k1, d1, bp1, bv1 = ref[2 * fr + 1]
        want = oracle.match_stereo(d0, k0, bp0, bv0, d1, k1, bp1, bv1, T0, T1, f[0], f[1], cfg.match_threshold)
        got_host = fe.match_stereo(d0, k0, bp0, bv0, d1, k1, bp1, bv1, T0, T1, f[0], f[1])
        for got in (rows[fr, :len(k0)], got_host):
            for fld in ("k1", "dist", "initialisable"):
                assert np.array_equal(got[fld], want[fld]), (fr, fld)
            assert np.array_equal(got["hp_W"].view(np.uint64), want["hp_W"].view(np.uint64)), fr
    return res, n_valid


def test_radtan8_rig_detect_describe_and_match_stereo(oracle):
    cfg = synth.radtan8_config()
    res, n_valid = _rig_end_to_end(oracle, cfg, 2, 5100)
    n_kp = sum(len(r[0]) for r in res)
    assert n_kp > 600 and n_valid > 0.9 * n_kp


def test_mixed_batch_radtan8_and_radtan_slots(oracle):
    """One batch with images of a RADTAN8 slot and of a RADTAN slot: the call takes the RADTAN8-capable
    compaction kernel, and the RADTAN images still back-project exactly as the oracle does."""
    cfg = dataclasses.replace(synth.radtan8_config(), cams=[synth.radtan8_config().cams[0],
                                                             synth.euroc_config().cams[0]])
    res, _ = _rig_end_to_end(oracle, cfg, 2, 5200, check_b1=False)
    # (the RADTAN images, 1 and 3, were compared with oracle.backproject_keypoints inside)
    assert len(res[1][0]) > 100 and res[1][3].sum() > 0.9 * len(res[1][0])


def test_radtan8_seeded_fuzz_small(oracle):
    """Random RADTAN8 cameras that stay monotonic inside a small image, through detect + describe and
    matchStereo."""
    rng = np.random.default_rng(808)
    base = synth.radtan8_config()
    done = 0
    while done < 20:
        w, h = 192, 128
        fu = rng.uniform(90.0, 200.0)
        k = (rng.uniform(-0.3, 0.7), rng.uniform(-0.05, 0.05), rng.uniform(-1e-3, 1e-3), rng.uniform(-1e-3, 1e-3),
             rng.uniform(-0.01, 0.01), rng.uniform(0.0, 1.0), rng.uniform(-0.05, 0.15), rng.uniform(-0.01, 0.01))
        cams = [synth.Camera(w, h, fu * s, fu * s * rng.uniform(0.98, 1.02), w / 2 + rng.uniform(-4, 4),
                             h / 2 + rng.uniform(-4, 4), 3, tuple(v * rng.uniform(0.95, 1.05) for v in k))
                for s in (1.0, rng.uniform(0.97, 1.03))]
        # monotonic inside the image: the radial map x -> x * rad(x^2) increases along the diagonal
        r = np.linspace(0.0, 1.2 * np.hypot(w, h) / 2 / cams[0].fu, 200)
        if any(np.any(np.diff(R8.distort(c, r, 0.0 * r, want_jac=False)[1]) <= 0) for c in cams):
            continue
        cfg = dataclasses.replace(base, w=w, h=h, cams=cams, uniformity_radius=10.0, abs_threshold=20,
                                  max_kpts=300)
        _rig_end_to_end(oracle, cfg, 1, 6000 + done, check_b1=(done % 5 == 0))
        done += 1


def test_radtan8_motion_stereo_host_and_blocks(oracle):
    cfg = synth.radtan8_config()
    cam = cfg.cams[0]
    twin = dataclasses.replace(cam, dist_type=0, d=(0.0, 0.0, 0.0, 0.0))  # the gates use fu, fv only
    fe = G.make_frontend(cfg)
    fe.set_camera(0, cam)
    rng = np.random.default_rng(31)
    n = 400
    T0 = (np.eye(3).reshape(-1), np.zeros(3))
    th = 0.05
    Rz = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]])
    T1 = (Rz.reshape(-1), np.array([0.35, 0.04, 0.02]))
    X = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-0.8, 0.8, n), rng.uniform(2.5, 9, n)], 1)

    def observe(T, noise):
        Cm = np.asarray(T[0]).reshape(3, 3)
        st, pt, _ = R8.project(cam, (X - np.asarray(T[1])) @ Cm)
        kp = np.zeros(n, dtype=oracle.KEYPOINT_DTYPE)
        kp["size"] = 12.0
        kp["x"] = np.where(st == 0, pt[:, 0], 5.0) + rng.normal(0, noise, n)
        kp["y"] = np.where(st == 0, pt[:, 1], 5.0) + rng.normal(0, noise, n)
        bp, bv = R8.backproject_keypoints(cam, kp)
        return kp, bp, bv

    kp0, bp0, bv0 = observe(T0, 0.3)
    kp1, bp1, bv1 = observe(T1, 0.3)
    d0 = rng.integers(0, 256, (n, 48), dtype=np.uint8)
    d1 = d0 ^ (rng.random((n, 48)) < 0.03).astype(np.uint8) * rng.integers(0, 256, (n, 48), dtype=np.uint8)
    perm = rng.permutation(n)
    d1, kp1, bp1, bv1 = d1[perm], kp1[perm], bp1[perm], bv1[perm]
    skip0 = (rng.random(n) < 0.1).astype(np.uint8)
    matched1 = (rng.random(n) < 0.1).astype(np.uint8)

    def accepted(rows):
        """The 4 px check recomputed with the restated projection; -1 where within 1e-6 of a decision edge."""
        out = np.zeros(n, dtype=np.int32)
        C1, r1 = np.asarray(T1[0]).reshape(3, 3), np.asarray(T1[1])
        for i in np.flatnonzero(rows["k1"] >= 0):
            hp = rows["hp_W"][i]
            hc = C1.T @ hp[:3] - (C1.T @ r1) * hp[3]
            head = -hc if hp[3] < 0 else hc
            st, pt, _ = R8.project(cam, head[None])
            e = np.hypot(float(kp1["x"][rows["k1"][i]]) - pt[0, 0], float(kp1["y"][rows["k1"][i]]) - pt[0, 1])
            edge = abs(e - 4.0) < 1e-6 or np.any(np.abs(pt[0] - [0, 0]) < 1e-6) or \
                np.any(np.abs(pt[0] - [cam.w, cam.h]) < 1e-6)
            out[i] = -1 if edge else int(st[0] == 0 and e < 4.0)
        return out

    import torch
    from okvis2_amd import multigpu
    K = cfg.max_kpts
    blk0 = torch.from_numpy(multigpu.pack_block_host(K, kp0, d0, bp0, bv0)).cuda()
    blk1 = torch.from_numpy(multigpu.pack_block_host(K, kp1, d1, bp1, bv1)).cuda()
    pad = lambda a: torch.from_numpy(np.concatenate([a, np.zeros(K - len(a), np.uint8)])).cuda()
    d_s0, d_m1 = pad(skip0), pad(matched1)
    d_out = torch.zeros((K, capi.MOTION_MATCH_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    n_acc = 0
    for s0, m1, ps0, pm1 in ((skip0, matched1, d_s0.data_ptr(), d_m1.data_ptr()), (None, None, None, None)):
        ref = oracle.match_motion_stereo(d0, kp0, bp0, bv0, s0, d1, kp1, bp1, bv1, m1, T0, T1, twin,
                                         cfg.match_threshold)
        got_host = fe.match_motion_stereo(cam, d0, kp0, bp0, bv0, s0, d1, kp1, bp1, bv1, m1, T0, T1)
        fe.match_motion_stereo_blocks_device(0, blk0.data_ptr(), blk1.data_ptr(), ps0, pm1, T0, T1,
                                             d_out.data_ptr())
        torch.cuda.synchronize()
        got_dev = d_out.cpu().numpy().view(capi.MOTION_MATCH_DTYPE).reshape(-1)[:n]
        for got in (got_host, got_dev):
            for f in ("k1", "dist", "initialisable"):
                assert np.array_equal(got[f], ref[f]), f
            assert np.array_equal(got["hp_W"].view(np.uint64), ref["hp_W"].view(np.uint64))
            want = accepted(got)
            sure = want >= 0
            assert np.array_equal(got["accepted"][sure], want[sure])
            n_acc += int((want == 1).sum())
        assert (ref["k1"] >= 0).sum() > 100
    assert n_acc > 200


def test_radtan8_match_to_map_landmarks(oracle):
    import os
    import map_synth
    gold = os.path.join(os.path.dirname(__file__), "golden")
    voc = np.fromfile(os.path.join(gold, "small_voc_desc.bin"), dtype=np.uint8).reshape(-1, 48)
    m = map_synth.make_map(6000, voc=voc)
    cfg = synth.radtan8_config()
    cam = cfg.cams[0]
    # current pose = identity: hp_C = hp_W exactly in every summation order, so the restated projection
    # of hp_W is bit-comparable with the device's
    T1 = (np.eye(3).reshape(-1), np.zeros(3))
    fe = G.make_frontend(cfg)
    fe.set_camera(0, cam)
    hp = m["hp"]
    head = np.where(hp[:, 3:4] < 0, -hp[:, :3], hp[:, :3])
    st, proj, _ = R8.project(cam, head)
    rng = np.random.default_rng(9)
    vis = np.flatnonzero(st == 0)
    pick = rng.choice(vis, 700, replace=False)
    kps = np.zeros(700, dtype=oracle.KEYPOINT_DTYPE)
    kps["x"] = proj[pick, 0] + rng.normal(0, 1.0, 700)
    kps["y"] = proj[pick, 1] + rng.normal(0, 1.0, 700)
    kps["size"] = 12.0
    desc = m["base"][pick] ^ ((rng.random((700, 48)) < 0.03) * rng.integers(1, 256, (700, 48))).astype(np.uint8)
    use = np.ones(700, dtype=np.uint8)
    for exclusive, thr in ((False, 20.0), (True, 150.0)):
        lm, bd, pool = fe.match_to_map_landmarks(0, hp, m["quality"], m["obs_begin"], m["obs_pose"], m["obs_desc"],
                                                 m["obs_bp"], m["poses"], T1, thr, exclusive, desc, kps, use)
        inside = (st != 4) & (st != 3) & (proj[:, 0] >= -thr) & (proj[:, 1] >= -thr) & \
            (proj[:, 0] <= cam.w + thr) & (proj[:, 1] <= cam.h + thr)
        assert not (pool["status"][~inside] != 0).any()  # failed restated projections are excluded
        kept = pool["status"] != 0
        assert kept.sum() > 500
        assert np.array_equal(pool["projection"][kept].view(np.uint64), proj[kept].view(np.uint64))
        # pooling itself does not see the camera model: against the oracle on an undistorted twin
        twin = dataclasses.replace(cam, dist_type=0, d=(0.0, 0.0, 0.0, 0.0))
        ref = oracle.prepare_landmarks(hp, m["quality"], m["obs_begin"], m["obs_pose"], m["obs_bp"], m["poses"], T1,
                                       twin, thr, exclusive)
        both = kept & (ref["status"] != 0)
        assert both.sum() > 300
        for k in ("status", "n_desc", "obs_rows"):
            assert np.array_equal(pool[k][both], ref[k][both]), k
        idx, pproj, begin, rows = map_synth.packed_set(pool, m["obs_desc"], 1)
        rl, rd = oracle.match_to_map(desc, kps, use, pproj, begin, rows, thr, cfg.match_threshold)
        rl = np.where(rl >= 0, idx[np.maximum(rl, 0)], -1)
        assert np.array_equal(lm, rl) and np.array_equal(bd, rd)
        assert (rl >= 0).sum() > 100
