"""GPU: the motion-stereo sweep before initialisation with its hypotheses made on the device, every call queued on one
side stream with nothing waited for and no host array in between: per older frame
okvfe_match_motion_stereo_blocks_batch_device with claims, landmark ids assigned to the claimed rows by torch ops on the
same stream, okvfe_ransac2d2d_hypotheses_blocks_device, okvfe_ransac2d2d_consensus_blocks_device on the lists it wrote
(landmark1_out == landmark1_dev), matched1 = (id >= 0) for the next step.  Two steps over 4 current multiframes of 2
cameras (the sweep of test_gpu_ransac2d2d_chain.py, whose helpers are used) equal the chain of restatements
(motion_claim_ref.py, ransac2d2d_hyp_ref.py, ransac2d2d_ref.py) byte for byte under both orders of the FP64 sums.

And the two outcomes the session's initialisation hangs on (Frontend.cpp:644-648), hypotheses -> consensus on
ransac2d2d_hyp_scenes.motion_scene: a general motion with 10 % wrong matches ends with the relative-pose success bit and
rotation_only 0, a pure rotation with rotation_only 1 -- both confirmed with the restatements on the CPU first."""
import dataclasses

import numpy as np
import pytest

import gate_scenes as G
import gpu_common
import motion_claim_ref as M
import ransac2d2d_hyp_ref as H2
import ransac2d2d_hyp_scenes as HS
import ransac2d2d_ref as R2
import ransac2d2d_scenes as S2
from okvis2_amd import capi, multigpu, synth
from test_gpu_ransac2d2d_chain import FILL, H, K, KNOWN_ID, N_CAMS, NEW_ID, REC, STEPS, W, _frames, _pad

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N_HYP = 50


def reference_chain(tree, sw):
    """test_gpu_ransac2d2d_chain.reference_chain with the hypothesis lists of the restatement (seed HS.SEED + step, the
    pair's index as its key) in the place of given ones"""
    n = len(sw["current"])
    matched1 = [m.copy() for m in sw["matched1"]]
    lm1 = [np.where(m != 0, KNOWN_ID + np.arange(len(m)), -1).astype(np.int32) for m in matched1]
    fus = [sw["current"][c]["cam"].fu for c in range(N_CAMS)]
    steps = []
    for j in range(STEPS):
        res, lm0 = [], []
        for b, (sc, old) in enumerate(zip(sw["current"], sw["older"][j])):
            pair = dict(sc, **{k: old[k] for k in ("d0", "kp0", "bp0", "bv0")})
            rows = M.match_rows(pair, old["skip0"], matched1[b], M.with_frame_size(sc["cam"], W, H))
            claimed, n_claimed, _ = M.claim_loop(rows, len(rows), matched1[b])
            ids = NEW_ID + (j * n + b) * K + np.arange(len(rows))
            l0 = np.where(claimed != 0, ids, -1).astype(np.int32)
            lm1[b][rows["k1"][claimed != 0]] = l0[claimed != 0]
            lm0.append(l0)
            res.append(dict(rows=rows, claimed=claimed, n_claimed=n_claimed))
        cons, hyps = [], []
        for mf in range(n // N_CAMS):
            cams, hyp = [], []
            for c in range(N_CAMS):
                b = mf * N_CAMS + c
                fr0, fr1 = _frames(sw, j, b, lm0[b], lm1[b])
                corr = R2.correspondences(tree, fr0, fr1, fus[c])
                h = H2.hypotheses(tree, corr, HS.SEED + j, mf, c, N_HYP)
                hyp.append(h)
                cams.append(S2.cam_entry(fr0, fr1, h["rot_H"], h["rel_H"], h["rot_valid"], h["rel_valid"]))
            ref = R2.run(tree, cams, fus)
            for c in range(N_CAMS):
                b = mf * N_CAMS + c
                lm1[b] = ref["cams"][c]["landmark1_out"].copy()
                matched1[b] = (lm1[b] >= 0).astype(np.uint8)
            cons.append(ref)
            hyps.append(hyp)
        steps.append(dict(res=res, cons=cons, hyps=hyps, lm0=lm0))
    return steps, lm1, matched1


def test_two_step_sweep_with_hypotheses_and_consensus_after_each_step(oracle, fp64_order):
    tree = fp64_order == "eigen_tree"
    cams = [synth.euroc_config().cams[0], synth.tumvi1024_config().cams[0]]
    sw = M.sweep_scene(cams, ("euroc", "tumvi"), steps=STEPS)
    n = len(sw["current"])
    n_mf = n // N_CAMS
    steps, lm1_ref, matched1_ref = reference_chain(tree, sw)
    assert all(sum(r["n_claimed"] for r in st["res"]) >= 50 for st in steps)
    assert sum(int(h["rel_valid"].sum()) for st in steps for hyp in st["hyps"] for h in hyp) >= 100
    assert any(ref["total_inliers"] >= 0 for st in steps for ref in st["cons"])

    fe = capi.Frontend(W, H, 38.0, 0, 150, K, match_threshold=G.THRESHOLD, max_batch=1, num_cameras=N_CAMS)
    try:
        for slot, cam in enumerate(cams):
            fe.set_camera(slot, M.with_frame_size(cam, W, H))
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
        block = lambda kp, d, bp, bv: multigpu.pack_block_host(K, kp, d, bp, bv)
        d_b1 = dev(np.stack([block(sc["kp1"], sc["d1"], sc["bp1"], sc["bv1"]) for sc in sw["current"]]))
        d_b0 = dev(np.stack([block(o["kp0"], o["d0"], o["bp0"], o["bv0"]) for step in sw["older"] for o in step]))
        d_m = dev(np.stack([_pad(m, 0, np.uint8) for m in sw["matched1"]]))
        d_skip = [dev(np.stack([_pad(o["skip0"], 0, np.uint8) for o in step])) for step in sw["older"]]
        d_lm1 = dev(np.stack([_pad(np.where(m != 0, KNOWN_ID + np.arange(len(m)), -1), -1, np.int32) for m in sw["matched1"]]))
        d_lm1 = torch.cat([d_lm1.reshape(-1), torch.zeros(1, dtype=torch.int32, device="cuda")])  # + a slot nobody reads
        d_lm0 = full((STEPS * n, K), -1, torch.int32)
        d_rows = [full((n, K, REC), FILL, torch.uint8) for _ in range(STEPS)]
        d_claimed = [full((n, K), FILL, torch.uint8) for _ in range(STEPS)]
        d_n = [full((n,), -7, torch.int32) for _ in range(STEPS)]
        out = []
        for j in range(STEPS):
            o = {k: full((n_mf, N_CAMS), S2.STATE_SENTINEL if k in S2.U8 else S2.SENTINEL,
                         torch.uint8 if k in S2.U8 else torch.int32) for k in S2.PER_CAM}
            o.update({k: full((n_mf,), S2.STATE_SENTINEL if k in S2.U8 else S2.SENTINEL,
                              torch.uint8 if k in S2.U8 else torch.int32) for k in S2.PER_PAIR})
            o.update(state=full((n_mf, N_CAMS, K), S2.STATE_SENTINEL, torch.uint8),
                     rot_H=full((n_mf, N_CAMS, N_HYP, 9), HS.DIST_SENTINEL, torch.float64),
                     rel_H=full((n_mf, N_CAMS, N_HYP, 12), HS.DIST_SENTINEL, torch.float64),
                     rot_valid=full((n_mf, N_CAMS, N_HYP), HS.STATE_SENTINEL, torch.uint8),
                     rel_valid=full((n_mf, N_CAMS, N_HYP), HS.STATE_SENTINEL, torch.uint8))
            out.append(o)
        block_of = torch.arange(n, device="cuda").reshape(n, 1) * K
        k0_of = torch.arange(K, device="cuda").reshape(1, K)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        T0, T1 = [sc["T0"] for sc in sw["current"]], [sc["T1"] for sc in sw["current"]]
        for j in range(STEPS):  # queued back to back
            fe.match_motion_stereo_blocks_batch_device(
                d_b0.data_ptr(), STEPS * n, d_b1.data_ptr(), n, np.arange(j * n, (j + 1) * n), np.arange(n),
                [b % N_CAMS for b in range(n)], T0, T1, d_skip[j].data_ptr(), d_m.data_ptr(), d_rows[j].data_ptr(),
                claim=dict(claimed=d_claimed[j].data_ptr(), n_claimed=d_n[j].data_ptr(), matched1_out=d_m.data_ptr()),
                stream=stream)
            with torch.cuda.stream(stream):  # the caller's addLandmark / setLandmarkId for the claimed rows
                k1 = d_rows[j][:, :, :4].contiguous().view(torch.int32).reshape(n, K).to(torch.int64)
                won = d_claimed[j] == 1
                ids = (NEW_ID + (j * n) * K + block_of + k0_of).to(torch.int32)
                d_lm0[j * n:(j + 1) * n] = torch.where(won, ids, torch.full_like(ids, -1))
                target = torch.where(won, block_of + k1, torch.full_like(k1, n * K))
                d_lm1.scatter_(0, target.reshape(-1), ids.reshape(-1))
            o = out[j]
            mf0, mf1 = np.arange(j * n_mf, (j + 1) * n_mf), np.arange(n_mf)
            fe.ransac2d2d_hypotheses_blocks_device(
                d_b0.data_ptr(), STEPS * n_mf, d_b1.data_ptr(), n_mf, mf0, mf1, list(range(N_CAMS)), d_lm0.data_ptr(),
                d_lm1.data_ptr(), None, 0, None, HS.SEED + j, N_HYP,
                fe.make_ransac2d2d_hypotheses_device(o["rot_H"].data_ptr(), o["rot_valid"].data_ptr(), o["rel_H"].data_ptr(),
                                                     o["rel_valid"].data_ptr()), stream=stream)
            res = fe.make_ransac2d2d_result_device(*[o[k].data_ptr() for k in S2.PER_CAM + S2.PER_PAIR],
                                                   state_ptr=o["state"].data_ptr(), landmark1_out_ptr=d_lm1.data_ptr())
            fe.ransac2d2d_consensus_blocks_device(
                d_b0.data_ptr(), STEPS * n_mf, d_b1.data_ptr(), n_mf, mf0, mf1, list(range(N_CAMS)), d_lm0.data_ptr(),
                d_lm1.data_ptr(), None, 0, o["rot_H"].data_ptr(), o["rot_valid"].data_ptr(), o["rel_H"].data_ptr(),
                o["rel_valid"].data_ptr(), N_HYP, res, stream=stream)
            with torch.cuda.stream(stream):  # removeObservation frees the current keypoint for the next older frame
                d_m.copy_((d_lm1[:n * K].reshape(n, K) >= 0).to(torch.uint8))
        stream.synchronize()  # the only synchronisation
        for j, st in enumerate(steps):
            claimed, n_claimed = d_claimed[j].cpu().numpy(), d_n[j].cpu().numpy()
            got = {k: v.cpu().numpy() for k, v in out[j].items()}
            for b, r in enumerate(st["res"]):
                n0 = len(r["rows"])
                assert np.array_equal(claimed[b, :n0], r["claimed"]) and int(n_claimed[b]) == r["n_claimed"], (j, b)
            for mf, (ref, hyp) in enumerate(zip(st["cons"], st["hyps"])):
                for c, h in enumerate(hyp):
                    for key in ("rot_H", "rot_valid", "rel_H", "rel_valid"):
                        assert np.array_equal(HS.bits(got[key][mf, c]), HS.bits(h[key])), (j, mf, c, key)
                head = tuple(int(got[k][mf]) for k in S2.PER_PAIR)
                assert head == (ref["total_inliers"], ref["rotation_only"], ref["success"]), (j, mf, head)
                for c, rc in enumerate(ref["cams"]):
                    per = tuple(int(got[k][mf, c]) for k in S2.PER_CAM)
                    assert per == tuple(rc[k] for k in S2.PER_CAM), (j, mf, c, per, [rc[k] for k in S2.PER_CAM])
                    n0 = len(rc["state"])
                    assert np.array_equal(got["state"][mf, c, :n0], rc["state"]), (j, mf, c)
        lm1, m = d_lm1.cpu().numpy()[:n * K].reshape(n, K), d_m.cpu().numpy()
        for b in range(n):
            n1 = len(lm1_ref[b])
            assert np.array_equal(lm1[b, :n1], lm1_ref[b]) and np.all(lm1[b, n1:] == -1), b
            assert np.array_equal(m[b, :n1], matched1_ref[b]), b
    finally:
        fe.close()


def test_general_motion_succeeds_and_pure_rotation_is_rotation_only(oracle, fp64_order):
    tree = fp64_order == "eigen_tree"
    sc = HS.motion_scene(oracle)
    hyp = HS.reference(tree, sc)
    # the lists of the restatement in the scene's pairs: the consensus' reference runs on them
    sc = dict(sc, pairs=[[dict(c, rot_H=h["rot_H"][:N_HYP], rel_H=h["rel_H"][:N_HYP], rot_valid=h["rot_valid"][:N_HYP],
                               rel_valid=h["rel_valid"][:N_HYP]) for c, h in zip(pair, hs)]
                         for pair, hs in zip(sc["pairs"], hyp)])
    refs = S2.reference(tree, sc)
    # confirmed on the CPU before the device is asked: 10 % wrong matches, relative pose taken with success; rotation only
    assert (refs[0]["success"], refs[0]["rotation_only"]) == (2, 0) and refs[0]["cams"][0]["rel_inliers"] >= 100
    assert (refs[1]["success"], refs[1]["rotation_only"]) == (1, 1)
    cams = sc["cams"]
    fe = gpu_common.make_frontend(dataclasses.replace(synth.euroc_config(), w=cams[0].w, h=cams[0].h, cams=list(cams),
                                                      max_kpts=S2.K))
    try:
        fe.set_camera(0, cams[0])
        T = S2.prepare(fe, sc)
        T["rot_H"].fill_(HS.DIST_SENTINEL), T["rel_H"].fill_(HS.DIST_SENTINEL)
        T["rot_valid"].fill_(HS.STATE_SENTINEL), T["rel_valid"].fill_(HS.STATE_SENTINEL)
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        fe.ransac2d2d_hypotheses_blocks_device(
            T["blocks0"].data_ptr(), 2, T["blocks1"].data_ptr(), 2, [0, 1], [0, 1], [0], T["lm0"].data_ptr(),
            T["lm1"].data_ptr(), None, 0, None, HS.SEED, N_HYP,
            fe.make_ransac2d2d_hypotheses_device(T["rot_H"].data_ptr(), T["rot_valid"].data_ptr(), T["rel_H"].data_ptr(),
                                                 T["rel_valid"].data_ptr()), stream=stream)
        S2.launch(fe, sc, T, stream=stream)
        stream.synchronize()
        got = S2.check(sc, T, refs, (sc["name"], fp64_order))
        assert got["success"].tolist() == [2, 1] and got["rotation_only"].tolist() == [0, 1]
    finally:
        fe.close()
