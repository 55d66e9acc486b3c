"""GPU: the motion-stereo sweep before initialisation, chained on one stream without a host synchronisation: per older
frame okvfe_match_motion_stereo_blocks_batch_device with claims, landmark ids assigned to the claimed rows by torch ops
on the same stream (the caller's addLandmark / setLandmarkId), okvfe_ransac2d2d_consensus_blocks_device with
landmark1_out == landmark1_dev, and matched1 = (id >= 0) for the next step (removeObservation frees the keypoint).
Two steps over 4 current multiframes of 2 cameras against the chain of references (motion_claim_ref.py for the rows and
claims, ransac2d2d_ref.py for the consensus)."""
import numpy as np
import pytest

import gate_scenes as G
import motion_claim_ref as M
import ransac2d2d_ref as R2
import ransac2d2d_scenes as S2
from okvis2_amd import capi, multigpu, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

W = H = 1024
K = 512
REC = capi.MOTION_MATCH_DTYPE.itemsize
FILL = 0xA5
STEPS, N_CAMS, N_HYP = 2, 2, 8
KNOWN_ID = 900000   # ids of the keypoints that carry a landmark before the sweep
NEW_ID = 1000       # ids handed out by the sweep: NEW_ID + (step n_blocks + block) K + k0


def _cam(sc):
    return M.with_frame_size(sc["cam"], W, H)


def _frames(sw, j, b, lm0, lm1):
    sc, old = sw["current"][b], sw["older"][j][b]
    zeros = lambda n: np.zeros((n, 48), np.uint8)
    return (dict(kps=old["kp0"], desc=zeros(len(old["kp0"])), bp=old["bp0"], bpv=old["bv0"], lm=lm0),
            dict(kps=sc["kp1"], desc=zeros(len(sc["kp1"])), bp=sc["bp1"], bpv=sc["bv1"], lm=lm1))


def _lists(sw, rng):
    """per (step, block): the hypothesis lists around the true relative pose of the block's camera"""
    out = []
    for j in range(STEPS):
        out.append([S2._hypotheses(*S2._relative(sc["T0"], sc["T1"]), N_HYP, rng, n_random=2) for sc in sw["current"]])
    return out


def reference_chain(tree, sw, lists):
    n = len(sw["current"])
    matched1 = [m.copy() for m in sw["matched1"]]
    lm1 = [np.where(m != 0, KNOWN_ID + np.arange(len(m)), -1).astype(np.int32) for m in matched1]
    fus = [sw["current"][c]["cam"].fu for c in range(N_CAMS)]
    steps = []
    for j in range(STEPS):
        res, lm0 = [], []
        for b, (sc, old) in enumerate(zip(sw["current"], sw["older"][j])):
            pair = dict(sc, **{k: old[k] for k in ("d0", "kp0", "bp0", "bv0")})
            rows = M.match_rows(pair, old["skip0"], matched1[b], _cam(sc))
            claimed, n_claimed, _ = M.claim_loop(rows, len(rows), matched1[b])
            ids = NEW_ID + (j * n + b) * K + np.arange(len(rows))
            l0 = np.where(claimed != 0, ids, -1).astype(np.int32)
            lm1[b][rows["k1"][claimed != 0]] = l0[claimed != 0]
            lm0.append(l0)
            res.append(dict(rows=rows, claimed=claimed, n_claimed=n_claimed))
        cons = []
        for mf in range(n // N_CAMS):
            cams = []
            for c in range(N_CAMS):
                b = mf * N_CAMS + c
                fr0, fr1 = _frames(sw, j, b, lm0[b], lm1[b])
                cams.append(S2.cam_entry(fr0, fr1, *lists[j][b]))
            ref = R2.run(tree, cams, fus)
            for c in range(N_CAMS):
                b = mf * N_CAMS + c
                lm1[b] = ref["cams"][c]["landmark1_out"].copy()
                matched1[b] = (lm1[b] >= 0).astype(np.uint8)
            cons.append(ref)
        steps.append(dict(res=res, cons=cons, lm0=lm0))
    return steps, lm1, matched1


def _pad(a, fill, dtype):
    out = np.full(K, fill, dtype)
    out[:len(a)] = a
    return out


def test_two_step_sweep_with_the_consensus_after_each_step(oracle, fp64_order):
    tree = fp64_order == "eigen_tree"
    cams = [synth.euroc_config().cams[0], synth.tumvi1024_config().cams[0]]
    sw = M.sweep_scene(cams, ("euroc", "tumvi"), steps=STEPS)
    n = len(sw["current"])
    n_mf = n // N_CAMS
    lists = _lists(sw, np.random.default_rng(7))
    steps, lm1_ref, matched1_ref = reference_chain(tree, sw, lists)
    # the chain does something: claims at both steps, a camera that removes outliers, a success
    assert all(sum(r["n_claimed"] for r in st["res"]) >= 50 for st in steps)
    assert any(c["removed"] for st in steps for ref in st["cons"] for c in ref["cams"])
    assert any(ref["total_inliers"] >= 0 for st in steps for ref in st["cons"])

    fe = capi.Frontend(W, H, 38.0, 0, 150, K, match_threshold=G.THRESHOLD, max_batch=1, num_cameras=N_CAMS)
    try:
        assert fe.max_keypoints == K
        for slot, cam in enumerate(cams):
            fe.set_camera(slot, M.with_frame_size(cam, W, H))
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        block = lambda kp, d, bp, bv: multigpu.pack_block_host(K, kp, d, bp, bv)
        d_b1 = dev(np.stack([block(sc["kp1"], sc["d1"], sc["bp1"], sc["bv1"]) for sc in sw["current"]]))
        d_b0 = dev(np.stack([block(o["kp0"], o["d0"], o["bp0"], o["bv0"]) for step in sw["older"] for o in step]))
        d_m = dev(np.stack([_pad(m, 0, np.uint8) for m in sw["matched1"]]))
        d_skip = [dev(np.stack([_pad(o["skip0"], 0, np.uint8) for o in step])) for step in sw["older"]]
        d_lm1 = dev(np.stack([_pad(np.where(m != 0, KNOWN_ID + np.arange(len(m)), -1), -1, np.int32) for m in sw["matched1"]]))
        d_lm1 = torch.cat([d_lm1.reshape(-1), torch.zeros(1, dtype=torch.int32, device="cuda")])  # + a slot nobody reads
        d_lm0 = torch.full((STEPS * n, K), -1, dtype=torch.int32, device="cuda")
        d_rot = [dev(np.stack([l[0] for l in lists[j]])) for j in range(STEPS)]
        d_rel = [dev(np.stack([l[1] for l in lists[j]])) for j in range(STEPS)]
        d_rows = [torch.full((n, K, REC), FILL, dtype=torch.uint8, device="cuda") for _ in range(STEPS)]
        d_claimed = [torch.full((n, K), FILL, dtype=torch.uint8, device="cuda") for _ in range(STEPS)]
        d_n = [torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(STEPS)]
        out = []
        for j in range(STEPS):
            full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
            o = {k: full((n_mf, N_CAMS), S2.STATE_SENTINEL if k in S2.U8 else S2.SENTINEL,
                         torch.uint8 if k in S2.U8 else torch.int32) for k in S2.PER_CAM}
            o.update({k: full((n_mf,), S2.STATE_SENTINEL if k in S2.U8 else S2.SENTINEL,
                              torch.uint8 if k in S2.U8 else torch.int32) for k in S2.PER_PAIR})
            o.update(match1=full((n_mf, N_CAMS, K), S2.SENTINEL, torch.int32),
                     state=full((n_mf, N_CAMS, K), S2.STATE_SENTINEL, torch.uint8))
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
            res = fe.make_ransac2d2d_result_device(
                *[o[k].data_ptr() for k in S2.PER_CAM + S2.PER_PAIR], match1_ptr=o["match1"].data_ptr(),
                state_ptr=o["state"].data_ptr(), landmark1_out_ptr=d_lm1.data_ptr())
            fe.ransac2d2d_consensus_blocks_device(
                d_b0.data_ptr(), STEPS * n_mf, d_b1.data_ptr(), n_mf, np.arange(j * n_mf, (j + 1) * n_mf), np.arange(n_mf),
                list(range(N_CAMS)), d_lm0.data_ptr(), d_lm1.data_ptr(), None, 0, d_rot[j].data_ptr(), None,
                d_rel[j].data_ptr(), None, N_HYP, res, stream=stream)
            with torch.cuda.stream(stream):  # removeObservation frees the current keypoint for the next older frame
                d_m.copy_((d_lm1[:n * K].reshape(n, K) >= 0).to(torch.uint8))
        stream.synchronize()  # the only synchronisation
        for j, st in enumerate(steps):
            rows, claimed, n_claimed = d_rows[j].cpu().numpy(), d_claimed[j].cpu().numpy(), d_n[j].cpu().numpy()
            got = {k: v.cpu().numpy() for k, v in out[j].items()}
            for b, r in enumerate(st["res"]):
                n0 = len(r["rows"])
                mine = rows[b, :n0].reshape(-1).view(capi.MOTION_MATCH_DTYPE)
                for f in ("k1", "dist", "initialisable", "accepted"):
                    assert np.array_equal(mine[f], r["rows"][f]), (j, b, f)
                assert np.array_equal(claimed[b, :n0], r["claimed"]) and int(n_claimed[b]) == r["n_claimed"], (j, b)
            for mf, ref in enumerate(st["cons"]):
                head = tuple(int(got[k][mf]) for k in S2.PER_PAIR)
                assert head == (ref["total_inliers"], ref["rotation_only"], ref["success"]), (j, mf, head)
                for c, rc in enumerate(ref["cams"]):
                    per = tuple(int(got[k][mf, c]) for k in S2.PER_CAM)
                    assert per == tuple(rc[k] for k in S2.PER_CAM), (j, mf, c, per, [rc[k] for k in S2.PER_CAM])
                    n0 = len(rc["match1"])
                    assert np.array_equal(got["match1"][mf, c, :n0], rc["match1"]), (j, mf, c)
                    assert np.array_equal(got["state"][mf, c, :n0], rc["state"]), (j, mf, c)
        lm1, m = d_lm1.cpu().numpy()[:n * K].reshape(n, K), d_m.cpu().numpy()
        for b in range(n):
            n1 = len(lm1_ref[b])
            assert np.array_equal(lm1[b, :n1], lm1_ref[b]) and np.all(lm1[b, n1:] == -1), b
            assert np.array_equal(m[b, :n1], matched1_ref[b]), b
    finally:
        fe.close()
