"""GPU (a context is needed, no kernel runs): every device-batch entry point that takes camera slots checks them through
one helper (rig_slots / rig_slot, okvfe_ctx.h) before anything is queued.  One row per entry point: with slot 0 set and
slot 1 never given intrinsics, a call that names slot 1 returns the status and the full okvfe_last_error text it always
returned -- the strings below are copied from the sources as they were before the helper existed, drift between the
entry points included ("frame" / "camera" / "pair" / nothing; NOT_READY against INVALID_ARGUMENT).  An empty batch over
valid slots is OKVFE_OK; an empty batch over a rig that names the bad slot is still the slot's error, because the rig
is checked first."""
import numpy as np
import pytest

import gpu_common as G
from okvis2_amd import capi, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

I = (np.eye(3).reshape(-1), np.zeros(3))
Q = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)  # a pose as seven parameters
NO_INTRINSICS = "camera slot 1 has no intrinsics (okvfe_set_camera)"


@pytest.fixture(scope="module")
def ctx():
    cfg = synth.euroc_config()
    fe = G.make_frontend(cfg, num_cameras=2)
    fe.set_camera(0, cfg.cams[0])  # slot 1 stays without intrinsics
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")  # every device pointer of every call: never touched
    return fe, buf.data_ptr(), buf


def _rows(fe, p):
    """name -> (status, message up to the slot text, call(cams, n)): `cams` are the slots of the rig or of the n frames /
    pairs, n the size of the batch"""
    F = capi.Frontend
    table = F.make_landmark_table_device(0, 0, 0, None, None, p, None, None, None, None)
    pool = F.make_landmark_pool_device()
    place = F.make_place_set_device(0, None)
    ransac = F.make_ransac_result_device(p, p, p, p)
    hyp = F.make_ransac_hypotheses_device(p, p)
    r2d = F.make_ransac2d2d_result_device(*[p] * 10)
    hessian = F.make_place_hessian_device(p, p, p)
    refine = F.make_place_refine_device(p, p)
    insert = F.make_stereo_insert_device(None, None, p, p)
    B = fe.gather_block_bytes()
    NR, IA = capi.ERR_NOT_READY, capi.ERR_INVALID_ARGUMENT
    rig = {  # the slots are the cameras of a rig, whatever the batch
        "okvfe_ransac3d2d_consensus_blocks_device": (NR, "frame 1: ", lambda c, n: fe.ransac3d2d_consensus_blocks_device(
            table, p, n, c, [I] * len(c), p, p, None, 4, ransac)),
        "okvfe_place_consensus_blocks_device": (NR, "frame 1: ", lambda c, n: fe.place_consensus_blocks_device(
            place, p, n, c, [I] * len(c), p, None, p, None, 4, 3, ransac, p)),
        "okvfe_ransac3d2d_hypotheses_blocks_device": (NR, "frame 1: ", lambda c, n: fe.ransac3d2d_hypotheses_blocks_device(
            table, p, n, c, [I] * len(c), p, None, 1, 4, hyp)),
        "okvfe_place_hypotheses_blocks_device": (NR, "frame 1: ", lambda c, n: fe.place_hypotheses_blocks_device(
            place, p, n, c, [I] * len(c), p, None, None, 1, 4, hyp)),
        "okvfe_place_hessian_blocks_device": (NR, "frame 1: ", lambda c, n: fe.place_hessian_blocks_device(
            place, p, n, c, [Q] * len(c), p, p, p, None, hessian)),
        "okvfe_place_refine_blocks_device": (NR, "frame 1: ", lambda c, n: fe.place_refine_blocks_device(
            place, p, n, c, [Q] * len(c), None, 0, None, p, p, p, None, 2, refine)),
        "okvfe_stereo_insert_blocks_device": (NR, "camera 1: ", lambda c, n: fe.stereo_insert_blocks_device(
            table, None, p, len(c) * B, B, n, [(0, 1)], c, [I] * (n * len(c)), p, p, None, insert)),
        "okvfe_ransac2d2d_consensus_blocks_device": (NR, "frame 1: ", lambda c, n: fe.ransac2d2d_consensus_blocks_device(
            p, 2, p, 2, list(range(n)), list(range(n)), c, p, p, None, 0, p, None, p, None, 4, r2d)),
    }
    frames = {  # one slot per frame or pair of the batch
        "okvfe_remove_outliers_blocks_device": (NR, "frame 1: ", lambda c, n: fe.remove_outliers_blocks_device(
            table, p, n, c, [I] * n, p, p, p)),
        "okvfe_match_to_map_table_blocks_device": (NR, "frame 1: ", lambda c, n: fe.match_to_map_table_blocks_device(
            table, p, n, c, [I] * n, 20.0, False, None, None, p, p)),
        "okvfe_match_to_map_table_uninitialised_blocks_device": (
            NR, "frame 1: ", lambda c, n: fe.match_to_map_table_uninitialised_blocks_device(
                table, pool, p, n, c, [I] * n, False, None, None, p, p, p, p, p)),
        "okvfe_match_motion_stereo_blocks_batch_device": (
            IA, "pair 1: ", lambda c, n: fe.match_motion_stereo_blocks_batch_device(p, 2, p, 2, None, None, c, [I] * n,
                                                                                   [I] * n, None, None, p)),
    }
    return rig, frames


def _raises(call, status, text):
    with pytest.raises(capi.OkvfeError) as e:
        call()
    assert e.value.status == status and str(e.value) == f"okvfe status {status}: {text}", str(e.value)


def test_a_slot_without_intrinsics(ctx):
    fe, p, _ = ctx
    rig, frames = _rows(fe, p)
    assert len(rig) + len(frames) == 12
    for name, (status, where, call) in {**rig, **frames}.items():
        _raises(lambda: call([0, 1], 2), status, f"{name}: {where}{NO_INTRINSICS}")
    # the single-block motion call: no name, no noun, INVALID_ARGUMENT
    _raises(lambda: fe.match_motion_stereo_blocks_device(1, p, p, None, None, I, I, p), capi.ERR_INVALID_ARGUMENT,
            NO_INTRINSICS)
    # the host seam of matchToMap keeps its own spelling of the same check
    kp = np.zeros(1, dtype=capi.KEYPOINT_DTYPE)
    _raises(lambda: fe.match_to_map_landmarks(1, np.zeros((1, 4)), np.ones(1), np.zeros(2, np.int32), [], [], [], [I], I, 20.0,
                                              False, np.zeros((1, 48), np.uint8), kp, np.ones(1, np.uint8)),
            capi.ERR_NOT_READY, f"okvfe_match_to_map_landmarks: {NO_INTRINSICS}")


def test_an_empty_batch_over_valid_slots_is_ok(ctx):
    fe, p, _ = ctx
    rig, frames = _rows(fe, p)
    for name, (_, _, call) in rig.items():
        call([0, 0], 0)  # (raises on any status but OKVFE_OK)
    for name, (_, _, call) in frames.items():
        call([], 0)


def test_the_rig_is_checked_before_the_empty_batch_returns(ctx):
    fe, p, _ = ctx
    rig, frames = _rows(fe, p)
    for name, (status, where, call) in rig.items():
        _raises(lambda: call([0, 1], 0), status, f"{name}: {where}{NO_INTRINSICS}")
    # (where the slots belong to the frames or pairs of the batch, an empty batch names none: the rows of `frames` have
    # no such case)
