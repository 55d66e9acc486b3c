"""GPU: the whole matchToMap chain on device-resident data, on one stream with nothing waited for in between --
okvfe_match_to_map_table_blocks_device, okvfe_ransac3d2d_consensus_blocks_device with landmark_out in place,
okvfe_remove_outliers_blocks_device in place, okvfe_match_to_map_table_uninitialised_blocks_device with the filtered
rows as previous_landmark_dev -- equal to the same chain of references (ransac_scenes.chain_scene) on one 2-camera
scene, under both orders of the FP64 sums."""
import dataclasses

import numpy as np
import pytest

import gpu_common as G
import map_scenes
import map_table_common as M
import map_table_uninit_common as U
import ransac_scenes as S
from okvis2_amd import synth

pytestmark = [pytest.mark.gpu]
torch = pytest.importorskip("torch")


@pytest.mark.parametrize("exclusive,thr", map_scenes.MODES)
def test_first_pass_consensus_removal_second_pass(oracle, fp64_order, exclusive, thr):
    tree = fp64_order == "eigen_tree"
    ch = S.chain_scene(oracle, tree, exclusive, thr)
    sc, cams, frames, cons = ch["sc"], ch["cams"], ch["frames"], ch["cons"][0]
    fe = G.make_frontend(dataclasses.replace(synth.euroc_config(), cams=cams))
    try:
        for i, c in enumerate(cams):
            fe.set_camera(i, c)
        K, nh = fe.max_keypoints, ch["H"].shape[1]
        tab = M.DeviceTable(fe, sc)
        T = U.prepare(fe, tab.n_landmarks, frames)
        H = torch.from_numpy(ch["H"]).cuda()
        head = torch.full((4,), S.SENTINEL, dtype=torch.int32, device="cuda")
        acc = torch.full((1,), S.STATE_SENTINEL, dtype=torch.uint8, device="cuda")
        hyp = torch.full((nh,), S.SENTINEL, dtype=torch.int32, device="cuda")
        state = torch.full((2, K), S.STATE_SENTINEL, dtype=torch.uint8, device="cuda")
        kept = torch.full((2,), S.SENTINEL, dtype=torch.int32, device="cuda")
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        ids = [0, 1]
        U.launch_first(fe, tab, T, ch["poses1"], ids, thr, exclusive, stream=stream)
        res = fe.make_ransac_result_device(head[0:].data_ptr(), head[1:].data_ptr(), head[2:].data_ptr(), acc.data_ptr(),
                                           hyp.data_ptr(), state.data_ptr(), None, T["lm"].data_ptr())
        fe.ransac3d2d_consensus_blocks_device(tab.desc, T["blocks"].data_ptr(), 1, ids, ch["T_SC"], T["lm"].data_ptr(),
                                              H.data_ptr(), None, nh, res, stream=stream)
        fe.remove_outliers_blocks_device(tab.desc, T["blocks"].data_ptr(), 2, ids, ch["poses2"], T["lm"].data_ptr(),
                                         T["lm"].data_ptr(), kept.data_ptr(), stream=stream)
        U.launch_second(fe, tab, T, ch["poses2"], ids, exclusive, previous="lm", stream=stream)
        got = U.collect(T, stream)
        assert head.cpu().numpy()[:3].tolist() == [cons["n_corr"], cons["best"], cons["n_inliers"]]
        assert int(acc.cpu()[0]) == cons["accepted"] == 1
        assert np.array_equal(hyp.cpu().numpy(), cons["hyp_inliers"])
        for c, fr in enumerate(frames):
            n = len(fr["desc"])
            assert np.array_equal(state.cpu().numpy()[c, :n], cons["state"][c]), ("state", c)
            filtered, k = ch["removed"][c]
            assert np.array_equal(got["lm"][c, :n], filtered), ("filtered rows", c)
            assert np.all(got["lm"][c, n:] == M.SENTINEL) and int(kept.cpu()[c]) == k, ("kept", c)
            U.check_frame(got, c, n, ch["second"][c], ("second pass", c))
    finally:
        fe.close()
