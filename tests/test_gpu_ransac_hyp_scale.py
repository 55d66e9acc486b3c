"""GPU: okvfe_ransac3d2d_hypotheses_blocks_device at tests/batch_scale.py's 3077 multiframes (a ragged last round of
work-groups): 16 distinct multiframes of the EuRoC pair on contexts of ransac_scenes.K keypoints, replicated in the
modular order with the sample key of a replica that of its anchor.  The 16 anchors are compared with the restatement,
every one of the 3077 multiframes with its anchor on the device, as bytes; the records behind the batch stay untouched.
One test, in a file of its own."""
import dataclasses

import numpy as np
import pytest

import batch_scale as BS
import gpu_common as G
import ransac_hyp_scenes as HS
import ransac_scenes as S
from okvis2_amd import synth

pytestmark = [pytest.mark.gpu]
torch = pytest.importorskip("torch")

OUTPUTS = ("H", "valid", "n_corr", "samples", "n_sol")


def test_hypotheses_at_3077_multiframes(oracle):
    oracle.set_reduction(True)
    d, n = BS.D, BS.N
    sc = S.general_scene(oracle, ("euroc", "euroc1"), n_mf=d)
    keys = [500 + 7 * i for i in range(d)]
    refs = HS.reference(True, sc, HS.N_HYP, keys=keys)
    assert sum(int(r["valid"].sum()) for r in refs) >= 500
    cams = sc["cams"]
    cfg = dataclasses.replace(synth.euroc_config(), w=cams[0].w, h=cams[0].h, cams=list(cams), max_kpts=S.K)
    fe = G.make_frontend(cfg)
    try:
        for i, c in enumerate(cams):
            fe.set_camera(i, c)
        tab = S.DeviceTable(fe, sc["hp"], sc["obs_begin"])
        T = HS.prepare(fe, sc, HS.N_HYP, keys=keys)
        C = len(cams)
        per_of = dict(dict.fromkeys(OUTPUTS, 1), blocks=C, lm=C, keys=1)
        modular, _ = BS.placements(n, d)
        tiled, guard = BS.tile_tensors(T, modular, d, per_of)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        HS.launch(fe, tab, sc, tiled, stream=stream, count=n)
        stream.synchronize()
        HS.check(sc, {k: (tiled[k][:d] if k in OUTPUTS else None) for k in tiled}, refs, ("3077", "anchors"))
        for k in OUTPUTS:
            assert BS.first_difference(tiled[k], d, n) is None, (k, BS.first_difference(tiled[k], d, n))
        assert BS.untouched(tiled, guard) == []
    finally:
        fe.close()
        torch.cuda.empty_cache()
