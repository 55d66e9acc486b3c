"""GPU: okvfe_ransac2d2d_hypotheses_blocks_device at tests/batch_scale.py's 3077 pairs (a ragged last round of
work-groups): 16 distinct one-camera pairs of 300 .. 690 correspondences on a context of 700 keypoints (several tiles of
older keypoints per block), replicated in the modular order with the sample key of a replica that of its anchor.  The 16
anchors are compared with the restatement, every one of the 3077 pairs with its anchor on the device, as bytes; the
records behind the batch stay untouched.  One test, in a file of its own."""
import dataclasses

import numpy as np
import pytest

import batch_scale as BS
import gpu_common as G
import ransac2d2d_hyp_scenes as HS
import ransac2d2d_scenes as S2
from okvis2_amd import synth

pytestmark = [pytest.mark.gpu]
torch = pytest.importorskip("torch")

K_SCALE = 700
N_HYP = 50
OUTPUTS = tuple(HS.OUT) + ("n_corr",)


def scale_scene(oracle, d, seed=83):
    rng = np.random.default_rng(seed)
    pairs = []
    for i in range(d):
        total = 300 + (390 * i) // (d - 1)
        nD = total // 10
        fr0, fr1, _ = S2.hand_camera(oracle, rng, 0, 0, total - nD, nD, free0=min(10, K_SCALE - total), free1=min(6, K_SCALE - total))
        pairs.append([HS._entry(fr0, fr1)])
    return S2.scene("hyp-scale", S2.euroc_pair()[:1], pairs)


def test_hypotheses_at_3077_pairs(oracle):
    oracle.set_reduction(True)
    d, n = BS.D, BS.N
    sc = scale_scene(oracle, d)
    keys = [500 + 7 * i for i in range(d)]
    refs = HS.reference(True, sc, keys=keys)
    assert sum(int(r[0]["rel_valid"][:N_HYP].sum()) for r in refs) >= 500
    assert [r[0]["n_corr"] for r in refs][::d - 1] == [300, 690]
    cams = sc["cams"]
    cfg = dataclasses.replace(synth.euroc_config(), w=cams[0].w, h=cams[0].h, cams=list(cams), max_kpts=K_SCALE)
    fe = G.make_frontend(cfg)
    try:
        fe.set_camera(0, cams[0])
        assert fe.max_keypoints == K_SCALE
        T = HS.prepare(fe, sc, N_HYP, keys=keys)
        per_of = dict(dict.fromkeys(OUTPUTS, 1), blocks0=1, blocks1=1, lm0=1, lm1=1, keys=1)
        modular, _ = BS.placements(n, d)
        tiled, guard = BS.tile_tensors(T, modular, d, per_of)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        ptr = lambda k: tiled[k].data_ptr()
        res = fe.make_ransac2d2d_hypotheses_device(ptr("rot_H"), ptr("rot_valid"), ptr("rel_H"), ptr("rel_valid"), ptr("n_corr"),
                                                   ptr("rot_samples"), ptr("rel_samples"), ptr("n_roots"))
        mf = np.arange(n, dtype=np.int32)
        fe.ransac2d2d_hypotheses_blocks_device(ptr("blocks0"), n, ptr("blocks1"), n, mf, mf, [0], ptr("lm0"), ptr("lm1"), None, 0,
                                               ptr("keys"), HS.SEED, N_HYP, res, stream)
        stream.synchronize()
        HS.check(sc, {k: (tiled[k][:d] if k in OUTPUTS else None) for k in tiled}, refs, ("3077", "anchors"), N_HYP)
        for k in OUTPUTS:
            assert BS.first_difference(tiled[k], d, n) is None, (k, BS.first_difference(tiled[k], d, n))
        assert BS.untouched(tiled, guard) == []
    finally:
        fe.close()
        torch.cuda.empty_cache()
