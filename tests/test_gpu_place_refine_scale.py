"""GPU: okvfe_place_refine_blocks_device at the benchmark's batch, 3072 multiframes of 2 x 700 keypoints: the shape at
which an earlier one-launch form of the refinement ended with an illegal memory access.  The scene is built as
test_gpu_batch_scale.test_place_hessian_at_the_benchmark_shape builds its own (16 distinct multiframes on the EuRoC pair,
blocks of 300 .. 700 keypoints of which most are terms), with starts as in the noisy scene (up to 3 degrees and 10 cm off
the scene's pose); the 16 anchors are compared with the restatement, and every one of the 3072 multiframes with its
anchor on the device, as bytes; the records behind the batch stay untouched.  One test, in a file of its own."""
import dataclasses

import numpy as np
import pytest

import batch_scale as BS
import gpu_common as G
import place_hessian_scenes as HS
import place_refine_device as RD
import place_refine_scenes as RS
from okvis2_amd import synth

pytestmark = [pytest.mark.gpu]
torch = pytest.importorskip("torch")

K = 700
EUROC = ("euroc", "euroc1")
FLOORS = (12, 338)   # (multiframes of the 16 with terms, fewest terms among them): those of the Hessian's test at this shape


def test_place_refine_at_the_benchmark_shape(oracle, monkeypatch):
    monkeypatch.setattr(HS, "K", K)
    oracle.set_reduction(True)
    d, n = BS.D, BS.N_BENCH
    sc = HS.general_scene(oracle, EUROC, n_mf=d, n_kps=(300, K))
    rng = np.random.default_rng(71)
    starts = [RS.perturbed(mf["pose"], rng, np.deg2rad(3.0) * rng.random(), 0.1 * rng.random()) for mf in sc["mfs"]]
    RS.with_starts(sc, rng, starts)
    refs = RS.reference(oracle, True, sc)
    terms = [r["n_terms"] for r in refs if r["n_terms"] > 0]
    assert (len(terms), min(terms)) == FLOORS, (len(terms), min(terms))
    statuses = [r["status"] for r in refs]
    print("statuses", statuses, "iterations", [r["n_iterations"] for r in refs])
    assert statuses.count(0) == d - FLOORS[0] and set(statuses) == {0, 1, 2}
    assert any(r["n_accepted"] < r["n_iterations"] for r in refs) and max(r["n_iterations"] for r in refs) == 10

    cams = sc["cams"]
    cfg = dataclasses.replace(synth.euroc_config(), w=cams[0].w, h=cams[0].h, cams=list(cams), max_kpts=K)
    fe = G.make_frontend(cfg)
    try:
        for i, c in enumerate(cams):
            fe.set_camera(i, c)
        assert fe.max_keypoints == K
        T = RD.prepare(fe, sc)
        for key in RD.OUTPUTS:
            T[key] = T[key][:d]
        C = len(cams)
        per_of = dict(dict.fromkeys(RD.OUTPUTS, 1), blocks=C, ml=C, state=C, verdict=1, hyp=1, best=1)
        modular, _ = BS.placements(n, d)
        tiled, guard = BS.tile_tensors(T, modular, d, per_of)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        RD.launch(fe, sc, tiled, n=n, stream=stream)
        stream.synchronize()
        # the anchors against the restatement (with the records behind the batch, which hold the sentinels still)
        got = {k: torch.cat([tiled[k][:d], tiled[k][n:]]).cpu().numpy() for k in RD.OUTPUTS}
        RD.check(got, refs, ("2 x 700", "anchors"))
        # every multiframe against its anchor, on the device
        for k in RD.OUTPUTS:
            assert BS.first_difference(tiled[k], d, n) is None, (k, BS.first_difference(tiled[k], d, n))
        assert BS.untouched(tiled, guard) == []
    finally:
        fe.close()
        torch.cuda.empty_cache()
