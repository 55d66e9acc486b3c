"""GPU: okvfe_ransac2d2d_consensus_blocks_device where the LDS state of ransac2d2d_consensus_kernel is used up: contexts of
1100 keypoints and of the call's limit (RANSAC2D2D_MAX_KEYPOINTS).  The record ring wraps (ring - 1, ring, ring + 1, two
laps and a partial chunk, K correspondences) and restarts per camera; the id table holds K ids in K + 1 slots, so that
the one empty slot alone ends the lookup of an absent id; probe runs of ids that share a home slot cross the table's end
into slot 0, with duplicate ids inside them (the first current keypoint of an id wins, in one tile and across tiles).
Every output byte for byte against ransac2d2d_ref.py under both orders of the FP64 sums, as in test_gpu_ransac2d2d.py;
the scenes' premises and their bite are test_capacity_scenes_host.py's."""
import dataclasses

import numpy as np
import pytest

import gpu_common as G
import ransac2d2d_scenes as S2
from okvis2_amd import capi, synth

pytestmark = [pytest.mark.gpu]
torch = pytest.importorskip("torch")

K_SMALL, K_MAX = 1100, capi.RANSAC2D2D_MAX_KEYPOINTS
N_SLOTS = K_MAX + 1
_FRONTENDS = {}


def _frontend(cams, Kc):
    key = (len(cams), Kc)
    if key not in _FRONTENDS:
        cfg = dataclasses.replace(synth.euroc_config(), w=cams[0].w, h=cams[0].h, cams=list(cams), max_kpts=Kc)
        fe = G.make_frontend(cfg)
        for i, c in enumerate(cams):
            fe.set_camera(i, c)
        _FRONTENDS[key] = fe
    assert _FRONTENDS[key].max_keypoints == Kc
    return _FRONTENDS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_frontends():
    yield
    while _FRONTENDS:
        _FRONTENDS.popitem()[1].close()


def _hooks():
    return capi.Frontend._test_ransac2d2d_ring_records(), capi.Frontend._test_ransac2d2d_chunk_records()


def _run(fe, sc, refs, what, alias=False, **kw):
    T = S2.prepare(fe, sc, alias=alias)
    S2.launch(fe, sc, T, **kw)
    return S2.check(sc, T, refs, what, alias=alias)


@pytest.mark.parametrize("Kc", (K_SMALL, K_MAX))
def test_ring_wraps(oracle, fp64_order, Kc):
    tree = fp64_order == "eigen_tree"
    ring, chunk = _hooks()
    sc = S2.ring_scene(oracle, ring, chunk, Kc)
    fe = _frontend(sc["cams"], Kc)
    refs = S2.reference(tree, sc)
    got = _run(fe, sc, refs, (sc["name"], fp64_order))
    print(sc["name"], fp64_order, "correspondences", got["n_corr"][:, 0].tolist(), "inliers", got["rel_inliers"][:, 0].tolist())
    assert got["n_corr"][:, 0].tolist() == list(S2.ring_totals(ring, chunk, Kc))
    assert int((got["state"] == 2).sum()) >= 4 * ring and int((got["state"] == 1).sum()) >= ring // 2
    _run(fe, sc, refs, (sc["name"], fp64_order, "in place"), alias=True)
    _run(fe, sc, S2.reference(tree, sc, remove_outliers=False), (sc["name"], fp64_order, "no removal"), remove_outliers=False)


def test_ring_restarts_per_camera(oracle, fp64_order):
    tree = fp64_order == "eigen_tree"
    ring, chunk = _hooks()
    sc = S2.ring_restart_scene(oracle, ring, chunk, K_SMALL)
    got = _run(_frontend(sc["cams"], K_SMALL), sc, S2.reference(tree, sc), (sc["name"], fp64_order))
    assert [tuple(r) for r in got["n_corr"].tolist()] == list(S2.ring_restart_totals(ring, chunk))


@pytest.mark.parametrize("with_added", (True, False), ids=("added", "null"))
def test_full_table(oracle, fp64_order, with_added):
    """K distinct current ids in K + 1 slots; 1000 older ids are absent: each of their lookups (in the compaction and in
    the final sweep) ends only at the one empty slot, after up to K probes"""
    tree = fp64_order == "eigen_tree"
    sc = S2.full_table_scene(oracle, K_MAX, with_added)
    fe = _frontend(sc["cams"], K_MAX)
    got = _run(fe, sc, S2.reference(tree, sc), (sc["name"], fp64_order))
    lm0 = sc["pairs"][0][0]["fr0"]["lm"]
    absent = np.isin(lm0, sc["absent"])
    print(sc["name"], fp64_order, "correspondences", int(got["n_corr"][0, 0]), "absent ids looked up", int(absent.sum()))
    assert int(absent.sum()) == 1000 and np.all(got["match1"][0, 0, :K_MAX][absent] == -1)
    assert int(got["n_corr"][0, 0]) == 2500


def test_collisions_across_the_table_end(oracle, fp64_order):
    tree = fp64_order == "eigen_tree"
    sc = S2.collision_scene(oracle, capi.Frontend._test_ransac2d2d_id_slot, N_SLOTS, K_SMALL)
    fe = _frontend(sc["cams"], K_SMALL)
    refs = S2.reference(tree, sc)
    got = _run(fe, sc, refs, (sc["name"], fp64_order))
    lm0 = sc["pairs"][0][0]["fr0"]["lm"]
    row0 = {int(l): k for k, l in enumerate(lm0.tolist()) if l >= 0}
    for lm, a, b, _ in sc["duplicates"]:  # (check has compared every row; this names the property)
        assert got["match1"][0, 0, row0[lm]] == min(a, b), (lm, a, b)
    assert np.all(got["match1"][0, 0, [row0[int(i)] for i in sc["clusters"]["absent"]]] == -1)
    _run(fe, sc, refs, (sc["name"], fp64_order, "in place"), alias=True)
