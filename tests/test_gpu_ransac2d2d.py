"""GPU: okvfe_ransac2d2d_consensus_blocks_device (ransac2d2d_consensus_kernel) against ransac2d2d_ref.py under both
orders of the FP64 sums: every output array byte for byte (counts, winners, branches, flags, per-hypothesis inliers,
match1, states, landmark rows; distances as uint64 patterns), rows at or past a block's keypoint count keep their
sentinels.  Scenes: ransac2d2d_scenes.py (general rigs of 1, 2 and 5 cameras over the four camera models, the directed
scene, the decision table and the two-camera orderings, both knife edges, the chunk edges, the block edges)."""
import dataclasses

import numpy as np
import pytest

import gpu_common as G
import ransac2d2d_scenes as S2
from okvis2_amd import capi, synth

pytestmark = [pytest.mark.gpu]
torch = pytest.importorskip("torch")

_FRONTENDS = {}


def _frontend(cams, n_set=None):
    """a context of the first camera's size with K = ransac2d2d_scenes.K whose first n_set slots hold `cams`"""
    n_set = len(cams) if n_set is None else n_set
    key = tuple((c.w, c.h, c.fu, c.fv, c.cu, c.cv, c.dist_type, tuple(c.d)) for c in cams) + (n_set,)
    if key not in _FRONTENDS:
        cfg = dataclasses.replace(synth.euroc_config(), w=cams[0].w, h=cams[0].h, cams=list(cams), max_kpts=S2.K)
        fe = G.make_frontend(cfg)
        for i, c in enumerate(cams[:n_set]):
            fe.set_camera(i, c)
        _FRONTENDS[key] = fe
    return _FRONTENDS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_frontends():
    yield
    while _FRONTENDS:
        _FRONTENDS.popitem()[1].close()


def _tree(fp64_order):
    return fp64_order == "eigen_tree"


def _run(fe, sc, refs, what, **kw):
    alias = kw.pop("alias", False)
    T = S2.prepare(fe, sc, optional=kw.pop("optional", True), alias=alias, merged=kw.pop("merged", False))
    S2.launch(fe, sc, T, **kw)
    return S2.check(sc, T, refs, what, alias=alias)


@pytest.mark.parametrize("spec", S2.GENERAL_SPECS, ids=S2.spec_id)
def test_general_scene(oracle, fp64_order, spec):
    tree = _tree(fp64_order)
    sc = S2.general_scene(oracle, spec)
    fe = _frontend(sc["cams"])
    assert fe.max_keypoints == S2.K
    refs = S2.reference(tree, sc)
    what = (sc["name"], fp64_order)
    got = _run(fe, sc, refs, what)
    assert int((got["state"] == 2).sum()) >= 16 and int((got["state"] == 1).sum()) >= 16
    _run(fe, sc, refs, what + ("in place",), alias=True)
    _run(fe, sc, refs, what + ("one block array, in place",), alias=True, merged=True)
    _run(fe, sc, refs, what + ("one block array",), merged=True)
    _run(fe, sc, refs, what + ("verdicts only",), optional=False)
    _run(fe, sc, S2.reference(tree, sc, remove_outliers=False), what + ("no removal",), remove_outliers=False)
    _run(fe, sc, S2.reference(tree, sc, use_valid=False), what + ("valid NULL",), use_valid=False)


def test_directed_scene(oracle, fp64_order):
    tree = _tree(fp64_order)
    sc = S2.directed_scene(oracle)
    fe = _frontend(sc["cams"])
    refs = S2.reference(tree, sc)
    got = _run(fe, sc, refs, (sc["name"], fp64_order))
    assert set(np.unique(got["branch"])) == {0, 1, 2}
    _run(fe, sc, refs, (sc["name"], fp64_order, "in place"), alias=True)
    _run(fe, sc, S2.reference(tree, sc, remove_outliers=False), (sc["name"], "no removal"), remove_outliers=False)


def test_decision_table(oracle, fp64_order):
    tree = _tree(fp64_order)
    for kind, invalid in (("true first", False), ("twice", False), ("better later", False), ("far", False),
                          ("true first", True)):
        sc = S2.decision_scene(oracle, kind, invalid)
        fe = _frontend(sc["cams"])
        refs = S2.reference(tree, sc)
        got = _run(fe, sc, refs, (sc["name"], fp64_order))
        if kind == "true first" and not invalid:
            n = len(S2.DECISION_CASES)
            heads = list(zip(got["branch"][:n, 0].tolist(), got["success"][:n].tolist(), got["total_inliers"][:n].tolist(),
                             got["rotation_only"][:n].tolist()))
            assert heads == [S2.DECISION_EXPECT[c] for c in S2.DECISION_CASES], heads
            assert got["removed"][n:].tolist() == [w["removed"] for w in S2.ORDER_EXPECT]
            _run(fe, sc, refs, (sc["name"], fp64_order, "in place"), alias=True)
            _run(fe, sc, S2.reference(tree, sc, remove_outliers=False), (sc["name"], "no removal"), remove_outliers=False)


def test_knife_edges(oracle, fp64_order):
    tree = _tree(fp64_order)
    sc = S2.knife_rotation(oracle, tree)
    got = _run(_frontend(sc["cams"]), sc, S2.reference(tree, sc), (sc["name"], fp64_order))
    assert list(got["state"][0, 0, sc["pairs"][0][0]["probes"]]) == [1, 2] and got["rot_inliers"][0, 0] == 13
    sc = S2.knife_relative(oracle, tree)
    got = _run(_frontend(sc["cams"]), sc, S2.reference(tree, sc), (sc["name"], fp64_order))
    print(sc["name"], got["rel_hyp_inliers"][0, 0])
    assert got["rel_hyp_inliers"][0, 0, 0] == got["rel_hyp_inliers"][0, 0, 1] + 1


def test_chunk_and_block_edges(oracle, fp64_order):
    tree = _tree(fp64_order)
    chunk = capi.Frontend._test_ransac2d2d_chunk_records()
    sc = S2.chunk_scene(oracle, chunk)
    got = _run(_frontend(sc["cams"]), sc, S2.reference(tree, sc), (sc["name"], fp64_order))
    assert got["n_corr"][:, 0].tolist() == [chunk - 1, chunk, chunk + 1, 2 * chunk + 1]
    sc = S2.edge_scene(oracle)
    got = _run(_frontend(sc["cams"]), sc, S2.reference(tree, sc), (sc["name"], fp64_order))
    assert got["n_corr"][:, 0].tolist() == [0, 0, 1, S2.K]
    _run(_frontend(sc["cams"]), sc, S2.reference(tree, sc), (sc["name"], fp64_order, "in place"), alias=True)


def test_batches_slices_and_a_side_stream(oracle, fp64_order):
    """batches of 1, 3 and 17 pairs; a call on a part of a batch touches that part only and the parts together equal
    one call; in place on a non-default stream"""
    tree = _tree(fp64_order)
    base = S2.general_scene(oracle, ("euroc", "euroc1"))
    fe = _frontend(base["cams"])
    refs3 = S2.reference(tree, base)
    for B in (1, 3, 17):
        sc = dict(base, pairs=[base["pairs"][i % 3] for i in range(B)])
        refs = [refs3[i % 3] for i in range(B)]
        T = S2.prepare(fe, sc)
        S2.launch(fe, sc, T)
        S2.check(sc, T, refs, ("batch", B, fp64_order))
    T = S2.prepare(fe, sc)
    S2.launch(fe, sc, T, first=5, count=4)
    torch.cuda.synchronize()
    untouched = [i for i in range(17) if not 5 <= i < 9]
    for key in S2.PER_CAM + S2.PER_PAIR + ("rot_hyp_inliers", "match1", "state"):
        t = T[key].cpu().numpy()[untouched]
        assert np.all(t == (S2.STATE_SENTINEL if t.dtype == np.uint8 else S2.SENTINEL)), key
    lm_out = T["lm1_out"].cpu().numpy().reshape(17, -1)
    assert np.all(lm_out[untouched] == S2.SENTINEL) and np.all(T["distance"].cpu().numpy()[untouched] == S2.DIST_SENTINEL)
    S2.launch(fe, sc, T, first=0, count=5)
    S2.launch(fe, sc, T, first=9, count=8)
    S2.check(sc, T, refs, ("slices",))
    stream = torch.cuda.Stream()
    T = S2.prepare(fe, sc, alias=True)
    S2.launch(fe, sc, T, stream=stream)
    stream.synchronize()
    S2.check(sc, T, refs, ("side stream",), alias=True)


def test_argument_errors_and_an_empty_batch(oracle):
    sc = S2.general_scene(oracle, ("euroc", "euroc1"))
    fe = _frontend(sc["cams"])
    T = S2.prepare(fe, sc)
    ptr = lambda k: T[k].data_ptr()
    res = fe.make_ransac2d2d_result_device(*[ptr(k) for k in S2.PER_CAM + S2.PER_PAIR], landmark1_out_ptr=ptr("lm1_out"))
    good = dict(blocks0_ptr=ptr("blocks0"), n_multiframes0=3, blocks1_ptr=ptr("blocks1"), n_multiframes1=3, mf0=[0, 1, 2],
                mf1=[0, 1, 2], cam_ids=[0, 1], landmark0_ptr=ptr("lm0"), landmark1_ptr=ptr("lm1"), added_ptr=None,
                n_landmarks=0, rot_hyp_ptr=ptr("rot_H"), rot_valid_ptr=None, rel_hyp_ptr=ptr("rel_H"), rel_valid_ptr=None,
                n_hyp=50, result=res)
    partial = fe.make_ransac2d2d_result_device(*[ptr(k) for k in S2.PER_CAM + S2.PER_PAIR[:2]], None)
    bad = (dict(n_hyp=0), dict(n_hyp=capi.RANSAC_MAX_HYPOTHESES + 1), dict(n_multiframes0=-1), dict(blocks0_ptr=None),
           dict(blocks1_ptr=None), dict(landmark0_ptr=None), dict(landmark1_ptr=None), dict(rot_hyp_ptr=None),
           dict(rel_hyp_ptr=None), dict(result=None), dict(result=partial), dict(threshold=float("nan")), dict(cam_ids=[]),
           dict(cam_ids=[0, 1, 0]), dict(n_landmarks=-1), dict(mf0=[0, 1, 3]), dict(mf1=[0, -1, 2]), dict(n_multiframes1=2))
    for change in bad:
        with pytest.raises(capi.OkvfeError) as e:
            fe.ransac2d2d_consensus_blocks_device(**dict(good, **change))
        assert e.value.status == capi.ERR_INVALID_ARGUMENT, change
    # with landmark1_out a current multiframe is resolved once per call; without it repeats are allowed
    with pytest.raises(capi.OkvfeError) as e:
        fe.ransac2d2d_consensus_blocks_device(**dict(good, mf1=[0, 1, 1]))
    assert e.value.status == capi.ERR_INVALID_ARGUMENT and "current multiframe 1 is named by pairs 1 and 2" in str(e.value)
    fe.ransac2d2d_consensus_blocks_device(**dict(good, mf0=[], mf1=[]))
    torch.cuda.synchronize()
    assert np.all(T["n_corr"].cpu().numpy() == S2.SENTINEL) and np.all(T["lm1_out"].cpu().numpy() == S2.SENTINEL)
    no_out = fe.make_ransac2d2d_result_device(*[ptr(k) for k in S2.PER_CAM + S2.PER_PAIR])
    fe.ransac2d2d_consensus_blocks_device(**dict(good, mf1=[1, 1, 1], result=no_out))
    torch.cuda.synchronize()
    half = _frontend(sc["cams"], n_set=1)
    with pytest.raises(capi.OkvfeError) as e:
        half.ransac2d2d_consensus_blocks_device(**good)
    assert e.value.status == capi.ERR_NOT_READY and "frame 1: camera slot 1" in str(e.value), str(e.value)
    big = G.make_frontend(dataclasses.replace(synth.euroc_config(), max_kpts=capi.RANSAC2D2D_MAX_KEYPOINTS + 1))
    try:
        big.set_camera(0, synth.euroc_config().cams[0])
        with pytest.raises(capi.OkvfeError) as e:
            big.ransac2d2d_consensus_blocks_device(**dict(good, cam_ids=[0]))
        assert e.value.status == capi.ERR_UNSUPPORTED
    finally:
        big.close()
