"""GPU: okvfe_ransac2d2d_hypotheses_blocks_device (ransac2d2d_hypotheses_kernel) against ransac2d2d_hyp_ref.py under
both orders of the FP64 sums: both hypothesis lists, their validity bytes, the samples, the root counts and the
correspondence counts byte for byte (doubles as uint64 patterns).  Scenes: ransac2d2d_scenes' general rigs of 1, 2 and 5
cameras over the four camera models, and ransac2d2d_hyp_scenes' counts (0, 1, 9, 10, 11, 64, 65, K correspondences; blocks
of 0, 1 and K keypoints) and directed cases."""
import dataclasses

import numpy as np
import pytest

import gpu_common as G
import ransac2d2d_hyp_scenes as HS
import ransac2d2d_scenes as S2
from okvis2_amd import capi, synth

pytestmark = [pytest.mark.gpu]
torch = pytest.importorskip("torch")

_FRONTENDS = {}


def _frontend(cams, max_kpts=S2.K):
    key = tuple((c.w, c.h, c.fu, c.fv, c.cu, c.cv, c.dist_type, tuple(c.d)) for c in cams) + (max_kpts,)
    if key not in _FRONTENDS:
        cfg = dataclasses.replace(synth.euroc_config(), w=cams[0].w, h=cams[0].h, cams=list(cams), max_kpts=max_kpts)
        fe = G.make_frontend(cfg)
        for i, c in enumerate(cams):
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


def _run(fe, sc, refs, what, n_hyp=50, **kw):
    T = HS.prepare(fe, sc, n_hyp, optional=kw.pop("optional", True), keys=kw.pop("keys", None), merged=kw.pop("merged", False))
    HS.launch(fe, sc, T, n_hyp, **kw)
    return HS.check(sc, T, refs, what, n_hyp)


@pytest.mark.parametrize("spec", S2.GENERAL_SPECS, ids=S2.spec_id)
def test_general_scene(oracle, fp64_order, spec):
    """rigs of 1, 2 and 5 cameras; the optional outputs present and absent; both sides in one block array"""
    tree = _tree(fp64_order)
    sc = S2.general_scene(oracle, spec)
    fe = _frontend(sc["cams"])
    refs = HS.reference(tree, sc)
    what = (sc["name"], fp64_order)
    got = _run(fe, sc, refs, what)
    assert int(got["rel_valid"].sum()) >= 50 and int(got["rot_valid"].sum()) >= 50, "the scene solves nothing"
    _run(fe, sc, refs, what + ("required only",), optional=False)
    _run(fe, sc, refs, what + ("one block array",), merged=True)


def test_counts_and_block_edges(oracle, fp64_order):
    tree = _tree(fp64_order)
    sc = HS.count_scene(oracle)
    fe = _frontend(sc["cams"])
    got = _run(fe, sc, HS.reference(tree, sc), (sc["name"], fp64_order))
    n = len(HS.COUNTS)
    assert got["n_corr"][:n, 0].tolist() == list(HS.COUNTS)
    assert got["n_corr"][n:, 0].tolist() == [0, 0, 1, S2.K]
    for pi, count in enumerate(got["n_corr"][:, 0].tolist()):
        if count < 10:   # skipped by the reference (:2300): nothing drawn, nothing solved
            assert not got["rot_valid"][pi].any() and not got["rel_valid"][pi].any()
            assert np.all(got["rot_samples"][pi] == -1) and np.all(got["rel_samples"][pi] == -1)
            assert np.all(got["rot_H"][pi] == 0.0) and np.all(got["rel_H"][pi] == 0.0)
        else:
            assert got["rel_samples"][pi].min() >= 0 and got["rot_valid"][pi].any()
            assert all(len(set(row)) == 8 for row in got["rel_samples"][pi, 0].tolist()), "a sample drawn twice"


def test_directed_scene(oracle, fp64_order):
    tree = _tree(fp64_order)
    sc = HS.directed_scene(oracle)
    fe = _frontend(sc["cams"])
    refs, census = HS.directed_reference(tree, sc)
    print({k: {b: v for b, v in c.items() if v} for k, c in census.items()})
    HS.assert_directed_branches(refs, census)
    got = _run(fe, sc, refs, (sc["name"], fp64_order), n_hyp=HS.MAX_HYP)
    kinds = {k: i for i, k in enumerate(HS.DIRECTED)}
    assert got["rel_valid"][kinds["general"], 0].sum() > got["rel_valid"][kinds["duplicates"], 0].sum()
    no_root = (got["n_roots"][kinds["unrelated"], 0] == 0) & (got["rel_valid"][kinds["unrelated"], 0] == 0)
    assert int(no_root.sum()) >= census["unrelated"]["no_root"] >= 2 and not got["rel_H"][kinds["unrelated"], 0][no_root].any()


def test_hypothesis_counts(oracle, fp64_order):
    """n_hyp 1, 50 and the maximum: hypothesis h does not depend on how many there are"""
    tree = _tree(fp64_order)
    sc = S2.general_scene(oracle, ("euroc", "euroc1"))
    fe = _frontend(sc["cams"])
    refs = HS.reference(tree, sc)
    for n_hyp in (1, 50, capi.RANSAC_MAX_HYPOTHESES):
        _run(fe, sc, refs, (sc["name"], fp64_order, n_hyp), n_hyp=n_hyp)


def test_batches_keys_slices_and_a_side_stream(oracle, fp64_order):
    """batches of 1, 3 and 257 pairs; a pair keeps its bytes wherever its key stands in the batch; a call on a part of
    a batch touches that part only and the parts together equal one call; a non-default stream"""
    tree = _tree(fp64_order)
    base = S2.general_scene(oracle, ("euroc", "euroc1"))
    fe = _frontend(base["cams"])
    refs3 = HS.reference(tree, base)
    n_hyp = 50
    one = dict(base, pairs=base["pairs"][:1])
    _run(fe, one, refs3[:1], ("batch", 1, fp64_order), n_hyp=n_hyp)
    for B in (3, 257):
        order = np.random.default_rng(B).permutation(B)    # the pair with key k stands at a place of its own
        sc = dict(base, pairs=[base["pairs"][i % 3] for i in order])
        refs = [refs3[i % 3] for i in order]
        _run(fe, sc, refs, ("batch", B, fp64_order), n_hyp=n_hyp, keys=[i % 3 for i in order])
    keys = [i % 3 for i in order]
    T = HS.prepare(fe, sc, n_hyp, keys=keys)
    HS.launch(fe, sc, T, n_hyp, first=5, count=4)
    got = HS.download(T)
    untouched = [i for i in range(257) if not 5 <= i < 9]
    for key, t in got.items():
        fill = {np.float64: HS.DIST_SENTINEL, np.uint8: HS.STATE_SENTINEL, np.int32: HS.SENTINEL}[t.dtype.type]
        assert np.all(t[untouched] == fill), key
    HS.launch(fe, sc, T, n_hyp, first=0, count=5)
    HS.launch(fe, sc, T, n_hyp, first=9, count=248)
    HS.check(sc, T, refs, ("slices",), n_hyp)
    stream = torch.cuda.Stream()
    T = HS.prepare(fe, sc, n_hyp, keys=keys)
    HS.launch(fe, sc, T, n_hyp, stream=stream)
    stream.synchronize()
    HS.check(sc, T, refs, ("side stream",), n_hyp)


def test_argument_errors_and_an_empty_batch(oracle):
    sc = S2.general_scene(oracle, ("euroc", "euroc1"))
    fe = _frontend(sc["cams"])
    n_hyp = 4
    T = HS.prepare(fe, sc, n_hyp)
    ptr = lambda k: T[k].data_ptr()
    res = fe.make_ransac2d2d_hypotheses_device(ptr("rot_H"), ptr("rot_valid"), ptr("rel_H"), ptr("rel_valid"))
    good = dict(blocks0_ptr=ptr("blocks0"), n_multiframes0=3, blocks1_ptr=ptr("blocks1"), n_multiframes1=3, mf0=[0, 1, 2],
                mf1=[0, 1, 2], cam_ids=[0, 1], landmark0_ptr=ptr("lm0"), landmark1_ptr=ptr("lm1"), added_ptr=None,
                n_landmarks=0, sample_keys_ptr=None, seed=1, n_hyp=n_hyp, result=res)
    fe.ransac2d2d_hypotheses_blocks_device(**good)
    partial = fe.make_ransac2d2d_hypotheses_device(ptr("rot_H"), ptr("rot_valid"), ptr("rel_H"), None)
    for change in (dict(blocks0_ptr=None), dict(blocks1_ptr=None), dict(landmark0_ptr=None), dict(landmark1_ptr=None),
                   dict(n_hyp=0), dict(n_hyp=capi.RANSAC_MAX_HYPOTHESES + 1), dict(n_landmarks=-1), dict(result=None),
                   dict(result=partial), dict(cam_ids=[]), dict(mf0=[0, 1, 3]), dict(mf1=[0, -1, 2]),
                   dict(n_multiframes0=-1), dict(cam_ids=[0, 1, 0]), dict(n_multiframes1=2)):
        with pytest.raises(capi.OkvfeError) as e:
            fe.ransac2d2d_hypotheses_blocks_device(**dict(good, **change))
        assert e.value.status == capi.ERR_INVALID_ARGUMENT, change
    torch.cuda.synchronize()
    before = {k: T[k].clone() for k in ("rot_H", "rel_H", "rot_valid", "rel_valid")}
    for k in before:
        T[k].fill_(3)
    fe.ransac2d2d_hypotheses_blocks_device(**dict(good, mf0=[], mf1=[]))      # an empty batch launches nothing
    torch.cuda.synchronize()
    assert all(bool((T[k] == 3).all()) for k in before)
    fe.ransac2d2d_hypotheses_blocks_device(**dict(good, mf1=[1, 1, 1]))       # a current multiframe may serve many pairs
    torch.cuda.synchronize()
    assert all(torch.equal(before[k][1], T[k][1]) for k in before), "pair 1 is (1, 1) in both calls"
    big = G.make_frontend(dataclasses.replace(synth.euroc_config(), max_kpts=capi.RANSAC2D2D_MAX_KEYPOINTS + 1))
    try:
        big.set_camera(0, synth.euroc_config().cams[0])
        with pytest.raises(capi.OkvfeError) as e:
            big.ransac2d2d_hypotheses_blocks_device(**dict(good, cam_ids=[0]))
        assert e.value.status == capi.ERR_UNSUPPORTED
    finally:
        big.close()
