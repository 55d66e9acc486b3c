"""GPU: okvfe_ransac3d2d_hypotheses_blocks_device and okvfe_place_hypotheses_blocks_device (ransac_hypotheses_kernel)
against the restatement tests/ransac_hyp_ref.py under both orders of the FP64 sums: hypotheses byte for byte (a NaN
standing for any NaN), hyp_valid, samples, n_solutions and n_correspondences for equality.  Every census scene of
ransac_hyp_scenes.py (rigs of 1, 2 and 5 cameras over the four camera models, noise-free and noisy, and the directed
cases); batches of 1, 3, 17 and 257 with 50, 50, 64 and 1 hypotheses; 0, 3, 4 and 5 correspondences, 255 / 256 / 257
across the ballot tiles, a camera with 3 correspondences beside one with 40; sample keys (a shuffled batch gives the
shuffled rows, equal keys give equal rows); slices of a batch leave the rest untouched; a side stream; the place policy
with its gate; the argument errors."""
import dataclasses

import numpy as np
import pytest

import gpu_common as G
import ransac_hyp_scenes as HS
import ransac_scenes as S
from okvis2_amd import capi, synth

pytestmark = [pytest.mark.gpu]
torch = pytest.importorskip("torch")

_FRONTENDS = {}


def _frontend(cams, n_set=None, Kc=S.K, octaves=0):
    n_set = len(cams) if n_set is None else n_set
    key = tuple((c.w, c.h, c.fu, c.fv, c.cu, c.cv, c.dist_type, tuple(c.d)) for c in cams) + (n_set, Kc, octaves)
    if key not in _FRONTENDS:
        cfg = dataclasses.replace(synth.euroc_config(), w=cams[0].w, h=cams[0].h, cams=list(cams), max_kpts=Kc,
                                  octaves=octaves)
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


def _run(fe, sc, refs, n_hyp, what, place=False, gates=None, **kw):
    tab = S.DeviceTable(fe, sc["hp"], sc["obs_begin"])
    T = HS.prepare(fe, sc, n_hyp, gates=gates, **kw)
    HS.launch(fe, tab, sc, T, place=place)
    return HS.check(sc, T, refs, what)


def test_every_census_scene(oracle, fp64_order):
    tree = _tree(fp64_order)
    valid = 0
    for sc, n_hyp in HS.census_scenes(oracle):
        fe = _frontend(sc["cams"])
        assert fe.max_keypoints == HS.K
        refs = HS.reference(tree, sc, n_hyp)
        got = _run(fe, sc, refs, n_hyp, (sc["name"], fp64_order))
        valid += int(got["valid"].sum())
        _run(fe, sc, refs, n_hyp, (sc["name"], fp64_order, "required outputs only"), optional=False)
    assert valid >= 1000


def _counts_scene(oracle):
    """2 cameras: multiframes with 0, 3, 4 and 5 correspondences in the first camera and none in the second; 3 beside
    40; 40 beside 3"""
    base = S.general_scene(oracle, ("euroc", "euroc1"))
    mf = base["mfs"][0]
    mfs = []
    for n0, n1 in ((0, 0), (3, 0), (4, 0), (5, 0), (3, 40), (40, 3)):
        frames = []
        for fr, n in zip(mf["frames"], (n0, n1)):
            lm = fr["lm"].copy()
            lm[np.flatnonzero(lm >= 0)[n:]] = -1
            frames.append(dict(fr, lm=lm))
        mfs.append(dict(mf, frames=frames))
    return dict(base, name="counts", mfs=mfs)


def test_correspondence_counts(oracle, fp64_order):
    tree = _tree(fp64_order)
    sc = _counts_scene(oracle)
    fe = _frontend(sc["cams"])
    refs = HS.reference(tree, sc, HS.N_HYP)
    got = _run(fe, sc, refs, HS.N_HYP, (sc["name"], fp64_order))
    assert got["n_corr"].tolist() == [0, 3, 4, 5, 43, 43]
    assert not got["valid"][:2].any() and np.all(got["samples"][0] == -1) and np.all(got["samples"][1, :, 1:] == -1)
    assert np.all(got["samples"][1, :, 0] >= 0) and np.all(got["samples"][2:4] >= 0)
    # 3 beside 40: a first draw in the small camera ends the hypothesis, one in the large camera stays there
    for mi, small in ((4, 0), (5, 1)):
        first = got["samples"][mi, :, 0] // HS.K
        assert set(first.tolist()) == {0, 1}
        assert np.all(got["samples"][mi][first == small][:, 1:] == -1) and not got["valid"][mi][first == small].any()
        assert np.all(got["samples"][mi][first != small] // HS.K == 1 - small)
    # 255, 256, 257 and 513 correspondences over three cameras: list positions across the tiles of 256 slots
    chunk = S.chunk_scene(oracle, 256)
    got = _run(_frontend(chunk["cams"]), chunk, HS.reference(tree, chunk, HS.N_HYP), HS.N_HYP, (chunk["name"], fp64_order))
    assert got["n_corr"].tolist() == [255, 256, 257, 513]


def test_batches_slices_keys_and_a_side_stream(oracle, fp64_order):
    tree = _tree(fp64_order)
    base = S.general_scene(oracle, ("euroc", "euroc1"))
    fe = _frontend(base["cams"])
    tab = S.DeviceTable(fe, base["hp"], base["obs_begin"])
    for B, n_hyp in ((1, 50), (3, 50), (17, 64), (257, 1)):
        sc = dict(base, mfs=[base["mfs"][i % 3] for i in range(B)])
        refs = HS.reference(tree, sc, n_hyp)   # (no keys: multiframe m samples under the key m)
        T = HS.prepare(fe, sc, n_hyp)
        assert T["keys"] is None
        HS.launch(fe, tab, sc, T)
        HS.check(sc, T, refs, ("batch", B, fp64_order))
    # slices of a batch of 17 under explicit keys: [5, 9) first, the rest untouched; then the rest
    sc = dict(base, mfs=[base["mfs"][i % 3] for i in range(17)])
    keys = [1000 + 3 * i for i in range(17)]
    refs = HS.reference(tree, sc, 50, keys=keys)
    T = HS.prepare(fe, sc, 50, keys=keys)
    HS.launch(fe, tab, sc, T, first=5, count=4)
    HS.check(sc, T, refs, ("slice",), only=range(5, 9))
    HS.launch(fe, tab, sc, T, first=0, count=5)
    HS.launch(fe, tab, sc, T, first=9, count=8)
    straight = HS.check(sc, T, refs, ("slices",))
    # the same multiframes shuffled, keys with them, on a side stream: the shuffled rows
    order = np.random.default_rng(5).permutation(17)
    shuffled = dict(sc, mfs=[sc["mfs"][i] for i in order])
    T = HS.prepare(fe, shuffled, 50, keys=[keys[i] for i in order])
    stream = torch.cuda.Stream()
    HS.launch(fe, tab, shuffled, T, stream=stream)
    stream.synchronize()
    got = HS.check(shuffled, T, [refs[i] for i in order], ("shuffled", fp64_order))
    for k in ("H", "valid", "samples", "n_sol", "n_corr"):
        assert np.array_equal(got[k].view(np.uint8), straight[k][order].view(np.uint8)), k
    # replicas under one key: equal rows (multiframes 0, 3, 6, .. are the same multiframe)
    T = HS.prepare(fe, sc, 50, keys=[77] * 17)
    HS.launch(fe, tab, sc, T)
    got = HS.download(T)
    for i in range(3, 17):
        for k in ("H", "valid", "samples", "n_sol"):
            assert np.array_equal(got[k][i].view(np.uint8), got[k][i % 3].view(np.uint8)), (i, k)
    assert not np.array_equal(got["samples"][0], got["samples"][1])


def test_place_policy_and_its_gate(oracle, fp64_order):
    """the kPlace policy: no test on the observations (a table without them gives other correspondences under the 3d2d
    policy), and gate 0 solves nothing"""
    tree = _tree(fp64_order)
    base = S.general_scene(oracle, "hilti")
    sc = dict(base, obs_begin=np.zeros_like(base["obs_begin"]))     # no landmark has an observation
    fe = _frontend(sc["cams"])
    for gates in (None, [0, 1, 2]):
        refs = HS.reference(tree, sc, HS.N_HYP, place=True, gates=gates)
        got = _run(fe, sc, refs, HS.N_HYP, (sc["name"], "place", gates, fp64_order), place=True, gates=gates)
        assert min(got["n_corr"].tolist()) > 100
        if gates is not None:
            assert not got["valid"][0].any() and np.all(got["samples"][0] == -1) and not got["H"][0].any()
            assert got["valid"][1].any() and got["valid"][2].any()
    got = _run(fe, sc, HS.reference(tree, sc, HS.N_HYP), HS.N_HYP, (sc["name"], "3d2d without observations", fp64_order))
    assert got["n_corr"].tolist() == [0, 0, 0]


def test_argument_errors_and_an_empty_batch(oracle):
    sc = S.general_scene(oracle, ("euroc", "euroc1"))
    fe = _frontend(sc["cams"])
    tab = S.DeviceTable(fe, sc["hp"], sc["obs_begin"])
    T = HS.prepare(fe, sc, 50)
    res = fe.make_ransac_hypotheses_device(T["H"].data_ptr(), T["valid"].data_ptr())
    good = dict(table=tab.desc, blocks_ptr=T["blocks"].data_ptr(), n_multiframes=3, cam_ids=[0, 1], poses_T_SC=sc["T_SC"],
                landmark_ptr=T["lm"].data_ptr(), sample_keys_ptr=None, seed=1, n_hyp=50, result=res)
    bad = (dict(n_hyp=0), dict(n_hyp=capi.RANSAC_MAX_HYPOTHESES + 1), dict(n_multiframes=-1), dict(blocks_ptr=None),
           dict(landmark_ptr=None), dict(result=None), dict(table=None), dict(cam_ids=[], poses_T_SC=[]),
           dict(cam_ids=[0, 1, 0], poses_T_SC=sc["T_SC"] + sc["T_SC"][:1]),
           dict(result=fe.make_ransac_hypotheses_device(T["H"].data_ptr(), None)),
           dict(result=fe.make_ransac_hypotheses_device(None, T["valid"].data_ptr())))
    for change in bad:
        with pytest.raises(capi.OkvfeError) as e:
            fe.ransac3d2d_hypotheses_blocks_device(**dict(good, **change))
        assert e.value.status == capi.ERR_INVALID_ARGUMENT, change
    pgood = dict(place_set=T["set"], blocks_ptr=T["blocks"].data_ptr(), n_multiframes=3, cam_ids=[0, 1],
                 poses_T_SC=sc["T_SC"], match_landmark_ptr=T["lm"].data_ptr(), gate_ptr=None, sample_keys_ptr=None, seed=1,
                 n_hyp=50, result=res)
    for change in (dict(n_hyp=0), dict(n_hyp=65), dict(n_multiframes=-1), dict(blocks_ptr=None), dict(place_set=None),
                   dict(match_landmark_ptr=None), dict(result=None), dict(cam_ids=[], poses_T_SC=[])):
        with pytest.raises(capi.OkvfeError) as e:
            fe.place_hypotheses_blocks_device(**dict(pgood, **change))
        assert e.value.status == capi.ERR_INVALID_ARGUMENT, change
    fe.ransac3d2d_hypotheses_blocks_device(**dict(good, n_multiframes=0))
    fe.place_hypotheses_blocks_device(**dict(pgood, n_multiframes=0))
    torch.cuda.synchronize()
    assert np.all(T["H"].cpu().numpy() == HS.H_SENTINEL) and np.all(T["valid"].cpu().numpy() == HS.BYTE_SENTINEL)
    # a slot without intrinsics: the frame and the slot are named
    half = _frontend(sc["cams"], n_set=1)
    for call, args in ((half.ransac3d2d_hypotheses_blocks_device, good), (half.place_hypotheses_blocks_device, pgood)):
        with pytest.raises(capi.OkvfeError) as e:
            call(**args)
        assert e.value.status == capi.ERR_NOT_READY and "frame 1: camera slot 1" in str(e.value), str(e.value)
    # an index list that does not fit in LDS (a scale space of 4 octaves: 8 x 1024 rows per block, two blocks):
    # refused before anything is launched
    big = _frontend(sc["cams"], Kc=1024, octaves=4)
    assert big.max_keypoints == 8192
    with pytest.raises(capi.OkvfeError) as e:
        big.ransac3d2d_hypotheses_blocks_device(**good)
    assert e.value.status == capi.ERR_UNSUPPORTED and "LDS" in str(e.value)
    torch.cuda.synchronize()
    assert np.all(T["H"].cpu().numpy() == HS.H_SENTINEL)
