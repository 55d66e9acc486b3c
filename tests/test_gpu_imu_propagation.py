"""GPU: okvfe_imu_propagation_blocks_device (k_imu.hip) against the restatement imu_ref.py, byte for byte (a NaN standing
for any NaN) and under both orders of the FP64 sums, through its three forms: the mean only, with the Jacobian F, with
the covariance P.  Every scene of imu_scenes.py in batches of 1, 3, 64, 65 and 257 multiframes (both sides of a wave and of
a work-group); one batch of every sample count from 2 to 40 with a -1, a t_end == t_start and an out-of-range multiframe;
guard records behind every output; optional outputs absent; a sliced call; a side stream; the gravity_C rows fed unchanged
to okvfe_detect_describe_batch_device after one download; and one call at 3077 multiframes tiled from 16 distinct ones,
whose anchors, replicas and second run are compared on the device."""
import numpy as np
import pytest

import batch_scale as BS
import gpu_common as G
import imu_scenes as SC
from okvis2_amd import capi, synth

pytestmark = [pytest.mark.gpu]
torch = pytest.importorskip("torch")

FORMS = ("mean", "jacobian", "covariance")
GUARD = 2                       # records behind every output that no call may touch
BATCHES = (1, 3, 64, 65, 257)
_TORCH = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32}


@pytest.fixture(scope="module")
def fe():
    f = capi.Frontend(64, 64, 10.0, 0, 50, 10)
    yield f
    f.close()


def _tree(fp64_order):
    return fp64_order == "eigen_tree"


def _outputs(n, n_cams):
    """sentinel-filled device outputs of n multiframes with GUARD records behind each"""
    out = {}
    for k, (w, t) in SC.OUTPUTS.items():
        out[k] = torch.full((n + GUARD, w), SC.SENTINEL, dtype=_TORCH[np.dtype(t)], device="cuda")
    out["T_WC"] = torch.full((n + GUARD, max(n_cams, 1), 7), SC.SENTINEL, dtype=torch.float64, device="cuda")
    out["gravity_C"] = torch.full((n + GUARD, max(n_cams, 1), 3), SC.SENTINEL, dtype=torch.float32, device="cuda")
    return out


def _result(out, form, cameras=True, jacobian=None, first=0):
    """the struct of device pointers for a form, `first` multiframes into the outputs"""
    ptr = lambda k: out[k].data_ptr() + first * out[k].stride(0) * out[k].element_size()
    jacobian = form != "mean" if jacobian is None else jacobian
    return capi.make_imu_result(
        ptr("pose"), ptr("speed_and_bias"), ptr("n_propagated"), ptr("status"), ptr("n_out_of_range"),
        ptr("jacobian") if jacobian else None, ptr("covariance") if form == "covariance" else None,
        ptr("T_WC") if cameras else None, ptr("gravity_C") if cameras else None)


def _upload(mfs):
    samples, begin, states = SC.pack(mfs)
    return torch.from_numpy(samples).cuda(), torch.from_numpy(begin).cuda(), torch.from_numpy(states).cuda()


def _check(out, refs, n_cams, form, what, cameras=True, jacobian=None, first=0, count=None):
    """the outputs equal the restatement's on multiframes [first, first + count); every other record, the guard records
    included, still holds the sentinel"""
    n = out["pose"].shape[0] - GUARD
    count = n - first if count is None else count
    jacobian = form != "mean" if jacobian is None else jacobian
    want = SC.expected(refs[first:first + count], n_cams, jacobian=jacobian, covariance=form == "covariance")
    got = {}
    for k, w in want.items():
        g = out[k].cpu().numpy()
        if k in ("T_WC", "gravity_C"):
            g = g[:, :n_cams]
            if not cameras:
                w = np.full_like(w, SC.SENTINEL)
        full = np.full_like(g, SC.SENTINEL)
        full[first:first + count] = w
        if not SC.same_bytes(g, full):
            bad = [m for m in range(len(g)) if not SC.same_bytes(g[m], full[m])]
            raise AssertionError((what, form, k, "multiframes", bad[:8], len(bad), "of", n, g[bad[0]].reshape(-1)[:6],
                                  full[bad[0]].reshape(-1)[:6]))
        got[k] = g[:n]
    return got


def _run(fe, mfs, refs, T_SC, form, what, stream=None, cameras=True, jacobian=None):
    n, n_cams = len(mfs), len(T_SC)
    smp, beg, sta = _upload(mfs)
    out = _outputs(n, n_cams)
    torch.cuda.synchronize()
    fe.imu_propagation_blocks_device(SC.PARAMS, smp.data_ptr(), beg.data_ptr(), sta.data_ptr(), n, T_SC if cameras else None,
                                     _result(out, form, cameras, jacobian), stream=stream)
    torch.cuda.synchronize()
    return _check(out, refs, n_cams, form, what, cameras, jacobian)


@pytest.mark.parametrize("form", FORMS)
def test_every_scene(fe, fp64_order, form):
    """the three rigs' scenes, whole (120 multiframes each: every branch of the census, both sides of every knife edge)"""
    refs, census = SC.references(_tree(fp64_order))
    for sc, rf in zip(SC.scenes(), refs):
        got = _run(fe, sc["mfs"], rf, sc["T_SC_params"], form, (sc["name"], fp64_order))
        assert (got["n_propagated"] == -1).sum() >= 6 and (got["status"] == 1).sum() == 6 and (got["status"] == 2).sum() == 6
        assert (got["n_out_of_range"] > 0).sum() >= 12 and np.isnan(got["pose"]).any() and got["n_propagated"].max() >= 30


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", BATCHES)
def test_batch_sizes(fe, fp64_order, form, n):
    """both sides of a wave (64 lanes, a multiframe each) and of a work-group, and a ragged last one"""
    refs, _ = SC.references(_tree(fp64_order))
    sc, rf = SC.scenes()[1], refs[1]
    pick = [(7 * n + i) % len(sc["mfs"]) for i in range(n)]
    _run(fe, [sc["mfs"][i] for i in pick], [rf[i] for i in pick], sc["T_SC_params"], form, ("batch", n, fp64_order))


@pytest.mark.parametrize("form", FORMS)
def test_every_sample_count_in_one_batch(fe, fp64_order, form):
    tree = _tree(fp64_order)
    sc = SC.mixed_batch()
    refs = [SC.reference_one(tree, mf, sc["T_SC_params"]) for mf in sc["mfs"]]
    got = _run(fe, sc["mfs"], refs, sc["T_SC_params"], form, ("mixed", fp64_order))
    counts = sorted(len(mf["ts"]) for mf in sc["mfs"] if mf["kind"] == "general")
    assert counts == list(range(2, 41))
    assert got["n_propagated"][5] == -1 and got["n_propagated"][17] == 0 and got["n_out_of_range"][30] > 0
    assert np.isnan(got["pose"][30]).any() and not np.isnan(got["pose"][17]).any()


def test_optional_outputs_absent(fe, fp64_order):
    refs, _ = SC.references(_tree(fp64_order))
    sc, rf = SC.scenes()[2], refs[2]
    for form in FORMS:
        _run(fe, sc["mfs"], rf, sc["T_SC_params"], form, ("no cameras", fp64_order), cameras=False)
    _run(fe, sc["mfs"], rf, sc["T_SC_params"], "covariance", ("P without F", fp64_order), jacobian=False)


@pytest.mark.parametrize("form", FORMS)
def test_sliced_call_on_a_side_stream(fe, fp64_order, form):
    """multiframes [first, first + count) of a batch through offset pointers, on a stream of the caller's: the records
    before and behind the slice keep their sentinels"""
    refs, _ = SC.references(_tree(fp64_order))
    sc, rf = SC.scenes()[1], refs[1]
    n, n_cams, first, count = len(sc["mfs"]), 2, 37, 70
    smp, beg, sta = _upload(sc["mfs"])
    out = _outputs(n, n_cams)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    fe.imu_propagation_blocks_device(SC.PARAMS, smp.data_ptr(), beg.data_ptr() + 4 * first, sta.data_ptr() + 8 * 18 * first,
                                     count, sc["T_SC_params"], _result(out, form, first=first), stream=side)
    side.synchronize()
    _check(out, rf, n_cams, form, ("slice", fp64_order), first=first, count=count)


def test_empty_batch_and_bad_arguments(fe):
    out = _outputs(1, 1)
    res = _result(out, "covariance")
    fe.imu_propagation_blocks_device(SC.PARAMS, out["pose"].data_ptr(), out["status"].data_ptr(), out["pose"].data_ptr(), 0,
                                     None, res)                     # n_multiframes == 0 launches nothing
    for bad in (dict(n=-1), dict(samples=None), dict(begin=None), dict(states=None), dict(result=None)):
        a = dict(samples=out["pose"].data_ptr(), begin=out["status"].data_ptr(), states=out["pose"].data_ptr(), n=1,
                 result=res)
        a.update(bad)
        with pytest.raises(capi.OkvfeError) as e:
            fe.imu_propagation_blocks_device(SC.PARAMS, a["samples"], a["begin"], a["states"], a["n"], None, a["result"])
        assert e.value.status == capi.ERR_INVALID_ARGUMENT
    no_pose = capi.make_imu_result(None, out["speed_and_bias"].data_ptr(), out["n_propagated"].data_ptr(),
                                   out["status"].data_ptr(), out["n_out_of_range"].data_ptr())
    with pytest.raises(capi.OkvfeError):
        fe.imu_propagation_blocks_device(SC.PARAMS, out["pose"].data_ptr(), out["status"].data_ptr(),
                                         out["pose"].data_ptr(), 1, None, no_pose)
    torch.cuda.synchronize()
    for k, t in out.items():
        assert bool((t == SC.SENTINEL).all()), k


def test_gravity_rows_feed_the_detector(oracle, fe):
    """gravity_C of one multiframe of two cameras, downloaded once, is the host gravity_C of
    okvfe_detect_describe_batch_device as it stands"""
    cfg = synth.euroc_config()
    sc = SC.scenes()[1]
    mf = sc["mfs"][0]
    ref = SC.reference_one(True, mf, sc["T_SC_params"])
    smp, beg, sta = _upload([mf])
    out = _outputs(1, 2)
    fe.imu_propagation_blocks_device(SC.PARAMS, smp.data_ptr(), beg.data_ptr(), sta.data_ptr(), 1, sc["T_SC_params"],
                                     _result(out, "mean"))
    torch.cuda.synchronize()
    grav = out["gravity_C"][:1].cpu().numpy().reshape(2, 3)
    assert SC.same_bytes(grav, ref["gravity_C"])
    det = G.make_frontend(cfg, max_batch=2)
    try:
        L, R, _ = synth.stereo_pair(cfg.w, cfg.h, 1234)
        for ci in range(2):
            det.set_camera(ci, cfg.cams[ci])
        d_img = torch.from_numpy(np.stack([L, R])).cuda()
        det.detect_describe_batch_device(d_img.data_ptr(), 2, np.array([0, 1], np.int32), grav,
                                         torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        det.check_capacity(2)
        for ci, img in enumerate((L, R)):
            k, d, _, _ = det.download(ci)
            rays, jac = oracle.awareness_maps(cfg.cams[ci])
            rk, rd = oracle.detect_describe(img, cfg.uniformity_radius, 0, cfg.abs_threshold, cfg.max_kpts,
                                            oracle.MODE_CAMERA_AWARE, rays, jac, np.float32(cfg.cams[ci].fu),
                                            tuple(float(v) for v in grav[ci]))
            G.assert_keypoints_equal(k, rk)
            assert np.array_equal(d, rd) and len(k) > 50
    finally:
        det.close()


@pytest.mark.parametrize("form", FORMS)
def test_at_3077_multiframes(fe, form):
    """16 distinct multiframes tiled to 3077 (batch_scale.N: a ragged last work-group, no power-of-two factor): the anchors
    equal the restatement, every replica equals its anchor, and a second run equals the first -- compared on the device"""
    sc = SC.distinct_batch()
    assert len(sc["mfs"]) == BS.D
    refs = [SC.reference_one(True, mf, sc["T_SC_params"]) for mf in sc["mfs"]]
    tiled, _ = BS.tile(sc, BS.N)
    smp, beg, sta = _upload(tiled["mfs"])
    runs = []
    for _ in range(2):
        out = _outputs(BS.N, 2)
        fe.imu_propagation_blocks_device(SC.PARAMS, smp.data_ptr(), beg.data_ptr(), sta.data_ptr(), BS.N,
                                         sc["T_SC_params"], _result(out, form))
        runs.append(out)
    torch.cuda.synchronize()
    first, second = runs
    for k, t in first.items():
        assert BS.first_difference(t, BS.D, BS.N) is None, (form, k, BS.first_difference(t, BS.D, BS.N))
        assert torch.equal(t.view(torch.uint8), second[k].view(torch.uint8)), (form, k)
        assert bool((t[BS.N:] == SC.SENTINEL).all()), (form, k)
    anchors = {k: torch.cat([t[:BS.D], t[BS.N:]]) for k, t in first.items()}
    _check(anchors, refs, 2, form, "anchors")
