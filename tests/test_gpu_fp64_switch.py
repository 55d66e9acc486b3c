"""okvfe_set_fp64_reduction reaches every family of kernels that follows it.  Two of them read a device symbol
(k_match.hip, k_map.hip), the others are launched in the instantiation the host flag names; a family left on the
default order would still pass every test that runs under the default alone.  One case per family, on the smallest
scene the builders of tests/*_scenes.py give (one or two multiframes, a one-camera rig, tens of keypoints):

  stereo        okvfe_match_stereo: the triangulated hp_W                     (k_match.hip, device symbol)
  landmarks     okvfe_match_to_map_landmarks: the projections of the pooling  (k_map.hip, device symbol)
  ransac3d2d    okvfe_ransac3d2d_consensus_blocks_device: the distances       (k_ransac.hip)
  hypotheses    okvfe_ransac3d2d_hypotheses_blocks_device: the hypotheses     (k_ransac_hyp.hip)
  ransac2d2d    okvfe_ransac2d2d_consensus_blocks_device: the distances       (k_ransac2d2d.hip)
  hessian       okvfe_place_hessian_blocks_device: H                          (k_place_hessian.hip)
  refine        okvfe_place_refine_blocks_device: the poses                   (k_place_refine.hip)
  imu           okvfe_imu_propagation_blocks_device: pose, F, P, T_WC         (k_imu.hip)

Each case calls its entry point under Eigen's order and under left to right; each output equals the reference of its
order byte for byte (the scene modules' own checks, every output of the call), and the two outputs differ.  A scene
qualifies only if its two references differ: test_references_of_the_two_orders_differ holds that on the CPU, for the
seeds below.  The GPU test sets the order itself, the oracle's together with the device's, and restores Eigen's."""
import dataclasses

import numpy as np
import pytest

import gate_scenes as GS
import imu_scenes as IS
import map_scenes as MS
import place_hessian_scenes as PHS
import place_refine_device as RD
import place_refine_scenes as PRS
import ransac2d2d_scenes as S2
import ransac_hyp_scenes as HYP
import ransac_scenes as S
from okvis2_amd import capi, synth

FAMILIES = ("stereo", "landmarks", "ransac3d2d", "hypotheses", "ransac2d2d", "hessian", "refine", "imu")
SPEC = ("nodist",)         # the one-camera rig without a distortion
N_HYP = 8
_SCENES, _REFS = {}, {}


def _same(a, b):
    """equal as bytes, every NaN standing for every other"""
    return PHS.same_bytes(np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1))


def _scene(oracle, family):
    if family in _SCENES:
        return _SCENES[family]
    if family == "stereo":
        sc = GS.pair_scene("euroc", 32, 32, seed=1)
    elif family == "landmarks":
        sc = MS.general_scene("euroc", 0, 40, 0)
    elif family in ("ransac3d2d", "hypotheses"):
        m = S.table(200)
        cams, T_SC = S.rig(SPEC)
        rng = np.random.default_rng(5)
        T_WS = (m["T1"][0].reshape(3, 3), m["T1"][1])
        make = S.make_frame if family == "ransac3d2d" else HYP.exact_frame
        frames = [make(oracle, cams[0], S.compose(T_WS, T_SC[0]), m["p"], S.usable_rows(m), 48, rng)]
        mf = dict(frames=frames, H=S.hypotheses(T_WS, N_HYP, rng, n_random=2), valid=np.ones(N_HYP, np.uint8), T_WS=T_WS)
        sc = S.scene("switch-" + family, cams, T_SC, m["hp"], m["obs_begin"], [mf])
    elif family == "ransac2d2d":
        cams, T_SC = S.rig(SPEC)
        rng = np.random.default_rng(6)
        T_WS0 = (S.rodrigues((0.3, 0.2, 1.0), 0.4), np.array([1.0, -2.0, 0.5]))
        T_WS1 = (T_WS0[0] @ S.rodrigues((1.0, 0.2, 0.0), 0.02), T_WS0[1] + T_WS0[0] @ np.array([0.25, 0.05, -0.1]))
        T0 = S.compose((T_WS0[0].reshape(-1), T_WS0[1]), T_SC[0])
        T1 = S.compose((T_WS1[0].reshape(-1), T_WS1[1]), T_SC[0])
        fr0, fr1 = S2._general_camera(oracle, cams[0], T0, T1, 48, rng, 0.04)
        rot_H, rel_H = S2._hypotheses(*S2._relative(T0, T1), N_HYP, rng, n_random=2)
        sc = S2.scene("switch-ransac2d2d", cams, [[S2.cam_entry(fr0, fr1, rot_H, rel_H)]])
    elif family == "hessian":
        sc = PHS.general_scene(oracle, SPEC, n_mf=2, seed=0, n_kps=(30, 60))
        sc["mfs"] = sc["mfs"][1:]        # (the first multiframe of a general scene is the full block)
    elif family == "refine":
        sc = PRS.general_scene(oracle, SPEC, n_mf=2, seed=0)
        sc["mfs"] = sc["mfs"][1:]
    else:
        rng = np.random.default_rng(7)
        sc = dict(name="switch-imu", T_SC_params=IS.scenes()[0]["T_SC_params"],
                  mfs=[IS.multiframe("general", i, rng, n=12) for i in range(2)])
    _SCENES[family] = sc
    return sc


def _reference(oracle, family, tree):
    """-> (what the scene module's check takes, the FP64 values the two orders are told apart by); the oracle is switched
    by the caller"""
    if (family, tree) in _REFS:
        return _REFS[family, tree]
    sc = _scene(oracle, family)
    if family == "stereo":
        ref = GS.run_pair(oracle, sc, False)
        assert (ref["k1"] >= 0).sum() >= 8
        out = ref, ref["hp_W"]
    elif family == "landmarks":
        ref = MS.run_oracle(oracle, sc, False, 20.0)
        assert (ref["status"] > 0).sum() >= 8
        out = ref, ref["projection"]
    elif family == "ransac3d2d":
        refs = S.reference(tree, sc)
        assert refs[0]["best"] >= 0 and refs[0]["dist_set"][0].sum() >= 8
        out = refs, refs[0]["distance"][0][refs[0]["dist_set"][0]]
    elif family == "hypotheses":
        refs = HYP.reference(tree, sc, N_HYP)
        assert refs[0]["valid"].sum() >= 4
        out = refs, refs[0]["H"]
    elif family == "ransac2d2d":
        refs = S2.reference(tree, sc)
        rc = refs[0]["cams"][0]
        assert rc["dist_set"].sum() >= 8
        out = refs, rc["distance"][rc["dist_set"]]
    elif family == "hessian":
        refs = PHS.reference(oracle, tree, sc)
        assert refs[0]["n_terms"] >= 8
        out = refs, refs[0]["H"]
    elif family == "refine":
        refs = PRS.reference(oracle, tree, sc)
        assert refs[0]["status"] in (1, 2) and refs[0]["n_accepted"] >= 1
        out = refs, refs[0]["pose"]
    else:
        refs = [IS.reference_one(tree, mf, sc["T_SC_params"]) for mf in sc["mfs"]]
        want = IS.expected(refs, len(sc["T_SC_params"]))
        assert all(r["n_propagated"] >= 4 for r in refs)
        out = refs, np.concatenate([want[k].reshape(-1) for k in ("pose", "speed_and_bias", "jacobian", "covariance", "T_WC")])
    _REFS[family, tree] = out
    return out


def _both_references(oracle, family):
    try:
        out = {}
        for tree in (True, False):
            oracle.set_reduction(tree)
            out[tree] = _reference(oracle, family, tree)
        return out
    finally:
        oracle.set_reduction(True)


@pytest.mark.parametrize("family", FAMILIES)
def test_references_of_the_two_orders_differ(oracle, family):
    """CPU: a scene on which both orders give the same bytes could not tell a family left on the default order"""
    refs = _both_references(oracle, family)
    assert np.asarray(refs[True][1]).size >= 7 and not _same(refs[True][1], refs[False][1]), family


def _frontend(oracle, family):
    sc = _scene(oracle, family)
    if family == "stereo":
        return capi.Frontend(sc["cam"].w, sc["cam"].h, 38.0, 0, 150, 64, match_threshold=GS.THRESHOLD)
    if family == "imu":
        return capi.Frontend(64, 64, 10.0, 0, 50, 10)
    import gpu_common as G
    cams = [sc["cam"]] if family == "landmarks" else list(sc["cams"])
    # (a general place scene has up to 119 keypoints a block; the hypotheses' reference names slots of ransac_hyp_scenes.K)
    kw = {} if family == "landmarks" else dict(max_kpts=HYP.K if family == "hypotheses" else 128)
    fe = G.make_frontend(dataclasses.replace(synth.euroc_config(), w=cams[0].w, h=cams[0].h, cams=cams, **kw))
    for i, c in enumerate(cams):
        fe.set_camera(i, c)
    return fe


def _run(oracle, fe, family, ref, what):
    """the family's entry point on its scene: every output against `ref` (the scene module's check), -> the values the
    orders are told apart by, as the device wrote them"""
    sc = _scene(oracle, family)
    if family == "stereo":
        got = fe.match_stereo(sc["d0"], sc["kp0"], sc["bp0"], sc["bv0"], sc["d1"], sc["kp1"], sc["bp1"], sc["bv1"],
                              sc["T0"], sc["T1"], sc["f0"], sc["f1"])
        for f in ("k1", "dist", "initialisable"):
            assert np.array_equal(got[f], ref[f]), (what, f)
        return got["hp_W"]
    if family == "landmarks":
        _, _, pool = fe.match_to_map_landmarks(0, sc["hp"], sc["quality"], sc["obs_begin"], sc["obs_pose"], sc["obs_desc"],
                                               sc["obs_bp"], sc["poses"], sc["T1"], 20.0, False, np.zeros((0, 48), np.uint8),
                                               np.zeros(0, oracle.KEYPOINT_DTYPE), np.zeros(0, np.uint8))
        for k in ("status", "n_desc", "obs_rows"):
            assert np.array_equal(pool[k], ref[k]), (what, k)
        for k in ("e_W", "r_W"):
            assert _same(pool[k], ref[k]), (what, k)
        return pool["projection"]
    if family == "ransac3d2d":
        tab = S.DeviceTable(fe, sc["hp"], sc["obs_begin"])
        T = S.prepare_consensus(fe, sc)
        S.launch_consensus(fe, tab, sc, T)
        got = S.check_consensus(sc, T, ref, what)
        return got["distance"][0, :len(ref[0]["dist_set"][0])][ref[0]["dist_set"][0]]
    if family == "hypotheses":
        tab = S.DeviceTable(fe, sc["hp"], sc["obs_begin"])
        T = HYP.prepare(fe, sc, N_HYP)
        HYP.launch(fe, tab, sc, T)
        return HYP.check(sc, T, ref, what)["H"][0]
    if family == "ransac2d2d":
        T = S2.prepare(fe, sc)
        S2.launch(fe, sc, T)
        ds = ref[0]["cams"][0]["dist_set"]
        return S2.check(sc, T, ref, what)["distance"][0, 0, :len(ds)][ds]
    if family == "hessian":
        T = PHS.prepare(fe, sc)
        PHS.launch(fe, sc, T)
        return PHS.check(sc, T, ref, what)["H"][0]
    if family == "refine":
        T = RD.prepare(fe, sc)
        RD.launch(fe, sc, T)
        return RD.check(RD.download(T), ref, what)["poses_out"][0]
    import test_gpu_imu_propagation as TI   # (its helpers: the call's outputs with guard records, and their check)
    got = TI._run(fe, sc["mfs"], ref, sc["T_SC_params"], "covariance", what)
    return np.concatenate([got[k].reshape(-1) for k in ("pose", "speed_and_bias", "jacobian", "covariance", "T_WC")])


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_switch_reaches_the_family(oracle, family):
    pytest.importorskip("torch")
    refs = _both_references(oracle, family)
    fe = _frontend(oracle, family)
    got = {}
    try:
        for tree in (True, False):
            oracle.set_reduction(tree)
            fe.set_fp64_reduction(tree)
            got[tree] = np.array(_run(oracle, fe, family, refs[tree][0], (family, "eigen_tree" if tree else "left_to_right")))
            assert _same(got[tree], refs[tree][1]), (family, tree)
    finally:
        oracle.set_reduction(True)
        fe.set_fp64_reduction(True)
        fe.close()
    assert not _same(got[True], got[False]), (family, "both orders gave the same bytes")
