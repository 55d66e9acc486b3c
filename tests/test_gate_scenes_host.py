"""CPU tier of the gate-census work: conditions on the scenes of gate_scenes.py that the oracle alone
can check, an independent restatement of the gate chain, and the oracle's plain entry points pinned
to the bytes they gave before the census variants were added.

 (a) census floor: over the scenes of a matcher, the oracle's sequential loop reaches every gate
     label of that matcher at least 16 times; every knife edge is reached once per side.
 (b) tests/gate_ref.py (numpy.longdouble, written from the reference's sources) gives the oracle's
     verdict for every gated pair whose smallest gate margin exceeds 1e-9, hp_W to 1e-9 relative;
     at most 1 % of the pairs may be exempt for a smaller margin.
 (c) the plain entry points return the census entry points' bytes, and the bytes recorded in
     tests/golden/gate_scene_digests.json from the oracle as it was before the census.

`python tests/gate_scenes.py` prints the census (label x matcher) of the committed scenes.

binary64 carries hp_W to about 2^-53 / sin^2 of the angle between the rays, so (b)'s 1e-9 asks the scenes to
keep the rays of a true pair more than 5e-4 rad apart (gate_scenes._pair_geometry, "far" and "base004").
"""
import hashlib
import json
import os

import numpy as np
import pytest

import gate_ref
import gate_scenes as S

FLOOR = 16
MARGIN = 1.0e-9
HP_REL = 1.0e-9
EXEMPT_CAP = 0.01

# labels a matcher's loop can reach (oracle/okvfe_oracle.h)
_TRI = ["det_singular", "l_small", "tn_small", "par_cos26_e1", "par_cos26_e2", "tri_cos26_e1", "tri_cos26_e2",
        "cos6_parallel", "nan_operand"]
LABELS = {
    "stereo": _TRI + ["bp_invalid", "depth0", "depth1", "ee_08"],
    "motion": _TRI + ["bp_invalid", "depth0", "depth1", "ee_05", "ee_08", "px4_accept", "px4_reject", "proj_status"],
    "uninit": _TRI + ["epipolar", "divergent", "near_parallel", "dist0", "dist1", "previous", "win_hp", "win_no_hp"],
    "map": ["radius_pass", "radius_fail", "min_replaced", "nan_operand"],
}


def test_census_labels_cover_the_header(oracle):
    labels = oracle.census_labels()
    assert len(labels) == len(set(labels)) == 28
    assert set(sum(LABELS.values(), [])) == set(labels)


def test_census_floor_every_label_of_every_matcher(oracle):
    tot = S.all_census(oracle)
    print("\n" + S.format_census(tot))
    low = [(m, lab, oracle.census_dict(tot[m])[lab]) for m in LABELS for lab in LABELS[m]
           if oracle.census_dict(tot[m])[lab] < FLOOR]
    assert not low, f"labels reached fewer than {FLOOR} times: {low}"
    # and nothing is counted where the loop cannot reach it
    stray = [(m, lab) for m in LABELS for lab, v in oracle.census_dict(tot[m]).items() if v and lab not in LABELS[m]]
    assert not stray, stray


# which census label a knife edge sits on, and which side of it counts the label
_KNIFE_LABEL = {"cos26": ("tri_cos26_e1", "tri_cos26_e2"), "parcos26": ("par_cos26_e1", "par_cos26_e2"),
                "cos6": ("cos6_parallel",), "ee08": ("ee_08",), "depth005": ("depth0",), "depth02": ("depth0",),
                "depth1_005": ("depth1",), "depth1_02": ("depth1",), "px4": ("px4_reject",), "l001": ("l_small",)}


@pytest.mark.usefixtures("fp64_order")
@pytest.mark.parametrize("gate", S.KNIFE_GATES)
def test_knife_edges_are_adjacent_values_with_the_gate_on_one_side(oracle, gate):
    scenes, motion, (lo, hi), calls = S.knife_edge(oracle, gate)
    assert calls <= 60, calls
    assert hi == np.nextafter(lo, type(lo)(np.inf)) and lo < hi
    counts = []
    for sc in scenes:
        cen = oracle.new_census()
        S.run_pair(oracle, sc, motion, cen)
        counts.append(sum(oracle.census_dict(cen)[lab] for lab in _KNIFE_LABEL[gate]))
    n = len(scenes[0]["kp0"])
    print(f"\n{gate}: lo={lo!r} hi={hi!r} calls={calls} gate counts per batch={counts}")
    if gate == "l001":  # "<" against "<=": the side that is not under 0.01 sits ON it
        tree = bool(oracle.lib().orc_get_reduction())
        assert S.lambda0_binary64(scenes[1], tree) == 0.01 and S.lambda0_binary64(scenes[0], tree) < 0.01
    if gate == "px4":  # both sides alternate inside each batch
        assert counts == [n // 2, n // 2]
    else:              # one batch per side: the gate fires for every pair of one side, for none of the other
        assert sorted(c > 0 for c in counts) == [False, True] and max(counts) >= n


def _gated_pairs(sc):
    """every (k0, k1) with Hamming distance under the threshold and both back-projections valid"""
    if len(sc["d0"]) == 0 or len(sc["d1"]) == 0:
        return np.zeros((0, 2), dtype=np.int64)
    b0, b1 = np.unpackbits(sc["d0"], axis=1), np.unpackbits(sc["d1"], axis=1)
    dist = b0.astype(np.int32) @ (1 - b1.T.astype(np.int32)) + (1 - b0.astype(np.int32)) @ b1.T.astype(np.int32)
    ok = (dist < S.THRESHOLD) & (sc["bv0"][:, None] != 0) & (sc["bv1"][None, :] != 0)
    return np.argwhere(ok)


def _oracle_pair(oracle, sc, k0, k1, motion):
    d = np.zeros((1, 48), dtype=np.uint8)
    one = lambda a, k: a[k:k + 1]
    if motion:
        r = oracle.match_motion_stereo(d, one(sc["kp0"], k0), one(sc["bp0"], k0), one(sc["bv0"], k0), None, d,
                                       one(sc["kp1"], k1), one(sc["bp1"], k1), one(sc["bv1"], k1), None, sc["T0"],
                                       sc["T1"], sc.get("oracle_cam", sc["cam"]), S.THRESHOLD)[0]
    else:
        r = oracle.match_stereo(d, one(sc["kp0"], k0), one(sc["bp0"], k0), one(sc["bv0"], k0), d, one(sc["kp1"], k1),
                                one(sc["bp1"], k1), one(sc["bv1"], k1), sc["T0"], sc["T1"], sc["f0"], sc["f1"],
                                S.THRESHOLD)[0]
    return bool(r["k1"] >= 0), not bool(r["initialisable"]), np.array(r["hp_W"])


def _binary64_rays(T, bp):
    v = np.asarray(bp, dtype=np.float64) @ np.asarray(T[0], dtype=np.float64).reshape(3, 3).T
    with np.errstate(all="ignore"):
        return v / np.sqrt((v * v).sum(axis=1))[:, None]


@pytest.mark.usefixtures("fp64_order")
@pytest.mark.parametrize("motion", [False, True], ids=["stereo", "motion"])
def test_longdouble_restatement_gives_the_oracle_verdict(oracle, motion):
    """EVERY gated pair of every pair scene: the matcher's verdict and hp_W from a single-pair call of the
    oracle's matcher, and the (valid, parallel) of its triangulation -- which the matcher's row does not show
    for a pair it rejects -- from orc_triangulate_fast on the same rays."""
    n_pairs = n_exempt = n_tri_exempt = 0
    wrong, tri_wrong, hp_off = [], [], []
    worst_hp = 0.0
    for sc in S.pair_scenes():
        pairs = _gated_pairs(sc)
        if len(pairs) == 0:
            continue
        k0, k1 = pairs[:, 0], pairs[:, 1]
        if motion:
            f0 = 0.5 * (sc["cam"].fu + sc["cam"].fv)
            s64 = sc["kp0"]["size"][k0].astype(np.float64) / f0 * 0.125
            hp, valid, parallel, margin = gate_ref.motion_pairs(sc["T0"], sc["T1"], sc["bp0"][k0], sc["bp1"][k1],
                                                                sc["kp0"]["size"][k0], f0)
        else:
            s64 = np.maximum(sc["kp0"]["size"][k0].astype(np.float64) / sc["f0"],
                             sc["kp1"]["size"][k1].astype(np.float64) / sc["f1"]) * 0.125
            hp, valid, parallel, margin = gate_ref.stereo_pairs(sc["T0"], sc["T1"], sc["bp0"][k0], sc["bp1"][k1],
                                                                sc["kp0"]["size"][k0], sc["kp1"]["size"][k1],
                                                                sc["f0"], sc["f1"])
        # the triangulation alone, with its own margin
        e0, e1 = _binary64_rays(sc["T0"], sc["bp0"][k0]), _binary64_rays(sc["T1"], sc["bp1"][k1])
        p0, p1 = np.asarray(sc["T0"][1], dtype=np.float64), np.asarray(sc["T1"][1], dtype=np.float64)
        n = len(pairs)
        _, t_valid, t_parallel, t_margin = gate_ref.triangulate_fast(np.broadcast_to(p0, (n, 3)), e0,
                                                                     np.broadcast_to(p1, (n, 3)), e1, s64)
        for i in range(n):
            where = (sc["name"], int(k0[i]), int(k1[i]))
            n_pairs += 1
            if t_margin[i] > MARGIN:
                _, o_tv, o_tp = oracle.triangulate_fast(p0, e0[i], p1, e1[i], s64[i])
                if (o_tv, o_tp) != (bool(t_valid[i]), bool(t_parallel[i])):
                    tri_wrong.append(where + (o_tv, o_tp, bool(t_valid[i]), bool(t_parallel[i]), float(t_margin[i])))
            else:
                n_tri_exempt += 1
            if not margin[i] > MARGIN:
                n_exempt += 1
                continue
            o_valid, o_parallel, o_hp = _oracle_pair(oracle, sc, int(k0[i]), int(k1[i]), motion)
            if o_valid != bool(valid[i]) or (o_valid and o_parallel != bool(parallel[i])):
                wrong.append(where + (o_valid, o_parallel, bool(valid[i]), bool(parallel[i]), float(margin[i])))
                continue
            if not o_valid:
                continue
            r = np.asarray(hp[i], dtype=np.float64)
            if np.isnan(o_hp).any() or np.isnan(r).any():
                if not np.array_equal(np.isnan(o_hp), np.isnan(r)):
                    hp_off.append(where + ("nan",))
                continue
            rel = float(np.max(np.abs(gate_ref.ld(o_hp[:3]) - hp[i][:3])) / np.sqrt(gate_ref.dot(hp[i][:3], hp[i][:3])))
            worst_hp = max(worst_hp, rel)
            if not rel <= HP_REL:
                hp_off.append(where + (rel,))
    print(f"\n{'motion' if motion else 'stereo'}: {n_pairs} gated pairs, {n_exempt} exempt (margin <= {MARGIN:g}; "
          f"{n_tri_exempt} for the triangulation alone), worst hp_W error {worst_hp:.3g} relative")
    assert n_pairs > 50000
    assert n_exempt <= EXEMPT_CAP * n_pairs and n_tri_exempt <= EXEMPT_CAP * n_pairs, (n_exempt, n_tri_exempt, n_pairs)
    assert not wrong, (len(wrong), wrong[:10])
    assert not tri_wrong, (len(tri_wrong), tri_wrong[:10])
    assert not hp_off, (len(hp_off), sorted(hp_off, key=lambda t: -t[3] if t[3] != "nan" else 0)[:10])


def test_triangulate_fast_restatement_on_the_uninitialised_scenes(oracle):
    """the same chain with the uninitialised matcher's inputs: pooled rays against current rays, sigma = 1 / f"""
    rng = np.random.default_rng(98)
    n_pairs = n_exempt = 0
    for sc in S.uninit_scenes():
        n_k, m = len(sc["desc"]), len(sc["pool"])
        if n_k == 0 or m == 0:
            continue
        k = rng.integers(0, n_k, 300)
        d = rng.integers(0, m, 300)
        ok = np.linalg.norm(sc["bp"][k], axis=1) > 0
        k, d = k[ok], d[ok]
        C1 = np.asarray(sc["T1"][0]).reshape(3, 3)
        e1 = (sc["bp"][k] / np.linalg.norm(sc["bp"][k], axis=1, keepdims=True)) @ C1.T
        p2 = np.broadcast_to(np.asarray(sc["T1"][1]), (len(k), 3))
        sigma = np.full(len(k), 1.0 / sc["focal"])
        hp, valid, parallel, margin = gate_ref.triangulate_fast(sc["r0"][d], sc["e0"][d], p2, e1, sigma)
        for i in range(len(k)):
            o_hp, o_valid, o_parallel = oracle.triangulate_fast(sc["r0"][d[i]], sc["e0"][d[i]], p2[i], e1[i], sigma[i])
            n_pairs += 1
            if not margin[i] > MARGIN:
                n_exempt += 1
                continue
            assert (o_valid, o_parallel) == (bool(valid[i]), bool(parallel[i])), (sc["name"], int(k[i]), int(d[i]))
    assert n_pairs > 2000 and n_exempt <= EXEMPT_CAP * n_pairs, (n_exempt, n_pairs)


# ---- (c) the plain entry points are what they were ---------------------------------------------------
def _legacy_ambiguous(oracle):
    """the scene of test_gpu_matchers.test_gated_matchers_large_and_ambiguous, array for array"""
    from okvis2_amd import synth
    cfg = synth.euroc_config()
    cam = cfg.cams[0]
    n = 1500
    rng = np.random.default_rng(21)
    T0 = (np.eye(3).reshape(-1), np.zeros(3))
    T1 = (np.eye(3).reshape(-1), np.array([0.11, 0.0, 0.0]))
    X = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.0, 1.0, n), rng.uniform(2.0, 12.0, n)], 1)

    def observe(T):
        Xc = X - np.asarray(T[1])
        kp = np.zeros(n, dtype=oracle.KEYPOINT_DTYPE)
        kp["size"] = 12.0
        for i in range(n):
            st, pt, _ = oracle.cam_project(cam, Xc[i])
            kp["x"][i], kp["y"][i] = pt if st == 0 else (5.0, 5.0)
        kp["x"] += rng.normal(0, 0.2, n).astype(np.float32)
        kp["y"] += rng.normal(0, 0.2, n).astype(np.float32)
        bp, bv = oracle.backproject_keypoints(cam, kp)
        return kp, bp, bv

    kp0, bp0, bv0 = observe(T0)
    kp1, bp1, bv1 = observe(T1)
    centres = rng.integers(0, 256, (60, 48), dtype=np.uint8)
    cl = rng.integers(0, 60, n)

    def perturb(p):
        return centres[cl] ^ ((rng.random((n, 48)) < p) * (1 << rng.integers(0, 8, (n, 48)))).astype(np.uint8)

    d0, d1 = perturb(0.08), perturb(0.08)
    perm = rng.permutation(n)
    d1, kp1, bp1, bv1 = d1[perm], kp1[perm], bp1[perm], bv1[perm]
    f = 0.5 * (cam.fu + cam.fv)
    skip0 = (rng.random(n) < 0.1).astype(np.uint8)
    matched1 = (rng.random(n) < 0.2).astype(np.uint8)
    return dict(name="legacy-ambiguous-1500", cam=cam, d0=d0, kp0=kp0, bp0=bp0, bv0=bv0, d1=d1, kp1=kp1, bp1=bp1,
                bv1=bv1, T0=T0, T1=T1, f0=f, f1=f, skip0=skip0, matched1=matched1)


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def scene_digests(oracle, census):
    """{name/matcher: sha256 of every output byte}; census: a counters array makes every call take the
    *_census entry point instead of the plain one"""
    out = {}
    for sc in S.pair_scenes() + [_legacy_ambiguous(oracle)]:
        out[sc["name"] + "/stereo"] = _sha(S.run_pair(oracle, sc, False, census))
        out[sc["name"] + "/motion"] = _sha(S.run_pair(oracle, sc, True, census))
    for sc in S.uninit_scenes():
        r = S.run_uninit(oracle, sc, census)
        out[sc["name"] + "/uninit"] = _sha(r[0], r[1], r[2], r[3], np.int32(r[4]))
    for sc in S.map_scenes():
        out[sc["name"] + "/map"] = _sha(*S.run_map(oracle, sc, census))
    return out


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gate_scene_digests.json")


def test_plain_entry_points_unchanged_and_equal_to_census_entry_points(oracle, fp64_order):
    plain = scene_digests(oracle, None)
    with_census = scene_digests(oracle, oracle.new_census())
    assert plain == with_census
    with open(GOLDEN) as f:
        recorded = json.load(f)[fp64_order]
    assert set(recorded) == set(plain)
    changed = sorted(k for k in plain if plain[k] != recorded[k])
    assert not changed, changed
