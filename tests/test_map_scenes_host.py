"""CPU tier of the landmark-preparation census: conditions on the tables of map_scenes.py that the
oracle alone can check, an independent restatement of Frontend.cpp:1219-1359, and the oracle's plain
entry point pinned to the bytes it gave before the census variant was added.

 (a) census floor: over the general scenes, orc_prepare_landmarks_census reaches every label at
     least 16 times in EACH mode (non-exclusive at threshold 20, exclusive at 150); the labels a mode
     cannot reach are listed with the reason, and must then count zero.
 (b) every knife edge is a pair of adjacent binary64 values with the oracle's verdict on one side each.
 (c) tests/map_ref.py (numpy.longdouble, written from the reference's sources) gives the oracle's
     status, n_desc and obs_rows for every landmark whose smallest margin exceeds 1e-9, and its
     projection, e_W and r_W to 1e-9 relative; at most 1 % of the landmarks may be exempt for a
     smaller margin.  The knife-edge tables are exempt by construction and counted on their own.
 (d) the plain entry point returns the census entry point's bytes, and the bytes recorded in
     tests/golden/map_scene_digests.json from the oracle as it was before the census.

`python tests/map_scenes.py` prints the census (label x mode) of the committed scenes.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import map_ref
import map_scenes as S

FLOOR = 16          # as tests/test_gate_scenes_host.py
MARGIN = 1.0e-9
REL = 1.0e-9
EXEMPT_CAP = 0.01

# Labels a mode cannot reach (they must count zero there), and why.
UNREACHABLE = {
    False: {
        "vp_kept_excl": "the exclusive call's label", "scale_kept_excl": "the exclusive call's label",
        # a non-exclusive call only scores views with cosVC >= cos(0.6) = 0.825 (or a NaN cosine)
        "acos_tiny": "cosVC < cos(0.6) was dropped before", "acos_small": "cosVC < cos(0.6) was dropped before",
        "acos_neg": "cosVC < cos(0.6) was dropped before",
        # acos <= 0.6 and scaleChange <= 0.5 after both tests: score <= 1, with equality only where BOTH sit on
        # their limit at once; no scene aims for that
        "not_stored_ge1": "score <= 1 after the view-point and scale tests",
    },
    True: {"vp_reject": "pruning is off in an exclusive call", "scale_reject": "pruning is off in an exclusive call"},
}
# In either mode: a stored score is below 1, so the slots still at their initial 1.0 are the worst ones, lowest
# index first: the first three stores go to (slot 0, row 0), (slot 1, row 0), (slot 2, row 1), every later one to row 2.
NEVER = ("write_s0_o1", "write_s1_o1", "write_s2_o0")


def test_prepare_census_labels_cover_the_header(oracle):
    labels = oracle.prepare_census_labels()
    assert len(labels) == len(set(labels)) == 39
    for mode in (False, True):
        assert set(UNREACHABLE[mode]) | set(NEVER) <= set(labels)


def test_census_floor_every_label_in_each_mode(oracle):
    tot = S.all_census(oracle)
    print("\n" + S.format_census(tot))
    for exclusive in (False, True):
        cen = oracle.prepare_census_dict(tot["exclusive" if exclusive else "non-exclusive"])
        off = set(UNREACHABLE[exclusive]) | set(NEVER)
        low = [(lab, v) for lab, v in cen.items() if lab not in off and v < FLOOR]
        assert not low, f"exclusive={exclusive}: labels reached fewer than {FLOOR} times: {low}"
        stray = [(lab, cen[lab]) for lab in off if cen[lab]]
        assert not stray, f"exclusive={exclusive}: counted where the loop cannot reach: {stray}"


def test_general_scenes_hold_the_inputs_the_census_cannot_name():
    """degenerate inputs that are not a branch of the loop: present in the tables"""
    for sc in S.general_scenes():
        w = sc["hp"][:, 3]
        for v in (1.0, 2.0, -1.0, 0.5, 1.0e-300):
            assert (w == v).sum() >= 4, (sc["name"], v)
        zero = w == 0.0
        assert (zero & np.signbit(w)).sum() >= 2 and (zero & ~np.signbit(w)).sum() >= 2, sc["name"]
        q = sc["quality"]
        for v in S.QUALITIES:
            assert ((q == v) | (np.isnan(q) & np.isnan(v))).sum() >= 8, (sc["name"], v)
        n_obs = np.diff(sc["obs_begin"])
        for v in (0, 1, 2, 3, 4, 40):
            assert (n_obs == v).sum() >= 8, (sc["name"], v)
        assert (np.linalg.norm(sc["obs_bp"], axis=1) == 0).sum() >= 16            # zero-length back-projections
        assert (sc["obs_pose"] == 0).sum() >= 16                                  # views from T1 itself
        assert np.array_equal(sc["poses"][0][0], sc["T1"][0]) and np.array_equal(sc["poses"][0][1], sc["T1"][1])
        at_centre = np.all(sc["hp"][:, :3] == sc["T1"][1][None, :] * w[:, None], axis=1) & (w != 0)
        assert at_centre.sum() >= 4, sc["name"]
        # a valid table for okvfe_match_to_map_landmarks
        assert sc["obs_begin"][0] == 0 and np.all(n_obs >= 0) and sc["obs_begin"][-1] == len(sc["obs_pose"])
        assert sc["obs_pose"].min() >= 0 and sc["obs_pose"].max() < len(sc["poses"])
        assert sc["obs_desc"].shape == (len(sc["obs_pose"]), 48) and sc["obs_bp"].shape == (len(sc["obs_pose"]), 3)


# which census label a knife edge sits on
_KNIFE_LABEL = {"margin_u_low": "margin_u_low", "margin_v_low": "margin_v_low", "margin_u_high": "margin_u_high",
                "margin_v_high": "margin_v_high", "z_invalid": "proj_invalid", "cos10": "is3d_first",
                "cos06": "vp_reject", "scale05": "scale_reject", "tie": "not_stored_tie", "clamp": "clamp_r"}


def _knife_cases():
    return [(e, x) for e in S.KNIFE_EDGES for x in S.knife_modes(e)]


@pytest.mark.usefixtures("fp64_order")
@pytest.mark.parametrize("edge,exclusive", _knife_cases(), ids=lambda v: str(v))
def test_knife_edges_are_adjacent_values_with_the_verdict_on_one_side(oracle, edge, exclusive):
    sc, thr, (lo, hi), calls = S.knife_edge(oracle, edge, exclusive)
    assert calls <= 70, calls
    assert lo < hi and hi == np.nextafter(lo, np.inf)
    verdict = S.knife_verdict(oracle, sc, thr, exclusive, edge)
    assert len(set(verdict[0::2])) == 1 and len(set(verdict[1::2])) == 1 and verdict[0] != verdict[1]
    counts = []
    for side in (0, 1):
        cen = oracle.new_prepare_census()
        S.run_oracle(oracle, S._one(sc, side), exclusive, thr, cen)
        counts.append(oracle.prepare_census_dict(cen)[_KNIFE_LABEL[edge]])
    print(f"\n{edge} exclusive={exclusive}: lo={lo!r} hi={hi!r} calls={calls} verdicts={verdict[:2]} label counts={counts}")
    assert sorted(counts) == [0, 1], counts
    ref = S.run_oracle(oracle, sc, exclusive, thr)
    cam = sc["cam"]
    if edge.startswith("margin"):  # the kept side sits ON the margin: kp == -thr, resp. w + thr (h + thr)
        kept = 1 if edge.endswith("low") else 0
        assert ref["status"][kept] == 1 and ref["status"][1 - kept] == 0
        want = -thr if edge.endswith("low") else (cam.w if "_u_" in edge else cam.h) + thr
        assert ref["projection"][kept, 0 if "_u_" in edge else 1] == want
    if edge == "scale05":          # strict >: the kept side's scale change IS 0.5
        assert counts == [0, 1] and abs(5.0 - (5.0 + lo)) / 5.0 == 0.5 and abs(5.0 - (5.0 + hi)) / 5.0 > 0.5
    if edge == "tie":              # strict <: the side that is not stored has the worst slot's score exactly
        assert counts == [0, 1] and abs(5.0 - (5.0 + hi)) / 5.0 == abs(5.0 - 6.5) / 5.0


def test_z_sign_rows(oracle):
    sc = S.z_sign_table()
    for exclusive, thr in S.MODES:
        cen = oracle.new_prepare_census()
        r = S.run_oracle(oracle, sc, exclusive, thr, cen)
        cen = oracle.prepare_census_dict(cen)
        assert np.all(r["status"][0::3] != 0) and np.all(r["status"][1::3] == 0) and np.all(r["status"][2::3] != 0)
        assert cen["proj_behind"] == 16 and cen["proj_successful"] == 32 and cen["head_negated"] == 16
        assert cen["proj_invalid"] == 0


def _compare(oracle, sc, exclusive, thr):
    """(number of landmarks, exempt ones, list of disagreements)"""
    got = S.run_oracle(oracle, sc, exclusive, thr)
    ref = map_ref.prepare_landmarks(sc["hp"], sc["quality"], sc["obs_begin"], sc["obs_pose"], sc["obs_bp"],
                                    sc["poses"], sc["T1"], S.oracle_camera(sc["cam"]), thr, exclusive)
    sure = ref["margin"] > MARGIN
    bad = []
    for k in ("status", "n_desc"):
        for l in np.flatnonzero(sure & (got[k] != ref[k])):
            bad.append((sc["name"], exclusive, k, int(l), int(got[k][l]), int(ref[k][l]), float(ref["margin"][l])))
    for l in np.flatnonzero(sure & np.any(got["obs_rows"] != ref["obs_rows"], axis=1)):
        bad.append((sc["name"], exclusive, "obs_rows", int(l), got["obs_rows"][l].tolist(), ref["obs_rows"][l].tolist()))
    for k in ("projection", "e_W", "r_W"):
        g, r = map_ref.ld(got[k]).reshape(len(sure), -1), ref[k].reshape(len(sure), -1)
        nan_g, nan_r = np.isnan(g), np.isnan(r)
        with np.errstate(all="ignore"):
            scale = np.sqrt(np.nansum(r * r, axis=1))[:, None]
            off = np.abs(g - r) > REL * np.where(scale > 0, scale, 1)
        wrong = sure & np.any((nan_g != nan_r) | (off & ~nan_r), axis=1)
        for l in np.flatnonzero(wrong):
            bad.append((sc["name"], exclusive, k, int(l), g[l].astype(float).tolist(), r[l].astype(float).tolist()))
    return len(sure), int((~sure).sum()), bad


@pytest.mark.usefixtures("fp64_order")
def test_longdouble_restatement_gives_the_oracle_rows(oracle):
    n = n_exempt = 0
    bad = []
    for sc in S.general_scenes() + [S.packing_scene(m, p) for m in S.PACK_SIZES for p in S.PACK_PATTERNS]:
        for exclusive, thr in S.MODES:
            a, b, c = _compare(oracle, sc, exclusive, thr)
            n, n_exempt, bad = n + a, n_exempt + b, bad + c
    n_knife = n_knife_exempt = 0
    for edge, exclusive in _knife_cases():
        sc, thr, _, _ = S.knife_edge(oracle, edge, exclusive)
        a, b, c = _compare(oracle, sc, exclusive, thr)
        n_knife, n_knife_exempt, bad = n_knife + a, n_knife_exempt + b, bad + c
    print(f"\n{n} landmark rows, {n_exempt} exempt (margin <= {MARGIN:g}): {100.0 * n_exempt / n:.3f} %; "
          f"knife-edge tables: {n_knife} rows, {n_knife_exempt} exempt")
    assert n > 100000
    assert n_exempt <= EXEMPT_CAP * n, (n_exempt, n)
    assert not bad, (len(bad), bad[:10])


# ---- (d) the plain entry point is what it was ---------------------------------------------------------
def _sha(r):
    h = hashlib.sha256()
    for k in ("status", "n_desc", "obs_rows", "projection", "e_W", "r_W"):
        a = np.ascontiguousarray(r[k])
        if a.dtype == np.float64:  # one pattern for every NaN (their sign and payload are not the oracle's to define)
            a = np.where(np.isnan(a), np.float64(np.nan), a)
        h.update(a.tobytes())
    return h.hexdigest()


def scene_digests(oracle, census):
    """{name/mode: sha256 of every output byte}; census: counters make every call take the census entry point"""
    import map_synth
    legacy = dict(map_synth.make_map(6000), name="map_synth-6000")
    out = {}
    for sc in [legacy] + S.general_scenes() + [S.packing_scene(m, "mixed") for m in (1, 1025, 3100)] + [S.z_sign_table()]:
        for exclusive, thr in S.MODES:
            out[sc["name"] + ("/exclusive" if exclusive else "/non-exclusive")] = _sha(
                S.run_oracle(oracle, sc, exclusive, thr, census))
    return out


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "map_scene_digests.json")


def test_plain_entry_point_unchanged_and_equal_to_census_entry_point(oracle, fp64_order):
    plain = scene_digests(oracle, None)
    with_census = scene_digests(oracle, oracle.new_prepare_census())
    assert plain == with_census
    with open(GOLDEN) as f:
        recorded = json.load(f)[fp64_order]
    assert set(recorded) == set(plain)
    changed = sorted(k for k in plain if plain[k] != recorded[k])
    assert not changed, changed
