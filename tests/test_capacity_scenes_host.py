"""CPU: the premises of the capacity scenes the GPU tier feeds the device-batch kernels -- correspondence counts relative
to the kernels' LDS rings, the load of their tables, cluster sizes and probe runs across a table's end (the insertion
simulated on the host), duplicate placements, runs on round boundaries -- and that every scene discriminates: a
deliberately WRONG variant of the Python reference (a ring that drops record `ring` and later, "last duplicate wins", a
lookup that gives up at the table's end, a sort of 4096 keys only) gives outputs that differ from the true reference's.
The kernels are never mutated: a mutated table without an empty slot would not fail, it would hang."""
import numpy as np
import pytest

import place_query_ref as RQ
import place_query_scenes as SQ
import ransac2d2d_ref as R2
import ransac2d2d_scenes as S2
import ransac_ref as R
import ransac_scenes as S
import stereo_insert_scenes as SI
from okvis2_amd import capi

N_SLOTS = capi.RANSAC2D2D_MAX_KEYPOINTS + 1
KS = (1100, capi.RANSAC2D2D_MAX_KEYPOINTS)
slot = capi.Frontend._test_ransac2d2d_id_slot


def _hooks():
    return capi.Frontend._test_ransac2d2d_ring_records(), capi.Frontend._test_ransac2d2d_chunk_records()


def _same(a, b):
    """two reference results of one pair agree in everything the GPU tier compares"""
    if (a["total_inliers"], a["rotation_only"], a["success"]) != (b["total_inliers"], b["rotation_only"], b["success"]):
        return False
    for ca, cb in zip(a["cams"], b["cams"]):
        if any(ca[k] != cb[k] for k in S2.PER_CAM):
            return False
        for k in ("rot_hyp_inliers", "rel_hyp_inliers", "match1", "state", "landmark1_out", "dist_set"):
            if not np.array_equal(ca[k], cb[k]):
                return False
        if not np.array_equal(ca["distance"].view(np.uint64), cb["distance"].view(np.uint64)):
            return False
    return True


# ---- the wrong variants of ransac2d2d_ref.correspondences ----------------------------------------------------------
def _filtered(corr, keep):
    return {k: v[keep] for k, v in corr.items()}


def _ring_drops(ring):
    """a ring that keeps the records below `ring` and drops the later ones"""
    true = R2.correspondences

    def wrong(tree, fr0, fr1, fu, added=None, census=None):
        corr = true(tree, fr0, fr1, fu, added, census)
        return _filtered(corr, np.arange(len(corr["kA"])) < ring)
    return wrong


def _last_duplicate_wins():
    """the LAST current keypoint of an id: the true reference on the current block read backwards"""
    true = R2.correspondences

    def wrong(tree, fr0, fr1, fu, added=None, census=None):
        back = {k: np.asarray(v)[::-1] for k, v in fr1.items()}
        corr = true(tree, fr0, back, fu, added, census)
        corr["kB"] = len(fr1["lm"]) - 1 - corr["kB"]
        return corr
    return wrong


def _lookup_stops_at_the_table_end():
    """a lookup that answers "none" when its probe reaches the last slot without a hit or an empty slot"""
    true = R2.correspondences

    def wrong(tree, fr0, fr1, fu, added=None, census=None):
        corr = true(tree, fr0, fr1, fu, added, census)
        tab = S2.id_table(fr1["lm"], added, slot, N_SLOTS)
        lm0 = np.asarray(fr0["lm"])
        keep = np.array([S2.table_lookup(tab, fr1["lm"], slot, int(lm0[k]), wrap=False)[0] >= 0 for k in corr["kA"]], bool)
        return _filtered(corr, keep)
    return wrong


def _defeats(monkeypatch, sc, wrong, tree=True):
    """the pairs of `sc` on which the wrong variant's outputs differ from the true reference's"""
    true = S2.reference(tree, sc)
    with monkeypatch.context() as m:
        m.setattr(R2, "correspondences", wrong)
        bad = S2.reference(tree, sc)
    return [i for i, (a, b) in enumerate(zip(true, bad)) if not _same(a, b)]


# ---- ransac2d2d ------------------------------------------------------------------------------------------------------
def test_the_hash_restated_on_the_host_is_the_kernels():
    rng = np.random.default_rng(5)
    ids = np.concatenate([[0, 1, 2**31 - 1, 2**22 - 1], rng.integers(0, 2**31, 996)])
    assert len(ids) == 1000
    assert S2.host_slot(ids, N_SLOTS).tolist() == [slot(int(i)) for i in ids]
    assert N_SLOTS == 4096 and S2.host_slot(ids, N_SLOTS).tolist() == [((int(i) * 2654435761) % 2**32) >> 20 for i in ids]
    assert set(capi.TEST_HOOKS) >= {"okvfe_test_ransac2d2d_ring_records", "okvfe_test_ransac2d2d_id_slot",
                                    "okvfe_test_ransac_ring_records"}
    assert all(hasattr(capi.lib(), n) for n in capi.TEST_HOOKS)


@pytest.mark.parametrize("Kc", KS)
def test_ring_scenes_wrap_the_ring(oracle, monkeypatch, Kc):
    ring, chunk = _hooks()
    sc = S2.ring_scene(oracle, ring, chunk, Kc)
    refs = S2.reference(True, sc)
    counts = [r["cams"][0]["n_corr"] for r in refs]
    assert counts == [ring - 1, ring, ring + 1, 2 * ring + chunk - 1, Kc] and counts[3] // ring == 2
    assert all(r["success"] == 2 and r["cams"][0]["removed"] == 1 for r in refs)
    # uneven tiles: the records a 256-keypoint tile of the older block adds
    tiles = [np.bincount(r["cams"][0]["corr"]["kA"] // 256).tolist() for r in refs]
    assert all(len(set(t)) > 1 for t in tiles[:4]), tiles
    beaten = _defeats(monkeypatch, sc, _ring_drops(ring))
    print(sc["name"], "correspondences", counts, "records per tile", tiles, "| a ring that drops record %d and later "
          "differs on pairs" % ring, beaten)
    assert beaten == [2, 3, 4]  # every pair past the ring's size
    two = S2.ring_restart_scene(oracle, ring, chunk, Kc)
    refs2 = S2.reference(True, two)
    counts2 = [tuple(c["n_corr"] for c in r["cams"]) for r in refs2]
    assert counts2 == list(S2.ring_restart_totals(ring, chunk))
    assert counts2[0][0] > ring > counts2[0][1] and counts2[1][0] < ring < counts2[1][1] and min(counts2[2]) > ring
    beaten2 = _defeats(monkeypatch, two, _ring_drops(ring))
    print(two["name"], "correspondences", counts2, "| the dropping ring differs on pairs", beaten2)
    assert beaten2 == [0, 1, 2]


@pytest.mark.parametrize("with_added", (True, False), ids=("added", "null"))
def test_full_table_scene_leaves_one_empty_slot(oracle, monkeypatch, with_added):
    Kc = capi.RANSAC2D2D_MAX_KEYPOINTS
    sc = S2.full_table_scene(oracle, Kc, with_added)
    cam = sc["pairs"][0][0]
    lm1, lm0 = cam["fr1"]["lm"], cam["fr0"]["lm"]
    assert len(lm1) == Kc == len(set(lm1.tolist())) and lm1.min() >= 0 and (sc["added"] is None) != with_added
    tab = S2.id_table(lm1, sc["added"], slot, N_SLOTS)
    assert int((tab < 0).sum()) == 1
    present = np.isin(lm0, lm1)
    absent = (lm0 >= 0) & ~present
    assert int(present.sum()) == 2500 and int(absent.sum()) == 1000 == len(sc["absent"]) and int((lm0 < 0).sum()) == Kc - 3500
    empty = int(np.flatnonzero(tab < 0)[0])
    steps = []
    for lm in lm0[absent].tolist():
        k, n = S2.table_lookup(tab, lm1, slot, lm)
        assert k == -1 and (int(slot(lm)) + n - 1) % N_SLOTS == empty
        steps.append(n)
    hit = [S2.table_lookup(tab, lm1, slot, lm)[1] for lm in lm0[present].tolist()]
    ref = S2.reference(True, sc)[0]["cams"][0]
    print(sc["name"], "load %d / %d" % (Kc, N_SLOTS), "absent lookups: %d, probes mean %.0f max %d" %
          (len(steps), np.mean(steps), max(steps)), "| hits: probes mean %.0f max %d" % (np.mean(hit), max(hit)),
          "| correspondences", ref["n_corr"])
    assert ref["n_corr"] == 2500 and max(steps) > N_SLOTS // 2 and sum(s > 1000 for s in steps) >= 100
    # present ids that sit behind the table's end from their home: a lookup that stops there loses them
    end = _defeats(monkeypatch, sc, _lookup_stops_at_the_table_end())
    print(sc["name"], "| a lookup that stops at the table's end differs:", bool(end))
    assert end == [0]


def test_collision_scene_runs_cross_the_table_end(oracle, monkeypatch):
    Kc = KS[0]
    sc = S2.collision_scene(oracle, slot, N_SLOTS, Kc)
    cam, cl, dups = sc["pairs"][0][0], sc["clusters"], sc["duplicates"]
    lm1, lm0 = cam["fr1"]["lm"], cam["fr0"]["lm"]
    assert sc["added"] is None and N_SLOTS - 6 <= cl["home_a"] < N_SLOTS
    assert len(set(cl["a_ids"].tolist())) >= 300 and all(slot(int(i)) == cl["home_a"] for i in cl["a_ids"])
    assert len(cl["b_ids"]) >= 64 and all(slot(int(i)) == cl["home_b"] for i in cl["b_ids"])
    assert set(cl["a_ids"].tolist()) | set(cl["b_ids"].tolist()) <= set(lm1.tolist())
    # the first cluster alone ends its run at the second's home; in the whole table the run goes on through it
    alone = S2.id_table(np.where(np.isin(lm1, cl["a_ids"]), lm1, -1), None, slot, N_SLOTS)
    end_alone = next(s % N_SLOTS for s in range(cl["home_a"], cl["home_a"] + N_SLOTS) if alone[s % N_SLOTS] < 0)
    assert end_alone == cl["home_b"] < cl["home_a"]  # (the run has wrapped)
    tab = S2.id_table(lm1, None, slot, N_SLOTS)
    run = next(n for n in range(N_SLOTS) if tab[(cl["home_a"] + n) % N_SLOTS] < 0)
    assert run >= len(cl["a_ids"]) + len(cl["b_ids"]) and np.all(tab[N_SLOTS - 3:] >= 0) and tab[0] >= 0
    past_end = sum(1 for s in range(0, run - 3) if lm1[tab[s]] in set(cl["a_ids"].tolist()))  # (slots 0 .. of the run)
    assert past_end >= 300
    # duplicates: both placements, both orders; the smaller keypoint is the table's and the reference's
    same = [d for d in dups if d[3]]
    other = [d for d in dups if not d[3]]
    assert len(dups) >= 64 and len(same) >= 32 and len(other) >= 32
    assert all(a // 256 == b // 256 for _, a, b, _ in same) and all(a // 256 != b // 256 for _, a, b, _ in other)
    assert all(lm1[a] == lm1[b] == lm for lm, a, b, _ in dups)
    for group in (same, other):
        assert sum(a < b for _, a, b, _ in group) >= 4 and sum(a > b for _, a, b, _ in group) >= 4, group
    ref = S2.reference(True, sc)[0]["cams"][0]
    row0 = {int(l): k for k, l in enumerate(lm0.tolist()) if l >= 0}
    for lm, a, b, _ in dups:
        assert S2.table_lookup(tab, lm1, slot, lm)[0] == min(a, b) == ref["match1"][row0[lm]]
    # the older block looks up cluster ids, duplicated ids and absent ids with homes inside the clusters
    assert set(cl["a_ids"].tolist()) | set(cl["b_ids"].tolist()) <= set(lm0.tolist())
    assert set(cl["absent"].tolist()) <= set(lm0.tolist()) and not set(cl["absent"].tolist()) & set(lm1.tolist())
    homes = [slot(int(i)) for i in cl["absent"]]
    assert homes.count(cl["home_a"]) >= 16 and homes.count(cl["home_b"]) >= 16 and homes.count(7) >= 16
    steps = [S2.table_lookup(tab, lm1, slot, int(i)) for i in cl["absent"]]
    assert all(k == -1 for k, _ in steps) and max(n for _, n in steps) > run - 8
    last = _defeats(monkeypatch, sc, _last_duplicate_wins())
    end = _defeats(monkeypatch, sc, _lookup_stops_at_the_table_end())
    print(sc["name"], "clusters", len(cl["a_ids"]), "+", len(cl["b_ids"]), "homes", cl["home_a"], cl["home_b"], "run", run,
          "slots,", past_end, "first-cluster ids past the table's end | duplicates", len(same), "same tile", len(other),
          "other tile | absent lookups", len(steps), "longest", max(n for _, n in steps), "| correspondences",
          ref["n_corr"], "| last-duplicate-wins differs:", bool(last), "| a lookup that stops at the table's end differs:",
          bool(end))
    assert last == [0] and end == [0]
    # ... and the other scenes are indifferent to these two variants (no duplicates, no run across the end)
    ring, chunk = _hooks()
    assert _defeats(monkeypatch, S2.ring_scene(oracle, ring, chunk, Kc), _last_duplicate_wins()) == []


# ---- 3d2d / place consensus ------------------------------------------------------------------------------------------
def test_lap_scene_runs_two_laps_of_the_ring(oracle, monkeypatch):
    ring, chunk = capi.Frontend._test_ransac_ring_records(), capi.Frontend._test_ransac_chunk_records()
    assert ring == 2 * chunk
    sc = S.lap_scene(oracle, ring, chunk)
    assert len(sc["cams"]) == 5 and len(sc["cams"]) * S.K < S.lap_totals(ring, chunk)[-1] <= len(sc["cams"]) * S.LAP_K
    refs = S.reference(True, sc)
    counts = [r["n_corr"] for r in refs]
    assert counts == [2 * ring - 1, 2 * ring, 2 * ring + 1, 2 * ring + chunk + 7]
    # the last partial chunk starts behind the second wrap: the records scored before it are whole chunks
    assert (counts[3] // chunk) * chunk > 2 * ring and counts[3] % chunk == 7
    # uneven tiles of 256 slots (camera-major: slot = camera * K + keypoint)
    tiles = [np.bincount((r["corr"]["cam"] * S.LAP_K + r["corr"]["row"]) // 256).tolist() for r in refs]
    assert all(len(set(t)) > 2 for t in tiles)
    assert all(r["best"] >= 0 and min(int((np.concatenate(r["state"]) == v).sum()) for v in (1, 2)) >= 16 for r in refs)
    assert [r["accepted"] for r in refs] == [1, 0, 1, 1]
    true = R.correspondences

    def wrong(*args, **kw):  # a ring that drops record `ring` and later
        corr = true(*args, **kw)
        return {k: v[:ring] for k, v in corr.items()}

    with monkeypatch.context() as m:
        m.setattr(R, "correspondences", wrong)
        bad = S.reference(True, sc)
    beaten = [i for i, (a, b) in enumerate(zip(refs, bad))
              if a["n_corr"] != b["n_corr"] or not np.array_equal(np.concatenate(a["state"]), np.concatenate(b["state"]))]
    print(sc["name"], "correspondences", counts, "of a ring of", ring, "| records per tile", tiles,
          "| a ring that drops record %d and later differs on multiframes" % ring, beaten)
    assert beaten == [0, 1, 2, 3]


# ---- bow_vectors -----------------------------------------------------------------------------------------------------
def _sorted_keys(voc, words):
    """the keys the kernel sorts: the words of the features whose weight is > 0"""
    words = np.concatenate(words)
    return np.sort(words[(words >= 0) & (voc["ww"][np.maximum(words, 0)] > 0)])


def _heads_per_round(keys):
    heads = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    return heads, np.bincount(heads // SQ.ROUND, minlength=-(-len(keys) // SQ.ROUND))


def test_bow_capacity_scene(oracle):
    voc = RQ.shipped_vocabulary(oracle)
    sc = SQ.capacity_scene(oracle, voc)
    refs = SQ.reference_vectors(oracle, voc, sc)
    totals = [sum(c) for c in sc["counts"]]
    assert sc["n_cams"] * sc["K"] == capi.BOW_MAX_FEATURES == 8192
    assert totals == [8192, 8191, 4097, 4096, SQ.LONG_RUN, SQ.LONG_RUN + 40, sum(SQ.BOUNDARY_COUNTS)]
    # the premise of the out-of-LDS descent of the SMALL tree: a context of 8192 keys leaves no room for its 820 nodes
    n_nodes = len(voc["word"])
    assert n_nodes <= SQ.LDS_NODES and n_nodes * 48 + 8192 * 4 > SQ.LDS_BUDGET >= n_nodes * 48 + 4096 * 4
    assert not SQ.nodes_in_lds(n_nodes, sc["n_cams"] * sc["K"]) and SQ.nodes_in_lds(n_nodes, 5 * 700)
    keys = [_sorted_keys(voc, r[0]) for r in refs]
    assert [len(k) for k in keys] == totals  # (every word of the shipped vocabulary has a weight > 0)
    # the long runs: rounds without a run head
    for m, floor in ((4, 19), (5, 18)):
        heads, per_round = _heads_per_round(keys[m])
        headless = int((per_round == 0).sum())
        run = int((keys[m] == sc["long_word"]).sum())
        print("multiframe", m, "keys", len(keys[m]), "words", len(refs[m][1]), "longest run", run, "rounds", len(per_round),
              "without a head", headless)
        assert run == SQ.LONG_RUN and headless >= floor
    assert len(refs[4][1]) == 1 and len(refs[5][1]) == 41
    start5 = int(np.flatnonzero(keys[5] == sc["long_word"])[0])
    assert 0 < start5 < SQ.ROUND  # the run begins inside round 0, behind smaller words
    # runs on round boundaries
    heads, per_round = _heads_per_round(keys[6])
    ends = np.concatenate([heads[1:], [len(keys[6])]])
    on = [(int(a), int(b)) for a, b in zip(heads, ends) if a % SQ.ROUND == 0]
    both = [(a, b) for a, b in on if b % SQ.ROUND == 0]
    print("multiframe 6 keys", len(keys[6]), "runs", len(heads), "lengths", (ends - heads).tolist(), "| starting on a round "
          "boundary", on, "| starting and ending on one", both)
    assert (ends - heads).tolist() == list(SQ.BOUNDARY_COUNTS) and np.array_equal(refs[6][1], np.sort(sc["boundary_words"]))
    assert len([a for a, _ in on if a > 0]) >= 2 and len(both) >= 1 and int((ends % SQ.ROUND == 0).sum()) >= 2
    # a sort that handles 4096 keys only: the vector of the first 4096 features
    beaten = []
    for m, cams in enumerate(sc["feats"]):
        _, ids, vals = RQ.bow_vector(oracle, voc, np.concatenate(cams)[:4096])
        if not (np.array_equal(ids, refs[m][1]) and np.array_equal(vals.view(np.uint64), refs[m][2].view(np.uint64))):
            beaten.append(m)
    print("a sort of 4096 keys only differs on multiframes", beaten)
    assert beaten == [0, 1, 2, 5, 6]  # (3 has 4096 features; 4's one word is normalised to 1.0 whatever its count)
    plain = dict(voc, normalise_l1=False)
    assert not np.array_equal(RQ.bow_vector(oracle, plain, np.concatenate(sc["feats"][4])[:4096])[2],
                              RQ.bow_vector(oracle, plain, np.concatenate(sc["feats"][4]))[2])


# ---- stereo_insert ---------------------------------------------------------------------------------------------------
def test_stereo_insert_table_edges(oracle):
    # (a) three cameras: n_cams K = 2^a - 1, the overlay has ONE slot more than it may hold
    Ka = next(k for k in range(1, 4097) if 3 * k == (1 << SI.lds_bytes(3, k)[1]) - 1 and 3 * k > 3 * SI.K)
    assert Ka == 341 and SI.lds_bytes(3, Ka) == (4 * (1023 + 1024 + 1023 + 1024), 10, 10)
    # (b) two cameras: the largest capacity the LDS limit admits
    Kb = SI.largest_capacity(2)
    assert Kb == 1625 and SI.lds_bytes(2, Kb)[0] <= SI.MAX_LDS < SI.lds_bytes(2, Kb + 1)[0]
    for n_cams, Kc in ((3, Ka), (2, Kb)):
        sc = SI.table_edge_scene(oracle, n_cams, Kc)
        _, ov_log2, kh_log2 = SI.lds_bytes(n_cams, Kc)
        mf = sc["mfs"][0]
        ids = np.concatenate(mf["ids"])
        assert all(len(k) == Kc for k in mf["kps"]) and len(set(ids.tolist())) == n_cams * Kc and ids.min() >= 0
        assert ids.max() < len(sc["hp"]) and not sc["initialised"].any()
        for p, (c0, c1) in enumerate(sc["pairs"]):
            r = mf["matches"][p]
            assert sorted(r["k1"].tolist()) == list(range(Kc)) and np.all(r["initialisable"] != 0)
            keys = set(mf["ids"][c0].tolist()) | set(mf["ids"][c1].tolist())
            assert len(keys) == 2 * Kc  # the pair's key table: 2 K entries
        (ref,), census = SI.reference_of(oracle, True, sc)
        matched, created, reinit, observations = ref["counts"].tolist()
        print(sc["name"], "pairs", sc["pairs"], "| key table %d / %d per pair" % (2 * Kc, 1 << kh_log2),
              "| overlay %d / %d" % (reinit, 1 << ov_log2), "| matched", matched, "created", created, "observations", observations)
        assert matched == n_cams * Kc and reinit == n_cams * Kc and created == 0
        assert all(np.all(a == 1) for a in ref["action"])
        if n_cams == 3:
            assert reinit == (1 << ov_log2) - 1
