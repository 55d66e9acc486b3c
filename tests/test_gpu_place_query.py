"""GPU: place recognition on device-resident batches -- okvfe_bow_vectors_blocks_device, okvfe_place_query_blocks_device,
okvfe_bow_database_add_blocks_device, okvfe_bow_database_check_device -- against place_query_ref.py (the oracle's chain per
multiframe, the transcription of Frontend.cpp:761-802, add as list appends), byte for byte: integers for equality,
doubles as uint64 patterns, no row exempt; rows the calls leave alone keep their sentinels.  Descriptors are vocabulary
leaves with a few bits flipped, packed straight into gather blocks."""
import numpy as np
import pytest

import place_query_ref as R
import place_query_scenes as S
from okvis2_amd import capi

pytestmark = [pytest.mark.gpu]
torch = pytest.importorskip("torch")

_FRONTENDS = {}


def _frontend(K):
    if K not in _FRONTENDS:
        _FRONTENDS[K] = capi.Frontend(128, 128, 10.0, 0, 50, K, num_cameras=1)
        assert _FRONTENDS[K].max_keypoints == K
    return _FRONTENDS[K]


@pytest.fixture(scope="module", autouse=True)
def _close_frontends():
    yield
    while _FRONTENDS:
        _FRONTENDS.popitem()[1].close()


def _vectors(fe, dev, voc, scene, stride=None, word_ids=True, stream=None, name="q"):
    """launches the vectors call on the scene's blocks; -> (BowVectorsDevice, stride)"""
    M, n_cams, K = len(scene["feats"]), scene["n_cams"], scene["K"]
    stride = min(n_cams * K, len(voc["ww"])) if stride is None else stride
    if "blocks" not in dev.t:
        dev.put("blocks", S.pack_blocks(scene))
    vd = dev.vocabulary(voc)
    vec = dev.vectors(M, stride, len(voc["ww"]), name)
    wptr = dev.out("word_ids", M * n_cams * K * 4) if word_ids else None
    torch.cuda.synchronize()  # the fills above ran on torch's stream
    fe.bow_vectors_blocks_device(vd, dev.ptr("blocks"), M, n_cams, vec, wptr, stream=stream)
    return vec, stride


def _check_word_ids(dev, scene, refs):
    M, n_cams, K = len(scene["feats"]), scene["n_cams"], scene["K"]
    got = dev.get("word_ids", np.int32, M, n_cams, K)
    for m, (words, _, _) in enumerate(refs):
        for c in range(n_cams):
            n = len(words[c])
            assert np.array_equal(got[m, c, :n], words[c]), (m, c)
            assert np.all(got[m, c, n:] == S.FILL_I32), (m, c)


def _prepare_query(dev, M, E, cap, with_scores, suppressible):
    """sentinel-filled outputs of a query call; E: the entries the database will hold when the call runs"""
    sptr = dev.out("scores", M * E * 8) if with_scores else None
    supp = None if suppressible is None else dev.put("supp", np.asarray(suppressible, np.uint8))
    cand = dev.candidates(M, cap)
    torch.cuda.synchronize()  # the fills above ran on torch's stream
    return sptr, supp, cand


def _query(fe, dev, oracle, dbd, db, vec, refs, suppressible, min_score, cap, with_scores, what, stream=None,
           prepared=None):
    """the query call against the reference: all scores (if asked for) and the candidates"""
    M, E = len(refs), len(db.entries)
    sptr, supp, cand = prepared or _prepare_query(dev, M, E, cap, with_scores, suppressible)
    fe.place_query_blocks_device(dbd, vec, M, cand, min_score=min_score, suppressible_ptr=supp, scores_ptr=sptr,
                                 stream=stream)
    ref_scores = [db.scores(oracle, ids, vals) for _, ids, vals in refs]
    if with_scores and E:
        got = dev.get("scores", np.uint64, M, E)
        for m in range(M):
            assert np.array_equal(got[m], ref_scores[m].view(np.uint64)), (what, m)
    walks = [R.walk(s, suppressible, min_score) for s in ref_scores]
    S.check_candidates(dev, M, cap, walks, what)
    return ref_scores, walks


@pytest.mark.parametrize("n_cams", [1, 2, 5])
def test_rigs_and_counts(oracle, n_cams):
    """rigs of 1, 2 and 5 cameras; blocks of 0, 1 and K keypoints; a multiframe without any feature"""
    K = 700
    voc = R.shipped_vocabulary(oracle)
    scene = S.rig_scene(oracle, voc, n_cams, K)
    fe, dev = _frontend(K), S.Dev(torch)
    refs = S.reference_vectors(oracle, voc, scene)
    vec, stride = _vectors(fe, dev, voc, scene)
    S.check_vectors(dev, refs, stride, n_cams)
    _check_word_ids(dev, scene, refs)
    assert len(refs[4][1]) == 0 and len(refs[5][1]) == 1 and max(len(r[1]) for r in refs) > 60
    db = S.host_database(oracle, voc, scene, 40)
    dbd = dev.database(db)
    for min_score, cap in ((R.MIN_SCORE, 8), (0.02, 40)):
        scores, walks = _query(fe, dev, oracle, dbd, db, vec, refs, None, min_score, cap, True, (n_cams, min_score))
    assert np.all(scores[4] == -1.0) and walks[4] == (0, [])  # no feature: nothing listed
    assert all(s[20] == -1.0 for s in scores)                 # the empty entry is never listed
    assert sum(s[21] == -1.0 for s in scores) >= 6            # an entry sharing no word with most queries
    assert max(len(w[1]) for w in walks) >= 3


def test_weightings_and_normalisation(oracle):
    """all four weightings, with and without normalise_l1"""
    K = 700
    base = R.shipped_vocabulary(oracle)
    scene = S.rig_scene(oracle, base, 2, K)
    fe, dev = _frontend(K), S.Dev(torch)
    seen = set()
    for weighting in range(4):
        for norm in (True, False):
            voc = dict(base, weighting=weighting, normalise_l1=norm)
            refs = S.reference_vectors(oracle, voc, scene)
            vec, stride = _vectors(fe, dev, voc, scene, word_ids=False)
            S.check_vectors(dev, refs, stride, (weighting, norm))
            seen.add(refs[0][2].tobytes())
    assert len(seen) == 4  # sums or not, normalised or not (the weight table is the vocabulary's under every weighting)


def test_weight_table_with_zeros_negatives_and_a_nan(oracle):
    K = 700
    base = R.shipped_vocabulary(oracle)
    scene = S.rig_scene(oracle, base, 2, K)
    plain = S.reference_vectors(oracle, base, scene)
    ww = base["ww"].copy()
    used = plain[0][1]
    ww[used[0::4]] = 0.0
    ww[used[1::4]] = -ww[used[1::4]]
    ww[used[2]] = np.nan
    voc = dict(base, ww=ww)
    fe, dev = _frontend(K), S.Dev(torch)
    refs = S.reference_vectors(oracle, voc, scene)
    assert 0 < len(refs[0][1]) < len(plain[0][1]) and not np.isnan(refs[0][2]).any()
    vec, stride = _vectors(fe, dev, voc, scene)
    S.check_vectors(dev, refs, stride, "weights")
    _check_word_ids(dev, scene, refs)  # the word of every feature, those of skipped words too


def test_synthetic_vocabulary_of_27000_words(oracle):
    """the descent out of LDS and the BowVector beyond any dense table; a leaf at depth 1, a single child, exact ties"""
    K = 300
    voc = R.synthetic_vocabulary(oracle)
    assert len(voc["word"]) > 1024 and len(voc["ww"]) > 27000
    rng = np.random.default_rng(9)
    scene = S.rig_scene(oracle, voc, 2, K, per_place=400)
    # features that stop at the depth-1 leaf, go through the single child, and meet two identical siblings
    cb, ci, word = voc["cb"], voc["ci"], voc["word"]
    depth1_leaf = int([c for c in ci[cb[0]:cb[1]] if cb[c + 1] == cb[c]][0])
    single = int([c for c in ci[cb[0]:cb[1]] if cb[c + 1] - cb[c] == 1][0])
    below_single = word[ci[cb[ci[cb[single]]]:cb[ci[cb[single]] + 1]]]
    twins = [(int(ci[cb[i]]), int(ci[cb[i] + 1])) for i in range(0, len(word), 10)
             if cb[i + 1] - cb[i] >= 2 and word[ci[cb[i]]] >= 0][:40]
    assert len(twins) == 40 and all(np.array_equal(voc["desc"][a], voc["desc"][b]) for a, b in twins)
    flips = np.zeros((20, 48), np.uint8)
    flips[np.arange(20), np.arange(20)] = 1
    special = np.concatenate([voc["desc"][[depth1_leaf] * 3], voc["desc"][[single] * 20] ^ flips,
                              voc["desc"][[b for _, b in twins]]])
    scene["feats"][8][0] = np.concatenate([special, S.view(voc, rng, scene["places"][0], K - len(special))])
    fe, dev = _frontend(K), S.Dev(torch)
    refs = S.reference_vectors(oracle, voc, scene)
    words8 = refs[8][0][0]
    assert (words8[:3] == word[depth1_leaf]).all() and np.isin(words8[3:23], below_single).all()
    # the first of two identical siblings wins, never the second (three of the 40 hang below a second twin higher up
    # and are carried elsewhere by that tie)
    assert (words8[23:63] == word[[a for a, _ in twins]]).sum() >= 30
    assert (words8[23:63] == word[[b for _, b in twins]]).sum() == 0
    vec, stride = _vectors(fe, dev, voc, scene)
    assert stride == 2 * K
    S.check_vectors(dev, refs, stride, "synthetic")
    _check_word_ids(dev, scene, refs)
    db = S.host_database(oracle, voc, scene, 30)
    dbd = dev.database(db)
    _, walks = _query(fe, dev, oracle, dbd, db, vec, refs, None, 0.01, 30, True, "synthetic")
    assert max(w[0] for w in walks) >= 10


def test_query_without_the_vocabulary_size_takes_the_merge(oracle):
    """n_vocabulary_words = 0: the sorted-vector path on the shipped vocabulary gives the dense table's bits"""
    K = 128
    voc = R.shipped_vocabulary(oracle)
    scene = S.rig_scene(oracle, voc, 1, K)
    fe, dev = _frontend(K), S.Dev(torch)
    refs = S.reference_vectors(oracle, voc, scene)
    vec, stride = _vectors(fe, dev, voc, scene)
    db = S.host_database(oracle, voc, scene, 50)
    dbd = dev.database(db)
    supp = (np.arange(50) % 3 != 0).astype(np.uint8)
    for nv in (len(voc["ww"]), 0):
        vec.n_vocabulary_words = nv
        _query(fe, dev, oracle, dbd, db, vec, refs, supp, 0.05, 50, True, ("merge", nv))


def test_query_vectors_longer_than_the_rows_staged_in_lds(oracle):
    """hand-built vectors of 4500 words (the vectors call cannot make one: 4096 words are staged, longer vectors are
    merged from memory) next to a short one, against entries that share few, many and no words"""
    fe, dev = _frontend(64), S.Dev(torch)
    rng = np.random.default_rng(31)
    n_words, stride = 12000, 5000

    def vector(n):
        ids = np.sort(rng.choice(n_words, n, replace=False)).astype(np.int32)
        v = rng.random(n) + 0.1
        return ids, v / v.sum()

    vecs = [vector(4500), vector(300), vector(4097), vector(4096)]
    db = R.Database(n_words)
    for n in (40, 3000, 0, 700, 5, 4500):
        db.add(*vector(n))
    refs = [(None, i, v) for i, v in vecs]
    vec = dev.vectors_from_host(vecs, stride, 0)
    dbd = dev.database(db)
    scores, walks = _query(fe, dev, oracle, dbd, db, vec, refs, None, 0.01, 6, True, "long vectors")
    assert all(s[2] == -1.0 for s in scores) and max(w[0] for w in walks) >= 5


@pytest.mark.parametrize("E", [0, 1, 255, 256, 257])
def test_database_sizes(oracle, E):
    """the chunk of 256 entries and its neighbours; an empty entry; scores_dev given and NULL; suppressible_dev NULL and
    given; cap below the count"""
    K = 64
    voc = R.shipped_vocabulary(oracle)
    scene = S.rig_scene(oracle, voc, 1, K)
    fe, dev = _frontend(K), S.Dev(torch)
    refs = S.reference_vectors(oracle, voc, scene)
    vec, stride = _vectors(fe, dev, voc, scene)
    S.check_vectors(dev, refs, stride, E)
    db = S.host_database(oracle, voc, scene, E, per_entry=40)
    dbd = dev.database(db)
    supp = (np.random.default_rng(E).random(E) < 0.6).astype(np.uint8)
    results = {}
    for with_scores in (True, False):
        for s in (None, supp):
            _, walks = _query(fe, dev, oracle, dbd, db, vec, refs, s, 0.03, max(E, 1), with_scores, (E, with_scores, s is None))
            results[(with_scores, s is None)] = (dev.get("c_entry", np.int32, len(refs), max(E, 1)).tobytes(),
                                                 dev.get("c_count", np.int32, len(refs)).tobytes())
    assert results[(True, True)] == results[(False, True)] and results[(True, False)] == results[(False, False)]
    if E >= 255:
        most = max(len(w[1]) for w in walks)
        assert most >= 6
        _query(fe, dev, oracle, dbd, db, vec, refs, supp, 0.03, 3, False, (E, "cap 3"))  # true count, first 3 stored
        _query(fe, dev, oracle, dbd, db, vec, refs, supp, 0.03, 0, False, (E, "cap 0"))


def _walk_scene_on_device(sc):
    """query m holds the one word m with value 1, entry e holds word m with value scores[m][e]: the score is that value"""
    M, E = sc["scores"].shape
    vecs = [(np.array([m], np.int32), np.array([1.0])) for m in range(M)]
    db = R.Database(M)
    for e in range(E):
        words = np.flatnonzero(sc["scores"][:, e] != -1.0).astype(np.int32)
        db.add(words, sc["scores"][words, e])
    return vecs, db


@pytest.mark.parametrize("n_vocabulary_words", [R.WALK_QUERIES, 0], ids=["dense", "merge"])
def test_walk_scenes(oracle, n_vocabulary_words):
    """the scenes whose census test_place_query_host.py asserts, with scores the device reproduces exactly: every
    situation of :780-802 across the 256-entry chunks, the ring and the final flush"""
    fe = _frontend(64)
    for sc in R.walk_scenes():
        dev = S.Dev(torch)
        vecs, db = _walk_scene_on_device(sc)
        M, E = sc["scores"].shape
        refs = [(None, i, v) for i, v in vecs]
        vec = dev.vectors_from_host(vecs, 4, n_vocabulary_words)
        dbd = dev.database(db)
        for supp in (sc["suppressible"], None):
            for cap in (max(E, 1), 2):
                scores, _ = _query(fe, dev, oracle, dbd, db, vec, refs, supp, sc["min_score"], cap, True, (E, cap))
        for m in range(M):
            assert np.array_equal(np.asarray(scores[m]).reshape(-1), sc["scores"][m]), (E, m)  # (the construction holds)


def test_adds(oracle):
    """none, some and all multiframes; appended entries equal the vectors; two adds and a query queued on one stream
    without a synchronisation in between; cap_entries exceeded; cap_words exceeded"""
    K = 128
    voc = R.shipped_vocabulary(oracle)
    scene = S.rig_scene(oracle, voc, 2, K)
    M = len(scene["feats"])
    fe, dev = _frontend(K), S.Dev(torch)
    refs = S.reference_vectors(oracle, voc, scene)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    vec, stride = _vectors(fe, dev, voc, scene, word_ids=False, stream=stream)
    some = [1, 4, 5, 9]
    db = S.host_database(oracle, voc, scene, 5)
    words0 = int(db.arrays()[0][-1])
    dbd = dev.database(db, cap_entries=5 + M + 4, cap_words=words0 + 2 * M * stride)
    prepared = _prepare_query(dev, M, 5 + len(some) + M, 8, True, None)
    fe.bow_database_add_blocks_device(dbd, vec, M, [], stream=stream)       # none
    assert dbd.n_entries == 5
    fe.bow_database_add_blocks_device(dbd, vec, M, some, stream=stream)     # some (one of them empty: multiframe 4)
    assert dbd.n_entries == 5 + len(some)
    fe.bow_database_add_blocks_device(dbd, vec, M, list(range(M)), stream=stream)  # all
    assert dbd.n_entries == 5 + len(some) + M
    for m in some + list(range(M)):
        db.add(refs[m][1], refs[m][2])
    _query(fe, dev, oracle, dbd, db, vec, refs, None, 0.05, 8, True, "after the adds", stream=stream,
           prepared=prepared)
    fe.bow_database_check_device(dbd, stream=stream)  # the one synchronisation
    begin, ids, vals = db.arrays()
    E = len(db.entries)
    assert np.array_equal(dev.get("db_begin", np.int32, E + 1), begin)
    assert np.array_equal(dev.get("db_ids", np.int32, len(ids)), ids)
    assert np.array_equal(dev.get("db_vals", np.uint64, len(vals)), vals.view(np.uint64))
    assert np.all(dev.get("db_begin", np.int32, dbd.cap_entries + 1)[E + 1:] == S.FILL_I32)
    assert np.all(dev.get("db_ids", np.int32, dbd.cap_words)[len(ids):] == S.FILL_I32)
    # cap_entries exceeded: an error before anything is launched, nothing changed
    before = {k: dev.t[k].clone() for k in ("db_begin", "db_ids", "db_vals", "db_overflow")}
    with pytest.raises(capi.OkvfeError) as e:
        fe.bow_database_add_blocks_device(dbd, vec, M, [0, 1, 2, 3, 4], stream=stream)
    assert e.value.status == capi.ERR_CAPACITY and dbd.n_entries == E
    for bad in ([2, 2], [3, 1], [M], [-1]):
        with pytest.raises(capi.OkvfeError) as e:
            fe.bow_database_add_blocks_device(dbd, vec, M, bad, stream=stream)
        assert e.value.status == capi.ERR_INVALID_ARGUMENT and dbd.n_entries == E
    torch.cuda.synchronize()
    assert all(torch.equal(dev.t[k], before[k]) for k in before)


def test_add_runs_out_of_words(oracle):
    """not enough room in ids / values: that entry and all later ones of the call are stored empty, overflow counts
    them, the check call reports it; a query afterwards never lists them"""
    K = 128
    voc = R.shipped_vocabulary(oracle)
    scene = S.rig_scene(oracle, voc, 2, K)
    M = len(scene["feats"])
    fe, dev = _frontend(K), S.Dev(torch)
    refs = S.reference_vectors(oracle, voc, scene)
    vec, stride = _vectors(fe, dev, voc, scene, word_ids=False)
    sizes = [len(r[1]) for r in refs]
    fit = 3  # multiframes 0..2 fit exactly, 3 does not; 4 (empty) and the rest follow it
    db = R.Database(len(voc["ww"]))
    dbd = dev.database(db, cap_entries=M, cap_words=sum(sizes[:fit]) + sizes[fit] - 1)
    fe.bow_database_add_blocks_device(dbd, vec, M, list(range(M)))
    assert dbd.n_entries == M
    with pytest.raises(capi.OkvfeError) as e:
        fe.bow_database_check_device(dbd)
    assert e.value.status == capi.ERR_CAPACITY and str(M - fit) in str(e.value)
    assert dev.get("db_overflow", np.int32, 1)[0] == M - fit
    for m in range(M):
        db.add(*(refs[m][1:] if m < fit else (np.zeros(0, np.int32), np.zeros(0))))
    begin, ids, vals = db.arrays()
    assert np.array_equal(dev.get("db_begin", np.int32, M + 1), begin)
    assert np.array_equal(dev.get("db_ids", np.int32, len(ids)), ids)
    assert np.all(dev.get("db_ids", np.int32, dbd.cap_words)[len(ids):] == S.FILL_I32)
    _, walks = _query(fe, dev, oracle, dbd, db, vec, refs, None, 0.05, M, True, "after the overflow")
    assert 1 <= max(w[0] for w in walks) <= fit  # the entries stored empty are never listed


def test_equal_to_the_b1_chain(oracle):
    """okvfe_fbrisk_transform -> okvfe_bow_vector -> okvfe_bow_query_l1 on one multiframe of the shipped vocabulary"""
    K = 700
    voc = R.shipped_vocabulary(oracle)
    scene = S.rig_scene(oracle, voc, 2, K)
    fe, dev = _frontend(K), S.Dev(torch)
    vec, stride = _vectors(fe, dev, voc, scene)
    db = S.host_database(oracle, voc, scene, 40)
    dbd = dev.database(db)
    M = len(scene["feats"])
    sptr, _, cand = _prepare_query(dev, M, 40, 4, True, None)
    fe.place_query_blocks_device(dbd, vec, M, cand, scores_ptr=sptr)
    m = 9
    feats = np.concatenate(scene["feats"][m])
    words, _ = fe.fbrisk_transform(feats, voc["desc"], voc["cb"], voc["ci"], voc["word"])
    ids, vals = capi.bow_vector(words, voc["ww"], voc["weighting"], voc["normalise_l1"])
    begin, dids, dvals = db.arrays()
    scores = fe.bow_query_l1(begin, dids, dvals, ids, vals)
    n = dev.get("q_n", np.int32, M)[m]
    assert n == len(ids) and n > 60
    assert np.array_equal(dev.get("q_ids", np.int32, M, stride)[m, :n], ids)
    assert np.array_equal(dev.get("q_vals", np.uint64, M, stride)[m, :n], vals.view(np.uint64))
    assert np.array_equal(dev.get("word_ids", np.int32, M, 2 * K)[m].reshape(2, K)[0, :len(scene["feats"][m][0])],
                          words[:len(scene["feats"][m][0])])
    assert np.array_equal(dev.get("scores", np.uint64, M, 40)[m], scores.view(np.uint64))


def test_the_largest_feature_count(oracle):
    """four cameras of 2048 keypoints, BOW_MAX_FEATURES keys: the 8192-key sort and its 32 run-length rounds (8192, 8191,
    4097 features; 4096 next to them), the descent of the SMALL tree out of LDS (8192 keys leave no room for its nodes),
    a run of 5000 keys (rounds without a run head; one weight added 5000 times) alone and behind smaller words, and runs
    that start and end on round boundaries; under the summing weightings with and without normalise_l1.  Then one query
    of these vectors against 40 entries.  The scene's premises: test_capacity_scenes_host.py."""
    base = R.shipped_vocabulary(oracle)
    scene = S.capacity_scene(oracle, base)
    n_cams, K, M = scene["n_cams"], scene["K"], len(scene["feats"])
    assert n_cams * K == capi.BOW_MAX_FEATURES and [sum(c) for c in scene["counts"]][:4] == list(S.CAPACITY_COUNTS)
    n_nodes = len(base["word"])
    assert n_nodes <= S.LDS_NODES and n_nodes * 48 + n_cams * K * 4 > S.LDS_BUDGET  # the nodes do not fit beside the keys
    assert not S.nodes_in_lds(n_nodes, n_cams * K)
    fe, dev = _frontend(K), S.Dev(torch)
    seen = set()
    for weighting in (0, 1):
        for norm in (True, False):
            voc = dict(base, weighting=weighting, normalise_l1=norm)
            refs = S.reference_vectors(oracle, voc, scene)
            vec, stride = _vectors(fe, dev, voc, scene)
            S.check_vectors(dev, refs, stride, ("capacity", weighting, norm))
            _check_word_ids(dev, scene, refs)
            assert refs[4][1].tolist() == [scene["long_word"]] and len(refs[5][1]) == 41
            seen.add(refs[4][2].tobytes())
    assert len(seen) == 2  # 1.0 normalised, 5000 additions of the weight otherwise
    refs = S.reference_vectors(oracle, base, scene)
    vec, stride = _vectors(fe, dev, base, scene)
    S.check_vectors(dev, refs, stride, "capacity")
    db = S.host_database(oracle, base, scene, 40)
    dbd = dev.database(db)
    scores, walks = _query(fe, dev, oracle, dbd, db, vec, refs, None, 0.02, 40, True, "capacity")
    print("capacity: words", [len(r[1]) for r in refs], "listed", [w[0] for w in walks], "candidates", [len(w[1]) for w in walks])
    assert max(w[0] for w in walks) >= 30


def test_refusals(oracle):
    """errors before anything is launched: a stride that could truncate, more features than the sort holds, NULLs"""
    K = 700
    voc = R.shipped_vocabulary(oracle)
    fe, dev = _frontend(K), S.Dev(torch)
    vd = dev.vocabulary(voc)
    blocks = dev.out("blocks", 64)
    vec = dev.vectors(1, 700, len(voc["ww"]))
    with pytest.raises(capi.OkvfeError) as e:
        fe.bow_vectors_blocks_device(vd, blocks, 1, 2, vec)  # min(1400, 729) = 729 > 700
    assert e.value.status == capi.ERR_INVALID_ARGUMENT and "stride" in str(e.value)
    with pytest.raises(capi.OkvfeError) as e:
        fe.bow_vectors_blocks_device(vd, blocks, 1, 12, dev.vectors(1, 729, 729))  # 8400 features
    assert e.value.status == capi.ERR_UNSUPPORTED and str(capi.BOW_MAX_FEATURES) in str(e.value)
    for args in ((None, blocks, 1, 1, vec), (vd, None, 1, 1, vec), (vd, blocks, -1, 1, vec), (vd, blocks, 1, 0, vec),
                 (vd, blocks, 1, 1, None)):
        with pytest.raises(capi.OkvfeError) as e:
            fe.bow_vectors_blocks_device(*args)
        assert e.value.status == capi.ERR_INVALID_ARGUMENT
    fe.bow_vectors_blocks_device(vd, blocks, 0, 1, vec)  # nothing to do is no error
    assert dev.get("q_n", np.int32, 1)[0] == S.FILL_I32
    db = dev.database(R.Database(729))
    with pytest.raises(capi.OkvfeError) as e:
        fe.place_query_blocks_device(db, vec, 1, None)
    assert e.value.status == capi.ERR_INVALID_ARGUMENT
    with pytest.raises(capi.OkvfeError) as e:
        fe.place_query_blocks_device(db, vec, 1, capi.PlaceCandidatesDevice(None, None, None, None, 4))
    assert e.value.status == capi.ERR_INVALID_ARGUMENT
