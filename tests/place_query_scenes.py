"""Scenes of the place-recognition tests (test_place_query_host.py, test_gpu_place_query.py, test_gpu_place_query_cpp.py)
and the device plumbing the GPU tests share: multiframes whose descriptors are vocabulary leaves with a few bits flipped,
packed straight into gather blocks (no detection), databases built by the reference chain, sentinel-filled outputs."""
import numpy as np

import place_query_ref as R
from okvis2_amd import capi, multigpu

SENTINEL = 0xF9
FILL_I32 = int(np.frombuffer(bytes([SENTINEL]) * 4, dtype=np.int32)[0])
FILL_U64 = int(np.frombuffer(bytes([SENTINEL]) * 8, dtype=np.uint64)[0])


# ---- features ---------------------------------------------------------------------------------------------------------
def place_leaves(voc, rng, n_places, per_place):
    leaves = np.flatnonzero(voc["word"] >= 0)
    return [rng.choice(leaves, min(per_place, len(leaves)), replace=False) for _ in range(n_places)]


def view(voc, rng, leaves, n, flip=0.004):
    """n features seen at a place: its leaves' descriptors, drawn with repetition, a few bits flipped"""
    d = voc["desc"][rng.choice(leaves, n)] if n else np.zeros((0, 48), np.uint8)
    flips = ((rng.random(d.shape) < flip) * rng.integers(1, 256, d.shape)).astype(np.uint8)
    return d ^ flips


def rig_scene(oracle, voc, n_cams, K, seed=3, n_places=4, per_place=90):
    """12 multiframes of n_cams cameras over n_places places.  Counts: full blocks, random ones, blocks of 0 and 1
    keypoints, and a multiframe without any feature.  Words are hit often (K features over 90 leaves)."""
    rng = np.random.default_rng(seed)
    places = place_leaves(voc, rng, n_places, per_place)
    counts = []
    for m in range(12):
        if m < 4:
            c = [K] * n_cams
        elif m == 4:
            c = [0] * n_cams                       # no feature at all
        elif m == 5:
            c = [1] + [0] * (n_cams - 1)           # one feature
        elif m == 6:
            c = [0] * (n_cams - 1) + [K]           # only the last camera sees something
        elif m == 7:
            c = [1] * n_cams
        else:
            c = [int(v) for v in rng.integers(K // 3, K + 1, n_cams)]
        counts.append(c)
    feats = [[view(voc, rng, places[m % n_places], n) for n in c] for m, c in enumerate(counts)]
    return dict(feats=feats, counts=counts, n_cams=n_cams, K=K, places=places, place_of=[m % n_places for m in range(12)])


# ---- capacity: BOW_MAX_FEATURES keys, long runs, runs on round boundaries -------------------------------------------------
CAPACITY_CAMS, CAPACITY_K = 4, 2048          # n_cams K = capi.BOW_MAX_FEATURES
CAPACITY_COUNTS = (8192, 8191, 4097, 4096)   # multiframes 0 .. 3: the 8192-key sort, one key of padding, 4096 + 1, 4096
LONG_RUN = 5000                              # multiframes 4 and 5: copies of one leaf's descriptor
BOUNDARY_COUNTS = (256, 300, 212) + (300,) * 14 + (152, 300, 300)   # multiframe 6: copies per leaf, in word order
ROUND = 256                                  # sorted keys the run-length pass of bow_vectors_kernel takes per round
LDS_BUDGET, LDS_NODES = 61 * 1024, 1024      # kBowLdsBudget, kVocLdsNodes


def nodes_in_lds(n_nodes, n_features):
    """bow_vectors_lds_bytes restated: the node descriptors are staged in LDS iff they fit beside the sort keys"""
    keys_cap = 256
    while keys_cap < n_features:
        keys_cap *= 2
    return n_nodes <= LDS_NODES and n_nodes * 48 + keys_cap * 4 <= LDS_BUDGET


def _deal(feats, n_cams, K):
    """features in order onto the cameras, K per camera while they last"""
    assert len(feats) <= n_cams * K
    return [feats[c * K:(c + 1) * K] for c in range(n_cams)]


def capacity_scene(oracle, voc, seed=13):
    """seven multiframes of CAPACITY_CAMS cameras with K = CAPACITY_K: the CAPACITY_COUNTS; LONG_RUN copies of one
    leaf; the same among 40 features of leaves with smaller and larger words; BOUNDARY_COUNTS copies of 20 leaves, shuffled.
    The copied leaves are leaves whose own descriptor descends to them."""
    rng = np.random.default_rng(seed)
    n_cams, K = CAPACITY_CAMS, CAPACITY_K
    leaves = np.flatnonzero(voc["word"] >= 0)
    words, _ = oracle.voc_transform(voc["desc"][leaves], voc["desc"], voc["cb"], voc["ci"], voc["word"])
    own = leaves[(words == voc["word"][leaves]) & (voc["ww"][voc["word"][leaves]] > 0)]
    own = own[np.argsort(voc["word"][own])]
    assert len(own) >= 60
    feats = [_deal(view(voc, rng, leaves, n), n_cams, K) for n in CAPACITY_COUNTS]
    middle = own[len(own) // 2]
    feats.append(_deal(np.repeat(voc["desc"][[middle]], LONG_RUN, axis=0), n_cams, K))
    around = np.concatenate([own[3:23], own[-23:-3]])
    mixed = np.concatenate([np.repeat(voc["desc"][[middle]], LONG_RUN, axis=0), voc["desc"][around]])
    feats.append(_deal(mixed[rng.permutation(len(mixed))], n_cams, K))
    twenty = own[np.linspace(0, len(own) - 1, len(BOUNDARY_COUNTS)).astype(int)]
    runs = np.repeat(voc["desc"][twenty], BOUNDARY_COUNTS, axis=0)
    feats.append(_deal(runs[rng.permutation(len(runs))], n_cams, K))
    places = place_leaves(voc, rng, 4, 90)
    return dict(feats=feats, counts=[[len(c) for c in cams] for cams in feats], n_cams=n_cams, K=K, places=places,
                long_word=int(voc["word"][middle]), boundary_words=voc["word"][twenty].astype(np.int32))


def reference_vectors(oracle, voc, scene):
    """per multiframe (words per camera, ids, values) of the concatenated features"""
    out = []
    for cams in scene["feats"]:
        words, ids, vals = R.bow_vector(oracle, voc, np.concatenate(cams))
        split = np.cumsum([len(c) for c in cams])[:-1]
        out.append((np.split(words, split), ids, vals))
    return out


def host_database(oracle, voc, scene, E, seed=8, per_entry=60):
    """E entries by the reference chain: views of the scene's places, an empty entry in the middle and a hand-built
    entry of one word (the last of the vocabulary, weight 1) that most queries do not contain"""
    rng = np.random.default_rng(seed + E)
    db = R.Database(len(voc["ww"]))
    for e in range(E):
        if E >= 3 and e == E // 2:
            db.add(np.zeros(0, np.int32), np.zeros(0))
        elif E >= 3 and e == E // 2 + 1:
            db.add(np.array([len(voc["ww"]) - 1], np.int32), np.array([1.0]))
        else:
            place = scene["places"][int(rng.integers(len(scene["places"])))]
            _, ids, vals = R.bow_vector(oracle, voc, view(voc, rng, place, int(rng.integers(per_entry // 2, per_entry + 1)), 0.01))
            db.add(ids, vals)
    return db


# ---- device plumbing ----------------------------------------------------------------------------------------------------
def pack_blocks(scene):
    """gather blocks m n_cams + c of the scene, host-packed; rows past a block's count hold random descriptors"""
    K = scene["K"]
    rng = np.random.default_rng(77)
    blocks = []
    for cams in scene["feats"]:
        for d in cams:
            n = len(d)
            b = multigpu.pack_block_host(K, np.zeros(n, capi.KEYPOINT_DTYPE), d, np.zeros((n, 3)), np.zeros(n, np.uint8))
            L = multigpu.block_layout(K)
            b[L["desc"] + n * 48:L["desc"] + K * 48] = rng.integers(0, 256, (K - n) * 48, dtype=np.uint8)
            blocks.append(b)
    return np.stack(blocks)


class Dev:
    """device arrays of one test, sentinel-filled; torch tensors keep them alive"""

    def __init__(self, torch):
        self.torch, self.t = torch, {}

    def put(self, name, a):
        a = np.ascontiguousarray(a)
        t = self.torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() if a.size else \
            self.torch.zeros(16, dtype=self.torch.uint8, device="cuda")
        self.t[name] = t
        return t.data_ptr()

    def out(self, name, nbytes):
        self.t[name] = self.torch.full((max(int(nbytes), 16),), SENTINEL, dtype=self.torch.uint8, device="cuda")
        return self.t[name].data_ptr()

    def ptr(self, name):
        return self.t[name].data_ptr()

    def get(self, name, dtype, *shape):
        self.torch.cuda.synchronize()  # every stream of the device
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return self.t[name][:n].cpu().numpy().view(dtype).reshape(*shape).copy()

    def vocabulary(self, voc):
        return capi.VocabularyDevice(
            len(voc["word"]), len(voc["ww"]), voc["weighting"], int(voc["normalise_l1"]), self.put("v_desc", voc["desc"]),
            self.put("v_cb", voc["cb"]), self.put("v_ci", voc["ci"]), self.put("v_word", voc["word"]),
            self.put("v_ww", np.asarray(voc["ww"], np.float64)))

    def vectors(self, M, stride, n_vocabulary_words, name="q"):
        return capi.BowVectorsDevice(self.out(name + "_n", M * 4), self.out(name + "_ids", M * stride * 4),
                                     self.out(name + "_vals", M * stride * 8), int(stride), int(n_vocabulary_words))

    def vectors_from_host(self, vecs, stride, n_vocabulary_words, name="q"):
        """hand-built vectors [(ids, vals)] uploaded as rows"""
        M = len(vecs)
        n = np.array([len(v[0]) for v in vecs], np.int32)
        ids = np.full((M, stride), FILL_I32, np.int32)
        vals = np.full((M, stride), FILL_U64, np.uint64).view(np.float64)
        for m, (i, v) in enumerate(vecs):
            ids[m, :len(i)] = i
            vals[m, :len(v)] = v
        return capi.BowVectorsDevice(self.put(name + "_n", n), self.put(name + "_ids", ids), self.put(name + "_vals", vals),
                                     int(stride), int(n_vocabulary_words))

    def database(self, db, cap_entries=None, cap_words=None, name="db"):
        """a host-built database (place_query_ref.Database, possibly empty) uploaded as it is, with room to grow"""
        begin, ids, vals = db.arrays()
        E = len(db.entries)
        cap_entries = E if cap_entries is None else cap_entries
        cap_words = len(ids) if cap_words is None else cap_words
        b = np.full(cap_entries + 1, FILL_I32, np.int32)
        b[:E + 1] = begin
        i = np.full(max(cap_words, 1), FILL_I32, np.int32)
        i[:len(ids)] = ids
        v = np.full(max(cap_words, 1), FILL_U64, np.uint64).view(np.float64)
        v[:len(vals)] = vals
        return capi.BowDatabaseDevice(self.put(name + "_begin", b), self.put(name + "_ids", i), self.put(name + "_vals", v),
                                      int(cap_entries), int(cap_words), E, self.put(name + "_overflow", np.zeros(1, np.int32)))

    def candidates(self, M, cap, name="c"):
        return capi.PlaceCandidatesDevice(self.out(name + "_listed", M * 4), self.out(name + "_count", M * 4),
                                          self.out(name + "_entry", M * cap * 4), self.out(name + "_score", M * cap * 8),
                                          int(cap))


def check_vectors(dev, refs, stride, what, name="q"):
    """n, ids and values of every multiframe against the reference, values as bit patterns; rows past n untouched"""
    M = len(refs)
    n = dev.get(name + "_n", np.int32, M)
    ids = dev.get(name + "_ids", np.int32, M, stride)
    vals = dev.get(name + "_vals", np.uint64, M, stride)
    for m, (_, rid, rval) in enumerate(refs):
        assert n[m] == len(rid), (what, m, n[m], len(rid))
        assert np.array_equal(ids[m, :n[m]], rid), (what, m)
        assert np.array_equal(vals[m, :n[m]], rval.view(np.uint64)), (what, m)
        assert np.all(ids[m, n[m]:] == FILL_I32) and np.all(vals[m, n[m]:] == FILL_U64), (what, m)


def check_candidates(dev, M, cap, ref_walks, what, name="c"):
    """n_listed, the true n_candidates, the first cap candidates and sentinels behind them"""
    listed = dev.get(name + "_listed", np.int32, M)
    count = dev.get(name + "_count", np.int32, M)
    entry = dev.get(name + "_entry", np.int32, M, cap) if cap else np.zeros((M, 0), np.int32)
    score = dev.get(name + "_score", np.uint64, M, cap) if cap else np.zeros((M, 0), np.uint64)
    for m, (n_listed, cands) in enumerate(ref_walks):
        assert listed[m] == n_listed, (what, m, listed[m], n_listed)
        assert count[m] == len(cands), (what, m, count[m], len(cands))
        k = min(len(cands), cap)
        assert entry[m, :k].tolist() == [c[0] for c in cands[:k]], (what, m)
        assert np.array_equal(score[m, :k], np.array([c[1] for c in cands[:k]], np.float64).view(np.uint64)), (what, m)
        assert np.all(entry[m, k:] == FILL_I32) and np.all(score[m, k:] == FILL_U64), (what, m)
