"""Reference of place recognition on batches (okvfe_bow_vectors_blocks_device, okvfe_place_query_blocks_device,
okvfe_bow_database_add_blocks_device): per multiframe the oracle's chain on the concatenated features
(orc_voc_transform -> orc_bow_vector -> orc_bow_query_l1), a literal transcription of the walk over the sorted results
(okvis_frontend/src/Frontend.cpp:761-802: a Python list of results, the four `if`s as written), `add` as list appends,
and the scenes the walk is tested on.  DBoW2 is not in the reference tree: the arithmetic is the oracle's restatement of
DBoW2's published loops (parity unpinned)."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MIN_SCORE = 0.4  # Frontend.cpp:802


# ---- vocabularies -----------------------------------------------------------------------------------------------------
def shipped_vocabulary(oracle, weighting=None, normalise_l1=True, weights=None):
    """the reference's 9^3 vocabulary (tests/golden/small_voc_tree.npz) as arrays"""
    t = np.load(os.path.join(GOLD, "small_voc_tree.npz"))
    word, weight = t["word"], t["weight"]
    n_words = int(word.max()) + 1
    ww = np.zeros(n_words)
    ww[word[word >= 0]] = weight[word >= 0]
    cb, ci = oracle.voc_tree_arrays(t["parent"])
    return dict(desc=np.ascontiguousarray(t["desc"], dtype=np.uint8), cb=cb, ci=ci,
                word=np.ascontiguousarray(word, dtype=np.int32), ww=ww if weights is None else np.asarray(weights, np.float64),
                weighting=int(t["weighting"]) if weighting is None else int(weighting), normalise_l1=bool(normalise_l1))


def synthetic_vocabulary(oracle, seed=5, branching=30, weighting=0, normalise_l1=True):
    """30 children per node and three levels (27 000 words) with random node descriptors (a child's is its parent's
    with bits flipped), plus what a k-means tree can contain: a leaf at depth 1 (the root's child 30), a node with a single child (the root's child 31, whose only child
    has 30 leaves), and exact distance ties between siblings (the first two children of every tenth node carry the same
    descriptor: the first wins).  Nodes are numbered level by level, parents first; words in node order."""
    rng = np.random.default_rng(seed)
    parent = [-1]
    level = [0]
    for depth in range(3):
        nxt = []
        for p in level:
            for _ in range(branching):
                parent.append(p)
                nxt.append(len(parent) - 1)
        if depth == 0:
            parent.append(0)                # a leaf at depth 1
            parent.append(0)                # a node with a single child ...
            single = len(parent) - 1
        if depth == 1:
            parent.append(single)
            nxt.append(len(parent) - 1)     # ... whose children are leaves at depth 3
        level = nxt
    parent = np.array(parent, dtype=np.int64)
    n = len(parent)
    # a child's descriptor is its parent's with a share of the bits flipped, fewer the deeper: as in a k-means tree a
    # descriptor near a node is nearest to that node's ancestors on the way down
    depth = np.zeros(n, dtype=np.int64)
    for i in range(1, n):
        depth[i] = depth[parent[i]] + 1
    share = np.array([0.0, 0.15, 0.08, 0.04])[depth]
    flips = np.packbits(rng.random((n, 384)) < share[:, None], axis=1)
    desc = np.zeros((n, 48), dtype=np.uint8)
    desc[0] = rng.integers(0, 256, 48, dtype=np.uint8)
    for i in range(1, n):
        desc[i] = desc[parent[i]] ^ flips[i]
    cb, ci = oracle.voc_tree_arrays(parent)
    for i in range(0, n, 10):
        if cb[i + 1] - cb[i] >= 2:
            desc[ci[cb[i] + 1]] = desc[ci[cb[i]]]
            if cb[ci[cb[i]] + 1] > cb[ci[cb[i]]]:  # inner twins: the second one's subtree follows its new descriptor
                stack = list(ci[cb[ci[cb[i] + 1]]:cb[ci[cb[i] + 1] + 1]])
                while stack:
                    c = int(stack.pop())
                    desc[c] = desc[parent[c]] ^ flips[c]
                    stack.extend(ci[cb[c]:cb[c + 1]])
    leaf = (cb[1:] - cb[:-1]) == 0
    word = np.full(n, -1, dtype=np.int32)
    word[leaf] = np.arange(int(leaf.sum()), dtype=np.int32)
    ww = 0.5 + rng.random(int(leaf.sum())) * 4.0
    return dict(desc=desc, cb=cb, ci=ci, word=word, ww=ww, weighting=int(weighting), normalise_l1=bool(normalise_l1))


def leaf_views(voc, rng, n, flip=0.01):
    """n features: descriptors of random leaves with a few bits flipped, as the query test of the B = 1 path builds them"""
    leaves = np.flatnonzero(voc["word"] >= 0)
    d = voc["desc"][rng.choice(leaves, n)]
    flips = ((rng.random(d.shape) < flip) * rng.integers(1, 256, d.shape)).astype(np.uint8)
    return d ^ flips


# ---- the oracle's chain -----------------------------------------------------------------------------------------------
def bow_vector(oracle, voc, feats):
    """(word of every feature, ascending word ids, values) of one multiframe's concatenated features"""
    feats = np.ascontiguousarray(feats, dtype=np.uint8).reshape(-1, 48)
    if len(feats) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0)
    words, _ = oracle.voc_transform(feats, voc["desc"], voc["cb"], voc["ci"], voc["word"])
    ids, vals = oracle.bow_vector(words, voc["ww"], voc["weighting"], voc["normalise_l1"])
    return words, ids, vals


class Database:
    """database.add as list appends (Frontend.cpp:896-898); entry ids are positions"""

    def __init__(self, n_words):
        self.entries, self.n_words = [], int(n_words)

    def add(self, ids, vals):
        self.entries.append((np.asarray(ids, np.int32).copy(), np.asarray(vals, np.float64).copy()))

    def arrays(self):
        begin = np.concatenate([[0], np.cumsum([len(e[0]) for e in self.entries])]).astype(np.int32)
        ids = np.concatenate([e[0] for e in self.entries] + [np.zeros(0, np.int32)]).astype(np.int32)
        vals = np.concatenate([e[1] for e in self.entries] + [np.zeros(0)]).astype(np.float64)
        return begin, ids, vals

    def scores(self, oracle, q_ids, q_vals):
        if not self.entries:
            return np.zeros(0)
        begin, ids, vals = self.arrays()
        return oracle.bow_query_l1(begin, ids, vals, q_ids, q_vals, self.n_words)


# ---- the walk ---------------------------------------------------------------------------------------------------------
def walk(scores, suppressible=None, min_score=MIN_SCORE):
    """Frontend.cpp:761-802 on the scores of all entries (-1 = not listed).  suppressible[id] stands for
    estimator.isPlaceRecognitionFrame(StateId(poseId)); None is the component walk of :700-719, which has no predicate.
    -> (number of listed entries, [(id, score)] of the candidates: the positions that reach the body of `if(p > 0.4)`)"""
    dBoWResult = [(e, float(s)) for e, s in enumerate(scores) if s != -1.0]
    dBoWResult.sort(key=lambda r: r[0])  # :761-765
    out = []
    for f in range(len(dBoWResult)):
        id_, p = dBoWResult[f]
        isPlaceRecognitionFrame = True if suppressible is None else bool(suppressible[id_])
        # nonmax suppression
        if f > 0:
            if dBoWResult[f - 1][1] > p and isPlaceRecognitionFrame:
                continue
            if f > 1:
                if dBoWResult[f - 2][1] > p and isPlaceRecognitionFrame:
                    continue
        if f + 1 < len(dBoWResult):
            if dBoWResult[f + 1][1] > p and isPlaceRecognitionFrame:
                continue
            if f + 2 < len(dBoWResult):
                if dBoWResult[f + 2][1] > p and isPlaceRecognitionFrame:
                    continue
        if p > min_score:
            out.append((id_, p))
    return len(dBoWResult), out


def walk_brute_force(scores, suppressible=None, min_score=MIN_SCORE):
    """the same answer from a window maximum over the listed neighbours"""
    scores = np.asarray(scores, dtype=np.float64)
    ids = np.flatnonzero(scores != -1.0)
    s = scores[ids]
    out = []
    for f in range(len(ids)):
        window = np.concatenate([s[max(f - 2, 0):f], s[f + 1:f + 3]])
        larger = bool(len(window)) and bool(np.max(window) > s[f])
        sup = True if suppressible is None else bool(suppressible[ids[f]])
        if not (sup and larger) and s[f] > min_score:
            out.append((int(ids[f]), float(s[f])))
    return len(ids), out


CENSUS_KEYS = ("by_f-1", "by_f-2", "by_f+1", "by_f+2", "equal_neighbour_kept", "first_kept", "last_kept", "few_listed",
               "unsuppressible_survivor", "exactly_min_score", "unlisted_between")


def census(scores, suppressible, min_score, counts):
    """adds the situations of one walk to counts (a dict over CENSUS_KEYS)"""
    scores = np.asarray(scores, dtype=np.float64)
    ids = np.flatnonzero(scores != -1.0)
    s = scores[ids]
    n = len(ids)
    if 0 < n < 3:
        counts["few_listed"] += 1
    if n >= 2:
        counts["unlisted_between"] += int(np.sum(scores[ids[0]:ids[-1]] == -1.0))
    cands = dict(walk(scores, suppressible, min_score)[1])
    for f in range(n):
        sup = True if suppressible is None else bool(suppressible[ids[f]])
        nb = {d: s[f + d] for d in (-1, -2, 1, 2) if 0 <= f + d < n}
        larger = [d for d in (-1, -2, 1, 2) if d in nb and nb[d] > s[f]]
        if sup and larger:
            counts["by_f%+d" % larger[0]] += 1  # the first test of :780-799 that fires
        kept = int(ids[f]) in cands
        if kept and not larger and any(v == s[f] for v in nb.values()):
            counts["equal_neighbour_kept"] += 1
        if kept and f == 0 and n > 1:
            counts["first_kept"] += 1
        if kept and f == n - 1 and n > 1:
            counts["last_kept"] += 1
        if kept and not sup and larger:
            counts["unsuppressible_survivor"] += 1
        if s[f] == min_score and not (sup and larger):
            assert not kept
            counts["exactly_min_score"] += 1


WALK_MIN_SCORE = 0.375  # a dyadic threshold, so that hand-built scores k / 16 meet it exactly
WALK_ENTRIES = (0, 1, 2, 3, 5, 12, 40, 255, 256, 257, 600)
WALK_QUERIES = 16


def walk_scenes():
    """One scene per database size: WALK_QUERIES score rows of k / 16 (k = 1..15; -1 = not listed) and one suppressible
    array (None for every third scene).  Scores of k / 16 can be produced exactly on the device: query m holds the one
    word m with value 1, entry e holds word m with value d, and |1 - d| - 1 - d = -2 d without rounding."""
    rng = np.random.default_rng(2024)
    scenes = []
    for i, E in enumerate(WALK_ENTRIES):
        listed = rng.random((WALK_QUERIES, E)) < np.linspace(0.15, 1.0, WALK_QUERIES)[:, None]
        # few levels: neighbours tie often; the threshold 6 / 16 is one of them
        k = rng.choice([2, 5, 6, 6, 7, 7, 8, 9, 12, 15], (WALK_QUERIES, E))
        scores = np.where(listed, k / 16.0, -1.0)
        if E >= 3:
            scores[0, :] = -1.0       # a query that lists nothing ...
            scores[1, :] = -1.0
            scores[1, E // 2] = 0.5   # ... one entry ...
            scores[2, :] = -1.0
            scores[2, [0, E - 1]] = [0.5, 0.75]  # ... and two, the ends of the database
        suppressible = None if i % 3 == 2 else (rng.random(E) < 0.7).astype(np.uint8)
        scenes.append(dict(E=E, scores=scores, suppressible=suppressible, min_score=WALK_MIN_SCORE))
    return scenes
