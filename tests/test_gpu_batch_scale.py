"""GPU: the device-batch entry points behind matchStereo at the benchmark's batch -- N = 3077 multiframes (16 distinct
ones x 192 + 5: more work-groups than the device holds at once, a ragged last round, no power-of-two factor), every
chain queued on one side stream with nothing waited for in between, under the context's default order of the FP64 sums.

Per chain and on every output of every link: the anchors (multiframes 0 .. 15) equal the family's restatement through the
family's own `check`; every other multiframe equals its anchor byte for byte (batch_scale.first_difference, on the
device); a shuffled placement gives the shuffled results; a second run over the same buffers and the same context
workspace gives the same bytes; the records behind the batch and the family's no-write rows keep their sentinels; and a
floor on what the 16 distinct multiframes produce, taken from the restatement, keeps all of this from being vacuous.

Chains: place (verify_place -> claims -> consensus -> Hessian; EuRoC pair, Hilti rig, RADTAN8, and 3072 x 2 x 700);
map (table first pass -> 3d2d consensus -> removeOutliers -> second pass; whole and in three slices) and the pooled map
route; the 3d2d consensus on the Hilti rig and RADTAN8; motion (motion-stereo matcher with claims -> 2d2d consensus, two
steps of the sweep), the 2d2d consensus alone on three rigs and stereo insert on four; query (bow vectors -> place
query -> database add, every entry checked); keyframe coverage and overlap pairs.  Where a family's scene has fewer
distinct multiframes than 16 (2, 3, 8, 10, 12), N stays 3077.

Growth and shrink: batches of 3, 3077 and 3 queued back to back on one stream; a 5-camera call on a second stream that
makes the context's parameter ring grow while a batch of 3077 is queued on the first; a ninth stream that evicts the
oldest per-stream workspace.  okvfe_test_context_sizes shows that the ring and the workspaces did change."""
import dataclasses
import time

import numpy as np
import pytest

import batch_scale as BS
import gpu_common as G
import map_scenes
import map_table_common as M
import map_table_uninit_common as U
import place_hessian_ref as PH
import place_hessian_scenes as HS
import place_ref as P
import place_scenes as PS
import ransac_scenes as S
from okvis2_amd import synth

pytestmark = [pytest.mark.gpu]
torch = pytest.importorskip("torch")

TREE = True     # the context default: Eigen's x0 + (x1 + x2)
EUROC = ("euroc", "euroc1")
_FRONTENDS = {}


def _frontend(cams, K, fresh=False):
    """a context of the first camera's size with K keypoints and the cameras in its slots"""
    key = tuple((c.w, c.h, c.fu, c.fv, c.cu, c.cv, c.dist_type, tuple(c.d)) for c in cams) + (K,)
    if fresh or key not in _FRONTENDS:
        cfg = dataclasses.replace(synth.euroc_config(), w=cams[0].w, h=cams[0].h, cams=list(cams), max_kpts=K)
        fe = G.make_frontend(cfg)
        for i, c in enumerate(cams):
            fe.set_camera(i, c)
        if fresh:
            return fe
        _FRONTENDS[key] = fe
    return _FRONTENDS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_frontends():
    yield
    while _FRONTENDS:
        _FRONTENDS.popitem()[1].close()
    torch.cuda.empty_cache()


def _full(shape, v, dt):
    return torch.full(shape, v, dtype=dt, device="cuda")


class Timer:
    def __init__(self, what):
        self.what, self.t0 = what, time.perf_counter()

    def lap(self, name):
        torch.cuda.synchronize()
        t = time.perf_counter()
        print("[batch-scale] %s: %s %.1f ms" % (self.what, name, 1.0e3 * (t - self.t0)))
        self.t0 = t


def run_scaled(chain, n=BS.N, placement=True, what="", stream=None):
    """the properties of the module's docstring for one chain: an object with d, per_of, outputs, prepared (the tensors of
    the d distinct multiframes, not yet run), launch(T, n, stream, index) with index[i] the distinct multiframe at
    position i, and check_anchors(T_anchors)"""
    if chain.prepared is None:      # (the callers assert the floors of the restatements first, on the CPU)
        chain.prepare()
    tm = Timer(what)
    d, per_of = chain.d, chain.per_of
    modular, shuffled = BS.placements(n, d)
    stream = torch.cuda.Stream() if stream is None else stream
    T, guard = BS.tile_tensors(chain.prepared, modular, d, per_of)
    torch.cuda.synchronize()
    tm.lap("tiled")
    chain.launch(T, n, stream, modular % d)
    stream.synchronize()
    tm.lap("first run")
    chain.check_anchors(BS.anchors(T, d, per_of))                      # anchors, and the family's no-write rows
    tm.lap("anchors checked")
    for k in chain.outputs:                                            # replicas
        assert BS.first_difference(T[k], d, n, per_of[k]) is None, (what, k, BS.first_difference(T[k], d, n, per_of[k]))
    assert BS.untouched(T, guard) == [], (what, "records behind the batch")
    tm.lap("replicas compared")
    snap = BS.snapshot(T, chain.outputs)                               # second run
    chain.launch(T, n, stream, modular % d)
    stream.synchronize()
    assert BS.changed(T, snap) == [], (what, "second run")
    assert BS.untouched(T, guard) == [], (what, "records behind the batch, second run")
    del snap
    tm.lap("second run")
    if placement:
        TS, guard_s = BS.tile_tensors(chain.prepared, shuffled, d, per_of)
        torch.cuda.synchronize()
        chain.launch(TS, n, stream, shuffled % d)
        stream.synchronize()
        for k in chain.outputs:
            assert BS.first_misplaced(TS[k], T[k], shuffled, per_of[k]) is None, (what, k, "shuffled placement")
        assert BS.untouched(TS, guard_s) == [], (what, "records behind the shuffled batch")
        tm.lap("shuffled placement")
    return T


# ---- place: verify_place -> claims -> consensus -> hessian -----------------------------------------------------------
# (accepted verdicts among the 16, fewest terms of an accepted multiframe, fewest matches of a multiframe): what
# place_ref.verify and place_hessian_ref.evaluate give for seed 0 (checked on the CPU before the first GPU run)
PLACE_FLOORS = {EUROC: (5, 226, 176), "hilti": (9, 468, 529), ("radtan8",): (8, 54, 50)}


class PlaceChain:
    """descriptors -> okvfe_verify_place_blocks_device -> okvfe_place_claims_blocks_device ->
    okvfe_place_consensus_blocks_device -> okvfe_place_hessian_blocks_device with residual and Jacobian rows"""
    outputs = ("kmin", "dmin", "n_matches", "n_points", "n_corr_claims", "gate", "ml", "n_corr", "best", "n_inl",
               "accepted", "verdict", "hyp_inliers", "state", "distance", "lm_out", "Hm", "n_terms", "n_singular",
               "residual", "jacobian")

    def __init__(self, oracle, spec, d=BS.D, K=PS.K):
        """the scene of d distinct multiframes and its restatements (CPU)"""
        self.spec, self.d, self.K = spec, d, K
        assert PS.K == K, "build the scene with place_scenes.K set to the context's capacity"
        sc = self.sc = PS.general_scene(oracle, spec, TREE, n_mf=d)
        cams = sc["cams"]
        fus = [c.fu for c in cams]
        rng = np.random.default_rng(77)
        self.poses = np.stack([HS.refined(mf["T_WS"], rng) for mf in sc["mfs"]])
        self.prm = np.array([HS.pose7(T) for T in sc["T_SC"]])
        self.refs = [P.verify(TREE, sc["hp"], mf["frames"], mf["kmin"], mf["dmin"], PS.MATCH_THRESHOLD, fus, sc["T_SC"],
                              mf["H"], mf["valid"], sc["min_inliers"]) for mf in sc["mfs"]]
        self.href = [PH.evaluate(oracle, TREE, sc["hp"], mf["frames"], cl["match_landmark"], co["state"], cams, self.prm,
                                 self.poses[mi], co["verdict"] == 3)
                     for mi, (mf, (cl, co)) in enumerate(zip(sc["mfs"], self.refs))]
        C = len(cams)
        per_mf = ("H", "valid", "n_matches", "n_points", "n_corr_claims", "gate", "n_corr", "best", "n_inl", "accepted",
                  "verdict", "hyp_inliers", "poses", "Hm", "n_terms", "n_singular")
        per_block = ("blocks", "kmin", "dmin", "ml", "state", "distance", "lm_out", "residual", "jacobian")
        self.per_of = dict([(k, 1) for k in per_mf] + [(k, C) for k in per_block])
        assert set(self.outputs) <= set(self.per_of)
        self.fe = self.prepared = None

    def prepare(self, fe=None):
        """the device tensors of the d distinct multiframes in a context (default: the module's of this rig)"""
        sc, d, K = self.sc, self.d, self.K
        self.fe = fe if fe is not None else _frontend(sc["cams"], K)
        assert self.fe.max_keypoints == K
        T = PS.prepare(self.fe, sc)
        T["pool"], T["desc_begin"] = S._dev(sc["set"]["pool"]), S._dev(sc["set"]["desc_begin"])
        T["kmin"].fill_(-5), T["dmin"].fill_(12345)        # values no matcher writes
        nb = d * len(sc["cams"])
        T.update(poses=S._dev(self.poses), Hm=_full((d, 36), HS.H_SENTINEL, torch.float64),
                 n_terms=_full((d,), HS.COUNT_SENTINEL, torch.int32), n_singular=_full((d,), HS.COUNT_SENTINEL, torch.int32),
                 residual=_full((nb, K, 2), HS.ROW_SENTINEL, torch.float64),
                 jacobian=_full((nb, K, 12), HS.ROW_SENTINEL, torch.float64))
        torch.cuda.synchronize()
        self.prepared = T
        return self

    def floors(self):
        """(accepted verdicts, fewest terms of an accepted multiframe, fewest matches of a multiframe)"""
        accepted = [i for i, (_, co) in enumerate(self.refs) if co["verdict"] == 3]
        return (len(accepted), min([self.href[i]["n_terms"] for i in accepted], default=0),
                min(cl["n_matches"] for cl, _ in self.refs))

    def launch(self, T, n, stream, index=None):
        fe, sc = self.fe, self.sc
        many = dict(sc, mfs=[sc["mfs"][0]] + [None] * (n - 1))   # (place_scenes' launchers take the batch from the scene)
        md = fe.make_map_device(len(sc["set"]["ids"]), T["desc_begin"].data_ptr(), T["pool"].data_ptr())
        C = len(sc["cams"])
        fe.verify_place_blocks_device(T["blocks"].data_ptr(), n * C, md, T["kmin"].data_ptr(), T["dmin"].data_ptr(), stream)
        PS.launch_claims(fe, many, T, stream)
        PS.launch_consensus(fe, many, T, stream=stream)
        res = fe.make_place_hessian_device(T["Hm"].data_ptr(), T["n_terms"].data_ptr(), T["n_singular"].data_ptr(),
                                           T["residual"].data_ptr(), T["jacobian"].data_ptr())
        fe.place_hessian_blocks_device(T["set"], T["blocks"].data_ptr(), n, list(range(C)), self.prm, T["poses"].data_ptr(),
                                       T["ml"].data_ptr(), T["state"].data_ptr(), T["verdict"].data_ptr(), res, stream)

    def check_anchors(self, A, first=None):
        """the first `first` (default: all d) multiframes of A against the restatements, through the families' checks"""
        sc, what = self.sc, ("place", S.spec_id(self.spec))
        m = self.d if first is None else first
        C, L = len(sc["cams"]), len(sc["hp"])
        sub = dict(sc, mfs=sc["mfs"][:m])
        got = PS.download({k: v[:m * self.per_of[k]] for k, v in A.items()
                           if k in self.per_of and v is not None and k not in ("residual", "jacobian", "Hm")})
        assert np.array_equal(got["kmin"], np.concatenate([mf["kmin"] for mf in sub["mfs"]]).reshape(-1, L)), what
        assert np.array_equal(got["dmin"].view(np.uint32), np.concatenate([mf["dmin"] for mf in sub["mfs"]]).reshape(-1, L)), what
        PS.check_claims(sub, got, [r[0] for r in self.refs[:m]], what)
        PS.check_consensus(sub, got, [r[1] for r in self.refs[:m]], what)
        hess = dict(H=A["Hm"][:m], n_terms=A["n_terms"][:m], n_singular=A["n_singular"][:m],
                    residual=A["residual"][:m * C], jacobian=A["jacobian"][:m * C])
        HS.check(sub, hess, self.href[:m], what)


_CHAINS = {}


def _chain(key, make):
    """chains are built once per module run: the scene, its restatements and the prepared tensors"""
    if key not in _CHAINS:
        _CHAINS[key] = make()
    return _CHAINS[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_chains():
    yield
    _CHAINS.clear()
    torch.cuda.empty_cache()    # (the batches are gigabytes: hand them back before the next module)


def _place_floor_asserts(T, n, d, floors):
    accepted, terms, matches = floors
    verdict, n_terms, n_matches = T["verdict"][:n], T["n_terms"][:n], T["n_matches"][:n]
    assert int((verdict[:d] == 3).sum()) == accepted >= 1 and int((verdict == 3).sum()) >= accepted * (n // d)
    assert int(n_terms[verdict == 3].min()) >= terms >= 16 and int(n_matches.min()) >= matches
    assert int(n_terms[verdict != 3].max()) == 0


@pytest.mark.parametrize("spec", [EUROC, "hilti", ("radtan8",)], ids=S.spec_id)
def test_place_chain(oracle, spec):
    """verify_place -> claims -> consensus -> Hessian at N = 3077 on the EuRoC pair, the 5-camera Hilti rig and the
    RADTAN8 camera (K = place_scenes.K = 256, about 330 landmarks in the set)"""
    chain = _chain(("place", spec), lambda: PlaceChain(oracle, spec))
    assert chain.floors() == PLACE_FLOORS[spec], chain.floors()     # not vacuous: the restatement's own figures ...
    T = run_scaled(chain, what="place " + S.spec_id(spec))
    _place_floor_asserts(T, BS.N, BS.D, PLACE_FLOORS[spec])          # ... and the device's, over the whole batch


PLACE_700_FLOORS = (0, 0, 201)   # (no multiframe accepted, see the test; at least 201 matches and correspondences each)
HESSIAN_700_FLOORS = (12, 338)   # (multiframes of the 16 with terms, fewest terms among them)


def test_place_chain_at_the_benchmark_shape(oracle, monkeypatch):
    """2 cameras x 700 keypoints, N = 3072: the shape tools/bench_place_hessian.py reports.  The claims kernel takes up
    to 12288 keypoints per block, so the chain starts at the descriptors as the others do.  place_scenes.general_scene
    holds at most 400 landmarks, so blocks of 700 keypoints carry too many wrong claims for a consensus to accept them:
    the matcher, the claims and the consensus have their full load here, the Hessian has its terms in
    test_place_hessian_at_the_benchmark_shape."""
    monkeypatch.setattr(PS, "K", 700)
    chain = _chain(("place", EUROC, 700), lambda: PlaceChain(oracle, EUROC, K=700))
    assert chain.floors() == PLACE_700_FLOORS, chain.floors()
    T = run_scaled(chain, n=BS.N_BENCH, what="place 2 x 700")
    n_matches, n_corr = T["n_matches"][:BS.N_BENCH], T["n_corr"][:BS.N_BENCH]
    assert int(n_matches.min()) >= PLACE_700_FLOORS[2] >= 16 and int(n_corr.min()) >= 16
    assert int((T["gate"][:BS.N_BENCH] == 2).sum()) == BS.N_BENCH        # every multiframe went through the consensus


class HessianChain:
    """okvfe_place_hessian_blocks_device alone over place_hessian_scenes.general_scene (states as a consensus leaves
    them), residual and Jacobian rows on"""
    outputs = ("H", "n_terms", "n_singular", "residual", "jacobian")

    def __init__(self, oracle, spec, K, n_kps, d=BS.D):
        assert HS.K == K, "build the scene with place_hessian_scenes.K set to the context's capacity"
        self.d, self.K = d, K
        sc = self.sc = HS.general_scene(oracle, spec, n_mf=d, n_kps=n_kps)
        self.refs = HS.reference(oracle, TREE, sc)
        C = len(sc["cams"])
        self.per_of = dict(blocks=C, ml=C, state=C, poses=1, verdict=1, H=1, n_terms=1, n_singular=1, residual=C, jacobian=C)
        self.fe = self.prepared = None

    def prepare(self, fe=None):
        self.fe = fe if fe is not None else _frontend(self.sc["cams"], self.K)
        assert self.fe.max_keypoints == self.K
        self.prepared = HS.prepare(self.fe, self.sc)
        return self

    def floors(self):
        """(multiframes with terms, fewest terms among them)"""
        terms = [r["n_terms"] for r in self.refs if r["n_terms"] > 0]
        return len(terms), min(terms, default=0)

    def launch(self, T, n, stream, index=None):
        HS.launch(self.fe, dict(self.sc, mfs=[None] * n), T, stream=stream)

    def check_anchors(self, A, first=None):
        m = self.d if first is None else first
        HS.check(self.sc, {k: A[k][:m * self.per_of[k]] for k in self.outputs}, self.refs[:m], ("hessian", self.K))


def test_place_hessian_at_the_benchmark_shape(oracle, monkeypatch):
    """place_hessian_kernel at 3072 multiframes of 2 x 700 keypoints, blocks of 300 .. 700 keypoints of which most are
    terms: a checked repeat of the run profiles/place_hessian.txt times"""
    monkeypatch.setattr(HS, "K", 700)
    chain = _chain(("hessian", 700), lambda: HessianChain(oracle, EUROC, 700, (300, 700)))
    assert chain.floors() == HESSIAN_700_FLOORS, chain.floors()
    T = run_scaled(chain, n=BS.N_BENCH, what="hessian 2 x 700")
    with_terms, fewest = HESSIAN_700_FLOORS
    n_terms = T["n_terms"][:BS.N_BENCH]
    assert int((n_terms[:BS.D] > 0).sum()) == with_terms >= 8 and int(n_terms[n_terms > 0].min()) >= fewest >= 16


# ---- map: table first pass -> ransac3d2d consensus -> removeOutliers -> table second pass ----------------------------
# (keypoints on not-yet-3-D landmarks, clutter) per block of the 16 distinct multiframes: full blocks (256), small ones
MAP_SIZES = ((100, 156), (150, 60), (40, 30), (1, 50), (120, 136), (80, 100), (200, 56), (10, 5),
             (90, 166), (140, 90), (60, 60), (30, 200), (128, 128), (20, 236), (180, 20), (70, 110))
MAP_FLOORS = (15, 28, 2278, 2092)   # MapChain.floors() of the restatements (ransac_scenes.chain_scene, seed 51)


class MapChain:
    """okvfe_match_to_map_table_blocks_device -> okvfe_ransac3d2d_consensus_blocks_device (landmark_out in place) ->
    okvfe_remove_outliers_blocks_device (in place) -> okvfe_match_to_map_table_uninitialised_blocks_device with the
    filtered rows as previous_landmark_dev: ransac_scenes.chain_scene over 16 multiframes of the EuRoC pair"""
    outputs = ("lm", "bd") + M.POOL_KEYS + ("n_corr", "best", "n_inl", "acc", "hyp", "state", "kept", "lm2", "bd2", "hp",
                                            "hs", "ctr")

    def __init__(self, oracle, d=BS.D, mode=0):
        self.d, self.K = d, S.K
        self.exclusive, self.thr = map_scenes.MODES[mode]
        ch = self.ch = S.chain_scene(oracle, TREE, self.exclusive, self.thr, sizes=MAP_SIZES[:d])
        assert max(len(f["desc"]) for f in ch["frames"]) == self.K and len(ch["cams"]) == 2
        self.first_bd = [M.reference_matches(oracle, ch["sc"], ch["refs1"][f], self.thr, (fr["kps"], fr["desc"], fr["use"]))[1]
                         for f, fr in enumerate(ch["frames"])]
        self.nh = ch["H"].shape[1]
        per_block = ("blocks", "use", "prev", "lm", "bd", "lm2", "bd2", "hp", "hs", "ctr", "state", "kept") + M.POOL_KEYS
        self.per_of = dict([(k, 2) for k in per_block] + [(k, 1) for k in ("H", "n_corr", "best", "n_inl", "acc", "hyp")])
        self.fe = self.prepared = self.tab = None

    def prepare(self, fe=None):
        ch, d, K = self.ch, self.d, self.K
        self.fe = fe if fe is not None else _frontend(ch["cams"], K)
        assert self.fe.max_keypoints == K
        if self.tab is None:
            self.tab = M.DeviceTable(self.fe, ch["sc"])       # (device pointers: any context of the process may use it)
        T = U.prepare(self.fe, self.tab.n_landmarks, ch["frames"])
        T.update(H=torch.from_numpy(ch["H"]).cuda(), n_corr=_full((d,), S.SENTINEL, torch.int32),
                 best=_full((d,), S.SENTINEL, torch.int32), n_inl=_full((d,), S.SENTINEL, torch.int32),
                 acc=_full((d,), S.STATE_SENTINEL, torch.uint8), hyp=_full((d, self.nh), S.SENTINEL, torch.int32),
                 state=_full((2 * d, K), S.STATE_SENTINEL, torch.uint8), kept=_full((2 * d,), S.SENTINEL, torch.int32))
        torch.cuda.synchronize()
        self.prepared = T
        return self

    def floors(self):
        """(accepted multiframes, fewest inliers of an accepted one, first-pass matches, second-pass matches of the 16)"""
        ch = self.ch
        acc = [c for c in ch["cons"] if c["accepted"]]
        return (len(acc), min(c["n_inliers"] for c in acc), sum(int((r >= 0).sum()) for r in ch["first"]),
                sum(int((r[0] >= 0).sum()) for r in ch["second"]))

    def workspace_bytes_per_frame(self):
        """include/okvfe.h on okvfe_match_to_map_table_blocks_device: 32 bytes per (frame, landmark) pair plus the
        keypoint order (an int32 per keypoint slot)"""
        return 32 * len(self.ch["sc"]["hp"]) + 4 * self.K

    def launch(self, T, n, stream, index=None):
        fe, ch, tab = self.fe, self.ch, self.tab
        index = np.arange(n) % self.d if index is None else index
        ids = [0, 1] * n
        p1 = [ch["poses1"][2 * int(k) + c] for k in index for c in (0, 1)]
        p2 = [ch["poses2"][2 * int(k) + c] for k in index for c in (0, 1)]
        ptr = lambda k: T[k].data_ptr()
        fe.match_to_map_table_blocks_device(tab.desc, ptr("blocks"), 2 * n, ids, p1, self.thr, self.exclusive, ptr("use"),
                                            U.pool_device(fe, T), ptr("lm"), ptr("bd"), stream)
        res = fe.make_ransac_result_device(ptr("n_corr"), ptr("best"), ptr("n_inl"), ptr("acc"), ptr("hyp"), ptr("state"),
                                           None, ptr("lm"))
        fe.ransac3d2d_consensus_blocks_device(tab.desc, ptr("blocks"), n, [0, 1], ch["T_SC"], ptr("lm"), ptr("H"), None,
                                              self.nh, res, stream=stream)
        fe.remove_outliers_blocks_device(tab.desc, ptr("blocks"), 2 * n, ids, p2, ptr("lm"), ptr("lm"), ptr("kept"),
                                         stream=stream)
        fe.match_to_map_table_uninitialised_blocks_device(
            tab.desc, U.pool_device(fe, T, projection=False), ptr("blocks"), 2 * n, ids, p2, self.exclusive, ptr("use"),
            ptr("lm"), ptr("lm2"), ptr("bd2"), ptr("hp"), ptr("hs"), ptr("ctr"), stream)

    def check_anchors(self, A, first=None):
        ch, K = self.ch, self.K
        m = self.d if first is None else first
        L = self.tab.n_landmarks
        torch.cuda.synchronize()
        g = {k: A[k][:m * self.per_of[k]].cpu().numpy() for k in self.outputs}
        for mi in range(m):
            cons, w = ch["cons"][mi], ("map", mi)
            head = (int(g["n_corr"][mi]), int(g["best"][mi]), int(g["n_inl"][mi]), int(g["acc"][mi]))
            assert head == (cons["n_corr"], cons["best"], cons["n_inliers"], cons["accepted"]), (w, head)
            assert np.array_equal(g["hyp"][mi], cons["hyp_inliers"]), (w, "hyp_inliers")
            for c in range(2):
                f = 2 * mi + c
                fr = ch["frames"][f]
                n = len(fr["desc"])
                M.check_pool({k: g[k][f][:L] for k in M.POOL_KEYS}, ch["refs1"][f], w + (c, "pool"))
                assert np.array_equal(g["bd"][f, :n], self.first_bd[f]) and np.all(g["bd"][f, n:] == M.SENTINEL), (w, c, "bd")
                assert np.array_equal(g["state"][f, :n], cons["state"][c]), (w, c, "state")
                assert np.all(g["state"][f, n:] == S.STATE_SENTINEL), (w, c, "state past the count")
                filtered, k = ch["removed"][f]
                assert np.array_equal(g["lm"][f, :n], filtered), (w, c, "filtered rows")
                assert np.all(g["lm"][f, n:] == M.SENTINEL) and int(g["kept"][f]) == k, (w, c, "kept")
                U.check_frame(g, f, n, ch["second"][f], w + (c, "second pass"))


def _map_chain(oracle):
    chain = _chain(("map",), lambda: MapChain(oracle))
    assert chain.floors() == MAP_FLOORS, chain.floors()
    return chain if chain.prepared is not None else chain.prepare()


def test_map_chain(oracle):
    """The four calls of the matchToMap chain at N = 3077 multiframes = 6154 frames (K = 256, 1400 landmarks).

    Workspace: the first pass asks 32 * 1400 + 4 * 256 = 45 824 bytes per frame, 282 MB for the
    6154 frames; tools/bench_map_table.py's 3072 frames of 700 keypoints against 5000 landmarks ask 500 MB.  Both are
    below the limit of 1 GiB: the benchmark's batch runs WHOLE, and so does this one.  The sliced path at this size
    is test_map_chain_in_slices."""
    chain = _map_chain(oracle)
    assert chain.floors() == MAP_FLOORS, chain.floors()
    assert 2 * BS.N * chain.workspace_bytes_per_frame() < (1 << 30) // 2    # whole, with room to spare
    assert 3072 * (32 * 5000 + 4 * 700) < (1 << 30) // 2                        # ... as the benchmark's
    T = run_scaled(chain, what="map")
    accepted, inliers, first, second = MAP_FLOORS
    acc, n_inl = T["acc"][:BS.N], T["n_inl"][:BS.N]
    assert int(acc[:BS.D].sum()) == accepted and int(acc.sum()) >= accepted * (BS.N // BS.D)
    assert int(n_inl[acc == 1].min()) >= inliers >= 16
    assert int((T["lm2"][:2 * BS.D] >= 0).sum()) == second >= 16 and int((T["lm2"][:2 * BS.N] >= 0).sum()) >= second * (BS.N // BS.D)
    assert first >= 16 * 16


def test_map_chain_in_slices(oracle):
    """the same batch in a fresh context whose workspace limit (the existing test hook) makes the 6154 frames 3 slices of
    2500, 2500 and 1154: the same bytes as the whole run, and a workspace of one slice's size"""
    chain = _map_chain(oracle)
    n, d = BS.N, chain.d
    per_frame = chain.workspace_bytes_per_frame()
    limit = 2500 * per_frame + per_frame // 2       # (room for 2500 frames and half a frame of whatever else a frame needs)
    assert limit // per_frame == 2500 and -(-2 * n // 2500) == 3 and 2 * n % 2500 == 1154
    order = BS.placements(n, d)[0]
    stream = torch.cuda.Stream()
    whole, _ = BS.tile_tensors(chain.prepared, order, d, chain.per_of)
    torch.cuda.synchronize()
    chain.launch(whole, n, stream)
    stream.synchronize()
    ws_whole = chain.fe._test_context_sizes(stream)["table_ws_bytes"]
    shared = chain.fe
    fe = _frontend(chain.ch["cams"], chain.K, fresh=True)
    try:
        fe._test_set_map_table_workspace_limit(limit)
        chain.fe = fe
        T, guard = BS.tile_tensors(chain.prepared, order, d, chain.per_of)
        torch.cuda.synchronize()
        chain.launch(T, n, stream)
        stream.synchronize()
        ws = fe._test_context_sizes(stream)["table_ws_bytes"]
        assert BS.changed(T, {k: whole[k] for k in chain.outputs}) == []
        assert BS.untouched(T, guard) == []
        assert ws_whole >= 2 * n * per_frame and 2500 * per_frame <= ws < 2501 * per_frame + 4096, (ws_whole, ws, limit)
    finally:
        chain.fe = shared
        fe.close()


class PooledMapChain:
    """okvfe_match_to_map_blocks_device, the older route over a pooled set with projections per frame, whose keypoint
    order lives in the per-stream map_perm workspace of n_frames * max_keypoints int32: 16 ragged frames (one full, one
    empty) of the scene of test_gpu_map_blocks.py at K = 256 against the oracle's single-frame loop"""
    outputs = ("lm", "bd")
    SIZES = (S.K, 0, 133, 255, 1, 200, 64, 65, 250, 17, 128, 129, 90, 222, 31, S.K)
    THR = 20.0

    def __init__(self, oracle, d=BS.D, n_lm=1500, seed=31):
        self.d, self.K = d, S.K
        cfg = synth.euroc_config()
        self.cams, K = list(cfg.cams), S.K
        rng = np.random.default_rng(seed)
        frames = []
        for n in self.SIZES[:d]:
            kps = np.zeros(n, dtype=oracle.KEYPOINT_DTYPE)
            kps["x"], kps["y"] = rng.uniform(30, 720, n), rng.uniform(30, 450, n)
            frames.append((kps, rng.integers(0, 256, (n, 48), dtype=np.uint8)))
        counts = rng.integers(1, 4, n_lm)
        counts[::19] = 0
        begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        pool = rng.integers(0, 256, (begin[-1], 48), dtype=np.uint8)
        proj = np.stack([np.stack([rng.uniform(0, 752, n_lm), rng.uniform(0, 480, n_lm)], 1) for _ in range(d)])
        use = (rng.random((d, K)) > 0.15).astype(np.uint8)
        for f, (kps, desc) in enumerate(frames):   # landmark l observes keypoint l of frame f, with one of its descriptors
            for l in range(0, min(len(kps), n_lm), 2):
                if counts[l]:
                    proj[f, l] = (kps["x"][l] + rng.normal(0, 3), kps["y"][l] + rng.normal(0, 3))
                    desc[l] = pool[begin[l] + rng.integers(0, counts[l])] ^ ((rng.random(48) < 0.05) * rng.integers(0, 256, 48)).astype(np.uint8)
        self.frames, self.begin, self.pool, self.proj, self.use, self.n_lm = frames, begin, pool, proj, use, n_lm
        self.refs = [oracle.match_to_map(desc, kps, use[f, :len(kps)], proj[f], begin, pool, self.THR, cfg.match_threshold)
                     for f, (kps, desc) in enumerate(frames)]
        self.per_of = dict(blocks=1, use=1, proj=1, lm=1, bd=1)
        self.fe = self.prepared = None

    def prepare(self, fe=None):
        from okvis2_amd import multigpu
        self.fe = fe if fe is not None else _frontend(self.cams, self.K)
        K, d = self.K, self.d
        blocks = np.stack([multigpu.pack_block_host(K, kps, desc, np.zeros((len(kps), 3)), np.zeros(len(kps), np.uint8))
                           for kps, desc in self.frames])
        self.prepared = dict(blocks=S._dev(blocks), use=S._dev(self.use), proj=S._dev(self.proj), begin=S._dev(self.begin),
                             pool=S._dev(self.pool), lm=_full((d, K), M.SENTINEL, torch.int32),
                             bd=_full((d, K), M.SENTINEL, torch.int32))
        torch.cuda.synchronize()
        return self

    def floors(self):
        """(matches of the 16 frames, frames with at least 16 of them)"""
        hits = [int((rl >= 0).sum()) for rl, _ in self.refs]
        return sum(hits), sum(h >= 16 for h in hits)

    def launch(self, T, n, stream, index=None):
        md = self.fe.make_map_device(self.n_lm, T["begin"].data_ptr(), T["pool"].data_ptr(), T["proj"].data_ptr())
        self.fe.match_to_map_blocks_device(T["blocks"].data_ptr(), n, T["use"].data_ptr(), md, self.THR, T["lm"].data_ptr(),
                                           T["bd"].data_ptr(), stream)

    def check_anchors(self, A, first=None):
        m = self.d if first is None else first
        torch.cuda.synchronize()
        lm, bd = A["lm"][:m].cpu().numpy(), A["bd"][:m].cpu().numpy()
        for f in range(m):
            n, (rl, rd) = len(self.frames[f][0]), self.refs[f]
            assert np.array_equal(lm[f, :n], rl) and np.array_equal(bd[f, :n], rd), ("pooled map", f)
            assert np.all(lm[f, n:] == M.SENTINEL) and np.all(bd[f, n:] == M.SENTINEL), ("pooled map", f, "past the count")


POOLED_MAP_FLOORS = (825, 12)   # PooledMapChain.floors() of the oracle's rows


def test_pooled_map_route(oracle):
    """N = 3077 frames; the map_perm workspace (okvfe_test_context_sizes) holds n_frames * 256 int32 afterwards"""
    chain = _chain(("pooled map",), lambda: PooledMapChain(oracle))
    assert chain.floors() == POOLED_MAP_FLOORS, chain.floors()
    fe = _frontend(chain.cams, chain.K, fresh=True)       # (a context whose workspace this call alone has sized)
    chain.prepare()
    shared, chain.fe = chain.fe, fe
    try:
        stream = torch.cuda.Stream()
        T = run_scaled(chain, what="pooled map", stream=stream)
        sizes = fe._test_context_sizes(stream)
        assert sizes["perm_entries"] == 1 and sizes["table_ws_entries"] == 0 and sizes["perm_bytes"] >= BS.N * chain.K * 4
    finally:
        chain.fe = shared
        fe.close()
    assert int((T["lm"][:BS.N] >= 0).sum()) >= POOLED_MAP_FLOORS[0] * (BS.N // BS.D)


# ---- the consensus of runRansac3d2d on the rigs the map chain's scene does not have ------------------------------------
RANSAC_FLOORS = {"hilti": (11, 435), ("radtan8",): (8, 117)}   # RansacChain.floors() of ransac_ref.consensus, seed 0


class RansacChain:
    """okvfe_ransac3d2d_consensus_blocks_device over ransac_scenes.general_scene, every optional output on"""
    outputs = ("n_corr", "best", "n_inl", "accepted", "hyp_inliers", "state", "distance", "lm_out")

    def __init__(self, oracle, spec, d=BS.D):
        self.spec, self.d, self.K = spec, d, S.K
        sc = self.sc = S.general_scene(oracle, spec, n_mf=d)
        self.refs = S.reference(TREE, sc)
        C = len(sc["cams"])
        self.per_of = dict([(k, 1) for k in ("H", "valid", "n_corr", "best", "n_inl", "accepted", "hyp_inliers")] +
                           [(k, C) for k in ("blocks", "lm", "state", "distance", "lm_out")])
        self.fe = self.prepared = self.tab = None

    def prepare(self, fe=None):
        self.fe = fe if fe is not None else _frontend(self.sc["cams"], self.K)
        self.tab = S.DeviceTable(self.fe, self.sc["hp"], self.sc["obs_begin"])
        self.prepared = S.prepare_consensus(self.fe, self.sc)
        return self

    def floors(self):
        """(accepted multiframes, fewest inliers of an accepted one)"""
        acc = [r["n_inliers"] for r in self.refs if r["accepted"]]
        return len(acc), min(acc, default=0)

    def launch(self, T, n, stream, index=None):
        S.launch_consensus(self.fe, self.tab, dict(self.sc, mfs=[self.sc["mfs"][0]] + [None] * (n - 1)), T, stream=stream)

    def check_anchors(self, A, first=None):
        m = self.d if first is None else first
        sub = dict(self.sc, mfs=self.sc["mfs"][:m])
        S.check_consensus(sub, {k: v[:m * self.per_of[k]] for k, v in A.items() if k in self.per_of and v is not None},
                          self.refs[:m], ("ransac", S.spec_id(self.spec)))


@pytest.mark.parametrize("spec", ["hilti", ("radtan8",)], ids=S.spec_id)
def test_ransac_consensus_on_the_other_rigs(oracle, spec):
    """the 5-camera Hilti rig and the RADTAN8 camera at N = 3077 (the EuRoC pair runs inside the map chain)"""
    chain = _chain(("ransac", spec), lambda: RansacChain(oracle, spec))
    assert chain.floors() == RANSAC_FLOORS[spec], chain.floors()
    T = run_scaled(chain, what="ransac " + S.spec_id(spec))
    accepted, inliers = RANSAC_FLOORS[spec]
    acc, n_inl = T["accepted"][:BS.N], T["n_inl"][:BS.N]
    assert int(acc[:BS.D].sum()) == accepted >= 8 and int(n_inl[acc == 1].min()) >= inliers >= 16


# ---- query: bow_vectors -> place_query -> bow_database_add ---------------------------------------------------------------
QUERY_FLOORS = (9, 5, 9)   # of place_query_ref's chain over the 12 multiframes, computed on the CPU


def _flat_rows(t, n, row_bytes):
    return t[:n * row_bytes].reshape(n, row_bytes)


def test_query_chain(oracle):
    """okvfe_bow_vectors_blocks_device -> okvfe_place_query_blocks_device -> okvfe_bow_database_add_blocks_device at
    N = 3077 = 12 x 256 + 5: place_query_scenes.rig_scene has 12 distinct multiframes of 2 cameras (K = 128, blocks of 0,
    1 and K keypoints, a multiframe without a feature).  The database starts with 40 entries and has room for every
    multiframe of two runs and of the shuffled run: all 40 + 3 N entries are compared with the reference's lists."""
    import place_query_ref as QR
    import place_query_scenes as QS
    from okvis2_amd import capi
    K, C, E0, cap = 128, 2, 40, 8
    n, d = BS.N, 12
    voc = QR.shipped_vocabulary(oracle)
    scene = QS.rig_scene(oracle, voc, C, K)
    refs = QS.reference_vectors(oracle, voc, scene)
    assert len(refs) == d
    db = QS.host_database(oracle, voc, scene, E0)
    ref_scores = [db.scores(oracle, ids, vals) for _, ids, vals in refs]
    walks = [QR.walk(s, None, QR.MIN_SCORE) for s in ref_scores]
    floors = (sum(len(r[1]) > 60 for r in refs), max(len(w[1]) for w in walks), sum(len(w[1]) > 0 for w in walks))
    assert floors == QUERY_FLOORS, floors       # (vectors of more than 60 words, most candidates, multiframes with any)
    stride = min(C * K, len(voc["ww"]))
    modular, shuffled = BS.placements(n, d)
    fe = capi.Frontend(128, 128, 10.0, 0, 50, K, num_cameras=1)
    try:
        dev = QS.Dev(torch)
        blocks16 = torch.from_numpy(QS.pack_blocks(scene)).cuda()
        vd = dev.vocabulary(voc)
        words0 = int(db.arrays()[0][-1])
        dbd = dev.database(db, cap_entries=E0 + 3 * n + 2, cap_words=words0 + 3 * n * stride)
        dbd40 = dev.database(QS.host_database(oracle, voc, scene, E0), name="db40")    # (the same entries: same seed)
        rows = dict(q_n=4, q_ids=stride * 4, q_vals=stride * 8, word_ids=C * K * 4, scores=E0 * 8, c_listed=4, c_count=4,
                    c_entry=cap * 4, c_score=cap * 8)
        stream = torch.cuda.Stream()
        results = {}
        for run, order in (("modular", modular), ("shuffled", shuffled)):
            T, _ = BS.tile_tensors(dict(blocks=blocks16), order, d, dict(blocks=C))
            dev.t["blocks"] = T["blocks"]
            vec = dev.vectors(n + BS.EXTRA, stride, len(voc["ww"]))
            wptr = dev.out("word_ids", (n + BS.EXTRA) * C * K * 4)
            sptr = dev.out("scores", (n + BS.EXTRA) * E0 * 8)
            cand = dev.candidates(n + BS.EXTRA, cap)
            torch.cuda.synchronize()
            adds = 1
            fe.bow_vectors_blocks_device(vd, dev.ptr("blocks"), n, C, vec, wptr, stream=stream)
            if run == "modular":     # the queries see the 40 entries: the scores' row length is the database's size
                fe.place_query_blocks_device(dbd, vec, n, cand, scores_ptr=sptr, stream=stream)
                stream.synchronize()
                first = {k: dev.t[k].clone() for k in rows}
                torch.cuda.synchronize()
                fe.bow_vectors_blocks_device(vd, dev.ptr("blocks"), n, C, vec, wptr, stream=stream)   # the second run
                fe.place_query_blocks_device(dbd, vec, n, cand, scores_ptr=sptr, stream=stream)
                fe.bow_database_add_blocks_device(dbd, vec, n, list(range(n)), stream=stream)
                adds = 2
            else:                    # the shuffled queries: against a second object of the same 40 entries
                fe.place_query_blocks_device(dbd40, vec, n, cand, scores_ptr=sptr, stream=stream)
            fe.bow_database_add_blocks_device(dbd, vec, n, list(range(n)), stream=stream)
            for _ in range(adds):
                for i in order:
                    db.add(refs[int(i) % d][1], refs[int(i) % d][2])
            fe.bow_database_check_device(dbd, stream=stream)     # waits for the stream; raises if an entry found no room
            if run == "modular":
                assert [k for k in rows if not torch.equal(dev.t[k], first[k])] == [], "second run"
            results[run] = {k: dev.t[k] for k in rows}
            for k, rb in rows.items():       # the records behind the batch
                assert bool((dev.t[k][n * rb:] == QS.SENTINEL).all()), (run, k)
            if run == "modular":
                QS.check_vectors(dev, refs, stride, "anchors")
                got = dev.get("word_ids", np.int32, d, C, K)
                for m, (words, _, _) in enumerate(refs):
                    for c in range(C):
                        assert np.array_equal(got[m, c, :len(words[c])], words[c]) and np.all(got[m, c, len(words[c]):] == QS.FILL_I32)
                scores = dev.get("scores", np.uint64, d, E0)
                assert all(np.array_equal(scores[m], ref_scores[m].view(np.uint64)) for m in range(d))
                QS.check_candidates(dev, d, cap, walks, "anchors")
                for k, rb in rows.items():
                    assert BS.first_difference(_flat_rows(dev.t[k], n, rb), d, n) is None, k
            else:
                for k, rb in rows.items():
                    assert BS.first_misplaced(_flat_rows(dev.t[k], n, rb), _flat_rows(results["modular"][k], n, rb), order) is None, k
        begin, ids, vals = db.arrays()
        E = len(db.entries)
        assert E == E0 + 3 * n == dbd.n_entries
        assert np.array_equal(dev.get("db_begin", np.int32, E + 1), begin)
        assert np.array_equal(dev.get("db_ids", np.int32, len(ids)), ids)
        assert np.array_equal(dev.get("db_vals", np.uint64, len(vals)), vals.view(np.uint64))
        assert np.all(dev.get("db_begin", np.int32, dbd.cap_entries + 1)[E + 1:] == QS.FILL_I32)
        assert np.all(dev.get("db_ids", np.int32, dbd.cap_words)[len(ids):] == QS.FILL_I32)
    finally:
        fe.close()


# ---- per frame: keyframe coverage and overlap pairs ------------------------------------------------------------------
PER_FRAME_FLOORS = (6, 209, 18)   # PerFrameChain.floors() of overlap_ref's masks


class PerFrameChain:
    """okvfe_keyframe_coverage_blocks_device over every block and okvfe_overlap_pairs_blocks_device over one pair per
    multiframe, with the per-image records: overlap_scenes.multiframes of the EuRoC pair (10 distinct multiframes, K =
    700, blocks of 0, 1, 20, 226 and K keypoints).  Pair i is (i, a position that holds distinct multiframe
    (distinct(i) + 1) % 10), so every pair is a replica of one of the ten pairs (v, (v + 1) % 10)."""
    outputs = ("frames_cov", "counts", "pairs_cov")

    def __init__(self, oracle=None):
        import keyframe_ref as KR
        import overlap_ref as OR
        import overlap_scenes as OS
        from okvis2_amd import capi
        self.OS, self.OR, self.capi = OS, OR, capi
        cfg = self.cfg = synth.euroc_config()
        self.d, self.K, self.C = OS.N_MULTIFRAMES, cfg.max_kpts, len(cfg.cams)
        mfs = self.mfs = OS.multiframes(cfg, self.K)
        self.pairs = [(v, (v + 1) % self.d) for v in range(self.d)]
        self.refs = [OR.overlap_counts(cfg.w, cfg.h, mfs[a], mfs[b], OS.KPTRAD) for a, b in self.pairs]
        # a frame's coverage with "matched = id != 0": side A of the multiframe against itself (every id of its own is
        # common), which overlap_ref paints for keypoints without finite coordinates as well
        self.frame_refs = [c for mf in mfs for c in OR.overlap_counts(cfg.w, cfg.h, mf, mf, OS.KPTRAD)["per_image"][0]]
        self.fields = KR.COVERAGE_FIELDS
        self.per_of = dict(blocks=self.C, ids=self.C, frames_cov=self.C, counts=1, pairs_cov=2 * self.C)
        self.fe = self.prepared = None

    def prepare(self, fe=None):
        self.fe = fe if fe is not None else _frontend(self.cfg.cams, self.K)
        assert self.fe.max_keypoints == self.K
        blocks, ids = self.OS.pack(self.mfs, self.K, self.C, 1)
        d, C = self.d, self.C
        self.prepared = dict(blocks=S._dev(blocks), ids=S._dev(ids), frames_cov=_full((d * C, 6), -7, torch.int32),
                             counts=_full((d, 8), -7, torch.int32), pairs_cov=_full((d * 2 * C, 6), -7, torch.int32))
        torch.cuda.synchronize()
        return self

    def floors(self):
        """(pairs of the 10 with an overlap strictly between 0 and 1, matched keypoints of their sides A, frames of the
        20 with a matched keypoint)"""
        return (sum(0.0 < r["overlap"] < 1.0 for r in self.refs), sum(r["n_matched"][0] for r in self.refs),
                sum(r["n_matched"] > 0 for r in self.frame_refs))

    def launch(self, T, n, stream, index=None):
        index = np.arange(n) % self.d if index is None else np.asarray(index)
        at = [np.flatnonzero(index == v) for v in range(self.d)]
        partner = [int(at[(int(v) + 1) % self.d][i % len(at[(int(v) + 1) % self.d])]) for i, v in enumerate(index)]
        self.fe.keyframe_coverage_blocks_device(T["blocks"].data_ptr(), n * self.C, T["ids"].data_ptr(),
                                                T["frames_cov"].data_ptr(), None, 0, self.OS.KPTRAD, stream)
        self.fe.overlap_pairs_blocks_device(T["blocks"].data_ptr(), self.C, 1, n, self.C, T["ids"].data_ptr(),
                                            list(range(n)), partner, T["counts"].data_ptr(), T["pairs_cov"].data_ptr(),
                                            self.OS.KPTRAD, stream)

    def check_anchors(self, A, first=None):
        capi, C, d = self.capi, self.C, self.d
        torch.cuda.synchronize()
        counts = np.ascontiguousarray(A["counts"][:d].cpu().numpy()).view(capi.OVERLAP_COUNTS_DTYPE).reshape(-1)
        for name in self.OR.COUNT_FIELDS:
            assert counts[name].tolist() == [r[name] for r in self.refs], ("overlap counts", name)
        cov = np.ascontiguousarray(A["pairs_cov"][:d * 2 * C].cpu().numpy()).view(capi.COVERAGE_DTYPE).reshape(d, 2, C)
        one = np.ascontiguousarray(A["frames_cov"][:d * C].cpu().numpy()).view(capi.COVERAGE_DTYPE).reshape(-1)
        for name in self.fields:
            assert cov[name].tolist() == [[[c[name] for c in side] for side in r["per_image"]] for r in self.refs], name
            assert one[name].tolist() == [r[name] for r in self.frame_refs], ("coverage", name)


def test_per_frame_calls(oracle):
    """keyframe coverage over 6154 blocks and 3077 overlap pairs (N = 3077 = 10 x 307 + 7 multiframes of 2 x 700)"""
    chain = _chain(("per frame",), lambda: PerFrameChain())
    assert chain.floors() == PER_FRAME_FLOORS, chain.floors()
    T = run_scaled(chain, what="per frame")
    counts = T["counts"][:BS.N]
    # (okvfe_overlap_counts: n_keypoints[2], n_matched[2], ...: column 2 is n_matched of side A)
    assert int((counts[:, 2] > 0).sum()) >= PER_FRAME_FLOORS[0] * (BS.N // chain.d)
    assert int(counts[:chain.d, 2].sum()) == PER_FRAME_FLOORS[1]


# ---- motion: the consensus of runRansac2d2d and matchStereo's landmark bookkeeping -------------------------------------
RANSAC2D2D_FLOORS = {EUROC: (2, 841), "hilti": (2, 2113), ("radtan8",): (2, 456)}   # of ransac2d2d_ref.run, seed 3
STEREO_INSERT_FLOORS = {"stereo-counts": (1152, 414), "euroc-stereo": (433, 91), "hilti-3": (601, 244),
                        "hilti-5": (1299, 481)}   # of stereo_insert_ref


class Ransac2d2dChain:
    """okvfe_ransac2d2d_consensus_blocks_device over ransac2d2d_scenes.general_scene: three distinct (older, current)
    pairs of a rig -- a pure rotation, a translation, a translation with swapped ids -- every optional output on"""

    def __init__(self, oracle, spec):
        import ransac2d2d_scenes as S2
        self.S2, self.spec, self.K = S2, spec, S2.K
        sc = self.sc = S2.general_scene(oracle, spec)
        self.d = len(sc["pairs"])
        self.refs = S2.reference(TREE, sc)
        C = len(sc["cams"])
        per_pair = S2.PER_CAM + S2.PER_PAIR + ("rot_H", "rel_H", "rot_valid", "rel_valid", "rot_hyp_inliers", "rel_hyp_inliers",
                                               "match1", "state", "distance")
        self.per_of = dict([(k, 1) for k in per_pair] + [(k, C) for k in ("blocks0", "blocks1", "lm0", "lm1", "lm1_out")])
        self.outputs = S2.PER_CAM + S2.PER_PAIR + ("rot_hyp_inliers", "rel_hyp_inliers", "match1", "state", "distance", "lm1_out")
        self.fe = self.prepared = None

    def prepare(self, fe=None):
        self.fe = fe if fe is not None else _frontend(self.sc["cams"], self.K)
        self.prepared = self.S2.prepare(self.fe, self.sc)
        return self

    def floors(self):
        """(pairs whose success flag is not 0, correspondences of all cameras of all pairs)"""
        return sum(r["success"] != 0 for r in self.refs), sum(c["n_corr"] for r in self.refs for c in r["cams"])

    def launch(self, T, n, stream, index=None):
        sc = dict(self.sc, pairs=[self.sc["pairs"][0]] + [None] * (n - 1))
        self.S2.launch(self.fe, sc, dict(T, n_mf0=n, n_mf1=n), stream=stream)

    def check_anchors(self, A, first=None):
        self.S2.check(self.sc, A, self.refs, ("ransac2d2d", S.spec_id(self.spec)))


@pytest.mark.parametrize("spec", [EUROC, "hilti", ("radtan8",)], ids=S.spec_id)
def test_ransac2d2d_consensus(oracle, spec):
    """N = 3077 = 3 x 1025 + 2 pairs of multiframes on the EuRoC pair, the 5-camera Hilti rig and the RADTAN8 camera"""
    chain = _chain(("ransac2d2d", spec), lambda: Ransac2d2dChain(oracle, spec))
    assert chain.floors() == RANSAC2D2D_FLOORS[spec], chain.floors()
    T = run_scaled(chain, what="ransac2d2d " + S.spec_id(spec))
    assert int((T["success"][:BS.N] != 0).sum()) >= RANSAC2D2D_FLOORS[spec][0] * (BS.N // chain.d) >= BS.N // chain.d


class StereoInsertChain:
    """okvfe_stereo_insert_blocks_device over a stereo_insert_scenes rig scene (K = 260).  The matcher rows and the
    optional outputs are pair-major, [pairs][multiframes][K]: they are tiled per pair, the call gets them as ONE array
    of N multiframes per pair assembled on the call's stream, and what it wrote comes back per pair for the comparison;
    two guard rows of K behind the whole array are checked through `tail_ok`."""

    def __init__(self, oracle, name):
        import stereo_insert_scenes as SI
        self.SI, self.name, self.K = SI, name, SI.K
        self.sc = {s["name"]: s for s in SI.rig_scenes(oracle)}[name]
        self.P, C = len(self.sc["pairs"]), len(self.sc["cams"])
        self.refs = SI.reference_of(oracle, TREE, self.sc)[0]
        self.d = len(self.sc["mfs"])
        per_pair = [k + str(p) for p in range(self.P) for k in ("matches", "action", "lm_row")]
        self.per_of = dict([("blocks", C), ("lm", C), ("lm_out", C), ("counts", 1), ("keyframe", 1)] + [(k, 1) for k in per_pair])
        self.outputs = ["counts", "lm_out"] + [k for k in per_pair if not k.startswith("matches")]
        self.fe = self.prepared = None

    def prepare(self, fe=None):
        from okvis2_amd import capi
        SI, cams = self.SI, self.sc["cams"]
        if fe is None:
            fe = _FRONTENDS.get(("stereo insert", self.name))
            if fe is None:
                fe = _FRONTENDS[("stereo insert", self.name)] = capi.Frontend(SI.W, SI.H, 10.0, 0, 50, SI.K, match_threshold=60,
                                                                            num_cameras=len(cams))
                for i, c in enumerate(cams):
                    fe.set_camera(i, c)
        self.fe = fe
        T = SI.prepare(fe, self.sc)
        for k in ("matches", "action", "lm_row"):       # [pairs][multiframes][...] -> per pair [multiframes][...]
            whole = T.pop(k)
            for p in range(self.P):
                T[k + str(p)] = whole[p].contiguous()
        T.pop("matches_np")
        self.prepared = T
        return self

    def floors(self):
        """(matches taken up, landmarks created: the sums of the counts' first two columns)"""
        c = np.array([r["counts"] for r in self.refs])
        return int(c[:, 0].sum()), int(c[:, 1].sum())

    def launch(self, T, n, stream, index=None):
        SI, P, K = self.SI, self.P, self.K
        index = np.arange(n) % self.d if index is None else index
        with torch.cuda.stream(stream):
            matches = torch.stack([T["matches" + str(p)][:n] for p in range(P)]).contiguous()
            action = torch.full((P * n * K + 2 * K,), SI.ACTION_SENTINEL, dtype=torch.uint8, device="cuda")
            lm_row = torch.full((P * n * K + 2 * K,), SI.SENTINEL, dtype=torch.int32, device="cuda")
        SI.launch(self.fe, self.sc, dict(T, mfs=[self.sc["mfs"][int(k)] for k in index], matches=matches, action=action,
                                         lm_row=lm_row), stream=stream)
        with torch.cuda.stream(stream):
            for p in range(P):
                T["action" + str(p)][:n].copy_(action[:P * n * K].view(P, n, K)[p])
                T["lm_row" + str(p)][:n].copy_(lm_row[:P * n * K].view(P, n, K)[p])
            T["tail_ok"] = (action[P * n * K:] == SI.ACTION_SENTINEL).all() & (lm_row[P * n * K:] == SI.SENTINEL).all()

    def check_anchors(self, A, first=None):
        assert bool(A["tail_ok"]), "rows behind the last pair's last multiframe were written"
        A = dict(A, mfs=self.sc["mfs"])
        for k in ("action", "lm_row"):
            A[k] = torch.stack([A[k + str(p)] for p in range(self.P)])
        self.SI.check(self.sc, A, self.refs, ("batch scale",))


@pytest.mark.parametrize("name", ["stereo-counts", "euroc-stereo", "hilti-3", "hilti-5"])
def test_stereo_insert(oracle, name):
    """N = 3077 multiframes: 8 distinct ones with blocks of 0, 1, 255, 256, 257 and K rows (3077 = 8 x 384 + 5); the
    EuRoC pair's 3 with a multiframe that is no keyframe; three cameras with every pair; Hilti's five cameras and nine
    pairs (2 distinct multiframes each: 3077 = 2 x 1538 + 1)"""
    chain = _chain(("stereo insert", name), lambda: StereoInsertChain(oracle, name))
    assert chain.floors() == STEREO_INSERT_FLOORS[name], chain.floors()
    T = run_scaled(chain, what="stereo insert " + name)
    assert bool(T["tail_ok"])
    counts = T["counts"][:BS.N]
    assert int(counts[:chain.d, 0].sum()) == STEREO_INSERT_FLOORS[name][0] >= 16
    assert int(counts[:, 0].sum()) >= STEREO_INSERT_FLOORS[name][0] * (BS.N // chain.d)


MOTION_FLOORS = (2639, 1050, 64, 32)   # MotionChain.floors() of motion_claim_ref and ransac2d2d_ref


class MotionChain:
    """The motion-stereo sweep before initialisation, two steps queued back to back as in test_gpu_ransac2d2d_chain.py:
    per step okvfe_match_motion_stereo_blocks_batch_device with claims (one pair per block, 256 bytes of parameters
    each through the ring), the caller's ids for the claimed rows by torch ops on the same stream,
    okvfe_ransac2d2d_consensus_blocks_device with landmark1_out in place, matched1 = (id >= 0) for the next step.
    The ids a block hands out are those of its DISTINCT block (a tiled input), so replicated multiframes give replicated
    rows, claims, ids and verdicts.  16 distinct multiframes of 2 cameras (EuRoC, TUM-VI), 1024 x 1024, K = 512."""

    def __init__(self, oracle, n_current=BS.D):
        import gate_scenes
        import motion_claim_ref as MC
        import ransac2d2d_scenes as S2
        import test_gpu_ransac2d2d_chain as RC
        from okvis2_amd import capi
        self.MC, self.S2, self.RC, self.capi, self.threshold = MC, S2, RC, capi, gate_scenes.THRESHOLD
        self.d, self.K, self.C, self.steps = n_current, RC.K, RC.N_CAMS, RC.STEPS
        self.cams = [synth.euroc_config().cams[0], synth.tumvi1024_config().cams[0]]
        sw = self.sw = MC.sweep_scene(self.cams, ("euroc", "tumvi"), n_current=n_current, steps=RC.STEPS)
        self.lists = RC._lists(sw, np.random.default_rng(7))
        self.ref_steps, self.lm1_ref, self.matched1_ref = RC.reference_chain(TREE, sw, self.lists)
        per_block = ["b1", "m_init", "lm1_init", "lm1", "m_next"]
        per_mf, self.outputs = [], ["lm1", "m_next"]
        for j in range(self.steps):
            per_block += [k + str(j) for k in ("b0_", "skip_", "ids_", "rot_", "rel_", "rows_", "claimed_", "ncl_", "lm0_")]
            per_mf += [k + "_" + str(j) for k in S2.PER_CAM + S2.PER_PAIR + ("match1", "state")]
            self.outputs += [k + str(j) for k in ("rows_", "claimed_", "ncl_", "lm0_")] + per_mf[-len(S2.PER_CAM + S2.PER_PAIR) - 2:]
        self.per_of = dict([(k, self.C) for k in per_block] + [(k, 1) for k in per_mf])
        self.fe = self.prepared = None

    def floors(self):
        """(claims of step 0, claims of step 1, cameras that remove outliers, pairs with a success code)"""
        st = self.ref_steps
        return (sum(r["n_claimed"] for r in st[0]["res"]), sum(r["n_claimed"] for r in st[1]["res"]),
                sum(bool(c["removed"]) for s in st for ref in s["cons"] for c in ref["cams"]),
                sum(ref["success"] != 0 for s in st for ref in s["cons"]))

    def prepare(self, fe=None):
        from okvis2_amd import multigpu
        RC, S2, sw, K, C, d = self.RC, self.S2, self.sw, self.K, self.C, self.d
        if fe is None:
            fe = _FRONTENDS.get(("motion",))
            if fe is None:
                fe = _FRONTENDS[("motion",)] = self.capi.Frontend(RC.W, RC.H, 38.0, 0, 150, K, match_threshold=self.threshold,
                                                                  max_batch=1, num_cameras=C)
                for slot, cam in enumerate(self.cams):
                    fe.set_camera(slot, self.MC.with_frame_size(cam, RC.W, RC.H))
        self.fe = fe
        assert fe.max_keypoints == K
        nb = d * C
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        block = lambda kp, ds, bp, bv: multigpu.pack_block_host(K, kp, ds, bp, bv)
        T = dict(b1=dev(np.stack([block(sc["kp1"], sc["d1"], sc["bp1"], sc["bv1"]) for sc in sw["current"]])),
                 m_init=dev(np.stack([RC._pad(m, 0, np.uint8) for m in sw["matched1"]])),
                 lm1_init=dev(np.stack([RC._pad(np.where(m != 0, RC.KNOWN_ID + np.arange(len(m)), -1), -1, np.int32)
                                        for m in sw["matched1"]])),
                 lm1=_full((nb, K), S2.SENTINEL, torch.int32), m_next=_full((nb, K), RC.FILL, torch.uint8))
        for j, step in enumerate(sw["older"][:self.steps]):
            s = str(j)
            T["b0_" + s] = dev(np.stack([block(o["kp0"], o["d0"], o["bp0"], o["bv0"]) for o in step]))
            T["skip_" + s] = dev(np.stack([RC._pad(o["skip0"], 0, np.uint8) for o in step]))
            T["ids_" + s] = dev((RC.NEW_ID + (j * nb + np.arange(nb)[:, None]) * K + np.arange(K)[None, :]).astype(np.int32))
            T["rot_" + s] = dev(np.stack([l[0] for l in self.lists[j]]))
            T["rel_" + s] = dev(np.stack([l[1] for l in self.lists[j]]))
            T["rows_" + s] = _full((nb, K, RC.REC), RC.FILL, torch.uint8)
            T["claimed_" + s] = _full((nb, K), RC.FILL, torch.uint8)
            T["ncl_" + s] = _full((nb,), -7, torch.int32)
            T["lm0_" + s] = _full((nb, K), -1, torch.int32)
            for k in S2.PER_CAM + S2.PER_PAIR + ("match1", "state"):
                u8 = k in S2.U8 or k == "state"
                shape = (d,) if k in S2.PER_PAIR else ((d, C) if k in S2.PER_CAM else (d, C, K))
                T[k + "_" + s] = _full(shape, S2.STATE_SENTINEL if u8 else S2.SENTINEL, torch.uint8 if u8 else torch.int32)
        torch.cuda.synchronize()
        self.prepared = T
        return self

    def launch(self, T, n, stream, index=None):
        fe, S2, K, C, sw = self.fe, self.S2, self.K, self.C, self.sw
        index = np.arange(n) % self.d if index is None else index
        nb = n * C
        T0 = [sw["current"][int(k) * C + c]["T0"] for k in index for c in range(C)]
        T1 = [sw["current"][int(k) * C + c]["T1"] for k in index for c in range(C)]
        slots = [b % C for b in range(nb)]
        with torch.cuda.stream(stream):     # the sweep's state, made afresh: a second launch starts where the first did
            m = T["m_init"][:nb].clone()
            w = torch.cat([T["lm1_init"][:nb].reshape(-1), torch.zeros(1, dtype=torch.int32, device="cuda")])  # + a slot nobody reads
            block_of = torch.arange(nb, device="cuda").reshape(nb, 1) * K
        for j in range(self.steps):
            s = str(j)
            fe.match_motion_stereo_blocks_batch_device(
                T["b0_" + s].data_ptr(), nb, T["b1"].data_ptr(), nb, None, None, slots, T0, T1, T["skip_" + s].data_ptr(),
                m.data_ptr(), T["rows_" + s].data_ptr(),
                claim=dict(claimed=T["claimed_" + s].data_ptr(), n_claimed=T["ncl_" + s].data_ptr(), matched1_out=m.data_ptr()),
                stream=stream)
            with torch.cuda.stream(stream):  # the caller's addLandmark / setLandmarkId for the claimed rows
                k1 = T["rows_" + s][:nb, :, :4].contiguous().view(torch.int32).reshape(nb, K).to(torch.int64)
                won = T["claimed_" + s][:nb] == 1
                ids = T["ids_" + s][:nb]
                T["lm0_" + s][:nb] = torch.where(won, ids, torch.full_like(ids, -1))
                target = torch.where(won, block_of + k1, torch.full_like(k1, nb * K))
                w.scatter_(0, target.reshape(-1), ids.reshape(-1))
            o = lambda k: T[k + "_" + s].data_ptr()
            res = fe.make_ransac2d2d_result_device(*[o(k) for k in S2.PER_CAM + S2.PER_PAIR], match1_ptr=o("match1"),
                                                   state_ptr=o("state"), landmark1_out_ptr=w.data_ptr())
            fe.ransac2d2d_consensus_blocks_device(
                T["b0_" + s].data_ptr(), n, T["b1"].data_ptr(), n, np.arange(n), np.arange(n), list(range(C)),
                T["lm0_" + s].data_ptr(), w.data_ptr(), None, 0, T["rot_" + s].data_ptr(), None, T["rel_" + s].data_ptr(), None,
                self.RC.N_HYP, res, stream=stream)
            with torch.cuda.stream(stream):  # removeObservation frees the current keypoint for the next older frame
                m.copy_((w[:nb * K].reshape(nb, K) >= 0).to(torch.uint8))
        with torch.cuda.stream(stream):
            T["lm1"][:nb].copy_(w[:nb * K].reshape(nb, K))
            T["m_next"][:nb].copy_(m)

    def check_anchors(self, A, first=None):
        capi, S2, C, d = self.capi, self.S2, self.C, self.d
        torch.cuda.synchronize()
        g = {k: A[k][:d * self.per_of[k]].cpu().numpy() for k in self.outputs}
        for j, st in enumerate(self.ref_steps):
            s = str(j)
            for b, r in enumerate(st["res"]):
                n0 = len(r["rows"])
                mine = np.ascontiguousarray(g["rows_" + s][b, :n0]).reshape(-1).view(capi.MOTION_MATCH_DTYPE)
                for f in ("k1", "dist", "initialisable", "accepted"):
                    assert np.array_equal(mine[f], r["rows"][f]), (j, b, f)
                assert np.array_equal(g["claimed_" + s][b, :n0], r["claimed"]) and int(g["ncl_" + s][b]) == r["n_claimed"], (j, b)
                assert np.all(g["rows_" + s][b, n0:] == self.RC.FILL) and np.all(g["claimed_" + s][b, n0:] == self.RC.FILL), (j, b)
                assert np.array_equal(g["lm0_" + s][b, :n0], st["lm0"][b]) and np.all(g["lm0_" + s][b, n0:] == -1), (j, b)
            for mf, ref in enumerate(st["cons"]):
                head = tuple(int(g[k + "_" + s][mf]) for k in S2.PER_PAIR)
                assert head == (ref["total_inliers"], ref["rotation_only"], ref["success"]), (j, mf, head)
                for c, rc in enumerate(ref["cams"]):
                    per = tuple(int(g[k + "_" + s][mf, c]) for k in S2.PER_CAM)
                    assert per == tuple(rc[k] for k in S2.PER_CAM), (j, mf, c, per)
                    n0 = len(rc["match1"])
                    assert np.array_equal(g["match1_" + s][mf, c, :n0], rc["match1"]), (j, mf, c)
                    assert np.all(g["match1_" + s][mf, c, n0:] == S2.SENTINEL), (j, mf, c)
                    assert np.array_equal(g["state_" + s][mf, c, :n0], rc["state"]), (j, mf, c)
                    assert np.all(g["state_" + s][mf, c, n0:] == S2.STATE_SENTINEL), (j, mf, c)
        for b in range(d * C):
            n1 = len(self.lm1_ref[b])
            assert np.array_equal(g["lm1"][b, :n1], self.lm1_ref[b]) and np.all(g["lm1"][b, n1:] == -1), b
            assert np.array_equal(g["m_next"][b, :n1], self.matched1_ref[b]), b


def test_motion_chain(oracle):
    """N = 3077 multiframes = 6154 (older block, current block, camera) pairs per step: 1.5 MB of pair records through
    the parameter ring per call, the largest upload of the group"""
    chain = _chain(("motion",), lambda: MotionChain(oracle))
    assert chain.floors() == MOTION_FLOORS, chain.floors()
    fe_sizes = []
    T = run_scaled(chain, what="motion")
    fe_sizes.append(chain.fe._test_context_sizes())
    assert fe_sizes[0]["ring_slot_bytes"] >= 2 * BS.N * 256          # (okvfe.h: 256 bytes per pair through the ring)
    for j in range(chain.steps):
        ncl = T["ncl_" + str(j)][:2 * BS.N]
        assert int(ncl[:2 * BS.D].sum()) == MOTION_FLOORS[j] >= 50 and int(ncl.sum()) >= MOTION_FLOORS[j] * (BS.N // BS.D)


# ---- growth and shrink --------------------------------------------------------------------------------------------------
def _three_sizes(chain, fe, what):
    """N = 3, 3077, 3 queued on one stream of one fresh context with nothing waited for, every call on buffers of its own;
    returns the context sizes seen after each call was queued"""
    n, d = BS.N, chain.d
    shared, chain.fe = chain.fe, fe
    try:
        stream = torch.cuda.Stream()
        batches = [BS.tile_tensors(chain.prepared, np.arange(m), d, chain.per_of) for m in (3, n, 3)]
        torch.cuda.synchronize()
        sizes = [fe._test_context_sizes(stream)]
        for (T, _), m in zip(batches, (3, n, 3)):
            chain.launch(T, m, stream)
            sizes.append(fe._test_context_sizes(stream))
        stream.synchronize()
        for (T, guard), m in zip(batches, (3, n, 3)):
            chain.check_anchors(BS.anchors(T, min(m, d), chain.per_of), first=min(m, d))
            assert BS.untouched(T, guard) == [], (what, m)
        T = batches[1][0]
        for k in chain.outputs:
            assert BS.first_difference(T[k], d, n, chain.per_of[k]) is None, (what, k)
        return sizes
    finally:
        chain.fe = shared


def test_map_chain_grows_and_shrinks_on_one_stream(oracle):
    """3 -> 3077 -> 3 multiframes: the parameter ring's slots and the stream's workspace grow under the queued small
    call (okvfe_test_context_sizes: both larger), and the second small call runs in the large buffers"""
    chain = _map_chain(oracle)
    fe = _frontend(chain.ch["cams"], chain.K, fresh=True)
    try:
        s0, s1, s2, s3 = _three_sizes(chain, fe, "map 3-3077-3")
    finally:
        fe.close()
    per_frame = chain.workspace_bytes_per_frame()
    assert s0["table_ws_bytes"] == 0 and 6 * per_frame <= s1["table_ws_bytes"] < 2 * BS.N * per_frame <= s2["table_ws_bytes"]
    assert s1["ring_slot_bytes"] < 2 * BS.N * 112 <= s2["ring_slot_bytes"]    # (112 bytes of pose and camera per frame)
    assert s3 == s2


def test_map_chain_grows_under_another_streams_batch(oracle):
    """Stream A: 1500 multiframes.  While that is queued, stream B: 3077 -- a larger ring slot than anything before it
    (ring_reserve drains A's pending slots and reallocates) and a second entry of the workspace list.  Then A again with
    3077: A's workspace is freed and allocated anew while B's batch is in flight.  All three results are right, and
    okvfe_test_context_sizes shows each growth."""
    chain = _map_chain(oracle)
    d, n, small = chain.d, BS.N, 1500
    per_frame = chain.workspace_bytes_per_frame()
    fe = _frontend(chain.ch["cams"], chain.K, fresh=True)
    shared, chain.fe = chain.fe, fe
    try:
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        batches = [BS.tile_tensors(chain.prepared, np.arange(m), d, chain.per_of) for m in (small, n, n)]
        torch.cuda.synchronize()
        chain.launch(batches[0][0], small, a)
        a1, b1 = fe._test_context_sizes(a), fe._test_context_sizes(b)
        chain.launch(batches[1][0], n, b)
        a2, b2 = fe._test_context_sizes(a), fe._test_context_sizes(b)
        chain.launch(batches[2][0], n, a)
        a3, b3 = fe._test_context_sizes(a), fe._test_context_sizes(b)
        torch.cuda.synchronize()
        assert a1["table_ws_entries"] == 1 and b1["table_ws_bytes"] == 0 and a1["table_ws_bytes"] >= 2 * small * per_frame
        assert a2["ring_slot_bytes"] > a1["ring_slot_bytes"] and a2["ring_slot_bytes"] >= 2 * n * 112
        assert a2["table_ws_entries"] == 2 and b2["table_ws_bytes"] >= 2 * n * per_frame
        assert a2["table_ws_bytes"] == a1["table_ws_bytes"] < 2 * n * per_frame
        assert a3["table_ws_bytes"] >= 2 * n * per_frame and b3["table_ws_bytes"] == b2["table_ws_bytes"]
        assert a3["ring_slot_bytes"] == a2["ring_slot_bytes"] and a3["table_ws_entries"] == 2
        for (T, guard), m in zip(batches, (small, n, n)):
            chain.check_anchors(BS.anchors(T, d, chain.per_of))
            for k in chain.outputs:
                assert BS.first_difference(T[k], d, m, chain.per_of[k]) is None, (m, k)
            assert BS.untouched(T, guard) == [], m
    finally:
        chain.fe = shared
        fe.close()


def test_map_chain_evicts_the_oldest_streams_workspace(oracle):
    """nine streams make one small call each: the list of per-stream workspaces holds eight, so the first stream's is
    freed (after a device synchronisation); a call on the first stream again gets a new one, and every result is right"""
    chain = _map_chain(oracle)
    d = chain.d
    fe = _frontend(chain.ch["cams"], chain.K, fresh=True)
    shared, chain.fe = chain.fe, fe
    try:
        streams = [torch.cuda.Stream() for _ in range(9)]
        batches = [BS.tile_tensors(chain.prepared, np.arange(3), d, chain.per_of) for _ in range(10)]
        torch.cuda.synchronize()
        for (T, _), s in zip(batches, streams):
            chain.launch(T, 3, s)
        seen = fe._test_context_sizes(streams[0])
        assert seen["table_ws_entries"] == 8 and seen["table_ws_bytes"] == 0
        assert fe._test_context_sizes(streams[1])["table_ws_bytes"] > 0
        chain.launch(batches[9][0], 3, streams[0])
        again = fe._test_context_sizes(streams[0])
        assert again["table_ws_entries"] == 8 and again["table_ws_bytes"] > 0
        assert fe._test_context_sizes(streams[1])["table_ws_bytes"] == 0      # (the second stream's went for it)
        torch.cuda.synchronize()
        for T, guard in batches:
            chain.check_anchors(BS.anchors(T, 3, chain.per_of), first=3)
            assert BS.untouched(T, guard) == []
    finally:
        chain.fe = shared
        fe.close()


FIVE = ("equi",) * 5


def test_place_chain_grows_the_ring_under_another_streams_batch(oracle):
    """One context with five camera slots.  Stream A: the 2-camera chain at N = 3077 (its rig records fit the ring's
    first slots: the slot size stays).  While that is queued, stream B: the 5-camera chain at N = 3, whose larger rig
    records make ring_reserve wait for A's pending slots, free both halves of the ring and allocate larger ones.  Then A
    again at N = 3077.  All three results equal their restatements and replicas.

    What this proves of the drain in ring_reserve: the results are right and the ring did grow.  It does not prove that
    the drain loop is needed: hipFree of the ring's device half waits for the device on its own."""
    two = _chain(("place", ("equi", "equi")), lambda: PlaceChain(oracle, ("equi", "equi")))
    five = _chain(("place", FIVE), lambda: PlaceChain(oracle, FIVE, d=3))
    assert two.floors() == (9, 234, 117) and five.floors() == (2, 464, 421)      # (the restatements' figures)
    fe = _frontend(five.sc["cams"], PS.K, fresh=True)
    n, d = BS.N, two.d
    try:
        two.prepare(fe), five.prepare(fe)
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        A1, A2 = (BS.tile_tensors(two.prepared, np.arange(n), d, two.per_of) for _ in range(2))
        B1 = BS.tile_tensors(five.prepared, np.arange(3), 3, five.per_of)
        torch.cuda.synchronize()
        s0 = fe._test_context_sizes(a)
        two.launch(A1[0], n, a)
        s1 = fe._test_context_sizes(a)
        five.launch(B1[0], 3, b)
        s2 = fe._test_context_sizes(a)
        two.launch(A2[0], n, a)
        s3 = fe._test_context_sizes(a)
        torch.cuda.synchronize()
        assert s0["ring_slot_bytes"] == s1["ring_slot_bytes"] and s0["ring_dev"] == s1["ring_dev"]      # A alone: no growth
        # (the new ring may lie where the old one did: the size tells, the address does not)
        assert s2["ring_slot_bytes"] > s1["ring_slot_bytes"] and s3 == s2
        for T, guard in (A1, A2):
            two.check_anchors(BS.anchors(T, d, two.per_of))
            for k in two.outputs:
                assert BS.first_difference(T[k], d, n, two.per_of[k]) is None, k
            assert BS.untouched(T, guard) == []
        five.check_anchors(BS.anchors(B1[0], 3, five.per_of))
        assert BS.untouched(*B1) == []
    finally:
        two.fe = five.fe = two.prepared = five.prepared = None
        fe.close()


def test_place_chain_three_sizes_on_one_stream(oracle):
    """3 -> 3077 -> 3 multiframes of the place chain on one stream: nothing of the context grows with the batch here
    (the rig records depend on the cameras alone), which the sizes show; the results are right all the same"""
    chain = _chain(("place", EUROC), lambda: PlaceChain(oracle, EUROC))
    fe = _frontend(chain.sc["cams"], PS.K, fresh=True)
    held = chain.prepared
    try:
        chain.prepare(fe)
        sizes = _three_sizes(chain, fe, "place 3-3077-3")
        assert all(s == sizes[0] for s in sizes)
    finally:
        chain.prepared = held
        chain.fe = _frontend(chain.sc["cams"], PS.K)
        fe.close()
