"""Scenes for okvfe_place_hessian_blocks_device, for small contexts (188 x 120, K = 320): per rig of
ransac_scenes.GENERAL_SPECS one general scene (1, 3 or 17 multiframes of keypoints at projections of set landmarks, with
the states a consensus would leave); a directed scene over the four camera models that reaches every label of
place_hessian_ref.CENSUS; multiframes with exact numbers of terms around the kernel's chunk; blocks of 0, 1 and K
keypoints; poses with an unnormalised, a zero and a NaN quaternion.  CPU only up to `prepare` and `launch`, which need
torch and a GPU.  Test infrastructure only."""
import dataclasses

import numpy as np

import place_hessian_ref as PH
import ransac_scenes as S

K = 320
W, H = 188, 120
COPIES = 16
H_SENTINEL = -4321.0
ROW_SENTINEL = -12345.0
COUNT_SENTINEL = -7
BATCH = {("radtan8",): 3, ("nodist",): 1, ("euroc", "euroc1"): 17, "hilti": 3}   # multiframes per general scene


def small(cam):
    """the camera at a quarter of its size: the contexts of these tests are 188 x 120"""
    return dataclasses.replace(cam, w=W, h=H, fu=cam.fu / 4, fv=cam.fv / 4, cu=cam.cu / 4, cv=cam.cv / 4)


def quaternion(C):
    """(x, y, z, w) of a rotation matrix (Shepperd's method; any quaternion will do: the call normalises it itself)"""
    C = np.asarray(C, dtype=np.float64).reshape(3, 3)
    t = np.array([C[0, 0], C[1, 1], C[2, 2], C[0, 0] + C[1, 1] + C[2, 2]])
    i = int(np.argmax(t))
    if i == 3:
        q = np.array([C[2, 1] - C[1, 2], C[0, 2] - C[2, 0], C[1, 0] - C[0, 1], 1.0 + t[3]])
    else:
        j, k = (i + 1) % 3, (i + 2) % 3
        q = np.zeros(4)
        q[i] = 1.0 + 2.0 * C[i, i] - t[3]
        q[j] = C[j, i] + C[i, j]
        q[k] = C[k, i] + C[i, k]
        q[3] = C[k, j] - C[j, k]
    return q / np.linalg.norm(q)


def pose7(T):
    """(C, r) -> (t[3], qx, qy, qz, qw), the PoseParameterBlock layout"""
    return np.concatenate([np.asarray(T[1], dtype=np.float64), quaternion(T[0])])


def rig(spec):
    cams, T_SC = S.rig(spec)
    return [small(c) for c in cams], T_SC


def scene(name, cams, T_SC, hp, mfs):
    return dict(name=name, cams=cams, T_SC=T_SC, T_SC_params=np.array([pose7(T) for T in T_SC]),
                hp=np.ascontiguousarray(hp, dtype=np.float64).reshape(-1, 4), mfs=mfs)


def _mf(frames, ml, state, pose, verdict=3):
    return dict(frames=frames, ml=[np.asarray(v, dtype=np.int32) for v in ml],
                state=[np.asarray(v, dtype=np.uint8) for v in state], pose=np.asarray(pose, dtype=np.float64),
                verdict=int(verdict))


def _states(rng, lm, p_inlier=0.7):
    """what a consensus leaves: 0 without a landmark, else 2 (inlier) or 1"""
    st = np.where(rng.random(len(lm)) < p_inlier, 2, 1).astype(np.uint8)
    st[lm < 0] = 0
    return st


def refined(T_WS, rng, angle=0.01, shift=0.02):
    """a pose near T_WS, as a solver would leave it"""
    C = np.asarray(T_WS[0], dtype=np.float64).reshape(3, 3) @ S.rodrigues(rng.normal(size=3), angle * rng.random())
    return pose7((C, np.asarray(T_WS[1]) + shift * rng.normal(size=3)))


def general_scene(oracle, spec, n_mf=None, seed=0, n_kps=(30, 120)):
    """ragged blocks (one full, one empty where there is more than one), a mix of verdicts beyond the first multiframe"""
    m = S.table()
    cams, T_SC = rig(spec)
    n_mf = BATCH[spec] if n_mf is None else n_mf
    rng = np.random.default_rng([seed, len(cams), n_mf])
    usable = S.usable_rows(m)
    mfs = []
    for i in range(n_mf):
        T_WS = (m["T1"][0].reshape(3, 3) @ S.rodrigues((0, 1, 0), 0.02 * (i % 5)), m["T1"][1] + np.array([0.05 * (i % 7), 0.0, 0.0]))
        frames = []
        for c, cam in enumerate(cams):
            n = K if (i + c) % 7 == 0 else int(rng.integers(*n_kps))
            if i == 1 and c == len(cams) - 1 and len(cams) > 1:
                n = 0
            frames.append(S.make_frame(oracle, cam, S.compose(T_WS, T_SC[c]), m["p"], usable, n, rng, wrong=0.15, none=0.1))
        ml = [f["lm"] for f in frames]
        mfs.append(_mf(frames, ml, [_states(rng, l) for l in ml], refined(T_WS, rng), 3 if i % 4 != 2 else (i // 4) % 3))
    return scene("general-" + S.spec_id(spec), cams, T_SC, m["hp"], mfs)


DIRECTED_KINDS = ("euroc", "equi", "nodist", "radtan8")
# camera coordinates a landmark is put at: outside on each side, behind, a singular depth, past the 8-coefficient model's
# guard (rho > 9), in the image
TARGETS = ((-2.5, 0.1, 1.0), (0.1, -2.5, 1.0), (2.5, 0.1, 1.0), (0.1, 2.5, 1.0), (0.02, 0.01, -2.0), (0.1, 0.1, 1.0e-13),
           (2.4, 2.4, 1.0), (0.05, 0.02, 1.0))
BAD_SIZES = (0.0, -12.0, np.nan, np.inf)


def directed_scene(oracle, seed=3):
    """One camera per model.  Multiframe 0 (verified): per camera COPIES keypoints on a landmark at every TARGETS point of
    that camera, on the last one with hp negated (w < 0) and with every BAD_SIZES size, and on landmarks shared between
    cameras c and c + 1; COPIES keypoints each of state 0, state 1 and of state 2 with a row of -1 and a row past the
    set.  Multiframes 1 and 2: the same rows under the verdicts 2 and 1; multiframe 3: verified again, at another pose."""
    cams = [small(S.camera(k)) for k in DIRECTED_KINDS]
    T_SC = S.rig(DIRECTED_KINDS)[1]
    m = S.table()
    rng = np.random.default_rng(seed)
    T_WS = m["T1"]
    pose = pose7(T_WS)
    C_WS, r_WS = PH.rotation(True, pose[3:]), pose[:3]
    hp, frames, mls, states = [], [], [], []

    def add(c, p_C, scale=1.0):
        """the landmark that lies at p_C in camera c (up to rounding), as scale (p_W, 1)"""
        prm = pose7(T_SC[c])
        p_S = PH.rotation(True, prm[3:]) @ np.asarray(p_C) + prm[:3]
        hp.append(scale * np.append(C_WS @ p_S + r_WS, 1.0))
        return len(hp) - 1

    shared = [add(c, TARGETS[-1]) for c in range(len(cams))]      # claimed in camera c and in camera c + 1
    for c, cam in enumerate(cams):
        rows, sizes, st = [], [], []
        for p_C in TARGETS:
            l = add(c, p_C)
            rows += [l] * COPIES
        rows += [add(c, TARGETS[-1], -1.0)] * COPIES + [add(c, TARGETS[-1], -2.0)] * COPIES
        sizes += [12.0] * len(rows)
        for s in BAD_SIZES:
            rows += [add(c, TARGETS[-1])] * COPIES
            sizes += [s] * COPIES
        rows += [shared[c]] * COPIES + [shared[(c + 1) % len(cams)]] * COPIES
        sizes += [18.0] * (2 * COPIES)
        st += [2] * len(rows)
        for state, row in ((0, -1), (1, shared[c]), (2, -1), (2, None)):
            rows += [row] * COPIES
            st += [state] * COPIES
            sizes += [12.0] * COPIES
        n = len(rows)
        assert n <= K
        kps = np.zeros(n, dtype=oracle.KEYPOINT_DTYPE)
        kps["x"], kps["y"] = rng.uniform(0, cam.w, n), rng.uniform(0, cam.h, n)
        kps["size"] = np.array(sizes, dtype=np.float32)
        bp, bpv = S.backproject(oracle, cam, kps)
        frames.append(dict(kps=kps, desc=np.zeros((n, 48), np.uint8), bp=bp, bpv=bpv, lm=np.zeros(n, np.int32)))
        mls.append(rows), states.append(st)
    L = len(hp)
    mls = [np.array([L + 3 if r is None else r for r in rows], dtype=np.int32) for rows in mls]
    other = refined(T_WS, rng)
    mfs = [_mf(frames, mls, states, pose, 3), _mf(frames, mls, states, pose, 2), _mf(frames, mls, states, pose, 1),
           _mf(frames, mls, states, other, 3)]
    return scene("directed", cams, T_SC, np.array(hp), mfs)


def term_count_scene(oracle, totals, spec="hilti", seed=31):
    """multiframes with exactly `totals` terms, spread over the cameras unevenly, every block full: the rows that are
    no terms lie between the others, so that the tiles of keypoints add uneven numbers of terms"""
    m = S.table()
    cams, T_SC = rig(spec)
    rng = np.random.default_rng([seed, len(cams)])
    usable = S.usable_rows(m)
    T_WS = m["T1"]
    mfs = []
    for total in totals:
        assert total <= len(cams) * K
        share = np.full(len(cams), total // len(cams))
        share[:total % len(cams)] += 1
        shift = int(min(K - share.max(), share.min()))
        share[0] += shift
        share[-1] -= shift
        frames, states = [], []
        for c, cam in enumerate(cams):
            fr = S.make_frame(oracle, cam, S.compose(T_WS, T_SC[c]), m["p"], usable, K, rng, wrong=0.1, none=0.0)
            st = np.ones(K, np.uint8)
            st[rng.permutation(K)[:share[c]]] = 2
            frames.append(fr), states.append(st)
        mfs.append(_mf(frames, [f["lm"] for f in frames], states, refined(T_WS, rng)))
    return scene("terms-" + "-".join(str(t) for t in totals), cams, T_SC, m["hp"], mfs)


def block_size_scene(oracle, seed=41):
    """blocks of 0, 1 and K keypoints, in every order over three cameras, every keypoint a term"""
    m = S.table()
    cams, T_SC = rig(("euroc", "euroc1", "euroc"))
    rng = np.random.default_rng(seed)
    usable = S.usable_rows(m)
    mfs = []
    for sizes in ((0, 1, K), (K, 0, 1), (1, K, 0), (0, 0, 0), (1, 1, 1)):
        frames = [S.make_frame(oracle, cam, S.compose(m["T1"], T_SC[c]), m["p"], usable, n, rng, wrong=0.0, none=0.0)
                  for c, (cam, n) in enumerate(zip(cams, sizes))]
        mfs.append(_mf(frames, [f["lm"] for f in frames], [np.full(len(f["lm"]), 2, np.uint8) for f in frames],
                       refined(m["T1"], rng)))
    return scene("block-sizes", cams, T_SC, m["hp"], mfs)


def pose_scene(oracle, seed=51):
    """one multiframe per pose: the true one, its quaternion times 3.5, a zero quaternion, a NaN translation, a NaN
    quaternion; the second camera's extrinsics carry an unnormalised quaternion as well"""
    m = S.table()
    cams, T_SC = rig(("euroc", "euroc1"))
    rng = np.random.default_rng(seed)
    usable = S.usable_rows(m)
    frames = [S.make_frame(oracle, cam, S.compose(m["T1"], T_SC[c]), m["p"], usable, 60, rng, wrong=0.1, none=0.1)
              for c, cam in enumerate(cams)]
    ml = [f["lm"] for f in frames]
    states = [_states(rng, l) for l in ml]
    p = pose7(m["T1"])
    poses = [p, np.concatenate([p[:3], 3.5 * p[3:]]), np.concatenate([p[:3], np.zeros(4)]),
             np.concatenate([[np.nan], p[1:]]), np.concatenate([p[:3], [p[3], np.nan, p[5], p[6]]])]
    sc = scene("poses", cams, T_SC, m["hp"], [_mf(frames, ml, states, q) for q in poses])
    sc["T_SC_params"][1, 3:] *= 0.25
    return sc


def reference(oracle, tree, sc, use_verdict=True, census=None):
    return [PH.evaluate(oracle, tree, sc["hp"], mf["frames"], mf["ml"], mf["state"], sc["cams"], sc["T_SC_params"],
                        mf["pose"], mf["verdict"] == 3 or not use_verdict, census) for mf in sc["mfs"]]


# ---- GPU side ----------------------------------------------------------------------------------------------------------
def prepare(fe, sc, optional=True):
    """the device tensors of a call over a scene (synchronises)"""
    import torch
    frames = [f for mf in sc["mfs"] for f in mf["frames"]]
    B, nb, Kc = len(sc["mfs"]), len(frames), fe.max_keypoints
    blocks, _ = S.pack_frames(fe, [dict(f, lm=np.zeros(0, np.int32)) for f in frames])
    ml = np.full((nb, Kc), S.PAST_COUNT_ROW, np.int32)   # (a term's row and state at or past the count: must be ignored)
    st = np.full((nb, Kc), 2, np.uint8)
    rows = [(r, s) for mf in sc["mfs"] for r, s in zip(mf["ml"], mf["state"])]
    for b, (r, s) in enumerate(rows):
        ml[b, :len(r)], st[b, :len(s)] = r, s
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
    T = dict(blocks=S._dev(blocks), hp=S._dev(sc["hp"]), ml=S._dev(ml), state=S._dev(st),
             poses=S._dev(np.stack([mf["pose"] for mf in sc["mfs"]])),
             verdict=S._dev(np.array([mf["verdict"] for mf in sc["mfs"]], dtype=np.uint8)),
             H=full((B, 36), H_SENTINEL, torch.float64), n_terms=full((B,), COUNT_SENTINEL, torch.int32),
             n_singular=full((B,), COUNT_SENTINEL, torch.int32))
    T["set"] = fe.make_place_set_device(len(sc["hp"]), T["hp"].data_ptr())
    if optional:
        T.update(residual=full((nb, Kc, 2), ROW_SENTINEL, torch.float64), jacobian=full((nb, Kc, 12), ROW_SENTINEL, torch.float64))
    torch.cuda.synchronize()
    return T


def launch(fe, sc, T, use_verdict=True, stream=None, residual=True, jacobian=True):
    """the call alone: nothing here waits for the device"""
    ptr = lambda k, on=True: None if not on or T.get(k) is None else T[k].data_ptr()
    res = fe.make_place_hessian_device(ptr("H"), ptr("n_terms"), ptr("n_singular"), ptr("residual", residual),
                                       ptr("jacobian", jacobian))
    fe.place_hessian_blocks_device(T["set"], T["blocks"].data_ptr(), len(sc["mfs"]), list(range(len(sc["cams"]))),
                                   sc["T_SC_params"], ptr("poses"), ptr("ml"), ptr("state"), ptr("verdict", use_verdict),
                                   res, stream)


def same_bytes(got, want):
    """equal as uint64 patterns, every NaN standing for every other (the sign and payload of a NaN that an operation
    makes are the processor's)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    canon = lambda a: np.where(np.isnan(a), np.float64(np.nan), a).view(np.uint64)
    return bool(np.array_equal(canon(got), canon(want)))


def check(sc, T, refs, what, residual=True, jacobian=True):
    """every output of every multiframe against the reference; rows that are no terms keep their sentinels"""
    import torch
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in T.items() if isinstance(v, torch.Tensor)}
    n_cams = len(sc["cams"])
    for mi, ref in enumerate(refs):
        w = what + (mi,)
        counts = (int(got["n_terms"][mi]), int(got["n_singular"][mi]))
        assert counts == (ref["n_terms"], ref["n_singular"]), (w, counts, ref["n_terms"], ref["n_singular"])
        assert same_bytes(got["H"][mi].reshape(6, 6), ref["H"]), (w, "H", got["H"][mi].reshape(6, 6), ref["H"])
        for key, on, rkey, width in (("residual", residual, "residual", 2), ("jacobian", jacobian, "jacobian", 12)):
            if key not in got:
                continue
            for c in range(n_cams):
                rows = got[key][mi * n_cams + c]
                term = np.zeros(len(rows), bool)
                if on:
                    term[ref["rows"][c]] = True
                    assert same_bytes(rows[term], ref[rkey][c]), (w, c, key)
                assert np.all(rows[~term] == ROW_SENTINEL), (w, c, key, "rows that are no terms")
    return got
