"""The GPU side of the tests of okvfe_place_refine_blocks_device: the device tensors of a call over a scene of
place_refine_scenes.py (on top of place_hessian_scenes.prepare), the call, and the comparison of every output of every
multiframe with the restatement's, byte for byte (a NaN standing for any NaN).  Every output tensor holds EXTRA
sentinel records behind the batch, which no call may touch.  Needs torch and a GPU.  Test infrastructure only."""
import numpy as np

import place_hessian_scenes as HS
import ransac_scenes as S

EXTRA = 2
POSE_SENTINEL = -777.0
COST_SENTINEL = -55.0
COUNT_SENTINEL = HS.COUNT_SENTINEL
H_SENTINEL = HS.H_SENTINEL
# key -> (records per multiframe row, dtype name, sentinel, the result struct's field)
OUTPUTS = dict(poses_out=(7, "float64", POSE_SENTINEL), status=(1, "int32", COUNT_SENTINEL),
               n_iterations=(1, "int32", COUNT_SENTINEL), n_accepted=(1, "int32", COUNT_SENTINEL),
               n_terms_out=(1, "int32", COUNT_SENTINEL), cost=(2, "float64", COST_SENTINEL),
               start_poses=(7, "float64", POSE_SENTINEL), H_out=(36, "float64", H_SENTINEL),
               n_singular_out=(1, "int32", COUNT_SENTINEL))
OPTIONAL = ("n_iterations", "n_accepted", "n_terms_out", "cost", "start_poses", "H_out", "n_singular_out")


def fresh_outputs(T, B):
    """(re)fills every output with its sentinel, EXTRA records behind the batch included"""
    import torch
    for key, (width, dt, fill) in OUTPUTS.items():
        shape = (B + EXTRA, width) if width > 1 else (B + EXTRA,)
        T[key] = torch.full(shape, fill, dtype=getattr(torch, dt), device="cuda")
    return T


def prepare(fe, sc):
    """the device tensors of a call over a scene (synchronises)"""
    import torch
    T = HS.prepare(fe, sc, optional=False)
    B = len(sc["mfs"])
    T["hyp"] = S._dev(np.stack([mf["hyp"] for mf in sc["mfs"]]).astype(np.float64))
    T["best"] = S._dev(np.array([mf["best"] for mf in sc["mfs"]], dtype=np.int32))
    if all(mf["initial"] is not None for mf in sc["mfs"]):
        T["initial"] = S._dev(np.stack([mf["initial"] for mf in sc["mfs"]]).astype(np.float64))
    fresh_outputs(T, B)
    torch.cuda.synchronize()
    return T


def launch(fe, sc, T, n=None, use_verdict=True, use_initial=False, max_iterations=None, stream=None, without=()):
    """the call alone: nothing here waits for the device.  without: optional outputs passed as NULL"""
    ptr = lambda k, on=True: None if not on or k in without or T.get(k) is None else T[k].data_ptr()
    res = fe.make_place_refine_device(ptr("poses_out"), ptr("status"), ptr("n_iterations"), ptr("n_accepted"),
                                      ptr("n_terms_out"), ptr("cost"), ptr("start_poses"), ptr("H_out"),
                                      ptr("n_singular_out"))
    n_hyp = T["hyp"].shape[1]
    fe.place_refine_blocks_device(T["set"], T["blocks"].data_ptr(), len(sc["mfs"]) if n is None else n,
                                  list(range(len(sc["cams"]))), sc["T_SC_params"], ptr("hyp", not use_initial), n_hyp,
                                  ptr("best", not use_initial), ptr("initial", use_initial), ptr("ml"), ptr("state"),
                                  ptr("verdict", use_verdict), sc["max_iterations"] if max_iterations is None else max_iterations,
                                  res, stream)


def download(T):
    import torch
    torch.cuda.synchronize()
    return {k: T[k].cpu().numpy() for k in OUTPUTS}


def check(got, refs, what, without=(), n_singular=None):
    """every output of every multiframe against its reference; the rows of an unverified multiframe and the records
    behind the batch keep their sentinels; an output passed as NULL keeps them everywhere"""
    B = len(refs)
    for key, (width, dt, fill) in OUTPUTS.items():
        rows = got[key]
        assert len(rows) == B + EXTRA and np.all(rows[B:] == fill), (what, key, "records behind the batch")
        if key in without or (key == "n_singular_out" and "H_out" in without):
            assert np.all(rows == fill), (what, key, "an output that was not asked for")
    on = lambda k: k not in without
    for mi, ref in enumerate(refs):
        w = what + (mi,)
        assert int(got["status"][mi]) == ref["status"], (w, int(got["status"][mi]), ref["status"])
        if ref["status"] == 0:
            assert np.all(got["poses_out"][mi] == POSE_SENTINEL) and np.all(got["start_poses"][mi] == POSE_SENTINEL), w
            assert not on("H_out") or not got["H_out"][mi].any(), w
            assert not on("cost") or not got["cost"][mi].any(), w
        else:
            assert HS.same_bytes(got["poses_out"][mi], ref["pose"]), (w, "pose", got["poses_out"][mi], ref["pose"])
            if on("start_poses"):
                assert HS.same_bytes(got["start_poses"][mi], ref["start_pose"]), (w, "start_pose")
            if on("cost"):
                assert HS.same_bytes(got["cost"][mi], ref["cost"]), (w, "cost", got["cost"][mi], ref["cost"])
            if on("H_out"):
                assert HS.same_bytes(got["H_out"][mi].reshape(6, 6), ref["H"]), (w, "H")
        for key, rkey in (("n_iterations", "n_iterations"), ("n_accepted", "n_accepted"), ("n_terms_out", "n_terms")):
            if on(key):
                assert int(got[key][mi]) == ref[rkey], (w, key, int(got[key][mi]), ref[rkey])
    return got
