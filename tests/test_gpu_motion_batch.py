"""GPU: okvfe_match_motion_stereo_blocks_batch_device -- matchMotionStereo for many (older block, current block, camera
slot) pairs in one launch, the frame-data part of its insertion loop (the claims), and the sweep over older frames
queued without a host synchronisation in between.

 - the batch's rows equal okvfe_match_motion_stereo_blocks_device pair by pair (whole 64-byte rows) and the CPU oracle
   (k1, dist, initialisable, accepted, hp_W as uint64), for permuted block indices, a shared older block, counts on
   both sides of the 64-row work-group and of the 256-descriptor LDS-resident limit, mixed camera models (both kRT8
   forms of the kernel), skip0 / matched1 present and absent, both orders of the FP64 sums;
 - claimed, n_claimed and matched1_out equal tests/motion_claim_ref.py on scenes where two k0 choose one k1;
 - a J = 3 sweep of 8 pairs per step on one non-default stream, and the C++ mirror's matchMotionStereoSweep on the
   same data through tests/cpp/motion_sweep_cli.cpp;
 - bad arguments are rejected before anything is launched.
One context of 1024 x 1024 holds the three camera models; the oracle is given each slot's camera with that frame size
(the projection's image bounds are the context's)."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import gate_scenes as S
import motion_claim_ref as R
from okvis2_amd import capi, multigpu, synth
from test_motion_batch_host import CLAIM_SPECS, sweep, sweep_camera

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 1024
K = 512
REC = capi.MOTION_MATCH_DTYPE.itemsize
FILL = 0xA5
CAMS = (synth.euroc_config().cams[0], synth.tumvi1024_config().cams[0], synth.radtan8_config().cams[0])
SLOT_OF_KIND = {"tumvi": 1}  # every other kind is observed through the EuRoC camera (slot 0); radtan8=True: slot 2

_FE = {}


def _frontend(octaves):
    """the module's two contexts: single scale (every keypoint of size 12) and a scale space of four layers, whose
    kernels read a keypoint's size class from its octave; slots 0 .. 2 = CAMS"""
    if octaves not in _FE:
        fe = capi.Frontend(W, H, 38.0, octaves, 150, K // max(1, 2 * octaves), match_threshold=S.THRESHOLD, max_batch=1,
                           num_cameras=4)
        assert fe.max_keypoints == K
        for slot, cam in enumerate(CAMS):
            fe.set_camera(slot, R.with_frame_size(cam, W, H))  # (a slot's camera has the context's frame size)
        _FE[octaves] = fe
    return _FE[octaves]


@pytest.fixture(scope="module", autouse=True)
def _close_frontends():
    yield
    while _FE:
        _FE.popitem()[1].close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _filled(*shape):
    return torch.full(shape, FILL, dtype=torch.uint8, device="cuda")


def _pad(a, n=K):
    return np.concatenate([np.asarray(a, np.uint8), np.zeros(n - len(a), np.uint8)])


def _block(sc, side):
    return multigpu.pack_block_host(K, sc["kp" + side], sc["d" + side], sc["bp" + side], sc["bv" + side])


def _slot(sc):
    return 2 if "oracle_cam" in sc else SLOT_OF_KIND.get(sc["kind"], 0)


def _oracle_cam(sc):
    return R.with_frame_size(sc.get("oracle_cam", sc["cam"]), W, H)


def _same_rows(got, ref, what, sc):
    """k1, dist, initialisable, accepted and the bits of hp_W against the oracle's rows"""
    assert len(got) == len(ref), what
    for f in ("k1", "dist", "initialisable", "accepted"):
        if f == "accepted" and "oracle_cam" in sc:
            # the oracle does not carry the 8-coefficient model: the 4 px verdict against its restatement
            want = S.radtan8_accepted(dict(sc, cam=R.with_frame_size(sc["cam"], W, H)), got)
            sure = want >= 0
            assert np.array_equal(got[f][sure], want[sure]) and sure.sum() >= len(want) - 2, (what, f)
            continue
        assert np.array_equal(got[f], ref[f]), (what, f, np.flatnonzero(got[f] != ref[f])[:8])
    g, r = np.ascontiguousarray(got["hp_W"]), np.ascontiguousarray(ref["hp_W"])
    nan = np.isnan(r)
    assert np.array_equal(np.isnan(g), nan), (what, "NaN rows differ")
    assert np.all((g.view(np.uint64) == r.view(np.uint64)) | nan), (what, "hp_W")


def _combine(older, current):
    """a pair of the older side of one scene and the current side of another (poses: the older scene's)"""
    out = dict(older)
    for k in ("d1", "kp1", "bp1", "bv1", "matched1"):
        out[k] = current[k]
    out["name"] = older["name"] + "+" + current["name"]
    return out


_POOL = []


def _pool():
    """nine pairs: counts 0, 1, 63, 64, 65, K on the older side and 0, 1, 256, 257, K on the current side, the three
    camera models, and pair 7 on the older block of pair 0"""
    if not _POOL:
        p = [S.pair_scene("general", 65, 257, seed=21),
             S.pair_scene("tumvi", 64, 256, seed=22),
             S.pair_scene("euroc", 63, 300, seed=23, radtan8=True),
             S.pair_scene("near", 1, K, seed=24),
             S.pair_scene("euroc", K, 1, seed=25),
             S.pair_scene("general", 0, 300, seed=26),
             S.pair_scene("tumvi", 300, 0, seed=27, invalid=0.1)]
        p.append(_combine(p[0], S.pair_scene("rot01", 10, 260, seed=28)))
        p.append(S.pair_scene("rot01", 300, 300, seed=29))
        _POOL.extend(p)
    return _POOL


def _layout(pairs, shared=()):
    """Blocks of a call in permuted order.  shared: (p, q) = pair p reads pair q's older block.
    -> (blocks0, blocks1 host arrays, idx0, idx1)"""
    n = len(pairs)
    owners = [p for p in range(n) if p not in dict(shared)]
    order0 = list(reversed(owners))                 # older blocks in reverse pair order
    order1 = [(p * 5 + 3) % n for p in range(n)] if n not in (5,) else list(reversed(range(n)))
    assert sorted(order1) == list(range(n))
    blocks0 = np.stack([_block(pairs[p], "0") for p in order0])
    blocks1 = np.stack([_block(pairs[p], "1") for p in order1])
    src = dict(shared)
    idx0 = np.array([order0.index(src.get(p, p)) for p in range(n)], np.int32)
    idx1 = np.array([order1.index(p) for p in range(n)], np.int32)
    return blocks0, blocks1, idx0, idx1


SUBSETS = {1: ([0], ()), 2: ([1, 2], ()), 9: (list(range(9)), ((7, 0),))}


@pytest.mark.usefixtures("fp64_order")
@pytest.mark.parametrize("flags", ["flags", "noflags"])
@pytest.mark.parametrize("n_pairs", [1, 2, 9])
def test_batch_equals_single_calls_and_oracle(oracle, n_pairs, flags):
    fe = _frontend(0)
    members, shared = SUBSETS[n_pairs]
    pairs = [_pool()[i] for i in members]
    blocks0, blocks1, idx0, idx1 = _layout(pairs, shared)
    d_b0, d_b1 = _dev(blocks0), _dev(blocks1)
    stride = fe.gather_block_bytes()
    assert blocks0.shape[1] == stride
    with_flags = flags == "flags"
    skip0 = np.stack([_pad(sc["skip0"]) for sc in pairs])
    matched1 = np.zeros((len(pairs), K), np.uint8)
    for p, sc in enumerate(pairs):
        matched1[idx1[p]] = _pad(sc["matched1"])
    d_skip0, d_matched1 = _dev(skip0), _dev(matched1)
    cams = [_slot(sc) for sc in pairs]
    assert n_pairs != 9 or set(cams) == {0, 1, 2}
    d_out = _filled(len(pairs), K, REC)
    fe.match_motion_stereo_blocks_batch_device(
        d_b0.data_ptr(), len(blocks0), d_b1.data_ptr(), len(blocks1), idx0, idx1, cams, [sc["T0"] for sc in pairs],
        [sc["T1"] for sc in pairs], d_skip0.data_ptr() if with_flags else None,
        d_matched1.data_ptr() if with_flags else None, d_out.data_ptr())
    d_one = _filled(len(pairs), K, REC)
    for p, sc in enumerate(pairs):
        fe.match_motion_stereo_blocks_device(
            cams[p], d_b0.data_ptr() + int(idx0[p]) * stride, d_b1.data_ptr() + int(idx1[p]) * stride,
            d_skip0.data_ptr() + p * K if with_flags else None,
            d_matched1.data_ptr() + int(idx1[p]) * K if with_flags else None, sc["T0"], sc["T1"],
            d_one.data_ptr() + p * K * REC)
    torch.cuda.synchronize()
    got, one = d_out.cpu().numpy(), d_one.cpu().numpy()
    assert np.array_equal(got, one), np.argwhere((got != one).any(axis=2))[:8]
    for p, sc in enumerate(pairs):
        n0 = len(sc["kp0"])
        assert np.all(got[p, n0:] == FILL), (p, "rows past the older count")
        ref = R.match_rows(sc, sc["skip0"] if with_flags else None, sc["matched1"] if with_flags else None,
                           _oracle_cam(sc))
        _same_rows(got[p, :n0].reshape(-1).view(capi.MOTION_MATCH_DTYPE), ref, (p, sc["name"]), sc)
    if n_pairs == 9:
        hits = sum(int((got[p, :len(sc["kp0"])].reshape(-1).view(capi.MOTION_MATCH_DTYPE)["k1"] >= 0).sum())
                   for p, sc in enumerate(pairs))
        assert hits > 200, hits


def _claim_pairs():
    return [R.contested_scene(kind, 300, 300, **kw) for kind, kw, _ in CLAIM_SPECS]


@pytest.mark.parametrize("mode", ["alias", "distinct", "null", "preset"])
def test_claims_equal_the_insertion_loop(oracle, mode):
    """alias: matched1_out is matched1_dev; distinct: another array with the same flags; null: no matched1_out (every
    k1 free); preset: matched1_dev NULL -- the matcher sees every current keypoint -- and matched1_out pre-set at half
    of the candidates' k1, which are never claimed."""
    fe = _frontend(2)  # (mixed size classes: the scenes that reach the 4 px rejection)
    pairs = _claim_pairs()
    n = len(pairs)
    blocks0, blocks1, idx0, idx1 = _layout(pairs)
    extra = np.zeros((1, blocks1.shape[1]), np.uint8)  # a current block no pair names
    blocks1 = np.concatenate([blocks1, extra])
    d_b0, d_b1 = _dev(blocks0), _dev(blocks1)
    cams = [_slot(sc) for sc in pairs]
    assert set(cams) == {0, 1}
    rng = np.random.default_rng(3)
    m_in = (rng.random((n + 1, K)) < 0.5).astype(np.uint8)  # (rows past the counts and the unused block: noise)
    refs, m_ref = [], m_in.copy()
    for p, sc in enumerate(pairs):
        n1 = len(sc["kp1"])
        if mode == "preset":
            rows = R.match_rows(sc, sc["skip0"], None, _oracle_cam(sc))
            cand = np.unique(rows["k1"][(rows["k1"] >= 0) & (rows["accepted"] != 0)])
            flags = np.zeros(n1, np.uint8)
            flags[cand[::2]] = 1
            assert flags.sum() >= 20
        else:
            flags = sc["matched1"]
            rows = R.match_rows(sc, sc["skip0"], flags, _oracle_cam(sc))
        m_in[idx1[p], :n1] = flags
        m_ref[idx1[p], :n1] = flags
        claimed, n_claimed, after = R.claim_loop(rows, len(rows), None if mode == "null" else flags)
        if mode == "preset":
            assert not np.any(flags[rows["k1"][claimed != 0]])
        if after is not None:
            m_ref[idx1[p], :n1] = after
        refs.append((rows, claimed, n_claimed))
    d_m = _dev(m_in)
    d_m_out = d_m if mode == "alias" else _dev(m_in) if mode in ("distinct", "preset") else None
    d_skip0 = _dev(np.stack([_pad(sc["skip0"]) for sc in pairs]))
    d_out, d_claimed = _filled(n, K, REC), _filled(n, K)
    d_n = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    fe.match_motion_stereo_blocks_batch_device(
        d_b0.data_ptr(), n, d_b1.data_ptr(), n + 1, idx0, idx1, cams, [sc["T0"] for sc in pairs],
        [sc["T1"] for sc in pairs], d_skip0.data_ptr(), None if mode == "preset" else d_m.data_ptr(), d_out.data_ptr(),
        claim=dict(claimed=d_claimed.data_ptr(), n_claimed=d_n.data_ptr(),
                   matched1_out=None if d_m_out is None else d_m_out.data_ptr()))
    torch.cuda.synchronize()
    got, claimed, n_claimed = d_out.cpu().numpy(), d_claimed.cpu().numpy(), d_n.cpu().numpy()
    total = 0
    for p, sc in enumerate(pairs):
        n0 = len(sc["kp0"])
        rows, c_ref, n_ref = refs[p]
        _same_rows(got[p, :n0].reshape(-1).view(capi.MOTION_MATCH_DTYPE), rows, (p, sc["name"]), sc)
        assert np.array_equal(claimed[p, :n0], c_ref), (p, np.flatnonzero(claimed[p, :n0] != c_ref)[:8])
        assert np.all(claimed[p, n0:] == FILL) and np.all(got[p, n0:] == FILL), p
        assert int(n_claimed[p]) == n_ref, (p, int(n_claimed[p]), n_ref)
        total += n_ref
    # per pair >= 32 contested and >= 32 uncontested free k1 (test_motion_batch_host.py); preset takes half of them
    floor = 5 * (32 if mode == "preset" else 64)
    assert total >= floor, total
    if d_m_out is not None:
        assert np.array_equal(d_m_out.cpu().numpy(), m_ref)  # the winners' bytes, everything else unchanged
        assert int((m_ref != m_in).sum()) == total
    if mode != "alias":
        assert np.array_equal(d_m.cpu().numpy(), m_in)  # matched1_dev is read only


def _sweep_arrays(sw):
    """blocks and per-step arguments of a sweep_scene: 8 current blocks, 24 older blocks in step-major order reversed"""
    n = len(sw["current"])
    steps = len(sw["older"])
    blocks1 = np.stack([_block(sc, "1") for sc in sw["current"]])
    older = [(j, b) for j in range(steps) for b in range(n)][::-1]
    blocks0 = np.stack([multigpu.pack_block_host(K, sw["older"][j][b]["kp0"], sw["older"][j][b]["d0"],
                                                 sw["older"][j][b]["bp0"], sw["older"][j][b]["bv0"]) for j, b in older])
    matched1 = np.stack([_pad(m) for m in sw["matched1"]])
    args = []
    for j in range(steps):
        idx0 = np.array([older.index((j, b)) for b in range(n)], np.int32)
        idx1 = np.arange(n, dtype=np.int32)
        cams = np.array([b % sw["n_cams"] for b in range(n)], np.int32)
        skip0 = np.stack([_pad(sw["older"][j][b]["skip0"]) for b in range(n)])
        args.append(dict(idx0=idx0, idx1=idx1, cams=cams, skip0=skip0, T0=[sc["T0"] for sc in sw["current"]],
                         T1=[sc["T1"] for sc in sw["current"]]))
    return blocks0, blocks1, matched1, args


def _check_sweep(sw, chain, final, rows, claimed, n_claimed, matched1, fill):
    """rows [step][pair][K][REC] uint8, claimed [step][pair][K], n_claimed [step][pair], matched1 [block][K]"""
    for j, step in enumerate(chain):
        for b, res in enumerate(step):
            n0 = len(res["rows"])
            _same_rows(rows[j][b, :n0].reshape(-1).view(capi.MOTION_MATCH_DTYPE), res["rows"], ("step", j, "pair", b),
                       sw["current"][b])
            assert np.all(rows[j][b, n0:] == fill) and np.all(claimed[j][b, n0:] == fill), (j, b)
            assert np.array_equal(claimed[j][b, :n0], res["claimed"]), (j, b)
            assert int(n_claimed[j][b]) == res["n_claimed"], (j, b)
    for b, m in enumerate(final):
        assert np.array_equal(matched1[b], _pad(m)), b


def test_sweep_queued_on_one_stream(oracle):
    fe = _frontend(0)
    sw = sweep()
    chain, final = R.sweep_chain(sw, sweep_camera)
    blocks0, blocks1, matched1, args = _sweep_arrays(sw)
    n, steps = len(sw["current"]), len(args)
    assert (n, steps) == (8, 3)
    d_b0, d_b1, d_m = _dev(blocks0), _dev(blocks1), _dev(matched1)
    d_skip = [_dev(a["skip0"]) for a in args]
    d_rows = [_filled(n, K, REC) for _ in range(steps)]
    d_claimed = [_filled(n, K) for _ in range(steps)]
    d_n = [torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(steps)]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    for j, a in enumerate(args):  # queued back to back; matched1 updated in place
        fe.match_motion_stereo_blocks_batch_device(
            d_b0.data_ptr(), len(blocks0), d_b1.data_ptr(), n, a["idx0"], a["idx1"], a["cams"], a["T0"], a["T1"],
            d_skip[j].data_ptr(), d_m.data_ptr(), d_rows[j].data_ptr(),
            claim=dict(claimed=d_claimed[j].data_ptr(), n_claimed=d_n[j].data_ptr(), matched1_out=d_m.data_ptr()),
            stream=stream)
    stream.synchronize()  # the only synchronisation
    _check_sweep(sw, chain, final, [t.cpu().numpy() for t in d_rows], [t.cpu().numpy() for t in d_claimed],
                 [t.cpu().numpy() for t in d_n], d_m.cpu().numpy(), FILL)


def test_cpp_sweep(oracle, tmp_path):
    """HipFrontend::matchMotionStereoSweep on the same data: a context per camera, each of its camera's own frame size,
    so the reference chain runs with the cameras as they are"""
    sw = sweep()
    chain, final = R.sweep_chain(sw)
    blocks0, blocks1, matched1, args = _sweep_arrays(sw)
    n, steps = len(sw["current"]), len(args)
    cli = tmp_path / "motion_sweep_cli"
    lib_dir = os.path.join(ROOT, "okvis2_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-o", str(cli),
                           os.path.join(ROOT, "tests", "cpp", "motion_sweep_cli.cpp"), "-L" + lib_dir, "-lokvfe",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    req, resp = tmp_path / "req.bin", tmp_path / "resp.bin"
    with open(req, "wb") as f:
        f.write(struct.pack("<i", sw["n_cams"]))
        for cam in CAMS[:sw["n_cams"]]:
            f.write(struct.pack("<iii", cam.w, cam.h, cam.dist_type))
            f.write(struct.pack("<8d", cam.fu, cam.fv, cam.cu, cam.cv, *cam.d[:4]))
        f.write(struct.pack("<ii", K, S.THRESHOLD))
        f.write(struct.pack("<iiiii", len(blocks0), n, blocks0.shape[1], steps, n))
        f.write(blocks0.tobytes())
        f.write(blocks1.tobytes())
        f.write(matched1.tobytes())
        pose = lambda T: np.concatenate([np.asarray(T[0]).reshape(-1), np.asarray(T[1])]).astype(np.float64).tobytes()
        for a in args:
            f.write(a["idx0"].tobytes() + a["idx1"].tobytes() + a["cams"].tobytes())
            f.write(b"".join(pose(T) for T in a["T0"]) + b"".join(pose(T) for T in a["T1"]))
            f.write(a["skip0"].tobytes())
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = lib_dir + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = subprocess.run([str(cli), str(req), str(resp)], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = np.fromfile(resp, dtype=np.uint8)
    per_step = n * K * REC + n * K + n * 4
    assert len(raw) == steps * per_step + n * K + 4
    rows, claimed, n_claimed = [], [], []
    for j in range(steps):
        part = raw[j * per_step:(j + 1) * per_step]
        rows.append(part[:n * K * REC].reshape(n, K, REC))
        claimed.append(part[n * K * REC:n * K * REC + n * K].reshape(n, K))
        n_claimed.append(part[n * K * REC + n * K:].copy().view(np.int32))
    m_after = raw[steps * per_step:steps * per_step + n * K].reshape(n, K)
    _check_sweep(sw, chain, final, rows, claimed, n_claimed, m_after, 0xF9)
    assert raw[-4:].copy().view(np.int32)[0] == 1  # a current block named twice made the sweep throw


def _raw_call(fe, **kw):
    """the entry point through ctypes with every argument explicit (None = NULL) -> (status, message)"""
    fn = capi.lib().okvfe_match_motion_stereo_blocks_batch_device
    p = lambda v: None if v is None else ctypes.c_void_p(int(v))
    st = fn(fe._h, p(kw["b0"]), kw["nb0"], p(kw["b1"]), kw["nb1"], kw["n"], capi._p(kw["idx0"]), capi._p(kw["idx1"]),
            capi._p(kw["cams"]), kw["T0"], kw["T1"], p(kw.get("skip0")), p(kw.get("matched1")), p(kw["out"]),
            kw.get("claim"), None)
    return st, capi.lib().okvfe_last_error(fe._h).decode()


def test_bad_arguments_are_rejected_before_any_launch(oracle):
    fe = _frontend(0)
    sc = _pool()[8]
    d_b0 = _dev(np.stack([_block(sc, "0")] * 2))
    d_b1 = _dev(np.stack([_block(sc, "1")] * 2))
    d_out, d_claimed = _filled(2, K, REC), _filled(2, K)
    d_n = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    P0 = (capi.Pose * 2)(capi.make_pose(*sc["T0"]), capi.make_pose(*sc["T0"]))
    P1 = (capi.Pose * 2)(capi.make_pose(*sc["T1"]), capi.make_pose(*sc["T1"]))
    claim = capi.MotionClaimDevice(d_claimed.data_ptr(), d_n.data_ptr(), None)
    i32 = lambda *v: np.array(v, np.int32)
    good = dict(b0=d_b0.data_ptr(), nb0=2, b1=d_b1.data_ptr(), nb1=2, n=2, idx0=i32(0, 1), idx1=i32(0, 1),
                cams=i32(0, 0), T0=P0, T1=P1, out=d_out.data_ptr(), claim=ctypes.byref(claim))
    INVALID = 1
    cases = [
        (dict(idx1=i32(1, 1)), ("current block 1", "pairs 0 and 1")),
        (dict(idx0=i32(0, 2)), ("pair 1", "older block 2")),
        (dict(idx1=i32(-1, 1)), ("pair 0", "current block -1")),
        (dict(b0=None), ("blocks0_dev",)),
        (dict(b1=None), ("blocks1_dev",)),
        (dict(cams=None), ("cam_ids",)),
        (dict(T0=None), ("T_WC0",)),
        (dict(T1=None), ("T_WC1",)),
        (dict(out=None), ("matches_dev",)),
        (dict(claim=ctypes.byref(capi.MotionClaimDevice(None, d_n.data_ptr(), None))), ("claimed",)),
        (dict(claim=ctypes.byref(capi.MotionClaimDevice(d_claimed.data_ptr(), None, None))), ("n_claimed",)),
        (dict(n=-1), ("negative",)),
        (dict(nb1=-2), ("negative",)),
        (dict(cams=i32(0, 4)), ("pair 1", "camera slot 4")),
        (dict(cams=i32(3, 0)), ("pair 0", "slot 3", "no intrinsics")),
    ]
    for change, words in cases:
        st, msg = _raw_call(fe, **dict(good, **change))
        assert st == INVALID, (change.keys(), st, msg)
        for w in words:
            assert w in msg, (w, msg)
    torch.cuda.synchronize()
    assert bool((d_out == FILL).all()) and bool((d_claimed == FILL).all()) and bool((d_n == -7).all())
    # n_pairs == 0 is fine and launches nothing, whatever else is passed
    st, msg = _raw_call(fe, **dict(good, n=0, cams=None, T0=None, T1=None))
    assert st == 0, msg
    torch.cuda.synchronize()
    assert bool((d_out == FILL).all()) and bool((d_n == -7).all())
    # the duplicate without claims: one frozen matched1 against two older frames
    st, msg = _raw_call(fe, **dict(good, idx1=i32(1, 1), claim=None))
    assert st == 0, msg
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    n0 = len(sc["kp0"])
    assert np.array_equal(got[0], got[1]) and np.all(got[0, n0:] == FILL)
    _same_rows(got[0, :n0].reshape(-1).view(capi.MOTION_MATCH_DTYPE), R.match_rows(sc, None, None, _oracle_cam(sc)),
               "duplicate without claims", sc)
    assert bool((d_claimed == FILL).all())


def test_claims_refuse_a_row_capacity_beyond_the_owner_table():
    big = capi.Frontend(128, 128, 10.0, 2, 50, 4096, match_threshold=S.THRESHOLD)  # four layers of 4096 rows each
    try:
        big.set_camera(0, R.with_frame_size(CAMS[0], 128, 128))
        Kb = big.max_keypoints
        assert Kb == 16384 > capi.MOTION_CLAIM_MAX_KEYPOINTS
        stride = big.gather_block_bytes()
        d_b = torch.zeros(stride, dtype=torch.uint8, device="cuda")  # one empty block on either side
        d_out, d_claimed = _filled(Kb, REC), _filled(Kb)
        d_n = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        T = (np.eye(3).reshape(-1), np.zeros(3))
        args = (d_b.data_ptr(), 1, d_b.data_ptr(), 1, None, None, [0], [T], [T], None, None, d_out.data_ptr())
        with pytest.raises(capi.OkvfeError) as e:
            big.match_motion_stereo_blocks_batch_device(
                *args, claim=dict(claimed=d_claimed.data_ptr(), n_claimed=d_n.data_ptr(), matched1_out=None))
        assert e.value.status == 4 and "12288" in str(e.value)  # OKVFE_ERR_UNSUPPORTED
        big.match_motion_stereo_blocks_batch_device(*args)  # matching alone has no such limit
        torch.cuda.synchronize()
        assert bool((d_out == FILL).all()) and bool((d_n == -7).all())
    finally:
        big.close()


def test_scale_space_context_equals_single_calls(oracle):
    """octaves = 2: mixed size classes, slots 0 and 1 with different fu -> one size-class table per slot"""
    fe = _frontend(2)
    pairs = [S.pair_scene("general", 200, 260, seed=31, mixed=True), S.pair_scene("tumvi", 150, 257, seed=32, mixed=True),
             S.pair_scene("euroc", 65, 100, seed=33, mixed=True)]
    blocks0, blocks1, idx0, idx1 = _layout(pairs)
    d_b0, d_b1 = _dev(blocks0), _dev(blocks1)
    stride = fe.gather_block_bytes()
    cams = [_slot(sc) for sc in pairs]
    assert cams == [0, 1, 0] and CAMS[0].fu != CAMS[1].fu
    d_out, d_one = _filled(3, K, REC), _filled(3, K, REC)
    fe.match_motion_stereo_blocks_batch_device(d_b0.data_ptr(), 3, d_b1.data_ptr(), 3, idx0, idx1, cams,
                                               [sc["T0"] for sc in pairs], [sc["T1"] for sc in pairs], None, None,
                                               d_out.data_ptr())
    for p, sc in enumerate(pairs):
        fe.match_motion_stereo_blocks_device(cams[p], d_b0.data_ptr() + int(idx0[p]) * stride,
                                             d_b1.data_ptr() + int(idx1[p]) * stride, None, None, sc["T0"], sc["T1"],
                                             d_one.data_ptr() + p * K * REC)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert np.array_equal(got, d_one.cpu().numpy())
    classes = set()
    for p, sc in enumerate(pairs):
        n0 = len(sc["kp0"])
        classes |= set(int(o) for o in sc["kp0"]["octave"])
        _same_rows(got[p, :n0].reshape(-1).view(capi.MOTION_MATCH_DTYPE), R.match_rows(sc, None, None, _oracle_cam(sc)),
                   (p, sc["name"]), sc)
    assert len(classes) >= 3
