"""Scenes for okvfe_imu_propagation and okvfe_imu_propagation_blocks_device: ragged batches of IMU sample lists (2 to 40
samples at 200 Hz with jitter, one empty list per scene) with the propagation's every branch in them, for rigs of 1, 2 and
5 cameras with the extrinsics of ransac_scenes.rig; the packing into the calls' layout; and the references, computed once
per order of okvfe_set_fp64_reduction.  Importing needs no GPU.  Test infrastructure only.

KINDS lists what a multiframe is built to reach.  The knife edges are pairs of ADJACENT doubles: gyro rates and
accelerations at g_max / a_max and the next double above; rates bisected so that theta_half lies on either side of 1.0e-6
and of pi / 4, and Phi on either side of 1.0e-4 and of pi / 4, in the restatement's own arithmetic."""
import functools

import numpy as np

import elementary_ref as E
import imu_ref as R
import ransac_scenes as S
from place_hessian_scenes import pose7

PARAMS = dict(a_max=176.0, g_max=7.8, sigma_g_c=12.0e-4, sigma_a_c=8.0e-3, sigma_gw_c=4.0e-6, sigma_aw_c=4.0e-5, g=9.81007)
RIGS = (("euroc",), ("euroc", "euroc1"), "hilti")
KINDS = ("general", "start_on_sample", "end_past_last", "duplicate_timestamp", "decreasing_timestamp", "end_equals_start",
         "end_before_start", "front_after_start", "gyro_at_g_max", "acc_at_a_max", "theta_half_at_1e-6", "phi_at_1e-4",
         "theta_half_at_pi_4", "phi_at_pi_4", "beyond_pi_4", "zero_rate", "nan_sample", "two_samples", "forty_samples",
         "empty")
EDGE_KINDS = ("gyro_at_g_max", "acc_at_a_max", "theta_half_at_1e-6", "phi_at_1e-4", "theta_half_at_pi_4", "phi_at_pi_4")
PER_KIND = 6                 # multiframes of a kind per scene: 18 over the three rigs; an edge kind alternates its two sides
SENTINEL = -4321.0
DT_NS = 5000000              # 200 Hz


def stamp(ns):
    """nanoseconds since the epoch -> (sec, nsec) uint32"""
    return np.array([ns // 1000000000, ns % 1000000000], dtype=np.uint32)


def bisect(pred, lo, hi):
    """adjacent doubles (a, b = nextafter(a)) with pred(a) and not pred(b); pred(lo) and not pred(hi) to begin with"""
    lo, hi = np.float64(lo), np.float64(hi)
    assert pred(lo) and not pred(hi)
    while np.nextafter(lo, np.inf) != hi:
        mid = lo + 0.5 * (hi - lo)
        if pred(mid):
            lo = mid
        else:
            hi = mid
    return lo, hi


def _theta_half(s, dt):
    """theta_half of an interval whose two rates are (s, 0, 0), with zero bias: the same in both reduction orders"""
    w = 0.5 * (np.float64(s) + np.float64(s)) - 0.0
    return (np.sqrt(w * w + 0.0 * 0.0 + 0.0 * 0.0) * 0.5) * dt


def _phi(s, dt):
    w = (0.5 * (np.float64(s) + np.float64(s)) - 0.0) * dt
    return np.sqrt(w * w + 0.0 * 0.0 + 0.0 * 0.0)


@functools.lru_cache(maxsize=None)
def edges():
    """kind -> the two adjacent rates (or the two adjacent sample values) on either side of its edge"""
    dt = R.time_diff(stamp(DT_NS), stamp(0))
    g, a = np.float64(PARAMS["g_max"]), np.float64(PARAMS["a_max"])
    return {
        "gyro_at_g_max": (g, np.nextafter(g, np.inf)),
        "acc_at_a_max": (a, np.nextafter(a, np.inf)),
        "theta_half_at_1e-6": bisect(lambda s: not _theta_half(s, dt) > E.SINC_EDGE, 1e-4, 1e-3),
        "phi_at_1e-4": bisect(lambda s: _phi(s, dt) < 1.0e-4, 1e-2, 3e-2),
        "theta_half_at_pi_4": bisect(lambda s: _theta_half(s, dt) <= E.PI_4, 300.0, 330.0),
        "phi_at_pi_4": bisect(lambda s: _phi(s, dt) <= E.PI_4, 150.0, 165.0),
    }


def _rotation_q(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def multiframe(kind, index, rng, n=None):
    """one multiframe of a kind: dict(kind, side, ts [n, 2] uint32, gyro, acc [n, 3], t_start, t_end, T_WS [7], sb [9]);
    n: the number of samples of a "general" multiframe (2 .. 40), else the kind's own"""
    n = {"two_samples": 2, "forty_samples": 40, "empty": 0}.get(kind, int(rng.integers(4, 41)) if n is None else n)
    edge = kind in EDGE_KINDS
    # 200 Hz with 0.2 ms of jitter; every third list crosses a full second
    t0 = 1403636580 * 1000000000 + (int(rng.integers(0, 900000000)) if index % 3 else 1000000000 - 2 * DT_NS - 17)
    step = np.full(max(n, 1), DT_NS, dtype=np.int64)
    if not edge:
        step = step + rng.integers(-200000, 200001, size=len(step))
    ns = t0 + np.concatenate([[0], np.cumsum(step)])[:n] if n else np.zeros(0, np.int64)
    gyro = rng.normal(0.0, 0.3, size=(n, 3))
    acc = rng.normal(0.0, 1.5, size=(n, 3)) + np.array([0.0, 0.0, 9.81])
    T_WS = np.concatenate([rng.normal(0.0, 2.0, size=3), _rotation_q(rng)])
    sb = np.concatenate([rng.normal(0.0, 1.0, size=3), rng.normal(0.0, 0.01, size=3), rng.normal(0.0, 0.05, size=3)])
    side = index % 2
    mid = lambda a, b: int(a + (b - a) * rng.uniform(0.2, 0.8))
    if n >= 2:
        start = mid(ns[0], ns[1]) if index % 4 else int(ns[0])
        last = int(rng.integers(max(1, n // 2), n))               # the sample at or after which the propagation ends
        end = int(ns[last]) if index % 3 == 1 else mid(ns[last - 1], ns[last])
        end = max(end, start + 1)
    else:
        start, end = t0, t0 + DT_NS
    if kind == "start_on_sample":
        k = int(rng.integers(1, max(2, n // 2)))
        start, end = int(ns[k]), int(ns[n - 1])
    elif kind == "end_past_last":
        end = int(ns[n - 1]) + int(rng.integers(1, DT_NS))
    elif kind in ("duplicate_timestamp", "decreasing_timestamp"):
        j = int(rng.integers(1, n - 2))
        ns[j + 1] = ns[j] if kind == "duplicate_timestamp" else ns[j] - int(rng.integers(1, DT_NS // 2))
        ns[n - 1] = max(ns[n - 1], ns[j] + DT_NS)                  # (the end stays within the list)
        start, end = int(ns[0]), int(ns[n - 1])
    elif kind == "end_equals_start":
        end = start
    elif kind == "end_before_start":
        start = mid(ns[1], ns[2])
        end = mid(ns[0], ns[1])
    elif kind == "front_after_start":
        start = int(ns[0]) - int(rng.integers(1, DT_NS))
    elif kind == "beyond_pi_4":
        gyro[int(rng.integers(1, n - 1))] = rng.choice([-1.0, 1.0], size=3) * rng.uniform(250.0, 400.0, size=3)
        start, end = int(ns[0]), int(ns[n - 1])
    elif kind == "zero_rate":
        gyro[:] = sb[3:6]
        if index % 2:
            gyro[:], sb[3:6] = 0.0, 0.0
    elif kind == "nan_sample":
        (gyro if index % 2 else acc)[int(rng.integers(1, n - 1)), int(rng.integers(0, 3))] = np.nan
        start, end = int(ns[0]), int(ns[n - 1])
    elif edge:
        lo_hi = edges()[kind]
        start, end = int(ns[0]), int(ns[n - 1])
        if kind in ("gyro_at_g_max", "acc_at_a_max"):
            # a sample in the middle is read raw: as omega_S_1 of one interval and omega_S_0 of the next
            v = (gyro if kind == "gyro_at_g_max" else acc)
            np.clip(v, -5.0, 5.0, out=v)
            v[int(rng.integers(1, n - 1)), int(rng.integers(0, 3))] = lo_hi[side] * (1.0 if index % 4 < 2 else -1.0)
        else:
            gyro[:] = np.array([lo_hi[side], 0.0, 0.0])
            sb[3:6] = 0.0
    return dict(kind=kind, side=side if edge else None, ts=np.stack([stamp(int(v)) for v in ns]) if n else
                np.zeros((0, 2), np.uint32), gyro=gyro, acc=acc, t_start=stamp(start), t_end=stamp(end), T_WS=T_WS, sb=sb)


@functools.lru_cache(maxsize=None)
def scenes():
    """one scene per rig: dict(name, T_SC_params [n_cams, 7], mfs)"""
    out = []
    for r, spec in enumerate(RIGS):
        T_SC = S.rig(spec)[1]
        rng = np.random.default_rng([77, r])
        mfs = [multiframe(kind, PER_KIND * r + i, rng) for i in range(PER_KIND) for kind in KINDS]
        out.append(dict(name="rig-" + S.spec_id(spec), T_SC_params=np.array([pose7((np.asarray(C).reshape(3, 3), t))
                                                                              for C, t in T_SC]), mfs=mfs))
    return out


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """one batch with every sample count from 2 to 40 and, in between, a multiframe that ends past its last sample
    (n_propagated = -1), one with t_end == t_start and one with an interval beyond pi / 4; on the two-camera rig"""
    rng = np.random.default_rng(99)
    mfs = [multiframe("general", n, rng, n=n) for n in range(2, 41)]
    for at, kind in ((5, "end_past_last"), (17, "end_equals_start"), (30, "beyond_pi_4")):
        mfs.insert(at, multiframe(kind, at, rng))
    return dict(name="mixed", T_SC_params=scenes()[1]["T_SC_params"], mfs=mfs)


DISTINCT_KINDS = ("general", "forty_samples", "end_past_last", "general", "end_equals_start", "beyond_pi_4", "two_samples",
                  "nan_sample", "general", "front_after_start", "empty", "duplicate_timestamp", "general", "zero_rate",
                  "start_on_sample", "gyro_at_g_max")


@functools.lru_cache(maxsize=None)
def distinct_batch():
    """the 16 distinct multiframes that batch_scale.tile replicates to the benchmark's size; on the two-camera rig"""
    rng = np.random.default_rng(16)
    return dict(name="distinct", T_SC_params=scenes()[1]["T_SC_params"],
                mfs=[multiframe(kind, i, rng) for i, kind in enumerate(DISTINCT_KINDS)])


def reference_one(tree, mf, T_SC_params=(), libm=False, census=None):
    return R.propagation(tree, PARAMS, mf["ts"], mf["gyro"], mf["acc"], mf["t_start"], mf["t_end"], mf["T_WS"], mf["sb"],
                         T_SC_params=T_SC_params, libm=libm, census=census)


@functools.lru_cache(maxsize=None)
def references(tree):
    """per scene the list of per-multiframe references (Jacobian and covariance included), and the census over all"""
    census = R.new_census()
    return [[reference_one(tree, mf, sc["T_SC_params"], census=census) for mf in sc["mfs"]] for sc in scenes()], census


# ---- the calls' layout ------------------------------------------------------------------------------------------------
def stamp_double(t):
    """(sec, nsec) in the eight bytes of a double: sec in the low word"""
    return np.array([int(t[0]) | (int(t[1]) << 32)], dtype=np.uint64).view(np.float64)[0]


def pack(mfs):
    """-> (samples [total, 8] float64, sample_begin [n + 1] int32, states [n, 18] float64)"""
    begin = np.zeros(len(mfs) + 1, np.int32)
    begin[1:] = np.cumsum([len(mf["ts"]) for mf in mfs])
    samples = np.zeros((max(int(begin[-1]), 1), 8))
    states = np.zeros((len(mfs), 18))
    for m, mf in enumerate(mfs):
        rows = samples[begin[m]:begin[m + 1]]
        rows[:, 0] = [stamp_double(t) for t in mf["ts"]]
        rows[:, 1:4], rows[:, 4:7] = mf["gyro"], mf["acc"]
        states[m, 0], states[m, 1] = stamp_double(mf["t_start"]), stamp_double(mf["t_end"])
        states[m, 2:9], states[m, 9:18] = mf["T_WS"], mf["sb"]
    return samples, begin, states


OUTPUTS = dict(pose=(7, np.float64), speed_and_bias=(9, np.float64), n_propagated=(1, np.int32), status=(1, np.int32),
               n_out_of_range=(1, np.int32), jacobian=(225, np.float64), covariance=(225, np.float64))


def expected(refs, n_cams, mean_only=False, jacobian=True, covariance=True):
    """what a call leaves in outputs that held SENTINEL everywhere: name -> array [n, ...] (T_WC and gravity_C per
    camera); an output the call leaves alone keeps the sentinel"""
    n = len(refs)
    out = {k: np.full((n, w), SENTINEL, dtype=t) for k, (w, t) in OUTPUTS.items()}
    out["T_WC"] = np.full((n, n_cams, 7), SENTINEL)
    out["gravity_C"] = np.full((n, n_cams, 3), SENTINEL, dtype=np.float32)
    for m, r in enumerate(refs):
        out["status"][m], out["n_out_of_range"][m] = r["status"], r["n_out_of_range"]
        if r["pose"] is None:
            continue
        out["n_propagated"][m] = r["n_propagated"]
        out["pose"][m], out["speed_and_bias"][m] = r["pose"], r["speed_and_bias"]
        out["T_WC"][m], out["gravity_C"][m] = r["T_WC"][:n_cams], r["gravity_C"][:n_cams]
        if r["jacobian"] is not None:
            out["jacobian"][m] = r["jacobian"].reshape(-1)
        if r["covariance"] is not None:
            out["covariance"][m] = r["covariance"].reshape(-1)
    if mean_only or not jacobian:
        out["jacobian"][:] = SENTINEL
    if mean_only or not covariance:
        out["covariance"][:] = SENTINEL
    return out


def same_bytes(a, b):
    """equal as bytes, any NaN standing for any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        canon = lambda v: np.where(np.isnan(v), v.dtype.type(np.nan), v).view(u)
        return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(canon(a), canon(b))
    return a.shape == b.shape and np.array_equal(a, b)


# ---- the request and response files of tests/cpp/imu_propagation_main.cpp and imu_propagation_cli.cpp ------------------
MAGIC = 0x494D5531


def write_request(path, mfs, T_SC_params, tree, jacobian=True, covariance=True):
    samples, begin, states = pack(mfs)
    n, n_cams = len(mfs), len(T_SC_params)
    n_begin = (n + 2) & ~1
    b = np.zeros(n_begin, np.int32)
    b[:n + 1] = begin
    total = int(begin[-1])
    head = np.array([MAGIC, n, n_cams, int(bool(tree)), int(jacobian), int(covariance), total, 0], np.int32)
    with open(path, "wb") as f:
        for a in (head, np.array([PARAMS[k] for k in R.PARAM_NAMES]), np.asarray(T_SC_params, np.float64), b,
                  samples[:total], states):
            f.write(np.ascontiguousarray(a).tobytes())


def read_response(path, n, n_cams):
    raw = open(path, "rb").read()
    n_begin = (n + 2) & ~1
    out, at = {}, 0

    def take(name, count, dtype, shape):
        nonlocal at
        size = count * np.dtype(dtype).itemsize
        out[name] = np.frombuffer(raw[at:at + size], dtype).reshape(shape).copy()
        at += size

    take("pose", 7 * n, np.float64, (n, 7))
    take("speed_and_bias", 9 * n, np.float64, (n, 9))
    for name in ("n_propagated", "status", "n_out_of_range"):
        take(name, n_begin, np.int32, (n_begin, 1))
        out[name] = out[name][:n]
    take("jacobian", 225 * n, np.float64, (n, 225))
    take("covariance", 225 * n, np.float64, (n, 225))
    take("T_WC", 7 * n * n_cams, np.float64, (n, n_cams, 7))
    take("gravity_C", 3 * n * n_cams, np.float32, (n, n_cams, 3))
    assert at == len(raw), (at, len(raw))
    return out
