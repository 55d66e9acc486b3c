"""CPU: the reference side of okvfe_match_motion_stereo_blocks_batch_device (tests/motion_claim_ref.py) and the
surface the call adds.

 - the closed form the claim kernel computes (per free k1 the smallest candidate k0) equals the literal sequential
   transcription of Frontend.cpp:1915-1958 on random candidate sets;
 - the scenes the GPU tests run hold what they are meant to exercise, on the oracle alone: contested and uncontested
   k1, rows the 4 px check rejected, and a sweep whose later steps depend on the earlier ones' claims;
 - include/okvfe.h declares the entry point, libokvfe.so exports it, and it rejects a NULL context;
 - the C++ mirror's two methods compile."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import motion_claim_ref as R
from okvis2_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "okvfe_match_motion_stereo_blocks_batch_device"

# (kind, keyword arguments of contested_scene, reaches the 4 px rejection?) -- shared with test_gpu_motion_batch.py
CLAIM_SPECS = (
    ("euroc", dict(seed=11), False),
    ("euroc", dict(seed=11, mixed=True), True),
    ("near", dict(seed=11, mixed=True), True),
    ("base0101", dict(seed=11, mixed=True), False),
    ("tumvi", dict(seed=11), False),
)


def _random_rows(rng, n0, n1, p_match, p_accept, spread):
    rows = np.zeros(n0, dtype=capi.MOTION_MATCH_DTYPE)
    k1 = rng.integers(0, max(1, int(n1 * spread)), n0)
    rows["k1"] = np.where(rng.random(n0) < p_match, k1, -1)
    rows["accepted"] = ((rng.random(n0) < p_accept) & (rows["k1"] >= 0)).astype(np.int32)
    return rows


def test_closed_form_equals_the_sequential_loop():
    rng = np.random.default_rng(2024)
    seen = dict(all_contested=0, none_contested=0, all_taken=0, no_flags=0, empty=0)
    for t in range(200):
        n0, n1 = int(rng.integers(0, 90)), int(rng.integers(1, 90))
        kind = t % 8
        if kind == 0:    # all contested: every candidate aims at one of two k1
            rows = _random_rows(rng, max(n0, 4), n1, 1.0, 1.0, 0.0)
            rows["k1"] = rng.integers(0, min(2, n1), len(rows))
            matched1 = np.zeros(n1, np.uint8)
            seen["all_contested"] += 1
        elif kind == 1:  # none contested: distinct k1
            n0 = min(n0, n1)
            rows = _random_rows(rng, n0, n1, 1.0, 1.0, 1.0)
            rows["k1"] = rng.permutation(n1)[:n0]
            matched1 = (rng.random(n1) < 0.2).astype(np.uint8)
            seen["none_contested"] += 1
        elif kind == 2:  # all taken
            rows = _random_rows(rng, n0, n1, 0.9, 0.9, 1.0)
            matched1 = np.ones(n1, np.uint8)
            seen["all_taken"] += 1
        elif kind == 3:  # matched1 absent: every k1 free
            rows = _random_rows(rng, n0, n1, 0.8, 0.8, 0.4)
            matched1 = None
            seen["no_flags"] += 1
        else:
            rows = _random_rows(rng, n0, n1, rng.random(), rng.random(), rng.uniform(0.1, 1.0))
            matched1 = (rng.random(n1) < rng.random()).astype(np.uint8)
        seen["empty"] += len(rows) == 0
        count0 = len(rows)
        a, na, ma = R.claim_loop(rows, count0, matched1)
        b, nb, mb = R.claim_closed(rows, count0, matched1)
        assert np.array_equal(a, b) and na == nb == int(a.sum()), t
        assert (ma is None and mb is None) or np.array_equal(ma, mb), t
        if kind == 0:
            assert na == len(np.unique(rows["k1"])), t
        if kind == 1:
            assert na == int((matched1[rows["k1"]] == 0).sum()), t
        if kind == 2:
            assert na == 0 and np.array_equal(ma, matched1), t
        # winners: distinct free k1, each the smallest k0 of its k1
        win = np.flatnonzero(a)
        assert len(np.unique(rows["k1"][win])) == len(win), t
    assert min(seen["all_contested"], seen["none_contested"], seen["all_taken"], seen["no_flags"]) >= 25, seen


@pytest.mark.parametrize("spec", CLAIM_SPECS, ids=lambda s: s[0] + ("-mixed" if s[1].get("mixed") else ""))
def test_contested_scenes_meet_their_floors(oracle, spec):
    kind, kw, rejecting = spec
    sc = R.contested_scene(kind, 300, 300, **kw)
    for matched1 in (sc["matched1"], None):
        rows = R.match_rows(sc, sc["skip0"], matched1)
        contested, single, rejected = R.contest_stats(rows, matched1)
        print(sc["name"], "flags" if matched1 is not None else "no flags", contested, single, rejected)
        assert contested >= 32, (sc["name"], contested)
        assert single >= 32, (sc["name"], single)
        if rejecting:
            assert rejected >= 16, (sc["name"], rejected)
        claimed, n, _ = R.claim_loop(rows, len(rows), matched1)
        assert n == contested + single  # one winner per free k1 that has a candidate


def sweep():
    cams = [synth.euroc_config().cams[0], synth.tumvi1024_config().cams[0]]
    return R.sweep_scene(cams, ("euroc", "tumvi"))


def sweep_camera(sc):
    """the oracle's camera of a sweep scene: the GPU tests run the sweep in one 1024 x 1024 context"""
    return R.with_frame_size(sc["cam"], 1024, 1024)


def test_sweep_steps_depend_on_the_earlier_claims(oracle):
    sw = sweep()
    assert len(sw["current"]) == 8 and len(sw["older"]) == 3
    steps, final = R.sweep_chain(sw, sweep_camera)
    for j in (1, 2):
        changed = 0
        for b, res in enumerate(steps[j]):
            sc, old = sw["current"][b], sw["older"][j][b]
            pair = dict(sc, **{k: old[k] for k in ("d0", "kp0", "bp0", "bv0")})
            frozen = R.match_rows(pair, old["skip0"], sw["matched1"][b], sweep_camera(sc))
            a = frozen.view(np.uint8).reshape(len(frozen), -1)
            c = res["rows"].view(np.uint8).reshape(len(frozen), -1)
            changed += int((a != c).any(axis=1).sum())
        print("step", j + 1, "rows that differ from the frozen-flags rows:", changed)
        assert changed >= 16, (j, changed)
    for b in range(8):
        n = sum(int(steps[j][b]["n_claimed"]) for j in range(3))
        assert int(final[b].sum()) == int(sw["matched1"][b].sum()) + n and n > 0, b


def test_header_declares_and_library_exports_the_entry_point():
    header = open(os.path.join(ROOT, "include", "okvfe.h")).read()
    assert re.search(r"okvfe_status\s+" + SYMBOL + r"\s*\(", header)
    assert "typedef struct okvfe_motion_claim_device" in header
    assert re.search(r"#define OKVFE_ABI_VERSION 8\b", header)  # symbols are only added
    assert SYMBOL in capi.EXPORTS
    lib = capi.lib()
    fn = getattr(lib, SYMBOL)  # AttributeError: the library does not export it
    fn.restype = ctypes.c_int32
    V = ctypes.c_void_p
    fn.argtypes = [V, V, ctypes.c_int32, V, ctypes.c_int32, ctypes.c_int32, V, V, V, V, V, V, V, V, V, V]
    assert fn(None, None, 0, None, 0, 0, None, None, None, None, None, None, None, None, None, None) == 1
    assert capi.MOTION_CLAIM_MAX_KEYPOINTS == 12288
    assert ctypes.sizeof(capi.MotionClaimDevice) == 3 * ctypes.sizeof(V)


_USER = r"""
#include "okvis2_amd/host/okvfe_frontend.hpp"
void user(okvfe::HipFrontend& f, const void* b, okvfe_motion_match* m, uint8_t* matched1,
          const std::vector<okvfe::HipFrontend::MotionSweepStep>& steps) {
  f.matchMotionStereoBlocks(0, b, 2, b, 2, {0, 1}, {1, 0}, std::vector<okvfe_pose>(2), std::vector<okvfe_pose>(2), nullptr, matched1, m);
  f.matchMotionStereoSweep(0, b, 2, b, 2, steps, matched1, nullptr);
}
"""


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "user.cpp"
    src.write_text(_USER)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + ROOT, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
