"""GPU: the C++ host mirror (okvis2_amd/host/okvfe_frontend.hpp) of place recognition on batches -- uploadVocabulary,
allocBowVectors, createPlaceDatabase, bowVectorsBlocks, placeDatabaseAdd, placeQueryBlocks, placeDatabaseCheck -- driven
from a C++ program (tests/cpp/place_query_cli.cpp) on one stream: the one-camera rig scene of place_query_scenes.py on
the shipped vocabulary, equal to what the Python path is held to (place_query_ref.py): integers for equality, doubles as
uint64 patterns; rows the calls leave alone keep the driver's fill bytes."""
import os
import struct
import subprocess

import numpy as np
import pytest

import place_query_ref as R
import place_query_scenes as S
from okvis2_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "cpp", "place_query_cli")
K = 128
ADD = [0, 1, 2, 3, 4, 6, 8, 9]  # (4: the multiframe without a feature -- an empty entry)
CAP = 1
MIN_SCORE = 0.05


def write_request(path, cam, voc, blocks, suppressible):
    with open(path, "wb") as f:
        f.write(struct.pack("<iii", cam.w, cam.h, cam.dist_type))
        f.write(struct.pack("<8d", cam.fu, cam.fv, cam.cu, cam.cv, *cam.d[:4]))
        f.write(struct.pack("<i", K))
        f.write(struct.pack("<5i", len(voc["word"]), len(voc["ww"]), len(voc["ci"]), voc["weighting"], int(voc["normalise_l1"])))
        for k, dt in (("desc", np.uint8), ("cb", np.int32), ("ci", np.int32), ("word", np.int32), ("ww", np.float64)):
            f.write(np.ascontiguousarray(voc[k], dtype=dt).tobytes())
        f.write(struct.pack("<ii", blocks.shape[0], blocks.shape[1]))
        f.write(blocks.tobytes())
        f.write(struct.pack("<i", len(ADD)))
        f.write(np.array(ADD, np.int32).tobytes())
        f.write(struct.pack("<ii", CAP, int(suppressible is not None)))
        f.write(struct.pack("<d", MIN_SCORE))
        if suppressible is not None:
            f.write(np.asarray(suppressible, np.uint8).tobytes())


def cli_env():
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "okvis2_amd") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return env


@pytest.mark.parametrize("with_suppressible", [True, False], ids=["flags", "all-suppressible"])
def test_cpp_chain(oracle, tmp_path, with_suppressible):
    assert os.path.exists(CLI), "run __graft_entry__.build() first"
    voc = R.shipped_vocabulary(oracle)
    scene = S.rig_scene(oracle, voc, 1, K)
    refs = S.reference_vectors(oracle, voc, scene)
    blocks = S.pack_blocks(scene)
    supp = (np.arange(len(ADD)) % 2).astype(np.uint8) if with_suppressible else None
    req, resp = tmp_path / "req.bin", tmp_path / "resp.bin"
    write_request(req, synth.euroc_config().cams[0], voc, blocks, supp)
    out = subprocess.run([CLI, str(req), str(resp)], env=cli_env(), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(resp, "rb").read()
    stride = struct.unpack("<i", raw[:4])[0]
    assert stride == min(K, len(voc["ww"]))
    nf, na = len(refs), len(ADD)
    sizes = [nf * 4, nf * stride * 4, nf * stride * 8, nf * K * 4, (na + 1) * 4, nf * 8, nf * CAP * 4, nf * CAP * 8,
             nf * na * 8, 4, 4]
    assert len(raw) == 4 + sum(sizes)
    parts, o = [], 4
    for n in sizes:
        parts.append(raw[o:o + n])
        o += n
    I = lambda i, *shape: np.frombuffer(parts[i], np.int32).reshape(*shape)
    U = lambda i, *shape: np.frombuffer(parts[i], np.uint64).reshape(*shape)
    n, ids, vals, words = I(0, nf), I(1, nf, stride), U(2, nf, stride), I(3, nf, K)
    db = R.Database(len(voc["ww"]))
    for m in ADD:
        db.add(refs[m][1], refs[m][2])
    for m, (w, rid, rval) in enumerate(refs):
        assert n[m] == len(rid) and np.array_equal(ids[m, :n[m]], rid), m
        assert np.array_equal(vals[m, :n[m]], rval.view(np.uint64)), m
        assert np.all(ids[m, n[m]:] == S.FILL_I32) and np.all(vals[m, n[m]:] == S.FILL_U64), m
        assert np.array_equal(words[m, :len(w[0])], w[0]) and np.all(words[m, len(w[0]):] == S.FILL_I32), m
    assert np.array_equal(I(4, na + 1), db.arrays()[0])
    counts, entry, score, scores = I(5, 2, nf), I(6, nf, CAP), U(7, nf, CAP), U(8, nf, na)
    most = 0
    for m, (_, rid, rval) in enumerate(refs):
        ref = db.scores(oracle, rid, rval)
        assert np.array_equal(scores[m], ref.view(np.uint64)), m
        n_listed, cands = R.walk(ref, supp, MIN_SCORE)
        assert (counts[0, m], counts[1, m]) == (n_listed, len(cands)), m
        k = min(len(cands), CAP)
        assert entry[m, :k].tolist() == [c[0] for c in cands[:k]], m
        assert np.array_equal(score[m, :k], np.array([c[1] for c in cands[:k]]).view(np.uint64)), m
        assert np.all(entry[m, k:] == S.FILL_I32) and np.all(score[m, k:] == S.FILL_U64), m
        most = max(most, len(cands))
    assert most > CAP  # the true count above the stored rows
    assert struct.unpack("<i", parts[9])[0] == 1   # one entry too many: OKVFE_ERR_CAPACITY, nothing changed
    assert struct.unpack("<i", parts[10])[0] == 1  # a malformed vocabulary is refused before it is uploaded
