#!/usr/bin/env python3
"""What the place-recognition query costs on device-resident batches: okvfe_bow_vectors_blocks_device +
okvfe_place_query_blocks_device (+ okvfe_bow_database_add_blocks_device), against the B = 1 host chain that was all there
was before them.

Workload: the shipped 9^3 vocabulary (tests/golden/small_voc_tree.npz); stereo multiframes of 2 x 700 keypoints whose
descriptors are vocabulary leaves with a few bits flipped (8 places of 300 leaves; 16 distinct multiframes repeated to
fill a batch); a database of E entries made the same way by the host chain; min_score 0.4, every entry suppressible.

Every (batch, database) pair is measured in ONE process of its own (a child of this one, under its own time limit),
variants alternating repetition by repetition; median and [p10, p90]; one JSON line per comparison.  Boxes differ by
several per cent: only same-run comparisons mean anything.
  (a) the three launches alone (vectors, query, add of every eighth multiframe), between device events on the stream
  (b) on the host clock, from gather blocks on the device (device) / descriptors on the host (baseline) to the
      candidates on the host:
      device    vectors + query on one stream, one synchronisation, n_candidates and the candidate rows downloaded
      baseline  per multiframe okvfe_fbrisk_transform + okvfe_bow_vector + okvfe_bow_query_l1 (each uploads its
                vocabulary / database and synchronises), the neighbour walk of Frontend.cpp:780-802 in numpy.
                Above 1024 multiframes it runs every sixth repetition only (it takes seconds); the line says how many.

    python tools/bench_place_query.py [--batches 1,256,3072] [--entries 240,2000] [--reps 30]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_map_table import band  # noqa: E402

MIN_SCORE = 0.4  # Frontend.cpp:802
CAP = 32


def vocabulary():
    t = np.load(os.path.join(ROOT, "tests", "golden", "small_voc_tree.npz"))
    parent, word, weight = t["parent"], t["word"].astype(np.int32), t["weight"]
    n = len(parent)
    order = np.argsort(parent[1:], kind="stable") + 1  # children in ascending id under ascending parents
    cb = np.zeros(n + 1, np.int32)
    np.add.at(cb, parent[1:] + 1, 1)
    cb = np.cumsum(cb).astype(np.int32)
    ww = np.zeros(int(word.max()) + 1)
    ww[word[word >= 0]] = weight[word >= 0]
    return dict(desc=np.ascontiguousarray(t["desc"], np.uint8), cb=cb, ci=order.astype(np.int32), word=word, ww=ww,
                weighting=int(t["weighting"]))


def walk_numpy(scores, min_score):
    """Frontend.cpp:780-802 with every entry suppressible -> (ids, scores) of the candidates"""
    idx = np.flatnonzero(scores != -1.0)
    s = scores[idx]
    larger = np.zeros(len(s), bool)
    for d in (1, 2):
        if len(s) > d:
            larger[d:] |= s[:-d] > s[d:]
            larger[:-d] |= s[d:] > s[:-d]
    keep = ~larger & (s > min_score)
    return idx[keep], s[keep]


def worker(M, E, args):
    import torch
    from okvis2_amd import capi, multigpu

    K, D = args.keypoints, args.distinct
    voc = vocabulary()
    capi.vocabulary_check(voc["desc"], voc["cb"], voc["ci"], voc["word"], voc["ww"], voc["weighting"], True)
    fe = capi.Frontend(752, 480, 38.0, 0, 150, K, max_batch=1, num_cameras=2)
    rng = np.random.default_rng(5)
    leaves = np.flatnonzero(voc["word"] >= 0)
    places = [rng.choice(leaves, 300, replace=False) for _ in range(8)]

    def view(p, n):
        d = voc["desc"][rng.choice(places[p], n)]
        return d ^ ((rng.random(d.shape) < 0.004) * rng.integers(1, 256, d.shape)).astype(np.uint8)

    def host_vector(feats):
        w, _ = fe.fbrisk_transform(feats, voc["desc"], voc["cb"], voc["ci"], voc["word"])
        return capi.bow_vector(w, voc["ww"], voc["weighting"], True)

    entries = [host_vector(view(e % 8, 2 * K)) for e in range(E)]
    begin = np.concatenate([[0], np.cumsum([len(e[0]) for e in entries])]).astype(np.int32)
    ids = np.concatenate([e[0] for e in entries]).astype(np.int32)
    vals = np.concatenate([e[1] for e in entries])
    feats = [[view(m % 8, K) for _ in range(2)] for m in range(D)]
    kp0, bp0, v0 = np.zeros(K, capi.KEYPOINT_DTYPE), np.zeros((K, 3)), np.zeros(K, np.uint8)
    blocks = np.stack([multigpu.pack_block_host(K, kp0, feats[m % D][c], bp0, v0) for m in range(M) for c in range(2)])
    host_feats = [np.concatenate(f) for f in feats]

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    zeros = lambda n, dt: torch.zeros(n, dtype=dt, device="cuda")
    n_add = max(1, M // 8)
    stride, nw = len(voc["ww"]), len(voc["ww"])
    words = int(begin[-1])
    db_begin = np.zeros(E + n_add + 1, np.int32)
    db_begin[:E + 1] = begin
    t = dict(blocks=dev(blocks), desc=dev(voc["desc"]), cb=dev(voc["cb"]), ci=dev(voc["ci"]), word=dev(voc["word"]),
             ww=dev(voc["ww"]), qn=zeros(M, torch.int32), qi=zeros(M * stride, torch.int32), qv=zeros(M * stride, torch.float64),
             begin=dev(db_begin), ids=zeros(words + n_add * stride, torch.int32), vals=zeros(words + n_add * stride, torch.float64),
             overflow=zeros(1, torch.int32), counts=zeros(2 * M, torch.int32), entry=zeros(M * CAP, torch.int32),
             score=zeros(M * CAP, torch.float64))
    t["ids"][:words] = dev(ids)
    t["vals"][:words] = dev(vals)
    p = lambda k: t[k].data_ptr()
    vd = capi.VocabularyDevice(len(voc["word"]), nw, voc["weighting"], 1, p("desc"), p("cb"), p("ci"), p("word"), p("ww"))
    vec = capi.BowVectorsDevice(p("qn"), p("qi"), p("qv"), stride, nw)
    dbd = capi.BowDatabaseDevice(p("begin"), p("ids"), p("vals"), E + n_add, words + n_add * stride, E, p("overflow"))
    cand = capi.PlaceCandidatesDevice(p("counts"), p("counts") + 4 * M, p("entry"), p("score"), CAP)
    stream = torch.cuda.Stream()
    pinned = dict(counts=torch.zeros(2 * M, dtype=torch.int32).pin_memory(), entry=torch.zeros(M * CAP, dtype=torch.int32).pin_memory(),
                  score=torch.zeros(M * CAP, dtype=torch.float64).pin_memory())
    add_index = list(range(0, M, 8))[:n_add]

    def vectors():
        fe.bow_vectors_blocks_device(vd, p("blocks"), M, 2, vec, stream=stream)

    def query():
        fe.place_query_blocks_device(dbd, vec, M, cand, min_score=MIN_SCORE, stream=stream)

    def add():
        dbd.n_entries = E  # (the same rows again every time)
        fe.bow_database_add_blocks_device(dbd, vec, M, add_index, stream=stream)
        dbd.n_entries = E

    def device_chain():
        vectors(), query()
        with torch.cuda.stream(stream):
            for k in pinned:
                pinned[k].copy_(t[k], non_blocking=True)
        stream.synchronize()
        n = pinned["counts"].numpy()[M:]
        rows = pinned["entry"].numpy().reshape(M, CAP)
        return [rows[m, :min(n[m], CAP)].copy() for m in range(M)], n.copy()

    def baseline_chain():
        out = []
        for m in range(M):
            qi, qv = host_vector(host_feats[m % D])
            s = fe.bow_query_l1(begin, ids, vals, qi, qv)
            out.append(walk_numpy(s, MIN_SCORE)[0])
        return out

    def by_events(fn):
        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            stream.synchronize()
            return e0.elapsed_time(e1) * 1e-3
        return run

    torch.cuda.synchronize()
    (cd, nd), cb = device_chain(), baseline_chain()
    equal = all(nd[m] == len(cb[m]) and np.array_equal(cd[m], cb[m][:CAP]) for m in range(M))
    ev = {k: [] for k in ("vectors", "query", "add")}
    fns = dict(vectors=by_events(vectors), query=by_events(query), add=by_events(add))
    for r in range(args.reps + 3):
        for k, f in fns.items():
            v = f()
            if r >= 3:
                ev[k].append(v)
    fe.bow_database_check_device(dbd, stream=stream)
    out = {k: band(v) for k, v in ev.items()}
    out.update(comparison=f"launch alone, M={M}, E={E}", reps=args.reps, keypoints=K, database_words=words, added=n_add,
               words_per_vector=round(float(t["qn"].float().mean().item()), 1))
    print(json.dumps(out), flush=True)
    every = 6 if M > 1024 else 1
    times = {"device": [], "baseline": []}
    device_chain()  # (the baseline ran above)
    for r in range(args.reps):
        for k, f in (("device", device_chain), ("baseline", baseline_chain)):
            if k == "baseline" and r % every:
                continue
            t0 = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t0)
    out = {k: band(v) for k, v in times.items()}
    out.update(comparison=f"to the candidates on the host, M={M}, E={E}", reps_device=len(times["device"]),
               reps_baseline=len(times["baseline"]),
               gain_ms=round(out["baseline"]["median_ms"] - out["device"]["median_ms"], 4),
               candidates_per_multiframe=round(float(nd.mean()), 2), candidates_equal=bool(equal))
    print(json.dumps(out), flush=True)
    fe.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", default="1,256,3072")
    ap.add_argument("--entries", default="240,2000")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--keypoints", type=int, default=700)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds per (batch, database) pair")
    ap.add_argument("--worker", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.reps < 30:
        ap.error("--reps: at least 30")
    if args.worker:
        M, E = (int(v) for v in args.worker.split(","))
        return worker(M, E, args)
    for M in [int(b) for b in args.batches.split(",")]:
        for E in [int(e) for e in args.entries.split(",")]:
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", f"{M},{E}", "--reps", str(args.reps), "--keypoints",
                   str(args.keypoints), "--distinct", str(args.distinct)]
            try:
                rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:  # nothing more is started on the device after a step that failed
                print(json.dumps(dict(comparison=f"M={M}, E={E}", error=f"the step ended with status {rc}")), flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
