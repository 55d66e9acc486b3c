"""Batches of the benchmark's size out of the scenes of the per-family scene modules: D distinct multiframes (with the
references of those D, computed once) replicated to N, in the modular order or in a fixed-seed shuffle that moves every
index; the device tensors of a family's `prepare` gathered to N multiframes on the device, every one with EXTRA records
behind the batch that no call may touch; and the comparison of N results with their D anchors on the device, as bytes.
Importing needs no GPU; the tensor helpers work on CPU tensors as well.  Test infrastructure only."""
import numpy as np

D = 16               # distinct multiframes of a scene
N_BENCH = 3072       # bench.py's default step, what every tools/bench_*.py reports
N = 16 * 192 + 5     # 3077: a ragged last round of work-groups, no power-of-two factor
EXTRA = 2            # records behind the batch in every tiled tensor
SHUFFLE_SEED = 20240607


def placements(n, d, seed=SHUFFLE_SEED):
    """(modular, shuffled): two orders of range(n).  Position i of a batch holds the multiframe order[i] of the modular
    batch, that is distinct order[i] % d.  The shuffle is a permutation without a fixed point."""
    modular = np.arange(n, dtype=np.int64)
    p = np.random.default_rng([seed, n, d]).permutation(n).astype(np.int64)
    for i in np.flatnonzero(p == modular):   # a fixed point swaps with its neighbour: neither stays (p is a permutation)
        j = (i + 1) % n
        if p[i] == i:                        # (unless the swap before this one has moved it already)
            p[i], p[j] = p[j], p[i]
    assert n < 2 or not np.any(p == modular)
    return modular, p


def tile(sc, n, refs=None, order=None, key="mfs"):
    """(the scene with sc[key][i] = distinct order[i] % D, i < n; the references in the same order, or None).  The
    entries are the distinct ones themselves, not copies: a reference is computed once per distinct multiframe."""
    d = len(sc[key])
    order = np.arange(n, dtype=np.int64) if order is None else np.asarray(order, dtype=np.int64)
    assert len(order) == n and (refs is None or len(refs) == d)
    index = order % d
    out = dict(sc)
    out[key] = [sc[key][int(k)] for k in index]
    out["tile"] = dict(d=d, n=n, index=index)
    return out, None if refs is None else [refs[int(k)] for k in index]


def _rows(t, n_rows):
    """the first n_rows records of t as bytes, [n_rows, bytes per record]"""
    import torch
    return t[:n_rows].contiguous().view(-1).view(torch.uint8).reshape(n_rows, -1) if n_rows else t[:0].reshape(0, 1)


def _first_true(bad, a, b_of):
    """bad [n] bool -> None, or (index, offset of the first byte at which a[index] and b_of(index) differ)"""
    if not bool(bad.any()):
        return None
    i = int(bad.nonzero()[0, 0])
    return i, int((a[i] != b_of(i)).nonzero()[0, 0])


def first_difference(t, d, n=None, per=1):
    """t: [n * per (+ records behind the batch), ...], `per` records per multiframe.  None, or (multiframe, byte offset
    within the multiframe's records) of the first multiframe whose bytes differ from those of its anchor, multiframe
    index % d.  Runs where t lives; NaNs compare as their bytes."""
    import torch
    n = t.shape[0] // per if n is None else n
    assert t.shape[0] >= n * per and n >= d
    b = _rows(t, n * per).reshape(n, -1)
    g = n // d
    body = (b[:g * d].reshape(g, d, -1) != b[:d]).any(dim=2).reshape(-1)
    tail = (b[g * d:] != b[:n - g * d]).any(dim=1)
    return _first_true(torch.cat([body, tail]), b, lambda i: b[i % d])


def first_misplaced(t, t_modular, order, per=1):
    """None, or (multiframe, byte offset) of the first multiframe i of t whose bytes differ from those of multiframe
    order[i] of t_modular"""
    import torch
    n = len(order)
    a, m = _rows(t, n * per).reshape(n, -1), _rows(t_modular, n * per).reshape(n, -1)
    idx = torch.as_tensor(np.asarray(order, dtype=np.int64), device=t.device)
    return _first_true((a != m[idx]).any(dim=1), a, lambda i: m[int(order[i])])


def tile_tensors(T, order, d, per_of, extra=EXTRA):
    """T: a family's prepared tensors over d distinct multiframes; per_of: key -> records per multiframe of the tensors
    that are per multiframe.  Returns (tiled, guard): every such tensor gathered on its device to len(order)
    multiframes, multiframe i a copy of distinct order[i] % d, followed by `extra` records that are copies of the
    tensor's first (in an output, the family's sentinel); every other entry of T as it is.  guard: key -> the bytes
    behind the batch, for `untouched`."""
    import torch
    out, guard = dict(T), {}
    for key, per in per_of.items():
        t = T.get(key)
        if t is None:
            continue
        assert t.shape[0] == d * per, (key, tuple(t.shape), d, per)
        idx = torch.as_tensor(np.asarray(order, dtype=np.int64) % d, device=t.device)
        # gathered as bytes: torch indexes no uint64 tensor on the device
        raw = t.contiguous().reshape(d, -1).view(torch.uint8)
        raw = torch.cat([raw[idx].reshape(len(order) * per, -1), raw[:1].reshape(per, -1)[:1].expand(extra, -1)])
        out[key] = raw.contiguous().view(t.dtype).reshape((len(order) * per + extra,) + tuple(t.shape[1:]))
        guard[key] = out[key][len(order) * per:].clone()
    return out, guard


def untouched(T, guard):
    """the keys whose records behind the batch no longer hold what tile_tensors put there (NaNs as bytes)"""
    import torch
    bad = []
    for key, g in guard.items():
        now = T[key][T[key].shape[0] - g.shape[0]:]
        if not torch.equal(_rows(now, now.shape[0]), _rows(g, g.shape[0])):
            bad.append(key)
    return bad


def anchors(T, d, per_of):
    """T with every tiled tensor cut to its first d multiframes (views): what a family's `check` takes with the scene
    of the d distinct multiframes"""
    return {k: (v[:d * per_of[k]] if k in per_of and v is not None else v) for k, v in T.items()}


def snapshot(T, keys):
    return {k: T[k].clone() for k in keys if T.get(k) is not None}


def changed(T, snap):
    """the keys whose bytes differ from the snapshot's"""
    import torch
    return [k for k, v in snap.items() if not torch.equal(_rows(T[k], T[k].shape[0]), _rows(v, v.shape[0]))]
