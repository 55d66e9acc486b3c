"""CPU: batch_scale.py held to its word on CPU tensors -- `tile` and `placements` are the permutations they claim, the
shuffle moves every index, `first_difference` and `first_misplaced` find one planted byte (in the last replica, in
replica 1, in an anchor, a NaN payload) and nothing in a clean tiling, the records behind a batch are watched."""
import numpy as np
import pytest

import batch_scale as BS

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("n,d", [(BS.N, BS.D), (BS.N_BENCH, BS.D), (3, 3), (17, 16), (35, 16)])
def test_placements_are_permutations_and_the_shuffle_moves_every_index(n, d):
    modular, shuffled = BS.placements(n, d)
    assert np.array_equal(modular, np.arange(n))
    assert np.array_equal(np.sort(shuffled), np.arange(n))
    assert not np.any(shuffled == np.arange(n))
    again = BS.placements(n, d)[1]
    assert np.array_equal(shuffled, again)                      # a fixed seed
    if n > 2 * d:
        assert np.mean(shuffled % d != np.arange(n) % d) > 0.8   # and most positions hold another distinct multiframe


def test_a_fixed_point_of_the_raw_shuffle_is_moved():
    # among these sizes the raw permutation has fixed points (seen on the CPU); none is left
    seen = 0
    for n in range(2, 60):
        raw = np.random.default_rng([BS.SHUFFLE_SEED, n, 4]).permutation(n)
        seen += int(np.any(raw == np.arange(n)))
        p = BS.placements(n, 4)[1]
        assert np.array_equal(np.sort(p), np.arange(n)) and not np.any(p == np.arange(n)), n
    assert seen > 10


def _scene(d):
    return dict(name="s", cams=[0, 1], mfs=[dict(id=i) for i in range(d)])


def test_tile_replicates_the_distinct_multiframes():
    sc = _scene(16)
    refs = [dict(ref=i) for i in range(16)]
    big, big_refs = BS.tile(sc, BS.N, refs)
    assert len(big["mfs"]) == BS.N == len(big_refs) and len(sc["mfs"]) == 16
    assert all(big["mfs"][i] is sc["mfs"][i % 16] and big_refs[i] is refs[i % 16] for i in range(BS.N))
    assert np.bincount(big["tile"]["index"]).tolist() == [193] * 5 + [192] * 11
    order = BS.placements(BS.N, 16)[1]
    shuf, shuf_refs = BS.tile(sc, BS.N, refs, order)
    assert all(shuf["mfs"][i] is big["mfs"][order[i]] and shuf_refs[i] is big_refs[order[i]] for i in range(BS.N))
    assert sorted(m["id"] for m in shuf["mfs"]) == sorted(m["id"] for m in big["mfs"])
    assert big["cams"] is sc["cams"] and BS.tile(sc, 5)[1] is None


def _tensors(d=16, per=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    return dict(blocks=torch.randint(0, 256, (d * per, 40), dtype=torch.uint8, generator=g),
                H=torch.rand((d, 6, 6), dtype=torch.float64, generator=g),
                count=torch.randint(0, 99, (d,), dtype=torch.int32, generator=g),
                out=torch.full((d * per, 5, 2), -12345.0, dtype=torch.float64), shared=torch.arange(7), none=None)


PER = dict(blocks=2, H=1, count=1, out=2, none=1)


@pytest.mark.parametrize("n", [16, 17, 35, BS.N])
def test_tile_tensors_and_a_clean_tiling(n):
    T = _tensors()
    order = BS.placements(n, 16)[0]
    big, guard = BS.tile_tensors(T, order, 16, PER)
    assert big["shared"] is T["shared"] and big["none"] is None and set(guard) == {"blocks", "H", "count", "out"}
    for key in guard:
        per = PER[key]
        assert big[key].shape[0] == n * per + BS.EXTRA and big[key].dtype == T[key].dtype
        for i in (0, 1, 15, n - 1):
            assert torch.equal(big[key][i * per:(i + 1) * per], T[key][(i % 16) * per:(i % 16 + 1) * per])
        assert BS.first_difference(big[key], 16, n, per) is None
    assert torch.all(big["out"][n * 2:] == -12345.0) and torch.equal(big["count"][n:], T["count"][:1].expand(2))
    a = BS.anchors(big, 16, PER)
    assert all(torch.equal(a[k], T[k]) for k in guard) and a["shared"] is T["shared"] and a["none"] is None
    assert BS.untouched(big, guard) == []
    big["out"][n * 2 + 1, 4, 1] = 0.0
    big["count"][n] += 1
    assert sorted(BS.untouched(big, guard)) == ["count", "out"]


@pytest.mark.parametrize("key,per", [("blocks", 2), ("H", 1), ("count", 1), ("out", 2)])
@pytest.mark.parametrize("where", ["last", "replica 1", "anchor"])
def test_first_difference_finds_one_planted_byte(key, per, where):
    n = BS.N
    big, _ = BS.tile_tensors(_tensors(), np.arange(n), 16, PER)
    t = big[key]
    mf = {"last": n - 1, "replica 1": 16 + 3, "anchor": 3}[where]
    record_bytes = t[0].numel() * t.element_size()
    offset = per * record_bytes - 3                         # in the multiframe's last record
    raw = t.view(-1).view(torch.uint8)
    raw[mf * per * record_bytes + offset] ^= 0x40
    got = BS.first_difference(t, 16, n, per)
    # a spoilt anchor shows at its first replica
    assert got == ((mf, offset) if where != "anchor" else (mf + 16, offset)), got


def test_nan_payloads_compare_as_bytes():
    n = 40
    T = dict(H=torch.full((16, 3), float("nan"), dtype=torch.float64))
    big, _ = BS.tile_tensors(T, np.arange(n), 16, dict(H=1))
    assert BS.first_difference(big["H"], 16, n) is None     # equal NaNs are equal
    big["H"].view(torch.int64)[33, 2] ^= 1                  # another payload, still a NaN
    assert torch.isnan(big["H"]).all() and BS.first_difference(big["H"], 16, n) == (33, 16)


def test_first_misplaced():
    n = 100
    modular, order = BS.placements(n, 16)
    T = _tensors()
    mod, _ = BS.tile_tensors(T, modular, 16, PER)
    shuf, _ = BS.tile_tensors(T, order, 16, PER)
    for key, per in (("blocks", 2), ("H", 1), ("count", 1)):
        assert BS.first_misplaced(shuf[key], mod[key], order, per) is None
        assert BS.first_misplaced(mod[key], mod[key], order, per) is not None    # the modular result is not the shuffled one
    shuf["H"].view(torch.uint8).view(-1)[77 * 288 + 9] ^= 1
    assert BS.first_misplaced(shuf["H"], mod["H"], order) == (77, 9)


def test_snapshot_and_changed():
    T = _tensors()
    snap = BS.snapshot(T, ("H", "count", "none"))
    assert set(snap) == {"H", "count"} and BS.changed(T, snap) == []
    T["count"][5] += 1
    assert BS.changed(T, snap) == ["count"]
