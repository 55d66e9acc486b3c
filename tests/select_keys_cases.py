"""Content and bookkeeping shared by tests/test_gpu_select_keys.py: images that put the self-ordering selection kernel
(select_lazy_kernel<true>, csrc/k_select.hip) into a named regime of its key scatter, and a restatement of the kernel's
chunk schedule so that a test can say which regime an image reaches from the oracle's candidate scores alone.

The schedule restated (k_select.hip, "chunks"): candidates are counted into kFuseBins = 496 log buckets of the score (16
per octave, bucket 0 = the highest scores); the bucket sequence is cut into chunks of whole buckets with targets 64, 128,
... 1024 candidates; a bucket that alone exceeds the target is a chunk of its own; at most kFuseSched = 40 chunk ends are
kept and whatever lies beyond them is ONE last chunk; a chunk of more than 1024 keys is split by key range.  The first
kFuseFirst * 256 = 5120 candidate records of an image stay in registers, the rest go through a second scatter loop."""
import functools

import numpy as np

from okvis2_amd import synth

FUSE_BINS, FUSE_SCHED, ROUND_CAP, FIRST_RECORDS = 496, 40, 1024, 5120


def fuse_bin(score: int) -> int:
    if score <= 0:
        return FUSE_BINS - 1
    e = int(score).bit_length() - 1
    b = ((e << 4) | ((score >> (e - 4)) & 15)) if e >= 4 else score
    return (FUSE_BINS - 1) - b


def chunk_sizes(scores) -> list:
    """sizes of the chunks the kernel cuts `scores` (one per candidate, any order) into"""
    n = len(scores)
    hist = np.zeros(FUSE_BINS, np.int64)
    for s in scores:
        hist[fuse_bin(int(s))] += 1
    end = np.cumsum(hist)
    sizes, pos, b, target = [], 0, 0, 64
    while pos < n and len(sizes) < FUSE_SCHED:
        x = b - 1
        while x + 1 < FUSE_BINS and end[x + 1] - pos <= target:
            x += 1
        e = int(end[x]) if x >= b else pos
        if e == pos:  # the next non-empty bucket alone exceeds the target
            x = b
            while end[x] <= pos:
                x += 1
            e = int(end[x])
        sizes.append(e - pos)
        pos, b, target = e, x + 1, min(2 * target, ROUND_CAP)
    if pos < n:
        sizes.append(n - pos)
    return sizes


def candidates(oracle, img, thr):
    return oracle.nms(oracle.harris_score(img), thr)


def threshold_for(oracle, img, count):
    """the absolute threshold at which `img` has exactly `count` candidates (scores at the cut must differ)"""
    s = np.sort(candidates(oracle, img, 1)["score"])[::-1]
    assert len(s) > count and s[count - 1] > s[count], (len(s), count)
    thr = int(s[count - 1])
    assert len(candidates(oracle, img, thr)) == count
    return thr


def camera_for(w, h):
    """a mildly distorted pinhole camera for an image of any size"""
    return synth.Camera(w, h, 0.62 * w, 0.63 * w, w / 2 - 0.7, h / 2 + 0.4, 1, (-0.05, 0.004, 0.0002, -0.0001))


def frozen(img):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    img.setflags(write=False)
    return img


def checker(w, h, cell, lo=40, hi=215):
    """exact two-level cells: every corner has one of very few scores"""
    yy, xx = np.mgrid[0:h, 0:w]
    return frozen(np.where(((xx // cell) + (yy // cell)) % 2 == 0, lo, hi))


def blob(w, h):
    img = np.full((h, w), 20, np.uint8)
    img[h // 2 - 5:h // 2 + 5, w // 2 - 5:w // 2 + 5] = 220
    return frozen(img)


@functools.lru_cache(maxsize=None)
def contrast_tiles(w=752, h=480, tw=107, th=80, cell=4, base=30.0, ratio=1.05):
    """exact checker tiles, every tile at a contrast of its own: each tile's ~1000 corners tie in a bucket of their own, so
    (almost) every bucket is a chunk and there are more of them than the schedule table holds"""
    img = np.full((h, w), 10, np.uint8)
    i = 0
    for ty in range(0, h, th):
        for tx in range(0, w, tw):
            hi = min(10 + int(round(base * ratio ** i)), 255)
            i += 1
            yy, xx = np.mgrid[ty:min(ty + th, h), tx:min(tx + tw, w)]
            img[ty:ty + th, tx:tx + tw] = np.where(((xx // cell) + (yy // cell)) % 2 == 0, 10, hi)
    return frozen(img)
