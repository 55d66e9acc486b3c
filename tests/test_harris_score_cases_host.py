"""CPU: the scenes of tests/harris_score_cases.py hold what they are meant to hold, and the operations score_row of
harris_kernel (csrc/k_harris.hip) is built from equal the definition over the whole of their register ranges.

1. Census: A, B, C of every pixel from the definition in numpy; the scenes of each shape together reach the floors
   recorded in the cases file -- every parity of (A, B), A and B both odd with (A + B) % 4 == 0 (the case the mask in
   front of the SAD exists for), both signs of C at |C| >= 2^12, A B >= 2^25, negative and positive scores, and the same
   in the rim-adjacent columns 1 and w - 2.
2. The arithmetic: numpy restatements of the kernel's operations (and-literal, v_sad_u16, shift, SDWA multiply, 24-bit
   multiply and multiply-add, subtract; int32 wrap-around as on the device) and of the measured form that takes C^2 + tq^2
   from v_dot2_i32_i16 on the i16 halves of C << 16 | tq, against A B - C^2 - tq^2 on random triples over the register
   ranges (A, B <= 16256, |C| <= 16256: larger than any image reaches, see the cases file) and on the corners of those
   ranges.
3. The oracle's score map of every scene equals the numpy definition (so the GPU tests compare against the definition)."""
import numpy as np
import pytest

import harris_score_cases as H


@pytest.mark.parametrize("shape", sorted(H.SHAPES))
def test_scenes_reach_the_floors(shape):
    got = H.census_of_shape(shape)
    print(shape, got)
    for k in H.CLASSES:
        want = H.FLOORS[shape][k]
        assert want[0] > 0 and want[1] > 0, k
        assert got[k][0] >= want[0] and got[k][1] >= want[1], (k, got[k], want)


@pytest.mark.parametrize("shape", sorted(H.SHAPES))
def test_every_listed_scene_does_its_part(shape):
    c = {name: H.census(H.scene(shape, name)) for name in H.NAMES}
    assert c["diag_pos"]["C_ge_2p12"][1] > 0 and c["diag_pos"]["C_le_m2p12"][0] == 0
    assert c["diag_neg"]["C_le_m2p12"][1] > 0 and c["diag_neg"]["C_ge_2p12"][0] == 0
    assert c["diag_pos"]["AB_ge_2p25"][1] > 0
    assert c["noise_half"]["odd_odd_sum_mod4_0"][1] > 0
    for k in ("parity_01", "parity_10", "parity_11"):
        assert c["noise_half"][k][1] > 0
    for name in ("edge_v", "edge_h", "stripes_2", "stripes_3"):  # one gradient only: det = 0, score = -tq^2
        assert c[name]["score_neg"][0] > 0 and c[name]["score_pos"][0] == 0
    for name in ("checker_2", "checker_3"):
        assert c[name]["score_pos"][1] > 0
    for name in ("flat", "stripes_1", "checker_1"):  # no gradient at all (period 2 cancels in both filters)
        assert c[name]["score_neg"][0] == 0 and c[name]["score_pos"][0] == 0
    A, B, Cc = H.abc(H.scene(shape, "stripes_2"))
    assert A.max() == 16256 and B.max() == 0  # the top of the range of A


M32 = (1 << 32) - 1


def _i32(x):
    return ((x & M32) ^ (1 << 31)) - (1 << 31)


def _tq_and_ab(A, B):
    """score_row's first four operations on int64 arrays holding 32-bit register values"""
    AB = (A | (B << 16)) & M32
    m = AB & 0xFFFEFFFE
    sad = (m & 0xFFFF) + (m >> 16)                           # v_sad_u16(m, 0, 0)
    ab = ((AB & 0xFFFF) * (AB >> 16)) & M32                  # v_mul_u32_u24_sdwa WORD_0 x WORD_1
    return sad >> 2, ab


def _kernel_score(A, B, Cc):
    """the kernel: v_mul_i32_i24, v_mad_i32_i24, v_sub"""
    tq, ab = _tq_and_ab(A, B)
    assert np.abs(Cc).max() < 1 << 23 and tq.max() < 1 << 23  # 24-bit operands
    return _i32(ab - _i32(tq * tq + _i32(Cc * Cc)))


def _dot_score(A, B, Cc):
    """the measured form: stream 1 carries C << 16, one v_or, one v_dot2_i32_i16(op, op, 0)"""
    tq, ab = _tq_and_ab(A, B)
    op = ((Cc << 16) & M32) | tq
    lo = ((op & 0xFFFF) ^ 0x8000) - 0x8000                   # the i16 halves, sign-extended
    hi = ((op >> 16) ^ 0x8000) - 0x8000
    return _i32(ab - ((lo * lo + hi * hi) & M32))


def _definition(A, B, Cc):
    tq = ((A >> 1) + (B >> 1)) >> 1
    return A * B - Cc * Cc - tq * tq


def test_the_kernels_operations_equal_the_definition():
    rng = np.random.default_rng(5)
    n = 1 << 20
    A = rng.integers(0, 16257, n)
    B = rng.integers(0, 16257, n)
    Cc = rng.integers(-16256, 16257, n)
    want = _definition(A, B, Cc)
    assert np.abs(want).max() < 1 << 31
    assert np.array_equal(_kernel_score(A, B, Cc), want)
    assert np.array_equal(_dot_score(A, B, Cc), want)
    assert (Cc >= 1 << 13).any() and (Cc <= -(1 << 13)).any() and (A * B >= 1 << 27).any()
    odd = (A & B & 1 == 1) & ((A + B) % 4 == 0)
    assert odd.sum() > 1000
    assert not np.array_equal(((A + B) >> 2)[odd], (((A >> 1) + (B >> 1)) >> 1)[odd])  # why the mask is there
    ends = np.array([0, 1, 2, 3, 16253, 16254, 16255, 16256])
    cs = np.array([16256, 16255, 1, 0, -1, -16255, -16256])
    A, B, Cc = (a.ravel() for a in np.meshgrid(ends, ends, cs, indexing="ij"))
    assert len(A) == 448
    assert np.array_equal(_kernel_score(A, B, Cc), _definition(A, B, Cc))
    assert np.array_equal(_dot_score(A, B, Cc), _definition(A, B, Cc))


@pytest.mark.parametrize("shape", sorted(H.SHAPES))
def test_oracle_equals_the_definition(oracle, shape):
    for name in H.NAMES:
        img = H.scene(shape, name)
        want = H.score_from_abc(*H.abc(img)).astype(np.int32)
        assert np.array_equal(H.reference(shape, name)[0], want), name
