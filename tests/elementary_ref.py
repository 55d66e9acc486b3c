"""numpy restatement of okvis2_amd/csrc/elementary_fixed.h: log_fixed, sin_fixed, cos_fixed and sinc_fixed as the same
sequence of IEEE float64 operations, one numpy operation per C operation (no contraction), on arrays of any shape.  The
literals are the header's.  Test infrastructure only."""
import numpy as np

PI_4 = 7.85398163397448278999e-01
SQRT2 = 1.41421356237309514547e+00
LN2_HI, LN2_LO = 6.93146705627441406250e-01, 4.74932503903167255529e-07
SIN = (-1.66666666666666657415e-01, 8.33333333333333321769e-03, -1.98412698412698412526e-04, 2.75573192239858925110e-06,
       -2.50521083854417202239e-08, 1.60590438368216133409e-10, -7.64716373181981640551e-13, 2.81145725434552059811e-15)
COS = (4.16666666666666643537e-02, -1.38888888888888894189e-03, 2.48015873015873015658e-05, -2.75573192239858882758e-07,
       2.08767569878681001866e-09, -1.14707455977297245073e-11, 4.77947733238738525345e-14, -1.56192069685862252711e-16)
LOG = (3.33333333333333314830e-01, 2.00000000000000011102e-01, 1.42857142857142849213e-01, 1.11111111111111104943e-01,
       9.09090909090909116141e-02, 7.69230769230769273470e-02, 6.66666666666666657415e-02, 5.88235294117647050660e-02,
       5.26315789473684181310e-02, 4.76190476190476164042e-02)
SINC_EDGE = 1.0e-6
C_2, C_4, C_6 = 1.66666666666666657415e-01, 8.33333333333333321769e-03, 1.98412698412698412526e-04   # sinc's 1/6, 1/120, 1/5040


def _horner(z, coeffs):
    p = np.float64(coeffs[-1])
    for c in coeffs[-2::-1]:
        p = np.float64(c) + z * p
    return p


def sin_fixed(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        ok = np.abs(x) <= PI_4
        z = x * x
        r = x + x * (z * _horner(z, SIN))
    return np.where(ok, r, np.nan)


def cos_fixed(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        ok = np.abs(x) <= PI_4
        z = x * x
        r = 1.0 - (0.5 * z - (z * z) * _horner(z, COS))
    return np.where(ok, r, np.nan)


def sinc_fixed(x):
    """-> (value, the fabs(x) > 1.0e-6 branch taken)"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        big = np.abs(x) > SINC_EDGE
        quotient = sin_fixed(x) / x
        x_2 = x * x
        x_4 = x_2 * x_2
        x_6 = (x_2 * x_2) * x_2
        poly = ((1.0 - C_2 * x_2) + C_4 * x_4) - C_6 * x_6
    return np.where(big, quotient, poly), big


def log_fixed(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        ok = x >= 1.0
        inf = x == np.inf
        bits = np.where(ok & ~inf, x, 1.0).view(np.uint64)
        k = (bits >> np.uint64(52)).astype(np.int64) - 1023
        m = ((bits & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FF0000000000000)).view(np.float64)
        up = m >= SQRT2
        m = np.where(up, m * 0.5, m)
        k = np.where(up, k + 1, k)
        f = (m - 1.0) / (m + 1.0)
        z = f * f
        f2 = 2.0 * f
        series = f2 + f2 * (z * _horner(z, LOG))
        dk = k.astype(np.float64)
        r = dk * LN2_HI + (dk * LN2_LO + series)
    return np.where(inf, np.inf, np.where(ok, r, np.nan))
