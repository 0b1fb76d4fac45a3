"""numpy complex128 references for the Gram and combine kernels (csrc/dq_gram.hip), the magnitude sums their error bounds
are written in, and seeded builders of the rows the tests use."""

import numpy as np
import torch

NP = {'c64': np.complex64, 'c128': np.complex128}
TORCH = {'c64': torch.complex64, 'c128': torch.complex128}
TOL = {'c64': 1e-4, 'c128': 1e-10}
U_T = {'c64': 2.0**-24, 'c128': 2.0**-53}
NMIN = {'c64': 1, 'c128': 0}                            # a row is at least one 16-byte vector

#: the row counts of the issue: one block, its edge, two blocks, the tile's edge, one row into the next tile
ROWS = (1, 2, 3, 15, 16, 17, 31, 32, 33)
#: coefficients whose products with small Gaussian integers are exact in float32
EXACT_COEFS = np.array([1, -1, 2, -2, 0.5, -0.5, 1j, -1j])


def gram_ref(a, b):
    """G[i, j] = sum_x conj(a[i, x]) b[j, x]"""
    return a.astype(np.complex128).conj() @ b.astype(np.complex128).T


def combine_ref(coef, s):
    """Y[m, x] = sum_j coef[m, j] s[j, x]"""
    return coef.astype(np.complex128) @ s.astype(np.complex128)


def gram_abs(a, b):
    """sum_x |a[i, x]| |b[j, x]| per entry"""
    return np.abs(a.astype(np.complex128)) @ np.abs(b.astype(np.complex128)).T


def gram_largest_term(a, b):
    """max_x |a[i, x]| |b[j, x]| per entry (row by row: no (M, N, 2^n) array)"""
    aa, bb = np.abs(a.astype(np.complex128)), np.abs(b.astype(np.complex128))
    return np.array([[(aa[i] * bb[j]).max() for j in range(bb.shape[0])] for i in range(aa.shape[0])])


def combine_abs(coef, s):
    """sum_j |coef[m, j]| |s[j, x]| per element"""
    return np.abs(coef.astype(np.complex128)) @ np.abs(s.astype(np.complex128))


def integer_rows(rng, rows, n, dt):
    """Gaussian integers with parts in {-1, 0, 1}: every partial sum of a Gram entry is an integer below 2^(n + 1)."""
    a = rng.integers(-1, 2, (rows, 1 << n)) + 1j * rng.integers(-1, 2, (rows, 1 << n))
    return a.astype(NP[dt])


def gaussian_rows(rng, rows, n, dt):
    """Unit complex Gaussians, rounded to the dtype (the reference is taken from the rounded values)."""
    a = (rng.standard_normal((rows, 1 << n)) + 1j * rng.standard_normal((rows, 1 << n))) / np.sqrt(2.0)
    return a.astype(NP[dt])


def exact_coefs(rng, m, k):
    return rng.choice(EXACT_COEFS, (m, k)).astype(np.complex128)


def gaussian_coefs(rng, m, k):
    return (rng.standard_normal((m, k)) + 1j * rng.standard_normal((m, k))) / np.sqrt(2.0)


def log2(v):
    assert v > 0 and v & (v - 1) == 0, v
    return v.bit_length() - 1


#: the boundaries of the Gram kernel's geometry, by name (``boundary_size`` turns a name into an n)
BOUNDARIES = ('minimum', 'short of a lane', 'below a wave', 'a wave', 'above a wave', 'below a unit', 'a unit', 'above a unit',
              'second stride')


def boundary_size(geom, dt, name):
    """The n of a boundary of ``BOUNDARIES`` for the geometry ``backend.gram_geometry`` exports (never below the minimum)."""
    lane, wave, unit = log2(geom.lane_cols), log2(geom.wave_cols), log2(geom.unit_cols)
    n = {'minimum': NMIN[dt], 'short of a lane': lane - 1, 'below a wave': wave - 1, 'a wave': wave, 'above a wave': wave + 1,
         'below a unit': unit - 1, 'a unit': unit, 'above a unit': unit + 1, 'second stride': unit + log2(geom.max_blocks) + 1}[name]
    return max(n, NMIN[dt])


def boundary_sizes(geom, dt, limit=20):
    """The n at which the Gram kernel's geometry changes, from ``backend.gram_geometry``: the minimum; a row shorter than
    a lane's segment; one on each side of a wave's share of a step (and the share itself); one on each side of a
    workgroup's unit (the upper one is the first n with more than one workgroup); the first n with a second grid-stride
    iteration of a single tile pair."""
    lane, wave, unit = log2(geom.lane_cols), log2(geom.wave_cols), log2(geom.unit_cols)
    stride = unit + log2(geom.max_blocks) + 1
    want = {NMIN[dt], lane - 1, wave - 1, wave, wave + 1, unit - 1, unit, unit + 1, stride}
    return sorted(n for n in want if NMIN[dt] <= n <= limit)


def gram_bound(n, dt, chain, max_blocks, mags):
    """The bound of |error| per entry.  complex64: at most ``chain`` real terms are summed in float32 (each product rounded
    once: chain + 1 roundings, + 1 for the conversion of the inputs' products into the double sum), everything after that
    in double along a path of at most 2^n additions.  complex128: every product and every addition in float64 -- 2 * 2^n
    real terms per entry, the waves and the workgroups' partial sums on top."""
    if dt == 'c64':
        return (2.0**-53 * 2.0**n + (chain + 2) * 2.0**-24) * mags
    return 2.0**-53 * (2.0 * 2.0**n + max_blocks + 2) * mags
