"""The collapse and the draw of a mid-circuit measurement in numpy complex128 / float64, straight from their definitions
(include/dq_hip.h, section 18): the reference of the test_collapse_* files."""

import numpy as np


def sub(i, bits):
    """sum_j bit_{bits[j]}(i) << (k - 1 - j)"""
    r = np.zeros_like(i)
    for j, p in enumerate(bits):
        r |= ((i >> p) & 1) << (len(bits) - 1 - j)
    return r


def ext(i, n, bits):
    """i with the measured bits squeezed out"""
    return sub(i, [p for p in range(n - 1, -1, -1) if p not in bits])


def sigma(i, z):
    return 1.0 - 2.0 * np.array([bin(int(v) & int(z)).count('1') & 1 for v in i])


def collapse(psi, n, bits, o, x, z, s, layout='full', transpose=False):
    """One sample: psi complex128, (o, x, z, s) its record; returns complex128."""
    mask = sum(1 << p for p in bits)
    idx = np.arange(1 << n, dtype=np.int64)
    psi = np.asarray(psi, dtype=np.complex128)
    if layout == 'full' and not transpose:
        src = idx ^ x
        return np.where(sub(src, bits) == o, s * sigma(src, z) * psi[src], 0)
    if layout == 'full':
        return np.where(sub(idx, bits) == o, s * sigma(idx, z) * psi[idx ^ x], 0)
    if transpose:
        return np.where(sub(idx, bits) == o, s * sigma(idx, z) * psi[ext(idx ^ x, n, bits)], 0)
    out = np.zeros(1 << (n - len(bits)), dtype=np.complex128)
    i = idx[sub(idx, bits) == o]
    out[ext(i ^ (x & ~mask), n, bits)] = s * sigma(i, z) * psi[i]
    return out


def draw(probs, u):
    """The smallest o with C(o) > u * T, C the running sum in index order; the CDF is returned too."""
    c = np.cumsum(np.asarray(probs, dtype=np.float64))
    return int(np.searchsorted(c, u * c[-1], side='right')), c
