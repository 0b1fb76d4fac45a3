"""numpy complex128 references of the diagonal operations, from three lines of index arithmetic

    sub(i) = sum_j bit_{bits[j]}(i) << (k - 1 - j),      on(i) = all control bits of i are 1

shared by test_diag_gpu.py and the derivative references (tests/_stream_grad_ref.py)."""

import numpy as np


def sub_index(n, bits):
    i = np.arange(1 << n, dtype=np.int64)
    k = len(bits)
    s = np.zeros_like(i)
    for j, p in enumerate(bits):
        s |= ((i >> p) & 1) << (k - 1 - j)
    return s


def on_mask(n, controls):
    cm = sum(1 << c for c in controls)
    return (np.arange(1 << n, dtype=np.int64) & cm) == cm


def diag_ref(x, d, n, bits, controls=()):
    f = d[..., sub_index(n, bits)]
    return np.where(on_mask(n, controls), f * x, x)


def phase_ref(x, c, t, n, bits, controls=()):
    f = np.exp(-1j * np.asarray(t, dtype=np.float64)[:, None] * c[sub_index(n, bits)])
    return np.where(on_mask(n, controls), f * x, x)


def scale_ref(x, c, s, n, bits, controls=()):
    """s c x inside the controls, 0 elsewhere."""
    return np.where(on_mask(n, controls), np.asarray(s, dtype=np.complex128)[:, None] * c[sub_index(n, bits)] * x, 0)


def cross_ref(bra, ket, c, n, bits, controls=()):
    """sum over the controls of c conj(bra) ket."""
    w = np.where(on_mask(n, controls), c[sub_index(n, bits)], 0.0)
    return (w * np.conj(bra) * ket).sum(-1)
