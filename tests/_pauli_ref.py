"""numpy complex128 references of the Pauli-string operations, from the formula

    (P psi)[i] = i^ny (-1)^popc((i ^ x) & z) psi[i ^ x],      ny = popc(x & z)

shared by the test_pauli_* files (index bit 0 is the least significant bit; wire w of an n-qubit register is bit
n - 1 - w)."""

import numpy as np

I_POW = (1, 1j, -1, -1j)


def parity(v):
    v = v.copy()
    for sh in (32, 16, 8, 4, 2, 1):
        v ^= v >> sh
    return v & 1


def pauli_apply(x, xmask, zmask):
    """P x for x of shape (..., 2**n), in complex128."""
    x = np.asarray(x, dtype=np.complex128)
    i = np.arange(x.shape[-1], dtype=np.int64)
    j = i ^ xmask
    return I_POW[bin(xmask & zmask).count('1') % 4] * (1 - 2 * parity(j & zmask)) * x[..., j]


def inside(n, controls):
    i = np.arange(1 << n, dtype=np.int64)
    cmask = sum(1 << c for c in controls)
    return (i & cmask) == cmask


def axpby_ref(x, xmask, zmask, a, c, controls=(), mode='gate'):
    x = np.asarray(x, dtype=np.complex128)
    n = x.shape[-1].bit_length() - 1
    a = np.asarray(a, dtype=np.complex128).reshape(-1, 1)
    c = np.asarray(c, dtype=np.complex128).reshape(-1, 1)
    y = a * x + c * pauli_apply(x, xmask, zmask)
    return np.where(inside(n, controls), y, x if mode == 'gate' else 0)


def rot_ref(x, xmask, zmask, theta, controls=()):
    theta = np.asarray(theta, dtype=np.float64)
    return axpby_ref(x, xmask, zmask, np.cos(theta / 2), -1j * np.sin(theta / 2), controls)


def cross_ref(bra, ket, xmask, zmask, controls=()):
    ket = np.asarray(ket, dtype=np.complex128)
    n = ket.shape[-1].bit_length() - 1
    return (inside(n, controls) * np.conj(np.asarray(bra, dtype=np.complex128)) * pauli_apply(ket, xmask, zmask)).sum(-1)


def masks_of(n, pauli, wires):
    """(xmask, zmask) of the letters ``pauli`` on ``wires`` (wire 0 = the most significant bit)."""
    xmask = zmask = 0
    for ch, w in zip(pauli.lower(), wires):
        bit = 1 << (n - 1 - w)
        if ch in 'xy':
            xmask |= bit
        if ch in 'yz':
            zmask |= bit
    return xmask, zmask


def dense_pauli(n, pauli, wires):
    """The 2^n x 2^n matrix of the string by Kronecker products (an independent route to the same operator)."""
    mats = {'i': np.eye(2), 'x': np.array([[0, 1], [1, 0]]), 'y': np.array([[0, -1j], [1j, 0]]), 'z': np.diag([1, -1])}
    per_wire = ['i'] * n
    for ch, w in zip(pauli.lower(), wires):
        per_wire[w] = ch
    out = np.eye(1, dtype=np.complex128)
    for ch in per_wire:
        out = np.kron(out, mats[ch])
    return out
