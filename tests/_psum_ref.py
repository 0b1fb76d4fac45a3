"""numpy complex128 references of the Pauli-sum operations, H = sum_t h_t P_t over terms ``(h, xmask, zmask)`` in the mask
convention of tests/_pauli_ref.py, shared by the test_psum_* files."""

import numpy as np

from _pauli_ref import dense_pauli, pauli_apply


def psum_apply_ref(x, terms):
    """H x for x of shape (..., 2**n): the sum of h_t * pauli_apply(x, x_t, z_t)."""
    x = np.asarray(x, dtype=np.complex128)
    out = np.zeros_like(x)
    for h, xmask, zmask in terms:
        out += h * pauli_apply(x, xmask, zmask)
    return out


def psum_cross_ref(bra, ket, terms):
    return (np.conj(np.asarray(bra, dtype=np.complex128)) * psum_apply_ref(ket, terms)).sum(-1)


def psum_axpby_ref(x, terms, a, c):
    a = np.asarray(a, dtype=np.complex128).reshape(-1, 1)
    c = np.asarray(c, dtype=np.complex128).reshape(-1, 1)
    return a * np.asarray(x, dtype=np.complex128) + c * psum_apply_ref(x, terms)


class PauliSums:
    """The family H = sum_t h_t P_t for tests/_stream_grad_ref.py: Hermitian, its support the whole state ('gate' and 'map'
    coincide), no rotation."""
    sign = +1

    def __init__(self, n, terms):
        self.n, self.terms = n, terms

    def support(self):
        return np.ones(1 << self.n, dtype=bool)

    def axpby(self, x, a, c, mode='gate'):
        batch = len(x)
        a, c = (np.broadcast_to(np.asarray(p).reshape(-1), (batch,)) if np.asarray(p).size == 1 else np.asarray(p) for p in (a, c))
        return psum_axpby_ref(x, self.terms, a, c)

    def cross(self, u, v):
        return psum_cross_ref(u, v, self.terms)


def abs_terms(terms):
    """|H|: the sum with |h_t| and every sign positive, as terms of plain flips."""
    return [(abs(h), xmask, 0) for h, xmask, _ in terms]


def string_of(n, xmask, zmask):
    """The letters-and-wires string of (xmask, zmask): wire w is bit n - 1 - w."""
    out = ''
    for w in range(n):
        bit = 1 << (n - 1 - w)
        if xmask & bit:
            out += f'y{w}' if zmask & bit else f'x{w}'
        elif zmask & bit:
            out += f'z{w}'
    return out


def hamiltonian_of(n, terms):
    """The list form ``[[h, 'x0y1'], ...]`` of the terms."""
    return [[h, string_of(n, xmask, zmask)] for h, xmask, zmask in terms]


def energy_per_string(cir, data, hamiltonian):
    """The route the package had before: sum_t h_t <P_t> through ``cir.observable`` and ``expectation()`` on a torch
    circuit, differentiable in ``data``.  The constant term is h <psi|psi>: nothing is normalised, and the float32
    constants of the Hadamards leave the norm at 1 - 1e-7."""
    import re

    import torch

    cir.reset_observable()
    const, coefs = 0.0, []
    for h, string in hamiltonian:
        factors = re.findall(r'([xyz])(\d+)', string)
        if not factors:
            const += h
            continue
        cir.observable([int(w) for _, w in factors], ''.join(p for p, _ in factors))
        coefs.append(h)
    state = cir(data)
    norm2 = (state.real ** 2 + state.imag ** 2).sum(dim=(-2, -1))
    return (cir.expectation() * torch.tensor(coefs, dtype=torch.float64, device=state.device)).sum(-1) + const * norm2


def dense_psum(n, hamiltonian):
    """The 2^n x 2^n matrix of the list form by Kronecker products (n <= 6): an independent route to the same operator."""
    import re

    assert n <= 6
    out = np.zeros((1 << n, 1 << n), dtype=np.complex128)
    for h, string in hamiltonian:
        factors = re.findall(r'([xyzXYZ])(\d+)', string)
        out += h * dense_pauli(n, ''.join(p for p, _ in factors), [int(w) for _, w in factors])
    return out
