"""Pauli-sum observables: ``H = sum_t h_t P_t`` with real coefficients, as the kernels of csrc/dq_psum.hip read it."""

from __future__ import annotations

import math
from typing import Any

import torch

from . import backend
from .gate import HamiltonianGate


def _real_coefficient(h: Any, string: str) -> float:
    if isinstance(h, torch.Tensor):
        if h.numel() != 1 or h.is_complex():
            raise ValueError(f'PauliSum: the coefficient of {string!r} must be one real number, got {h.dtype} {tuple(h.shape)}')
        h = h.item()
    if isinstance(h, complex) or not isinstance(h, (int, float)) and not hasattr(h, '__float__'):
        raise ValueError(f'PauliSum: the coefficient of {string!r} must be real, got {h!r}')
    h = float(h)
    if not math.isfinite(h):
        raise ValueError(f'PauliSum: the coefficient of {string!r} is not finite ({h})')
    return h


class PauliSum:
    """The observable ``H = sum_t h_t P_t`` on ``nqubit`` wires from the list form of ``HamiltonianGate`` and
    ``PauliEvolution``, ``[[0.5, 'x0y1'], [-1, 'z3y1'], [0.25, '']]`` (an empty string is the constant term).  The
    coefficients are real constants: they carry no gradient.

    Equal strings are merged and zero coefficients dropped; the terms are grouped by flip mask (wire w is index bit
    ``nqubit - 1 - w``, a Y sets its bit in the flip mask and in the sign mask), and within a group the terms whose
    ``i^ny`` is real come before those whose ``i^ny`` is imaginary, its sign folded into the weight.  ``terms`` is the
    merged list ``(h, xmask, zmask)`` in that order, ``table`` the :class:`backend.PsumTable` the kernels take.

    ``qmath.expectation_pauli_sum`` and ``qmath.apply_pauli_sum`` evaluate ``<psi|H|psi>`` and ``H|psi>`` in one launch
    each: one read of the state per flip mask plus one, whatever the number of strings."""

    def __init__(self, hamiltonian: list, nqubit: int):
        n = int(nqubit)
        if n < 1 or n > 40:
            raise ValueError(f'PauliSum: nqubit={nqubit} out of range [1, 40]')
        if not isinstance(hamiltonian, list) or not hamiltonian:
            raise ValueError('PauliSum: the Hamiltonian must be a non-empty list of [coefficient, string] pairs')
        merged: dict[tuple[int, int], float] = {}
        for h, factors in HamiltonianGate._terms(hamiltonian):
            string = ''.join(f'{p}{w}' for p, w in factors)
            h = _real_coefficient(h, string)
            wires = [w for _, w in factors]
            if len(set(wires)) != len(wires):
                raise ValueError(f'PauliSum: a wire is repeated in {string!r}')
            if any(w >= n for w in wires):
                raise ValueError(f'PauliSum: {string!r} has a wire outside [0, {n})')
            xmask = sum(1 << (n - 1 - w) for p, w in factors if p in 'xy')
            zmask = sum(1 << (n - 1 - w) for p, w in factors if p in 'yz')
            merged[xmask, zmask] = merged.get((xmask, zmask), 0.0) + h
        # (imaginary i^ny, xmask, zmask): groups by rising flip mask, real-weight terms first
        keys = sorted((k for k, h in merged.items() if h != 0.0), key=lambda k: (k[0], bin(k[0] & k[1]).count('1') & 1, k[1]))
        if not keys:
            raise ValueError('PauliSum: every coefficient is zero')
        self.nqubit = n
        self.terms = [(merged[k], *k) for k in keys]
        xmasks, bounds, zmasks, weights = [], [0], [], []
        for t, (h, xmask, zmask) in enumerate(self.terms):
            ny = bin(xmask & zmask).count('1') % 4
            if not xmasks or xmasks[-1] != xmask:
                if xmasks:
                    bounds.append(t)
                xmasks.append(xmask)
                bounds.append(t)                        # (the start of the imaginary-weight terms: moved below)
            if ny % 2 == 0:
                bounds[-1] = t + 1
            zmasks.append(zmask)
            weights.append(-h if ny >= 2 else h)
        bounds.append(len(self.terms))
        self.table = backend.PsumTable(n, xmasks, bounds, zmasks, weights)

    nterms = property(lambda self: self.table.nterms, doc='strings after merging')
    ngroups = property(lambda self: self.table.ngroups, doc='distinct flip masks')

    def device_table(self, device) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """(xmasks, bounds, zmasks, weights) on ``device``, cached per device."""
        return self.table.on(device)

    def __repr__(self) -> str:
        return f'PauliSum(nqubit={self.nqubit}, nterms={self.nterms}, ngroups={self.ngroups})'
