"""Pauli-sum observables: ``H = sum_t h_t P_t`` with real coefficients, as the kernels of csrc/dq_psum.hip read it."""

from __future__ import annotations

import math
from typing import Any

import torch

from . import backend
from .gate import ArbitraryGate, HamiltonianGate, _FlatGate, _OneAngle


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

    norm_bound = property(lambda self: self.table.norm_bound,
                          doc='the sum of |h_t| over the strings other than the empty one: a rigorous bound of ||H - constant|| '
                              '(every Pauli string has norm 1: the triangle inequality)')
    constant = property(lambda self: self.table.constant, doc='the coefficient of the empty string')

    def chebyshev_order(self, t: float, tol: float) -> int:
        """The number of orders -- launches, about -- that ``exp(-i t H)`` takes at tolerance ``tol``: the smallest K with
        ``2 sum_{k > K} |J_k(norm_bound |t|)| < tol``."""
        return backend.chebyshev_order(self.norm_bound * abs(float(t)), tol)

    def device_table(self, device) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """(xmasks, bounds, zmasks, weights) on ``device``, cached per device."""
        return self.table.on(device)

    def __repr__(self) -> str:
        return f'PauliSum(nqubit={self.nqubit}, nterms={self.nterms}, ngroups={self.ngroups})'


class PauliSumEvolution(_OneAngle, _FlatGate, ArbitraryGate):
    """``exp(-i H t)`` for ``H = sum_j coef_j P_j`` given as ``HamiltonianGate`` takes it -- ``[[0.5, 'x0y1'], [-1, 'z3y1'],
    [0.25, '']]``, real coefficients, wires anywhere in the register, the constant term included -- or as a
    :class:`PauliSum`, with one parameter ``t``: a Chebyshev expansion in H, accurate to ``tol`` (default 1e-6 in a
    complex64 circuit, 1e-12 in a complex128 one) whether or not the strings commute, on any number of wires
    (``ops.psum_evolve``: about ``norm_bound * |t|`` plus a few dozen launches of one read of the state per flip mask).
    :class:`PauliEvolution` is the Trotter product for the same list.  ``t`` is trainable (``requires_grad=True``), fixed
    (``t=``), or fed from the circuit's data (``encode=True``; a batch of data gives one ``t`` per sample); it is read on the
    host at every run, so a circuit with this gate cannot be captured into a graph."""

    _param_names = ('t',)
    get_matrix = None                                   # (no matrix: not one of the circuit's vectorised one-angle gates)

    def __init__(self, hamiltonian, t=None, nqubit=1, tol=None, requires_grad=False, name='PauliSumEvolution', den_mat=False,
                 tsr_mode=False):
        if isinstance(hamiltonian, PauliSum):
            if hamiltonian.nqubit != nqubit:
                raise ValueError(f'PauliSumEvolution: the PauliSum is for {hamiltonian.nqubit} qubits, the gate for {nqubit}')
            self.hamiltonian = hamiltonian
        else:
            if not isinstance(hamiltonian, list) or not hamiltonian:
                raise ValueError("PauliSumEvolution: the Hamiltonian is a PauliSum or a list such as [[0.5, 'x0y1'], [0.25, '']]")
            try:
                self.hamiltonian = PauliSum(hamiltonian, nqubit)
            except ValueError as exc:
                raise ValueError(f'PauliSumEvolution: {exc}') from exc
        if tol is not None and not (float(tol) > 0.0 and math.isfinite(float(tol))):
            raise ValueError(f'PauliSumEvolution: tol must be a positive number, got {tol!r}')
        self.tol = None if tol is None else float(tol)
        n = self.hamiltonian.nqubit
        support = 0
        for _, xmask, zmask in self.hamiltonian.terms:
            support |= xmask | zmask
        wires = [w for w in range(n) if support >> (n - 1 - w) & 1] or [0]
        super().__init__(name=name, nqubit=nqubit, wires=wires, den_mat=den_mat, tsr_mode=tsr_mode)
        self._one_angle([t], requires_grad)

    def apply_flat(self, x: torch.Tensor) -> torch.Tensor:
        """(B, 2**n) -> (B, 2**n)."""
        from . import ops

        return ops.psum_evolve(x, self._angle(), self.hamiltonian, self.tol)

    def extra_repr(self) -> str:
        return f'terms={self.hamiltonian.nterms}, groups={self.hamiltonian.ngroups}, tol={self.tol}, ' + _OneAngle.extra_repr(self)
