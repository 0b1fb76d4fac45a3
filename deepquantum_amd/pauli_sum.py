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
    select_bits = property(lambda self: max(1, (self.nterms - 1).bit_length()),
                           doc='the select wires a SELECT over the strings needs: ceil(log2 nterms), and 1 for a single string')

    def chebyshev_order(self, t: float, tol: float, bounds: tuple[float, float] | None = None) -> int:
        """The number of orders -- launches, about -- that ``exp(-i t H)`` takes at tolerance ``tol``: the smallest K with
        ``2 sum_{k > K} |J_k(norm_bound |t|)| < tol``; with ``bounds=(lo, hi)``, half their width in place of ``norm_bound``."""
        a = self.norm_bound if bounds is None else backend._evolve_window(self.table, bounds, 'PauliSum.chebyshev_order')[0]
        return backend.chebyshev_order(a * abs(float(t)), tol)

    def spectral_bounds(self, tol: float = 1e-3, margin: float = 0.01, seed: int = 0, dtype: torch.dtype = torch.complex64,
                        device: Any = None) -> tuple[float, float]:
        """``(lo, hi)`` around the spectrum of H from two short Lanczos runs without vectors (:meth:`extremal`, lowest and
        highest, to a residual of ``tol * norm_bound``): each Ritz value moved OUTWARD by its residual estimate plus ``margin``
        times the width between the two, the result clipped into the rigorous ``[constant - norm_bound, constant + norm_bound]``.
        Cached per argument set.  Made for ``bounds=`` of the evolution (``evolve_pauli_sum``, ``PauliSumEvolution``), whose
        order then follows the true width of the spectrum and not the loose ``norm_bound``.

        This is NOT a rigorous bound.  A small residual proves that an eigenvalue lies that close to the Ritz value, not that
        it is the extreme one: a start vector with no weight on the extreme eigenvector never finds it (a Gaussian random
        start has weight on everything, almost surely).  Why it is safe in practice all the same: a Ritz value that has
        settled to ``tol`` misses the true edge by far less than the margin, and an eigenvalue a relative ``delta`` outside
        the interval only makes the Chebyshev polynomial of order K grow like ``cosh(K sqrt(2 delta))`` -- for the delta
        that can be left and the K of an evolution, a factor next to 1.  Where a proof is needed, leave ``bounds`` out."""
        key = (float(tol), float(margin), int(seed), dtype, None if device is None else str(torch.device(device)))
        cache = self.__dict__.setdefault('_spectral_bounds', {})
        if key not in cache:
            if not (float(margin) >= 0.0 and math.isfinite(float(margin))):
                raise ValueError(f'PauliSum.spectral_bounds: margin must be a number >= 0, got {margin!r}')
            rigorous = (self.constant - self.norm_bound, self.constant + self.norm_bound)
            if self.norm_bound == 0.0:
                cache[key] = rigorous
            else:
                kw = dict(tol=tol, vector=False, dtype=dtype, device=device, seed=seed)
                low, high = self.extremal('lowest', **kw), self.extremal('highest', **kw)
                width = float(high.value) - float(low.value)
                lo = float(low.value) - float(low.residual) - float(margin) * width
                hi = float(high.value) + float(high.residual) + float(margin) * width
                cache[key] = (max(lo, rigorous[0]), min(hi, rigorous[1]))
        return cache[key]

    def extremal(self, which: str = 'lowest', **kw):
        """The lowest or highest eigenvalue of H and its eigenvector by Lanczos steps on the device:
        ``qmath.pauli_sum_extremal(self, which=which, **kw)``, which lists the keywords (``tol``, ``max_steps``, ``start``,
        ``vector``, ``dtype``, ``device``, ``seed``) and what this is not: one pair only, a start-dependent vector in a
        degenerate level, a complex64 residual that stalls near 1e-7 * norm_bound."""
        from . import qmath

        return qmath.pauli_sum_extremal(self, which=which, **kw)

    def ground_state(self, **kw):
        """The ground energy and ground state: ``self.extremal('lowest', **kw)``."""
        return self.extremal('lowest', **kw)

    def subspace_matrices(self, states: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """``(Hs, S)`` for a handful of (M, 2**n) ``states`` V: the projected Hamiltonian ``Hs[i, j] = <v_i|H|v_j>`` and the
        overlap matrix ``S[i, j] = <v_i|v_j>``, complex128 (M, M) -- what a generalised eigenproblem ``Hs c = E S c`` in
        the span of V (subspace diagonalisation, several Ritz pairs of a Krylov basis) is made of.  ``H V`` is one
        ``apply_psum_axpby`` launch, the two matrices one Gram launch each (``qmath.gram_matrix``); ``S`` is exactly
        Hermitian, ``Hs`` Hermitian within rounding.  Differentiable in the states."""
        from . import ops, qmath

        v = qmath._gram_states(states, 'PauliSum.subspace_matrices')
        if v.shape[1] != 1 << self.nqubit:
            raise ValueError(f'PauliSum.subspace_matrices: the PauliSum is for {self.nqubit} qubits, the states have '
                             f'{v.shape[1]} amplitudes')
        zero = torch.zeros(v.shape[0], dtype=torch.complex128, device=v.device)
        hv = ops.psum_axpby(v, zero, torch.ones_like(zero), self)
        return ops.gram(v, hv), ops.gram(v, v)

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
    host at every run, so a circuit with this gate cannot be captured into a graph.  ``bounds=(lo, hi)``: an interval that
    holds the spectrum of H (``PauliSum.spectral_bounds``), in place of ``constant -+ norm_bound``: fewer orders, forward and
    backward."""

    _param_names = ('t',)
    get_matrix = None                                   # (no matrix: not one of the circuit's vectorised one-angle gates)

    def __init__(self, hamiltonian, t=None, nqubit=1, tol=None, requires_grad=False, name='PauliSumEvolution', den_mat=False,
                 tsr_mode=False, bounds=None):
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
        if bounds is not None:
            backend._evolve_window(self.hamiltonian.table, bounds, 'PauliSumEvolution')
            bounds = (float(bounds[0]), float(bounds[1]))
        self.bounds = bounds
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

        if self.bounds is None:
            return ops.psum_evolve(x, self._angle(), self.hamiltonian, self.tol)
        return ops.psum_evolve(x, self._angle(), self.hamiltonian, self.tol, self.bounds)

    def extra_repr(self) -> str:
        bounds = '' if self.bounds is None else f'bounds={self.bounds}, '
        return (f'terms={self.hamiltonian.nterms}, groups={self.hamiltonian.ngroups}, tol={self.tol}, ' + bounds
                + _OneAngle.extra_repr(self))


def _select_wires(wires, what: str, noun: str) -> list[int]:
    wires = [wires] if isinstance(wires, int) else list(wires)
    if not all(isinstance(w, int) for w in wires):
        raise ValueError(f'{what}: {noun} must be integers, got {wires}')
    return wires


class SelectPauli(_FlatGate, ArbitraryGate):
    """SELECT of a linear combination of unitaries: ``sum_s |s><s| (x) c_s P_s`` -- for every value s of the k select
    wires ``wires`` (``wires[0]`` the most significant bit of s) its own Pauli string ``P_s`` with a phase ``c_s = i^phases[s]``
    on the system wires -- in one read and one write of the state whatever the number of strings, exact
    (``dq_apply_select_pauli_*``), where a loop of controlled strings between X flips is one pass per string.

    ``paulis``: at most 2^k strings in the factor notation of ``HamiltonianGate`` (``'x0y2'``, ``''`` for the identity), a
    wire number w inside a string meaning ``system_wires[w]`` (default: every wire that is neither a select wire nor a
    control, in rising order); missing entries up to 2^k are the identity.  Or a :class:`PauliSum` on ``len(system_wires)``
    wires: its merged ``terms``, in their order, are the strings and the signs of the coefficients the phases (0 for
    h > 0, 2 for h < 0) -- the magnitudes belong to PREPARE (``cir.block_encode``) and are ignored here.  The strings and
    phases are constants."""

    def __init__(self, paulis, nqubit=1, wires=None, system_wires=None, phases=None, controls=None, name='SelectPauli',
                 den_mat=False):
        what = 'SelectPauli'
        n = int(nqubit)
        if wires is None:
            raise ValueError(f'{what}: wires lists the select wires, the most significant bit of s first')
        wires = _select_wires(wires, what, 'the select wires')
        controls = _select_wires([] if controls is None else controls, what, 'the controls')
        k = len(wires)
        if k < 1 or k > backend.SELECT_MAX_BITS:
            raise ValueError(f'{what}: 1 to {backend.SELECT_MAX_BITS} select wires, got {k}')
        taken = wires + controls
        if len(set(taken)) != len(taken) or any(w < 0 or w >= n for w in taken):
            raise ValueError(f'{what}: repeated wires, or wires outside [0, {n}): select wires {wires}, controls {controls}')
        if system_wires is None:
            system_wires = [w for w in range(n) if w not in taken]
        else:
            system_wires = _select_wires(system_wires, what, 'the system wires')
            if len(set(system_wires)) != len(system_wires):
                raise ValueError(f'{what}: repeated wires in system_wires {system_wires}')
            if any(w < 0 or w >= n for w in system_wires):
                raise ValueError(f'{what}: a system wire outside [0, {n}): {system_wires}')
            if set(system_wires) & set(taken):
                raise ValueError(f'{what}: system_wires {system_wires} touches a select or control wire '
                                 f'(select wires {wires}, controls {controls})')
        m = len(system_wires)
        if isinstance(paulis, PauliSum):
            if paulis.nqubit != m:
                raise ValueError(f'{what}: the PauliSum is for {paulis.nqubit} qubits, the system register has {m} wires')
            if phases is not None:
                raise ValueError(f'{what}: the phases of a PauliSum are the signs of its coefficients; phases must be None')
            # (a term's masks are over the PauliSum's own index bits: wire w of it is bit m - 1 - w)
            strings = [[(('y' if x >> (m - 1 - w) & z >> (m - 1 - w) & 1 else 'x' if x >> (m - 1 - w) & 1 else 'z'), w)
                        for w in range(m) if (x | z) >> (m - 1 - w) & 1] for _, x, z in paulis.terms]
            phases = [0 if h > 0 else 2 for h, _, _ in paulis.terms]
        else:
            if not isinstance(paulis, (list, tuple)) or not all(isinstance(p, str) for p in paulis) or not paulis:
                raise ValueError(f"{what}: paulis is a PauliSum or a non-empty list of strings such as ['x0y2', '']")
            strings = [HamiltonianGate._terms([[1.0, p]])[0][1] for p in paulis]
            for p, factors in zip(paulis, strings):
                if ''.join(f'{a}{w}' for a, w in factors) != p.lower().replace(' ', ''):
                    raise ValueError(f'{what}: {p!r} is not a string of factors such as x0y2')
        if len(strings) > 2**k:
            raise ValueError(f'{what}: too many strings for {k} select wires: {len(strings)} > {2**k}')
        phases = [0] * len(strings) if phases is None else list(phases)
        if len(phases) != len(strings):
            raise ValueError(f'{what}: {len(phases)} phases for {len(strings)} strings')
        if any(not isinstance(q, int) or q < 0 or q > 3 for q in phases):
            raise ValueError(f'{what}: a phase is a power of i in 0..3, got {phases}')
        entries = []
        for factors in strings:
            string = ''.join(f'{a}{w}' for a, w in factors)
            ws = [w for _, w in factors]
            if len(set(ws)) != len(ws):
                raise ValueError(f'{what}: a wire is repeated in {string!r}')
            if any(w >= m for w in ws):
                raise ValueError(f'{what}: {string!r} has a wire outside the system register of {m} wires')
            xmask = sum(1 << (n - 1 - system_wires[w]) for a, w in factors if a in 'xy')
            zmask = sum(1 << (n - 1 - system_wires[w]) for a, w in factors if a in 'yz')
            entries.append((xmask, zmask))
        entries += [(0, 0)] * (2**k - len(entries))
        phases += [0] * (2**k - len(phases))
        super().__init__(name=name, nqubit=n, wires=wires, controls=controls, den_mat=den_mat)
        self.system_wires = system_wires
        self.nstrings = len(strings)
        self.table = backend.SelectTable(n, [(x, z, q) for (x, z), q in zip(entries, phases)])
        self._mark_precision(torch.device('cpu'))        # (integer tables have no precision)

    def apply_flat(self, x: torch.Tensor) -> torch.Tensor:
        """(B, 2**n) -> (B, 2**n)."""
        from . import ops

        return ops.select_pauli(x, self.table, self._bits(self.wires), self._bits(self.controls), dagger=self.inv_mode)

    def extra_repr(self) -> str:
        s = f'wires={self.wires}, strings={self.nstrings}'
        return s if self.controls == [] else s + f', controls={self.controls}'
