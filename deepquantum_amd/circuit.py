"""``QubitCircuit`` and ``DistributedQubitCircuit``: the circuit driver, API-compatible with the
reference's circuit.py (:81-1623 and :1625-1770) for the statevector path.

Differences that matter for performance, none for results:

* ``forward`` does not loop over ``nn.Sequential(self.operators)`` gate by gate; it collects every
  operator's kernel primitives and lets ``executor.run`` fuse them into HBM passes (no-grad) or run
  one differentiable kernel per gate (autograd).
* 2-D ``data`` is not ``torch.vmap``-ed over the circuit: encoders receive the whole (B, npara) slice
  and produce batched (B, D, D) matrices; the kernels take a per-sample matrix stride.

Out of scope here: density matrices, MPS, channels, MBQC patterns, circuit cutting,
QASM, drawing -- the corresponding entry points raise ``NotImplementedError``.
"""

from __future__ import annotations

import math
import weakref

from copy import copy
from typing import Any

import numpy as np
import torch
from torch import nn

from . import _functorch, executor, ops, qmath
from .gate import (
    CNOT, Barrier, CostPhase, DiagonalGate, ExcitationGate, Fredkin, Hadamard, HamiltonianGate, ImaginarySwap, LatentGate, MultiplexedGate, MultiplexedRotation, PauliEvolution,
    PauliRot, PauliX, PauliY, PauliZ, PermutationGate, PhaseShift, ProjectionJ, ReconfigurableBeamSplitter, Reset, Rx, Rxx, Rxy, Ry, Ryy, Rz, Rzz, SDaggerGate, SGate, Swap,
    TDaggerGate, TGate, Toffoli, U3Gate, UAnyGate,
)
from .layer import CnotLayer, CnotRing, HLayer, Observable, RxLayer, RyLayer, RzLayer, U3Layer, XLayer, YLayer, ZLayer
from .channel import (
    AmplitudeDamping, BitFlip, Depolarizing, GeneralizedAmplitudeDamping, Pauli, PhaseDamping, PhaseFlip,
)
from .operation import Channel, Gate, Layer, Operation
from .qmath import amplitude_encoding, sample2expval, slice_state_vector
from .state import DistributedQubitState, QubitState


def _runs_flat(op: Any) -> bool:
    """The operator has no matrix primitive: it runs through ``apply_flat`` between two fused stretches -- ``Reset``
    (``_state_dependent``: its matrices depend on the state) and the diagonal gates (``_runs_flat``: a stand-alone pass)."""
    return getattr(op, '_state_dependent', False) or getattr(op, '_runs_flat', False)


class QubitCircuit(Operation):
    """A circuit on ``nqubit`` qubits: gate builders, ``cir(data, state)``, ``expectation()``,
    ``measure()``, ``get_unitary()``."""

    def __init__(
        self,
        nqubit: int,
        init_state: Any = 'zeros',
        name: str | None = None,
        den_mat: bool = False,
        reupload: bool = False,
        mps: bool = False,
        chi: int | None = None,
        shots: int = 1024,
    ) -> None:
        if mps:
            raise NotImplementedError('deepquantum_amd: matrix product states are out of scope (SURVEY section 2)')
        super().__init__(name=name, nqubit=nqubit, wires=None, den_mat=den_mat)
        self.reupload = reupload
        self.mps = False
        self.chi = chi
        self.shots = shots
        self.set_init_state(init_state)
        self.operators = nn.Sequential()
        self.encoders: list = []
        self.observables = nn.ModuleList()
        self.state = None
        self.ndata = 0
        self.depth = np.array([0] * nqubit)
        self.wires_measure: list[int] = []
        self.wires_condition: list[int] = []

    # ---- state / bookkeeping ------------------------------------------------------------------------
    def set_init_state(self, init_state: Any) -> None:
        if isinstance(init_state, QubitState):
            assert self.nqubit == init_state.nqubit
            self.den_mat = init_state.den_mat
            self.init_state = init_state
        else:
            self.init_state = QubitState(nqubit=self.nqubit, state=init_state, den_mat=self.den_mat)

    def __add__(self, rhs: 'QubitCircuit') -> 'QubitCircuit':
        assert self.nqubit == rhs.nqubit
        cir = QubitCircuit(nqubit=self.nqubit, init_state=self.init_state, name=self.name, den_mat=self.den_mat,
                           reupload=self.reupload)
        cir.operators = self.operators + rhs.operators
        cir.encoders = self.encoders + rhs.encoders
        cir.observables = rhs.observables
        cir.npara = self.npara + rhs.npara
        cir.ndata = self.ndata + rhs.ndata
        cir.depth = self.depth + rhs.depth
        cir.wires_measure = rhs.wires_measure
        cir.wires_condition = list(set(self.wires_condition + rhs.wires_condition))
        return cir

    def init_para(self) -> None:
        for op in self.operators:
            op.init_para()

    def init_encoder(self) -> None:
        """Re-draw the encoder parameters (scrubs batched buffers before ``state_dict()``)."""
        for op in self.encoders:
            op.init_para()

    def reset_circuit(self, init_state: Any = 'zeros') -> None:
        self.set_init_state(init_state)
        self.operators = nn.Sequential()
        self.encoders = []
        self.observables = nn.ModuleList()
        self.state = None
        self.npara = 0
        self.ndata = 0
        self.depth = np.array([0] * self.nqubit)
        self.wires_measure = []
        self.wires_condition = []

    def amplitude_encoding(self, data: Any) -> torch.Tensor:
        return amplitude_encoding(data, self.nqubit)

    def observable(self, wires: int | list[int] | None = None, basis: str = 'z') -> None:
        self.observables.append(Observable(nqubit=self.nqubit, wires=wires, basis=basis, den_mat=self.den_mat,
                                           tsr_mode=False))

    def reset_observable(self) -> None:
        self.observables = nn.ModuleList()

    @property
    def max_depth(self) -> int:
        return max(self.depth)

    # ---- forward ------------------------------------------------------------------------------------
    def prims(self, decompose: bool = True) -> list:
        out = []
        for op in self.operators:
            out.extend(op.prims(decompose))
        return out

    def _apply(self, fn: Any, *args, **kwargs):
        # (the tiny buffers of all gates move in one copy per dtype: utils.BulkMove)
        from .utils import BulkMove

        if not isinstance(fn, BulkMove) and len(self.operators) >= 8:
            fn = BulkMove(fn, self)
        return super()._apply(fn, *args, **kwargs)

    def _run_operators(self, flat: torch.Tensor, zero: bool = False) -> torch.Tensor:
        """All operators on a (B, 2**n) state: maximal stretches of gates go to the executor (fused passes),
        the operations that run through ``apply_flat`` (``Reset``, ``DiagonalGate``, ``CostPhase``, ``PauliRot``, ``PauliEvolution``, ``PermutationGate``, ``MultiplexedGate``, ``MultiplexedRotation``, ``ExcitationGate``, ``SelectPauli``) run between them.  ``zero``: ``flat`` is |0..0> (vec |0..0><0..0| of a
        density matrix alike: index 0 is 1, everything else 0)."""
        if self.den_mat:
            prims = []
            for op in self.operators:
                prims.extend(op.dm_prims())
            return executor.run(flat, prims, zero_state=zero)
        nops = len(self.operators)
        last = id(self.operators[-1]) if nops else 0
        dep = self.__dict__.get('_state_dep')          # (operators it was computed for: how many, the last one; answer)
        if dep is None or dep[0] != nops or dep[1] != last:
            dep = self.__dict__['_state_dep'] = (nops, last, any(_runs_flat(op) for op in self.operators))
        if not dep[2]:
            # no-grad runs: the Z-type observables' values come out of the last pass (executor.run(expect_z=...))
            self._expz = None
            ez = None
            if not torch.is_grad_enabled() and len(self.observables) > 0:
                masks = sorted({ob.pauli_masks()[1] for ob in self.observables if ob.pauli_masks()[0] == 0})
                if masks and len(masks) <= 64:
                    ez = {'masks': masks}
            out = executor.run(flat, self.prims(), expect_z=ez, zero_state=zero)
            if ez is not None and ez.get('values') is not None:
                self._expz = ez
            return out
        x, pending = flat, []
        for op in self.operators:
            if _runs_flat(op):
                if pending:
                    x, pending = executor.run(x, pending, zero_state=zero), []
                zero = False
                x = op.apply_flat(x)
            else:
                pending.extend(op.prims())
        return executor.run(x, pending, zero_state=zero) if pending else x

    def _precompute_matrices(self) -> list:
        """Evaluate the matrices of all single-parameter gates of one class in ONE vectorised call
        (identical element-wise arithmetic, hence bit-identical values) instead of a handful of tiny
        device kernels per gate.  Returns the gates whose ``_precomputed`` must be cleared afterwards."""
        groups: dict = {}
        for op in self.operators:
            if getattr(op, '_param_names', None) == ('theta',) and type(op).get_matrix is not None:
                if op._fixed_matrix() is not None:   # fixed angle, unchanged since the last evaluation
                    continue
                th = op.theta
                key = (type(op), getattr(op, 'plane', None), th.dtype, th.device, th.numel())
                groups.setdefault(key, []).append(op)
        touched = []
        for (cls, _plane, _dt, _dev, numel), gates in groups.items():
            if len(gates) < 2:
                continue
            thetas = torch.stack([(-g.theta if g.inv_mode else g.theta).reshape(-1) for g in gates])  # (G, B)
            mats = gates[0].get_matrix(thetas.reshape(-1))
            d = mats.shape[-1]
            # one unbind instead of a select per gate: autograd then stacks the gates' matrix gradients in ONE kernel
            # (a select's backward is a zero-fill plus a copy per gate, and an add per gate to sum them up)
            parts = (mats.reshape(len(gates), numel, d, d) if numel > 1 else mats.reshape(len(gates), d, d)).unbind(0)
            for g, m in zip(gates, parts, strict=True):
                g.__dict__['_precomputed'] = m
                g.__dict__['_matrix_cache'] = m.detach()
                g._stamp()
                touched.append(g)
        return touched

    def __getstate__(self) -> dict:
        # the expectation values cached by the last pass belong to one state tensor of THIS object (a weak reference
        # says which): a pickled, saved or copied circuit starts without them
        d = self.__dict__.copy()
        d['_expz'] = None
        return d

    def forward(self, data: torch.Tensor | None = None, state: Any = None) -> torch.Tensor:
        """Run the circuit.  ``data``: 1-D (one sample) or 2-D (batch) encoder inputs; ``state``:
        (2**n, 1) or (B, 2**n, 1) initial state (default: the circuit's ``init_state``).  Returns the
        final state with the leading batch dimension the reference would return
        (reference: circuit.py:180-263)."""
        if state is None:
            state = self.init_state
        zero = False
        if isinstance(state, QubitState):
            # (the constructor's |0..0>, untouched since: the first passes skip what is still known to be zero)
            state, zero = state._state_and_claim()
        if self.ndata == 0:
            data = None
        self.state = None  # release the previous result first: the caching allocator hands the block back
        self._expz = None
        if data is None or data.ndim == 1:
            out = self._forward_helper(data, state, zero)
            if out.ndim == 2:
                out = out.unsqueeze(0)
            if state.ndim == 2:
                out = out.squeeze(0)
            self.state = out
        else:
            assert data.ndim == 2
            assert state.ndim in (2, 3)
            out = self._forward_helper(data, state, zero)
            if out.ndim == 2:          # batch of one sample
                out = out.unsqueeze(0)
            self.state = out
            self.encode(data[-1])
        if self._expz is not None:
            self._expz['state'] = weakref.ref(self.state)      # (the values belong to THIS tensor: `expectation` checks)
        return self.state

    def _forward_helper(self, data: torch.Tensor | None = None, state: Any = None, zero: bool = False) -> torch.Tensor:
        self.encode(data)
        if state is None:
            state = self.init_state
        if isinstance(state, QubitState):
            state, zero = state._state_and_claim()
        dim = 4**self.nqubit if self.den_mat else 2**self.nqubit
        flat = state.reshape(-1, dim)
        if data is not None and data.ndim == 2 and flat.shape[0] != data.shape[0]:
            assert flat.shape[0] == 1, 'batch of data and batch of states differ'
            flat = flat.expand(data.shape[0], dim)
        touched = self._precompute_matrices()
        try:
            x = self._run_operators(flat, zero)
        finally:
            for g in touched:
                g.__dict__['_precomputed'] = None
        if x is flat or (not executor.ops._is_wrapped(x) and not executor.ops._is_wrapped(state)
                         and x.data_ptr() == state.data_ptr()):
            x = x.clone()
        return (self.matrix_rep(x) if self.den_mat else self.vector_rep(x)).squeeze(0)

    def encode(self, data: torch.Tensor | None) -> None:
        """Feed ``data`` to the encoders in order; with ``reupload`` the data wraps around
        (reference: circuit.py:265-293).  ``data`` may be (ndata,) or (B, ndata)."""
        if data is None:
            return
        width = data.shape[-1]
        if not self.reupload:
            assert width >= self.ndata, 'The circuit needs more data, or consider data re-uploading'
        # Differentiated data: the columns come from ONE unbind -- one autograd node whose backward stacks the gates'
        # angle gradients in one kernel -- instead of a slice per layer and a slice per gate, whose backwards are a zero
        # fill, a copy and an add EACH (the reference's gradient benchmark at n = 8, 4 layers: 207 of a gradient's 365
        # launches).  Same views, same shapes, same values.
        if data.requires_grad and torch.is_grad_enabled() and not _functorch.is_wrapped_tensor(data):
            # The angles of the previous call are views into ITS autograd graph.  While one of them lives, so does the
            # AccumulateGrad node of the caller's leaf -- and the new graph made below would reuse that node, stream and all:
            # after eager steps on the default stream a capture of the step on another stream then dies in
            # hipStreamEndCapture (PyTorch warns about the mismatch; tests/test_circuit_gpu.py).  Let go of them first.
            for op in self.encoders:
                for gate in (op.gates if isinstance(op, Layer) else (op,)):
                    bufs = gate.__dict__.get('_buffers')
                    if bufs:
                        for name in getattr(gate, '_param_names', ()):
                            t = bufs.get(name)
                            # (plain autograd only: a wrapper that a torch.func transform left behind is not touched)
                            if t is not None and not _functorch.is_wrapped_tensor(t) and t.grad_fn is not None:
                                bufs[name] = t.detach()
                                gate.__dict__['_matrix_key'] = None        # (it names the old tensors; `init_para` drops it anyway)
                            t = None                                        # (this frame must not be the last holder either)
        cols = data.unbind(-1) if (data.requires_grad and torch.is_grad_enabled() and width > 1) else None

        def piece(src: torch.Tensor, a: int, b: int) -> torch.Tensor:      # src[..., a:b]
            if cols is None or src is not data or b <= a:
                return src[..., a:b]
            return cols[a].unsqueeze(-1) if b - a == 1 else torch.stack(cols[a:b], dim=-1)

        count = 0
        for op in self.encoders:
            count_up = count + op.npara
            src = data
            if self.reupload and count_up > width:
                reps = int(np.ceil(count_up / width))
                src = torch.cat([data] * reps, dim=-1)
            if type(op).init_para is Layer.init_para and count_up <= src.shape[-1]:
                at = count                 # (what Layer.init_para does with src[..., count:count_up], gate by gate)
                for gate in op.gates:
                    gate.init_para(piece(src, at, at + gate.npara))
                    at += gate.npara
            else:
                op.init_para(piece(src, count, count_up))
            count = count_up % width

    # ---- read-out -----------------------------------------------------------------------------------
    def measure(self, shots: int | None = None, with_prob: bool = False, wires: int | list[int] | None = None,
                block_size: int = 2**24, sampler: str = 'multinomial') -> dict | list[dict] | None:
        if shots is None:
            shots = self.shots
        else:
            self.shots = shots
        if wires is None:
            wires = list(range(self.nqubit))
        self.wires_measure = self._convert_indices(wires)
        if self.state is None:
            return None
        return qmath.measure(self.state, shots=shots, with_prob=with_prob, wires=self.wires_measure,
                             den_mat=self.den_mat, block_size=block_size, sampler=sampler)

    def sample(self, shots: int | None = None, wires: int | list[int] | None = None,
               generator: torch.Generator | None = None) -> torch.Tensor | None:
        """Raw measurement outcomes of the final state of the last forward as a device tensor: int64 (shots,), or
        (B, shots) for a batch -- see :func:`qmath.sample` for the outcome convention and ``generator``.  ``shots`` is
        kept as in :meth:`measure`."""
        if shots is None:
            shots = self.shots
        else:
            self.shots = shots
        if wires is None:
            wires = list(range(self.nqubit))
        self.wires_measure = self._convert_indices(wires)
        if self.state is None:
            return None
        return qmath.sample(self.state, self.nqubit, shots=shots, wires=self.wires_measure, generator=generator,
                            den_mat=self.den_mat)

    def reduced_density_matrix(self, wires: int | list[int]) -> torch.Tensor:
        """Reduced density matrix of ``wires`` (in that matrix order, ``wires[0]`` the most significant bit) of the final
        state of the last forward: (2**k, 2**k), or (B, 2**k, 2**k) for a batch.  A state vector goes through
        :func:`qmath.reduced_density_matrix` (1 to 10 wires, not normalised); a density matrix (``den_mat=True``)
        through :func:`qmath.partial_trace`."""
        if self.state is None:
            raise RuntimeError('reduced_density_matrix: run the circuit first')
        if self.den_mat:
            return qmath.density_matrix_rdm(self.state, self.nqubit, wires)
        return qmath.reduced_density_matrix(self.state, self.nqubit, wires)

    def entanglement_entropy(self, wires: int | list[int], alpha: float = 1.0, base: float | None = None) -> torch.Tensor:
        """Entropy of the normalised reduced density matrix of ``wires`` of the final state: (B,) real, or a 0-d tensor
        for a single state.  See :func:`qmath.entanglement_entropy` for ``alpha``, ``base`` and the eigenvalue cut-off.
        A density matrix is mixed, so there the entropy is that of ``wires`` themselves (no complement)."""
        if self.state is None:
            raise RuntimeError('entanglement_entropy: run the circuit first')
        if not self.den_mat:
            return qmath.entanglement_entropy(self.state, self.nqubit, wires, alpha=alpha, base=base)
        alpha = float(alpha)
        if not alpha > 0:
            raise ValueError(f'entanglement_entropy: alpha must be > 0, got {alpha}')
        rho = qmath.density_matrix_rdm(self.state, self.nqubit, wires)
        single = rho.ndim == 2
        rho = rho.unsqueeze(0) if single else rho
        tau = 1e-12 if rho.dtype == torch.complex128 else 1e-6
        val = qmath._entropy_of(rho, alpha, base, tau).to(rho.real.dtype)
        return val.squeeze(0) if single else val

    def expectation_cost(self, cost: torch.Tensor, wires: int | list[int] | None = None) -> torch.Tensor:
        """``<C> = sum_i cost[sub(i)] |psi_i|^2`` of the final state of the last forward for a classical cost table over
        ``wires`` (all by default): (B,) real, or 0-d for a single state; see :func:`qmath.expectation_cost`."""
        if self.state is None:
            raise RuntimeError('expectation_cost: run the circuit first')
        if self.den_mat:
            raise NotImplementedError('expectation_cost: den_mat=True (density matrices) is not supported')
        return qmath.expectation_cost(self.state, self.nqubit, cost, wires)

    def expectation_pauli_sum(self, H) -> torch.Tensor:
        """``Re <psi|H|psi>`` of the final state of the last forward for a sum of Pauli strings ``H`` -- a ``PauliSum`` or
        the list form ``[[0.5, 'x0y1'], [-1, 'z3y1'], [0.25, '']]``: (B,) real, or 0-d for a single state, the whole sum
        in one launch; see :func:`qmath.expectation_pauli_sum`."""
        if self.state is None:
            raise RuntimeError('expectation_pauli_sum: run the circuit first')
        if self.den_mat:
            raise NotImplementedError('expectation_pauli_sum: den_mat=True (density matrices) is not supported')
        return qmath.expectation_pauli_sum(self.state, self.nqubit, H)

    def kernel_matrix(self, x1: torch.Tensor, x2: torch.Tensor | None = None) -> torch.Tensor:
        """The fidelity kernel ``K[i, j] = |<phi(x1_i)|phi(x2_j)>|^2`` of the circuit as a feature map: the circuit runs on
        the rows of ``x1`` (and of ``x2``) as encoder data, as ``forward`` with 2-D data does, and every final state meets
        every other in one launch (:func:`qmath.fidelity_kernel`): real float64 (M, N).  ``x2=None``: the symmetric
        ``K(x1, x1)`` from one run and half the reads.  Differentiable in the circuit's trainable parameters
        (kernel-target alignment) and in the data."""
        what = 'kernel_matrix'
        if self.den_mat:
            raise NotImplementedError(f'{what}: den_mat=True (density matrices) is not supported: the kernel is an overlap '
                                      'of state vectors')
        if self.ndata == 0:
            raise ValueError(f'{what}: the circuit has no encoders (add gates with encode=True): every row would give one state')

        def states(x):
            if not isinstance(x, torch.Tensor) or x.ndim not in (1, 2):
                raise ValueError(f'{what}: data must be a (rows, ndata) tensor')
            out = self.forward(x.reshape(1, -1) if x.ndim == 1 else x)
            if not isinstance(out, torch.Tensor):
                raise NotImplementedError(f'{what}: the circuit returns a {type(out).__name__}, not a batch of state vectors')
            return out.reshape(out.shape[0], -1)

        a = states(x1)
        return qmath.fidelity_kernel(a, None if x2 is None else states(x2))

    def expectation(self, shots: int | None = None) -> torch.Tensor:
        """Expectation value of every registered observable, stacked on the last dimension
        (reference: circuit.py:381-428)."""
        assert len(self.observables) > 0, 'There is no observable'
        assert isinstance(self.state, torch.Tensor), 'There is no final state'
        assert self.wires_condition == [], 'Expectation with conditional measurement is NOT supported'
        out = []
        if shots is None:
            done = {}
            ez = getattr(self, '_expz', None)
            if ez is not None and ez.get('state') is not None and ez['state']() is self.state and not self.den_mat:
                # taken from the registers of the forward's last pass (DQ_FG_EXPZ): no read of the state
                single = self.state.ndim == 2
                for i, ob in enumerate(self.observables):
                    xm, zm = ob.pauli_masks()
                    if xm == 0 and zm in ez['masks']:
                        v = ez['values'][:, ez['masks'].index(zm)].to(self.state.real.dtype)
                        done[i] = v[0] if single else v
            if not self.den_mat and not ops._is_batched(self.state) and len(done) < len(self.observables):
                # all Z-type strings (the ZZ terms of a cost Hamiltonian, examples/qaoa.py:31-44) in one read of
                # the state instead of one pass each
                ztype = [(i, ob.pauli_masks()[1]) for i, ob in enumerate(self.observables)
                         if ob.pauli_masks()[0] == 0 and i not in done]
                if len(ztype) >= 2:
                    single = self.state.ndim == 2
                    flat = self.state.reshape(1 if single else self.state.shape[0], -1)
                    vals = ops.expect_z_multi(flat, [z for _, z in ztype])
                    for k, (i, _z) in enumerate(ztype):
                        done[i] = vals[0, k] if single else vals[:, k]
            for i, ob in enumerate(self.observables):
                out.append(done[i] if i in done else
                           qmath.expectation(self.state, observable=ob, den_mat=self.den_mat))
        else:
            self.shots = shots
            dtype, device = self.state.real.dtype, self.state.device
            for ob in self.observables:
                basis_cir = QubitCircuit(nqubit=self.nqubit, den_mat=self.den_mat)
                for wire, b in zip(ob.wires, ob.basis, strict=True):
                    if b == 'x':
                        basis_cir.h(wire)
                    elif b == 'y':
                        basis_cir.sdg(wire)
                        basis_cir.h(wire)
                basis_cir.to(device, dtype)
                with torch.no_grad():
                    basis_cir(state=self.state)
                samples = basis_cir.measure(shots=shots, wires=sum(ob.wires, []))
                if isinstance(samples, list):
                    ev = torch.cat([sample2expval(s).to(device, dtype) for s in samples])
                else:
                    ev = sample2expval(samples).to(device, dtype)
                    if self.state.ndim == 2:
                        ev = ev.squeeze(0)
                out.append(ev)
        return torch.stack(out, dim=-1)

    def defer_measure(self, with_prob: bool = False):
        rst = self.measure(shots=1, with_prob=with_prob, wires=self.wires_condition)
        if self.state.ndim == 2:
            key = [*rst][0]
            state = self._slice_state_vector(self.state, self.wires_condition, key)
            return (state, key, rst[key][1]) if with_prob else state
        states, keys, probs = [], [], []
        for i, d in enumerate(rst):
            key = [*d][0]
            states.append(self._slice_state_vector(self.state[i], self.wires_condition, key))
            if with_prob:
                keys.append(key)
                probs.append(d[key][1])
        return (torch.stack(states), keys, probs) if with_prob else torch.stack(states)

    def post_select(self, bits: str) -> torch.Tensor:
        return self._slice_state_vector(self.state, self.wires_condition, bits)

    def _slice_state_vector(self, state: torch.Tensor, wires: int | list[int], bits: str, normalize: bool = True):
        return slice_state_vector(state, self.nqubit, self._convert_indices(wires), bits, normalize)

    def get_unitary(self) -> torch.Tensor:
        """2^n x 2^n matrix of the circuit: the gate kernels applied to all columns of the identity at
        once (batch = 2^n), instead of the reference's chain of Kronecker-built dense GEMMs
        (reference: circuit.py:467-477)."""
        ops_ = [op for op in self.operators if not isinstance(op, Barrier)]
        if not ops_:
            return torch.eye(2**self.nqubit, dtype=torch.cfloat)
        flat = [op for op in ops_ if getattr(op, '_runs_flat', False)]
        if flat:             # (no matrix primitive: the columns of the identity go through the circuit as a batch)
            dtype, device = flat[0]._state_like()
            cols = self._run_operators(torch.eye(2**self.nqubit, dtype=dtype, device=device))
            return cols.T.contiguous() if not cols.requires_grad else cols.T
        prims = self.prims(decompose=True)
        if not prims:
            return torch.eye(2**self.nqubit, dtype=torch.cfloat)
        ref = prims[0].matrix
        eye = torch.eye(2**self.nqubit, dtype=ref.dtype, device=ref.device)
        cols = executor.run(eye, prims)
        return cols.T.contiguous() if not cols.requires_grad else cols.T

    def get_amplitude(self, bits: str) -> torch.Tensor:
        assert len(bits) == self.nqubit
        idx = int(bits, 2)
        return self.state.reshape(-1, 2**self.nqubit)[:, idx].squeeze()

    def get_prob(self, bits: str, wires: int | list[int] | None = None) -> torch.Tensor:
        if wires is not None:
            wires = self._convert_indices(wires)
            if len(wires) != self.nqubit:
                sub = slice_state_vector(self.state.reshape(1, -1) if self.state.ndim == 2 else self.state,
                                         self.nqubit, wires, bits, False)
                p = (torch.abs(sub) ** 2).sum(-1)
                return p.squeeze(0) if self.state.ndim == 2 else p
        return torch.abs(self.get_amplitude(bits)) ** 2

    def inverse(self, encode: bool = False) -> 'QubitCircuit':
        name = self.name + '_inverse' if isinstance(self.name, str) else self.name
        cir = QubitCircuit(nqubit=self.nqubit, name=name, den_mat=self.den_mat, reupload=self.reupload)
        for op in reversed(self.operators):
            inv = op.inverse()
            cir.add(inv)
            if encode and op in self.encoders:
                cir.encoders.append(inv)
        cir.wires_condition = self.wires_condition
        if encode:
            cir.npara, cir.ndata = self.npara, self.ndata
        else:
            cir.npara, cir.ndata = self.npara + self.ndata, 0
        return cir

    # ---- construction -------------------------------------------------------------------------------
    def add(self, op: Operation, encode: bool = False, wires: int | list[int] | None = None,
            controls: int | list[int] | None = None) -> None:
        """Append a gate, a layer or another circuit (reference: circuit.py:820-897)."""
        assert isinstance(op, Operation)
        if wires is not None:
            assert isinstance(op, Gate)
            wires = self._convert_indices(wires)
            controls = self._convert_indices([] if controls is None else controls)
            assert not set(wires) & set(controls), 'Use repeated wires'
            assert len(wires) == len(op.wires), 'Invalid input'
            op = copy(op)
            op.wires = wires
            op.controls = controls
        if isinstance(op, QubitCircuit):
            assert self.nqubit == op.nqubit
            self.operators += op.operators
            self.encoders += op.encoders
            self.observables = op.observables
            self.npara += op.npara
            self.ndata += op.ndata
            self.depth += op.depth
            self.wires_measure = op.wires_measure
            self.wires_condition = list(set(self.wires_condition + op.wires_condition))
            return
        op.tsr_mode = True
        if isinstance(op, Channel):
            assert self.den_mat, 'channels act on density matrices: QubitCircuit(..., den_mat=True)'
            self.operators.append(op)
            self.depth[op.wires[0]] += 1
        elif isinstance(op, Gate):
            op.den_mat = self.den_mat
            self.operators.append(op)
            for i in op.wires + op.controls:
                self.depth[i] += 1
            if op.condition:
                self.wires_condition = list(set(self.wires_condition + op.controls))
        elif isinstance(op, Layer):
            for gate in op.gates:
                gate.den_mat = self.den_mat
            self.operators.extend(op.gates)
            for wire in op.wires:
                for i in wire:
                    self.depth[i] += 1
        else:
            raise NotImplementedError(f'{type(op).__name__} is outside the statevector path')
        if encode:
            assert not op.requires_grad, 'Please set requires_grad of the operation to be False'
            self.encoders.append(op)
            self.ndata += op.npara
        else:
            self.npara += op.npara

    def _add_param(self, cls, wires, inputs, controls, condition, encode, **extra) -> None:
        requires_grad = (not encode) and inputs is None
        gate = cls(inputs=inputs, nqubit=self.nqubit, wires=wires, controls=controls, condition=condition,
                   requires_grad=requires_grad, **extra)
        self.add(gate, encode=encode)

    def _add_fixed(self, cls, wires, controls=None, condition=False) -> None:
        self.add(cls(nqubit=self.nqubit, wires=wires, controls=controls, condition=condition))

    # single-qubit, parametric
    def u3(self, wires, inputs=None, controls=None, condition=False, encode=False):
        self._add_param(U3Gate, wires, inputs, controls, condition, encode)

    def cu(self, control, target, inputs=None, encode=False):
        self._add_param(U3Gate, [target], inputs, [control], False, encode)

    def p(self, wires, inputs=None, controls=None, condition=False, encode=False):
        self._add_param(PhaseShift, wires, inputs, controls, condition, encode)

    def cp(self, control, target, inputs=None, encode=False):
        self._add_param(PhaseShift, [target], inputs, [control], False, encode)

    def rx(self, wires, inputs=None, controls=None, condition=False, encode=False):
        self._add_param(Rx, wires, inputs, controls, condition, encode)

    def ry(self, wires, inputs=None, controls=None, condition=False, encode=False):
        self._add_param(Ry, wires, inputs, controls, condition, encode)

    def rz(self, wires, inputs=None, controls=None, condition=False, encode=False):
        self._add_param(Rz, wires, inputs, controls, condition, encode)

    def crx(self, control, target, inputs=None, encode=False):
        self._add_param(Rx, [target], inputs, [control], False, encode)

    def cry(self, control, target, inputs=None, encode=False):
        self._add_param(Ry, [target], inputs, [control], False, encode)

    def crz(self, control, target, inputs=None, encode=False):
        self._add_param(Rz, [target], inputs, [control], False, encode)

    def j(self, wires, inputs=None, plane='xy', controls=None, condition=False, encode=False):
        self._add_param(ProjectionJ, wires, inputs, controls, condition, encode, plane=plane)

    # single-qubit, fixed
    def x(self, wires, controls=None, condition=False):
        self._add_fixed(PauliX, wires, controls, condition)

    def y(self, wires, controls=None, condition=False):
        self._add_fixed(PauliY, wires, controls, condition)

    def z(self, wires, controls=None, condition=False):
        self._add_fixed(PauliZ, wires, controls, condition)

    def h(self, wires, controls=None, condition=False):
        self._add_fixed(Hadamard, wires, controls, condition)

    def s(self, wires, controls=None, condition=False):
        self._add_fixed(SGate, wires, controls, condition)

    def sdg(self, wires, controls=None, condition=False):
        self._add_fixed(SDaggerGate, wires, controls, condition)

    def t(self, wires, controls=None, condition=False):
        self._add_fixed(TGate, wires, controls, condition)

    def tdg(self, wires, controls=None, condition=False):
        self._add_fixed(TDaggerGate, wires, controls, condition)

    def ch(self, control, target):
        self._add_fixed(Hadamard, [target], [control])

    def cs(self, control, target):
        self._add_fixed(SGate, [target], [control])

    def csdg(self, control, target):
        self._add_fixed(SDaggerGate, [target], [control])

    def ct(self, control, target):
        self._add_fixed(TGate, [target], [control])

    def ctdg(self, control, target):
        self._add_fixed(TDaggerGate, [target], [control])

    # two- and three-qubit
    def cnot(self, control, target):
        self.add(CNOT(nqubit=self.nqubit, wires=[control, target]))

    def cx(self, control, target):
        self._add_fixed(PauliX, [target], [control])

    def cy(self, control, target):
        self._add_fixed(PauliY, [target], [control])

    def cz(self, control, target):
        self._add_fixed(PauliZ, [target], [control])

    def swap(self, wires, controls=None, condition=False):
        self._add_fixed(Swap, wires, controls, condition)

    def iswap(self, wires, controls=None, condition=False):
        self._add_fixed(ImaginarySwap, wires, controls, condition)

    def rxx(self, wires, inputs=None, controls=None, condition=False, encode=False):
        self._add_param(Rxx, wires, inputs, controls, condition, encode)

    def ryy(self, wires, inputs=None, controls=None, condition=False, encode=False):
        self._add_param(Ryy, wires, inputs, controls, condition, encode)

    def rzz(self, wires, inputs=None, controls=None, condition=False, encode=False):
        self._add_param(Rzz, wires, inputs, controls, condition, encode)

    def rxy(self, wires, inputs=None, controls=None, condition=False, encode=False):
        self._add_param(Rxy, wires, inputs, controls, condition, encode)

    def rbs(self, wires, inputs=None, controls=None, condition=False, encode=False):
        self._add_param(ReconfigurableBeamSplitter, wires, inputs, controls, condition, encode)

    def crxx(self, control, target1, target2, inputs=None, encode=False):
        self._add_param(Rxx, [target1, target2], inputs, [control], False, encode)

    def cryy(self, control, target1, target2, inputs=None, encode=False):
        self._add_param(Ryy, [target1, target2], inputs, [control], False, encode)

    def crzz(self, control, target1, target2, inputs=None, encode=False):
        self._add_param(Rzz, [target1, target2], inputs, [control], False, encode)

    def crxy(self, control, target1, target2, inputs=None, encode=False):
        self._add_param(Rxy, [target1, target2], inputs, [control], False, encode)

    def toffoli(self, control1, control2, target):
        self.add(Toffoli(nqubit=self.nqubit, wires=[control1, control2, target]))

    def ccx(self, control1, control2, target):
        self._add_fixed(PauliX, [target], [control1, control2])

    def fredkin(self, control, target1, target2):
        self.add(Fredkin(nqubit=self.nqubit, wires=[control, target1, target2]))

    def cswap(self, control, target1, target2):
        self._add_fixed(Swap, [target1, target2], [control])

    # arbitrary
    def any(self, unitary, wires=None, minmax=None, controls=None, name='uany'):
        self.add(UAnyGate(unitary=unitary, nqubit=self.nqubit, wires=wires, minmax=minmax, controls=controls, name=name))

    def latent(self, wires=None, minmax=None, inputs=None, controls=None, encode=False, name='latent'):
        requires_grad = (not encode) and inputs is None
        self.add(LatentGate(inputs=inputs, nqubit=self.nqubit, wires=wires, minmax=minmax, controls=controls,
                            name=name, requires_grad=requires_grad), encode=encode)

    def hamiltonian(self, hamiltonian, t=None, wires=None, minmax=None, controls=None, encode=False,
                    name='hamiltonian'):
        requires_grad = (not encode) and t is None
        self.add(HamiltonianGate(hamiltonian=hamiltonian, t=t, nqubit=self.nqubit, wires=wires, minmax=minmax,
                                 controls=controls, name=name, requires_grad=requires_grad), encode=encode)

    def diagonal(self, diag, wires=None, minmax=None, controls=None, name='diagonal'):
        """A fixed diagonal unitary given by its 2^k entries (``wires[0]`` = the entry index's most significant bit; all
        wires by default): see :class:`DiagonalGate`."""
        self.add(DiagonalGate(diag=diag, nqubit=self.nqubit, wires=wires, minmax=minmax, controls=controls, name=name,
                              den_mat=self.den_mat))

    def permutation(self, perm, wires=None, minmax=None, controls=None, name='permutation'):
        """The classical reversible map ``|x> -> |perm(x)>`` given by its table of 2^k integers, a bijection of
        ``range(2^k)`` (``wires[0]`` = the most significant bit of ``x``; all wires by default): see
        :class:`PermutationGate`."""
        self.add(PermutationGate(perm=perm, nqubit=self.nqubit, wires=wires, minmax=minmax, controls=controls, name=name,
                                 den_mat=self.den_mat))

    def bit_oracle(self, f, xwires, ywires, controls=None, name='bit_oracle'):
        """``|x>|y> -> |x>|y xor f(x)>`` for a table ``f`` of 2^len(xwires) integers below 2^len(ywires), as one
        :class:`PermutationGate` on ``xwires + ywires`` (the first wire of each list = its most significant bit)."""
        xwires = [xwires] if isinstance(xwires, int) else list(xwires)
        ywires = [ywires] if isinstance(ywires, int) else list(ywires)
        f = torch.as_tensor(f).reshape(-1)
        if f.is_floating_point() or f.is_complex() or f.dtype == torch.bool:
            raise ValueError(f'bit_oracle: the table must hold integers, got {f.dtype}')
        f = f.to(torch.int64).cpu()
        kx, ky = len(xwires), len(ywires)
        if kx < 1 or ky < 1 or kx + ky > 31:
            raise ValueError(f'bit_oracle: at least one wire of each kind and at most 31 in all, got {kx} + {ky}')
        if f.shape[0] != 2**kx:
            raise ValueError(f'bit_oracle: f over {kx} wires has {2**kx} entries, got {f.shape[0]}')
        if int(f.min()) < 0 or int(f.max()) >= 2**ky:
            raise ValueError(f'bit_oracle: the values of f must lie in [0, {2**ky}), got {int(f.min())} .. {int(f.max())}')
        x = torch.arange(2**kx, dtype=torch.int64).reshape(-1, 1)
        y = torch.arange(2**ky, dtype=torch.int64).reshape(1, -1)
        perm = ((x << ky) | (y ^ f.reshape(-1, 1))).reshape(-1)
        self.permutation(perm, wires=xwires + ywires, controls=controls, name=name)

    def modmul(self, a, mod, wires=None, controls=None, name='modmul'):
        """``|x> -> |a x mod N>`` for ``x < N`` (``x >= N`` stays) on ``wires`` (all by default; the first = the most
        significant bit) in one pass and without ancillas; ``gcd(a, N) = 1`` and ``N <= 2^k`` are required."""
        if wires is None:
            wires = list(range(self.nqubit))
        wires = [wires] if isinstance(wires, int) else list(wires)
        self.permutation(qmath.modmul_table(a, mod, len(wires)), wires=wires, controls=controls, name=name)

    def multiplexer(self, unitaries, wires, controls=None, name='multiplexer'):
        """A multiplexer (uniformly controlled gate): ``unitaries[s]``, a table of shape (2^k, 2, 2), on the LAST wire of
        ``wires`` for every value s of the k wires before it (``wires[0]`` = the most significant bit of s): see
        :class:`MultiplexedGate`."""
        self.add(MultiplexedGate(unitaries=unitaries, nqubit=self.nqubit, wires=wires, controls=controls, name=name,
                                 den_mat=self.den_mat))

    def ucr(self, axis, angles=None, wires=None, controls=None, name=None, requires_grad=False):
        """A multiplexed rotation: ``R_axis(angles[s])`` (``axis`` one of 'x', 'y', 'z') on the LAST wire of ``wires`` for
        every value s of the k wires before it (``wires[0]`` = the most significant bit of s), 2^k angles: fixed, or with
        ``requires_grad=True`` one trainable parameter of 2^k entries (``angles=None``: random): see
        :class:`MultiplexedRotation`."""
        if wires is None:
            raise ValueError('ucr: wires lists at least one select wire and then the target')
        if angles is None and not requires_grad:
            raise ValueError('ucr: angles=None (random angles) needs requires_grad=True')
        self.add(MultiplexedRotation(axis=axis, angles=angles, nqubit=self.nqubit, wires=wires, controls=controls,
                                     name=name or f'ucr{axis}', den_mat=self.den_mat, requires_grad=requires_grad))

    def ucrx(self, angles=None, wires=None, controls=None, requires_grad=False):
        self.ucr('x', angles, wires, controls=controls, requires_grad=requires_grad)

    def ucry(self, angles=None, wires=None, controls=None, requires_grad=False):
        self.ucr('y', angles, wires, controls=controls, requires_grad=requires_grad)

    def ucrz(self, angles=None, wires=None, controls=None, requires_grad=False):
        self.ucr('z', angles, wires, controls=controls, requires_grad=requires_grad)

    def prepare_state(self, state, wires=None, controls=None):
        """Appends the gates that map ``|0..0>`` of ``wires`` (all by default) to the vector ``state`` of 2^k entries,
        ``wires[0]`` the most significant bit of its index -- anywhere in a circuit, on some of the wires, under controls:
        one ``ry``, k - 1 multiplexed Ry of 1 .. k - 1 select wires, and a diagonal of the phases (left out for a real
        non-negative vector).  The vector is normalised, and the angles are formed, in float64."""
        if wires is None:
            wires = list(range(self.nqubit))
        wires = [wires] if isinstance(wires, int) else list(wires)
        k = len(wires)
        phi = torch.as_tensor(state).detach().cpu().reshape(-1)
        phi = phi.to(torch.complex128)
        if k < 1 or phi.shape[0] != 2**k:
            raise ValueError(f'prepare_state: a state on {k} wires has {2**k} entries, got {phi.shape[0]}')
        norm = float(torch.linalg.vector_norm(phi))
        if not norm > 0.0 or norm == float('inf'):
            raise ValueError('prepare_state: the vector must have a finite, non-zero norm')
        phi = phi / norm
        p = phi.real**2 + phi.imag**2
        for j in range(k):
            pj = p.reshape(2**j, 2, -1).sum(-1)
            theta = 2 * torch.atan2(pj[:, 1].sqrt(), pj[:, 0].sqrt())           # (an empty branch: atan2(0, 0) = 0)
            if j == 0:
                self.ry(wires[0], inputs=theta[0], controls=controls)
            else:
                self.ucry(theta, wires[:j] + [wires[j]], controls=controls)
        if bool((phi.imag != 0).any()) or bool((phi.real < 0).any()):
            self.diagonal(torch.exp(1j * torch.angle(phi)), wires=wires, controls=controls, name='prepare_state_phase')

    def cost_phase(self, cost, wires=None, minmax=None, inputs=None, controls=None, encode=False, name='cost_phase'):
        """``exp(-i t diag(cost))`` for a table of 2^k real costs (all wires by default) with one parameter ``t``: trainable,
        given by ``inputs``, or fed from ``data`` with ``encode=True``: see :class:`CostPhase`."""
        requires_grad = (not encode) and inputs is None
        self.add(CostPhase(cost=cost, nqubit=self.nqubit, wires=wires, minmax=minmax, inputs=inputs, controls=controls,
                           name=name, den_mat=self.den_mat, requires_grad=requires_grad), encode=encode)

    def pauli_rot(self, pauli, wires=None, inputs=None, controls=None, encode=False, name='pauli_rot'):
        """``exp(-i theta/2 P)`` for the Pauli string ``pauli`` (one letter of ``xyzi`` per wire of ``wires``; all wires by
        default) with one parameter ``theta``: trainable, given by ``inputs``, or fed from ``data`` with ``encode=True``:
        see :class:`PauliRot`."""
        requires_grad = (not encode) and inputs is None
        self.add(PauliRot(pauli=pauli, nqubit=self.nqubit, wires=wires, inputs=inputs, controls=controls, name=name,
                          den_mat=self.den_mat, requires_grad=requires_grad), encode=encode)

    def pauli_evolution(self, hamiltonian, t=None, steps=1, order=1, encode=False, name='pauli_evolution'):
        """A first- or second-order Trotter product of ``steps`` slices for ``exp(-i H t)``, ``H`` a list such as
        ``[[0.5, 'x0y1'], [-1, 'z3y1']]``, with one parameter ``t``: see :class:`PauliEvolution`."""
        requires_grad = (not encode) and t is None
        self.add(PauliEvolution(hamiltonian=hamiltonian, t=t, nqubit=self.nqubit, steps=steps, order=order, name=name,
                                den_mat=self.den_mat, requires_grad=requires_grad), encode=encode)

    def pauli_sum_evolution(self, hamiltonian, t=None, tol=None, encode=False, name='pauli_sum_evolution', bounds=None):
        """``exp(-i H t)`` for ``H`` a list such as ``[[0.5, 'x0y1'], [-1, 'z3y1'], [0.25, '']]`` or a ``PauliSum``, to the
        tolerance ``tol`` whether or not the strings commute (a Chebyshev expansion, no Trotter error), with one parameter
        ``t`` -- trainable, given, or fed from ``data`` with ``encode=True``: see :class:`PauliSumEvolution`.  ``bounds=(lo,
        hi)``: an interval that holds the spectrum of H (``PauliSum.spectral_bounds``), for fewer orders."""
        from .pauli_sum import PauliSumEvolution

        requires_grad = (not encode) and t is None
        self.add(PauliSumEvolution(hamiltonian=hamiltonian, t=t, nqubit=self.nqubit, tol=tol, name=name, den_mat=self.den_mat,
                                   requires_grad=requires_grad, bounds=bounds), encode=encode)

    def select_pauli(self, paulis, wires, system_wires=None, phases=None, controls=None):
        """SELECT ``sum_s |s><s| (x) i^phases[s] P_s``: for every value s of the select wires ``wires`` (``wires[0]`` = the
        most significant bit of s) the Pauli string ``paulis[s]`` on ``system_wires`` (``paulis``: a list of strings such as
        ``['x0y2', '']``, or a ``PauliSum``, whose signs become the phases), in one pass: see :class:`SelectPauli`."""
        from .pauli_sum import SelectPauli

        self.add(SelectPauli(paulis=paulis, nqubit=self.nqubit, wires=wires, system_wires=system_wires, phases=phases,
                             controls=controls, den_mat=self.den_mat))

    def block_encode(self, H, wires, system_wires=None, controls=None) -> float:
        """Appends the block encoding ``PREPARE^dagger SELECT PREPARE`` of ``H = sum_t h_t P_t`` (a ``PauliSum`` on
        ``len(system_wires)`` wires, or its list form) with the select wires ``wires``, at least ``H.select_bits`` of them,
        and returns ``lam = sum_t |h_t|``, the constant term included (``H.norm_bound + |H.constant|`` but for the upward
        rounding of ``norm_bound``).  PREPARE is the ``ry`` / ``ucry`` sequence of :meth:`prepare_state` for the real vector
        ``sqrt(|h_t| / lam)`` on the select wires, SELECT one :class:`SelectPauli` with the signs of the ``h_t`` -- the only
        part under ``controls`` --, PREPARE^dagger the same rotations in reverse order with negated angles.  The circuit U so
        appended is Hermitian and unitary, and ``(<0|_select (x) 1) U (|0>_select (x) 1) = H / lam``."""
        from .pauli_sum import PauliSum, SelectPauli

        wires = [wires] if isinstance(wires, int) else list(wires)
        ctrl = [] if controls is None else [controls] if isinstance(controls, int) else list(controls)
        if system_wires is None:
            system_wires = [w for w in range(self.nqubit) if w not in wires and w not in ctrl]
        if not isinstance(H, PauliSum):
            try:
                H = PauliSum(H, len(system_wires))
            except ValueError as exc:
                raise ValueError(f'block_encode: {exc}') from exc
        if len(wires) < H.select_bits:
            raise ValueError(f'block_encode: {H.nterms} strings need at least {H.select_bits} select wires, got {len(wires)}')
        select = SelectPauli(paulis=H, nqubit=self.nqubit, wires=wires, system_wires=system_wires, controls=controls,
                             den_mat=self.den_mat)
        weights = [abs(h) for h, _, _ in H.terms]
        lam = math.fsum(weights)
        amplitude = torch.zeros(2 ** len(wires), dtype=torch.float64)
        amplitude[:len(weights)] = torch.tensor(weights, dtype=torch.float64).div(lam).sqrt()
        start = len(self.operators)
        self.prepare_state(amplitude, wires=wires)
        prepare = self.operators[start:]
        self.add(select)
        for op in reversed(prepare):
            self.add(op.inverse())
        return lam

    def qubitization_walk(self, H, wires, system_wires=None) -> float:
        """Appends the qubitization walk operator ``W = (2 |0><0| - 1)_select U`` of ``H``: :meth:`block_encode` and then the
        reflection about ``|0..0>`` of the select wires, a diagonal ``[1, -1, .., -1]``.  Returns ``lam``: on an eigenvector
        of H with eigenvalue E, ``<0, psi| W^j |0, psi> = cos(j arccos(E / lam))``."""
        lam = self.block_encode(H, wires, system_wires=system_wires)
        wires = [wires] if isinstance(wires, int) else list(wires)
        reflection = -torch.ones(2 ** len(wires), dtype=torch.cfloat)
        reflection[0] = 1
        self.diagonal(reflection, wires=wires, name='qubitization_reflection')
        return lam

    def excitation(self, create, annihilate, inputs=None, controls=None, fermionic=True, encode=False, name='excitation'):
        """``exp(theta (E - E^dagger))`` for ``E = a^dagger_{create[0]} .. a_{annihilate[0]} ..`` (Jordan-Wigner over wire
        numbers; ``fermionic=False``: the qubit excitation without the string), a rotation by the full angle ``theta`` that
        touches only its subspace.  ``theta`` is trainable, given by ``inputs``, or fed from ``data`` with ``encode=True``:
        see :class:`ExcitationGate`."""
        requires_grad = (not encode) and inputs is None
        self.add(ExcitationGate(create=create, annihilate=annihilate, nqubit=self.nqubit, inputs=inputs, controls=controls,
                                fermionic=fermionic, requires_grad=requires_grad, name=name, den_mat=self.den_mat),
                 encode=encode)

    def single_excitation(self, wires, inputs=None, controls=None, fermionic=True, encode=False):
        """The single excitation from wire ``p`` to wire ``q`` of ``wires=[p, q]``: ``create=[q], annihilate=[p]``."""
        if len(wires) != 2:
            raise ValueError(f'single_excitation: wires=[p, q] expected, got {wires}')
        self.excitation([wires[1]], [wires[0]], inputs=inputs, controls=controls, fermionic=fermionic, encode=encode,
                        name='single_excitation')

    def double_excitation(self, wires, inputs=None, controls=None, fermionic=True, encode=False):
        """The double excitation from wires ``p, q`` to ``r, s`` of ``wires=[p, q, r, s]``: ``create=[r, s], annihilate=[p, q]``."""
        if len(wires) != 4:
            raise ValueError(f'double_excitation: wires=[p, q, r, s] expected, got {wires}')
        self.excitation(list(wires[2:]), list(wires[:2]), inputs=inputs, controls=controls, fermionic=fermionic, encode=encode,
                        name='double_excitation')

    # layers
    def xlayer(self, wires=None):
        self.add(XLayer(nqubit=self.nqubit, wires=wires))

    def ylayer(self, wires=None):
        self.add(YLayer(nqubit=self.nqubit, wires=wires))

    def zlayer(self, wires=None):
        self.add(ZLayer(nqubit=self.nqubit, wires=wires))

    def hlayer(self, wires=None):
        self.add(HLayer(nqubit=self.nqubit, wires=wires))

    def _add_param_layer(self, cls, wires, inputs, encode):
        requires_grad = (not encode) and inputs is None
        self.add(cls(nqubit=self.nqubit, wires=wires, inputs=inputs, requires_grad=requires_grad), encode=encode)

    def rxlayer(self, wires=None, inputs=None, encode=False):
        self._add_param_layer(RxLayer, wires, inputs, encode)

    def rylayer(self, wires=None, inputs=None, encode=False):
        self._add_param_layer(RyLayer, wires, inputs, encode)

    def rzlayer(self, wires=None, inputs=None, encode=False):
        self._add_param_layer(RzLayer, wires, inputs, encode)

    def u3layer(self, wires=None, inputs=None, encode=False):
        self._add_param_layer(U3Layer, wires, inputs, encode)

    def cxlayer(self, wires=None):
        self.add(CnotLayer(nqubit=self.nqubit, wires=wires))

    def cnot_ring(self, minmax=None, step=1, reverse=False):
        self.add(CnotRing(nqubit=self.nqubit, minmax=minmax, step=step, reverse=reverse))

    def barrier(self, wires=None):
        self.add(Barrier(nqubit=self.nqubit, wires=wires))

    def reset(self, wires=None, postselect=0):
        """Add a reset operation (reference: circuit.py:1603-1607)."""
        assert not self.den_mat and not self.mps, 'Currently NOT supported'
        self.add(Reset(nqubit=self.nqubit, wires=wires, postselect=postselect))

    # explicitly out of scope -----------------------------------------------------------------------
    def _out_of_scope(self, *a, **k):
        raise NotImplementedError('outside the accelerated statevector path (SURVEY section 2, OUT OF SCOPE)')

    pattern = draw = transform_cut2move = get_subexperiments = _out_of_scope

    def qasm(self) -> str:
        """OpenQASM 2.0 text of the circuit (reference: circuit.py:570-627)."""
        from .qasm3 import cir_to_qasm2

        for op in self.operators:
            if getattr(op, '_runs_flat', False):
                op.qasm_refusal()
        return cir_to_qasm2(self)

    # noise channels (density matrices only; reference: circuit.py:1540-1601) ---------------------------
    def _add_channel(self, cls, wires, inputs, encode) -> None:
        assert self.den_mat, 'channels act on density matrices: QubitCircuit(..., den_mat=True)'
        requires_grad = not encode and inputs is None
        self.add(cls(inputs=inputs, nqubit=self.nqubit, wires=wires, requires_grad=requires_grad), encode=encode)

    def bit_flip(self, wires, inputs=None, encode=False):
        self._add_channel(BitFlip, wires, inputs, encode)

    def phase_flip(self, wires, inputs=None, encode=False):
        self._add_channel(PhaseFlip, wires, inputs, encode)

    def depolarizing(self, wires, inputs=None, encode=False):
        self._add_channel(Depolarizing, wires, inputs, encode)

    def pauli(self, wires, inputs=None, encode=False):
        self._add_channel(Pauli, wires, inputs, encode)

    def amp_damp(self, wires, inputs=None, encode=False):
        self._add_channel(AmplitudeDamping, wires, inputs, encode)

    def phase_damp(self, wires, inputs=None, encode=False):
        self._add_channel(PhaseDamping, wires, inputs, encode)

    def gen_amp_damp(self, wires, inputs=None, encode=False):
        self._add_channel(GeneralizedAmplitudeDamping, wires, inputs, encode)
    cut = move = _out_of_scope


class DistributedQubitCircuit(QubitCircuit):
    """Circuit on an index-bit-sharded state, one process per GPU (reference: circuit.py:1625-1770)."""

    def __init__(self, nqubit: int, name: str | None = None, reupload: bool = False, shots: int = 1024) -> None:
        super().__init__(nqubit=nqubit, init_state='zeros', name=name, reupload=reupload, shots=shots)
        #: extension (off = the reference's behaviour: ``forward`` returns the shards in canonical qubit order).  On: the
        #: qubits stay where the circuit's last remap put them; expectation values of Pauli strings are taken from the
        #: shards as they lie, and the canonical order is restored -- one or two collective exchanges -- the first time
        #: ``state.amps`` is read.  That read must then happen on EVERY rank (a collective hides behind it); code that
        #: looks at the amplitudes on one rank only must leave this off.
        self.lazy_layout = False

    def set_init_state(self, init_state: Any = 'zeros') -> None:
        if isinstance(init_state, DistributedQubitState):
            self.init_state = init_state
        elif init_state == 'zeros':
            self.init_state = DistributedQubitState(self.nqubit)

    @torch.no_grad()
    def forward(self, data: torch.Tensor | None = None, state: DistributedQubitState | None = None):
        """Run the circuit on the sharded state.  ``data`` may be 1-D (as in the reference) or 2-D: then every
        rank holds one shard per sample, (B, 2^L), and the whole batch moves through the same kernels and
        exchange steps (extension; the reference's sharded state has no batch dimension)."""
        from .distributed import dist_run

        if self.ndata == 0:
            data = None
        batch = data.shape[0] if (data is not None and data.ndim == 2) else None
        if state is None:
            if self.init_state.batch != batch:
                old = self.init_state._buffers['amps']
                self.init_state = DistributedQubitState(self.nqubit, batch, device=old.device, dtype=old.dtype)
            self.init_state.reset(lazy=True)       # (the shard is cleared only if the passes behind |0..0> cannot do without)
            fresh = True
        else:
            self.init_state = state
            fresh = False
        with torch.enable_grad():
            self.encode(data)
        touched = self._precompute_matrices()
        try:
            masks = sorted({ob.pauli_masks()[1] for ob in self.observables if ob.pauli_masks()[0] == 0})
            # (only a no-grad forward reads the values: the adjoint `expectation()` of a training step never does)
            ez = masks if (masks and len(masks) <= 64 and executor.CONFIG['fused_expectation']
                           and not torch.is_grad_enabled()) else None
            self.state = dist_run(self.init_state, self.operators, keep_layout=self.lazy_layout, expect_z=ez, fresh_zero=fresh)
        finally:
            for g in touched:
                g.__dict__['_precomputed'] = None
        if batch is not None:
            self.encode(data[-1])
        return self.state

    def measure(self, shots=None, with_prob=False, wires=None, block_size=2**24):
        from .distributed import measure_dist

        if shots is None:
            shots = self.shots
        else:
            self.shots = shots
        if wires is None:
            wires = list(range(self.nqubit))
        self.wires_measure = self._convert_indices(wires)
        if self.state is None:
            return None
        return measure_dist(self.state, shots=shots, with_prob=with_prob, wires=self.wires_measure,
                            block_size=block_size)

    def reduced_density_matrix(self, wires: int | list[int]) -> torch.Tensor:
        raise NotImplementedError('reduced_density_matrix: sharded states are not supported')

    def entanglement_entropy(self, wires: int | list[int], alpha: float = 1.0, base: float | None = None) -> torch.Tensor:
        raise NotImplementedError('entanglement_entropy: sharded states are not supported')

    def expectation_pauli_sum(self, H) -> torch.Tensor:
        raise NotImplementedError('expectation_pauli_sum: sharded states are not supported')

    def kernel_matrix(self, x1: torch.Tensor, x2: torch.Tensor | None = None) -> torch.Tensor:
        raise NotImplementedError('kernel_matrix: sharded states are not supported')

    def expectation(self, shots: int | None = None) -> torch.Tensor:
        from . import executor
        from .adjoint import adjoint_expectation, adjoint_expectations

        assert len(self.observables) > 0, 'There is no observable'
        assert isinstance(self.state, DistributedQubitState), 'There is no final state'
        if shots is not None:
            # sampled estimate (reference circuit.py:1739-1758): rotate every observable into the Z basis on a copy of
            # the shards, sample its wires with measure_dist, average the parities; the value lives on rank 0 (the other
            # ranks return an empty tensor per observable, as in the reference)
            from copy import deepcopy

            from .distributed import measure_dist

            if self.state.batch is not None:
                raise NotImplementedError('sampled expectation values of a batched sharded state')
            self.shots = shots
            dtype, device = self.state.amps.real.dtype, self.state.amps.device
            out = []
            for ob in self.observables:
                cir_basis = DistributedQubitCircuit(self.nqubit)
                for wire, basis in zip(ob.wires, ob.basis, strict=True):
                    if basis == 'x':
                        cir_basis.h(wire)
                    elif basis == 'y':
                        cir_basis.sdg(wire)
                        cir_basis.h(wire)
                cir_basis.to(device)
                if dtype == torch.float64:
                    cir_basis.to(torch.double)
                with torch.no_grad():
                    state = cir_basis(state=deepcopy(self.state)) if cir_basis.operators else self.state
                    samples = measure_dist(state, shots=shots, wires=sum(ob.wires, []))
                if self.state.rank == 0:
                    out.append(sample2expval(samples).to(device, dtype).squeeze(0))
                else:
                    out.append(torch.tensor([], dtype=dtype, device=device))
            return torch.stack(out, dim=-1)
        if self.state.batch is not None or not torch.is_grad_enabled():
            # forward-only evaluation (also the only one defined for batched shards)
            from .distributed import cached_expect_z, expect_pauli_dist

            ez = cached_expect_z(self.state)           # Z-type strings: reduced by the forward's last pass (DQ_FG_EXPZ)
            out = []
            for ob in self.observables:
                xm, zm = ob.pauli_masks()
                if ez is not None and xm == 0 and zm in ez['masks']:
                    # (`state.amps` would restore the canonical shard order -- an exchange -- under lazy_layout)
                    cdt = self.state._buffers['amps'].dtype
                    v = ez['values'][:, ez['masks'].index(zm)].to(torch.float64 if cdt == torch.complex128 else torch.float32)
                    out.append(v[0] if self.state.batch is None else v)
                else:
                    out.append(expect_pauli_dist(self.state, ob))
            return torch.stack(out, dim=-1)
        if not executor.CONFIG['joint_adjoint']:       # the reference's structure: one sweep per observable
            return torch.stack([adjoint_expectation(self.state, self.operators, ob) for ob in self.observables], dim=-1)
        return adjoint_expectations(self.state, self.operators, self.observables)

    def cnot(self, control: int, target: int) -> None:
        super().cx(control, target)

    def toffoli(self, control1: int, control2: int, target: int) -> None:
        super().ccx(control1, control2, target)
