"""Math entry points of the statevector path, API-compatible with the reference's qmath.py for the
functions the QubitCircuit hot path uses.  All heavy lifting is delegated to the HIP kernels through
``ops`` / ``backend``; only shape bookkeeping happens here."""

from __future__ import annotations

import math
from collections import Counter
from typing import TYPE_CHECKING, Any, NamedTuple

import torch
from torch import nn

from . import backend, ops

if TYPE_CHECKING:
    from .layer import Observable


def is_power_of_two(n: int) -> bool:
    return n > 0 and (n & (n - 1)) == 0


def inverse_permutation(permute_shape: list[int]) -> list[int]:
    """``inv`` with ``inv[permute_shape[i]] = i`` (reference: qmath.py:84-94)."""
    inv = [0] * len(permute_shape)
    for i, p in enumerate(permute_shape):
        inv[p] = i
    return inv


def modmul_table(a: int, mod: int, k: int) -> torch.Tensor:
    """The table of ``x -> a x mod N`` on k bits as a bijection of ``range(2^k)``: ``a x mod N`` for ``x < N`` and ``x``
    itself for ``x >= N`` (int64, (2^k,)).  ``gcd(a, N) = 1`` makes it one; ``1 <= N <= 2^k``."""
    a, mod, k = int(a), int(mod), int(k)
    if k < 1 or k > 31:
        raise ValueError(f'modmul_table: k={k} outside [1, 31]')
    if mod < 1 or mod > 2**k:
        raise ValueError(f'modmul_table: the modulus {mod} must lie in [1, 2^{k} = {2**k}]')
    if math.gcd(a, mod) != 1:
        raise ValueError(f'modmul_table: gcd({a}, {mod}) = {math.gcd(a, mod)}: x -> {a} x mod {mod} is not reversible')
    x = torch.arange(2**k, dtype=torch.int64)
    return torch.where(x < mod, (x * (a % mod)) % mod, x)           # (a mod N < 2^31 and x < 2^31: no overflow)


def amplitude_encoding(data: Any, nqubit: int) -> torch.Tensor:
    """Normalised state(s) of ``nqubit`` qubits from raw amplitudes, zero padded or truncated
    (reference: qmath.py:456-482).  Returns (batch, 2**n, 1)."""
    if not isinstance(data, (torch.Tensor, nn.Parameter)):
        data = torch.tensor(data)
    single = data.ndim == 1 or (data.ndim == 2 and data.shape[-1] == 1)
    batch = 1 if single else data.shape[0]
    data = data.reshape(batch, -1)
    dim = 2**nqubit
    state = torch.zeros(batch, dim, dtype=data.dtype, device=data.device) + 0j
    data = nn.functional.normalize(data[:, :dim], p=2, dim=-1)
    width = min(dim, data.shape[1])
    state[:, :width] = data[:, :width]
    return state.unsqueeze(-1)


def evolve_state(state: torch.Tensor, matrix: torch.Tensor, nqudit: int, wires: list[int], qudit: int = 2) -> torch.Tensor:
    """``(U on wires) psi`` for a tensor-form state (batch, 2, ..., 2); returns the same shape.

    Drop-in for the reference seam qmath.evolve_state (qmath.py:485-506); the permute / reshape /
    matmul chain there becomes one gate kernel.  Only qubits (qudit = 2) are on this path."""
    if qudit != 2:
        raise NotImplementedError('deepquantum_amd accelerates the qubit path only (qudit == 2)')
    shape = state.shape
    flat = state.reshape(shape[0], -1)
    bits = [nqudit - 1 - w for w in wires]
    return ops.apply_gate(flat, matrix, bits, []).reshape(shape)


def multi_kron(lst: list[torch.Tensor]) -> torch.Tensor:
    """Kronecker product of a list, balanced tree order (reference: qmath.py:390-405)."""
    if len(lst) == 1:
        return lst[0].contiguous()
    mid = len(lst) // 2
    return torch.kron(multi_kron(lst[:mid]), multi_kron(lst[mid:])).contiguous()


def slice_state_vector(state: torch.Tensor, nqubit: int, wires: list[int], bits: str, normalize: bool = True) -> torch.Tensor:
    """Project ``wires`` onto ``bits`` and return the remaining (batch, 2**(n-len)) amplitudes
    (reference: qmath.py:365-387)."""
    if len(bits) == 1:
        bits = bits * len(wires)
    assert len(wires) == len(bits)
    mask = value = 0
    for w, b in zip(wires, bits, strict=True):
        assert b in '01'
        mask |= 1 << (nqubit - 1 - w)
        value |= int(b) << (nqubit - 1 - w)
    flat = state.reshape(-1, 2**nqubit)
    if not flat.is_contiguous():
        flat = flat.contiguous()
    out = backend.pack(flat, mask, value) if not flat.requires_grad else _slice_autograd(flat, nqubit, wires, bits)
    if normalize:
        out = nn.functional.normalize(out, p=2, dim=-1)
    return out


def _slice_autograd(flat: torch.Tensor, nqubit: int, wires: list[int], bits: str) -> torch.Tensor:
    x = flat.reshape([-1] + [2] * nqubit)
    axes = [w + 1 for w in wires]
    pm = axes + [i for i in range(nqubit + 1) if i not in axes]
    x = x.permute(pm)
    for b in bits:
        x = x[int(b)]
    return x.reshape(flat.shape[0], -1)


def block_sample(probs: torch.Tensor, shots: int = 1024, block_size: int = 2**24) -> list:
    """Two-level multinomial sampling over blocks of ``block_size`` outcomes so that
    ``torch.multinomial`` never sees more than 2**24 categories (reference: qmath.py:543-565)."""
    nblocks = -(-len(probs) // block_size)
    if nblocks == 1:
        return torch.multinomial(probs, shots, replacement=True).cpu().numpy().tolist()
    pad = nblocks * block_size - len(probs)
    padded = torch.cat([probs, probs.new_zeros(pad)]) if pad else probs
    block_p = padded.reshape(nblocks, block_size).sum(1)
    picks = Counter(torch.multinomial(block_p, shots, replacement=True).cpu().numpy().tolist())
    samples: list = []
    for blk, cnt in picks.items():
        lo = blk * block_size
        hi = min(lo + block_size, len(probs))
        sub = torch.multinomial(probs[lo:hi], cnt, replacement=True) + lo
        samples.extend(sub.cpu().numpy().tolist())
    return samples


def is_density_matrix(rho: torch.Tensor) -> bool:
    """Hermitian, unit trace, positive semi-definite; 2-D or batched 3-D (reference: qmath.py:117-149).
    The spectrum is computed on the host (Hermitian eigensolver) with a small tolerance for round-off."""
    if not isinstance(rho, torch.Tensor) or rho.ndim not in (2, 3):
        return False
    if not is_power_of_two(rho.shape[-2]) or not is_power_of_two(rho.shape[-1]) or rho.shape[-1] != rho.shape[-2]:
        return False
    if rho.ndim == 2:
        rho = rho.unsqueeze(0)
    rho = rho.detach()
    if not torch.allclose(rho, rho.mH):
        return False
    trace = rho.diagonal(dim1=-2, dim2=-1).sum(-1)
    if not torch.allclose(trace, torch.ones_like(trace)):
        return False
    eig = torch.linalg.eigvalsh(rho.cpu())
    return bool((eig >= -1e-6).all())


def partial_trace(rho: torch.Tensor, nqudit: int, trace_lst: list[int], qudit: int = 2) -> torch.Tensor:
    """Trace out the qudits in ``trace_lst`` of (batch, d^n, d^n) density matrices
    (reference: qmath.py:408-436)."""
    if rho.ndim == 2:
        rho = rho.unsqueeze(0)
    assert rho.ndim == 3 and rho.shape[1] == rho.shape[2] == qudit**nqudit
    b = rho.shape[0]
    keep = [i for i in range(nqudit) if i not in trace_lst]
    letters = list(range(1, 2 * nqudit + 1))            # einsum index ids: rows 1..n, columns n+1..2n
    for i in trace_lst:
        letters[nqudit + i] = letters[i]                # repeated index = traced
    out = [letters[i] for i in keep] + [letters[nqudit + i] for i in keep]
    red = torch.einsum(rho.reshape([b] + [qudit] * 2 * nqudit), [0] + letters, [0] + out)
    d = qudit ** len(keep)
    return red.reshape(b, d, d).squeeze(0)


def evolve_den_mat(state: torch.Tensor, matrix: torch.Tensor, nqudit: int, wires: list[int], qudit: int = 2) -> torch.Tensor:
    """rho -> U rho U^dagger for U on ``wires`` of a (batch, 2, ..., 2) tensor with 2n qubit axes
    (reference: qmath.py:509-540): the gate kernel on the row bits, its conjugate on the column bits."""
    if qudit != 2:
        raise NotImplementedError('deepquantum_amd: qudits with d != 2 belong to the photonic path')
    from . import executor
    from .operation import lift_to_density_matrix

    shape = state.shape
    prim = executor.Prim('gen', matrix, tuple(nqudit - 1 - w for w in wires), ())
    out = executor.run(state.reshape(shape[0], -1), lift_to_density_matrix([prim], nqudit))
    return out.reshape(shape)


def _parity(x: torch.Tensor) -> torch.Tensor:
    for shift in (32, 16, 8, 4, 2, 1):
        x = x ^ (x >> shift)
    return x & 1


def measure(
    state: torch.Tensor,
    shots: int = 1024,
    with_prob: bool = False,
    wires: int | list[int] | None = None,
    den_mat: bool = False,
    block_size: int = 2**24,
    sampler: str = 'multinomial',
) -> dict | list[dict]:
    """Sample bit strings from |psi|^2 (reference: qmath.py:568-638).  Probabilities and marginals are
    computed by the HIP reduction kernels; sampling stays ``torch.multinomial`` on the device.
    ``sampler='inverse_cdf'`` draws with :func:`sample` instead (no |psi|^2 temporary; ``block_size`` is unused) and
    returns the same dict format."""
    if sampler == 'inverse_cdf':
        return _measure_inverse_cdf(state, shots, with_prob, wires, den_mat)
    if sampler != 'multinomial':
        raise ValueError(f"measure: sampler must be 'multinomial' or 'inverse_cdf', got {sampler!r}")
    if den_mat:
        assert is_density_matrix(state), 'Please input density matrices'
        state = state.diagonal(dim1=-2, dim2=-1)
    single = state.ndim == 1 or (state.ndim == 2 and state.shape[-1] == 1)
    batch = 1 if single else state.shape[0]
    flat = state.reshape(batch, -1)
    if not flat.is_contiguous():
        flat = flat.contiguous()
    dim = flat.shape[-1]
    assert is_power_of_two(dim), 'The length of the quantum state is not in the form of 2^n'
    n = dim.bit_length() - 1
    if wires is not None:
        if isinstance(wires, int):
            wires = [wires]
        wires = sorted(wires)
    nbits = len(wires) if wires else n
    with torch.no_grad():
        if den_mat:                                   # the diagonal of rho already holds the probabilities
            all_probs = torch.abs(flat)
            if wires is not None and len(wires) != n:
                axes = [w + 1 for w in wires]
                pm = [0] + axes + [i for i in range(1, n + 1) if i not in axes]
                all_probs = all_probs.reshape([batch] + [2] * n).permute(pm).reshape(batch, 2 ** len(wires), -1).sum(-1)
        elif wires is None or len(wires) == n:
            all_probs = backend.probs(flat)
        else:           # one read of the state whatever the number of wires (dq_marginal_*)
            all_probs = backend.marginal(flat, [n - 1 - w for w in wires]).to(flat.real.dtype)
    results = []
    for i in range(batch):
        probs = all_probs[i]
        counts = Counter(block_sample(probs, shots, block_size))
        res = {bin(k)[2:].zfill(nbits): v for k, v in counts.items()}
        if with_prob:
            for k in res:
                res[k] = res[k], probs[int(k, 2)]
        results.append(res)
    return results[0] if batch == 1 else results


def _density_diagonal(state: torch.Tensor, nqubit: int, what: str) -> tuple[torch.Tensor, bool]:
    """(2**n, 2**n) or (B, 2**n, 2**n) density matrices -> their real diagonals (B, 2**n) and whether it was a single one."""
    dim = 1 << nqubit
    if not isinstance(state, torch.Tensor) or state.ndim not in (2, 3) or tuple(state.shape[-2:]) != (dim, dim):
        raise ValueError(f'{what}: a density matrix of {nqubit} qubits must have the shape (2**n, 2**n) or (B, 2**n, 2**n); '
                         f'got {tuple(getattr(state, "shape", ()))}')
    diag = state.diagonal(dim1=-2, dim2=-1)
    diag = diag.real if diag.is_complex() else diag
    return diag.reshape(-1, dim), state.ndim == 2


def sample(
    state: torch.Tensor,
    nqubit: int,
    shots: int = 1024,
    wires: int | list[int] | None = None,
    generator: torch.Generator | None = None,
    den_mat: bool = False,
) -> torch.Tensor:
    """Raw measurement outcomes as a device tensor: int64 (shots,) for a single state, (B, shots) for a batch.

    ``state`` is (2**n,), (2**n, 1), (B, 2**n), (B, 2**n, 1) or (B, 2, ..., 2); with ``den_mat=True`` (2**n, 2**n) or
    (B, 2**n, 2**n).  It need not be normalised.  An outcome is the integer whose binary string over the measured wires
    in ascending wire order is the key :func:`measure` gives: ``bin(v)[2:].zfill(len(wires))``; ``wires=None`` measures
    all of them.  The uniforms are ``torch.rand(B, shots, dtype=float64, device=state.device, generator=generator)``,
    so the same generator state gives the same samples; outcome s of sample b is the smallest index i whose cumulative
    probability exceeds ``u[b, s]`` (``backend.sample_indices``: a tree of partial sums, 1.6 % of a complex64 state, no
    |psi|^2 temporary and no host synchronisation).  A subset of wires keeps those bits of the full index -- an exact
    sample of the marginal without forming it.  Runs under ``no_grad``."""
    from .state import DistributedQubitState

    if isinstance(state, DistributedQubitState):
        raise NotImplementedError('sample: sharded states are not supported (measure_dist is the sharded route)')
    n = int(nqubit)
    shots = int(shots)
    if shots < 1:
        raise ValueError(f'sample: shots must be >= 1, got {shots}')
    with torch.no_grad():
        if den_mat:
            if n < 1 or n > 15:
                raise ValueError(f'sample: nqubit={nqubit} out of range for a density matrix (1..15)')
            flat, single = _density_diagonal(state, n, 'sample')
        else:
            flat, single = _state_batch(state, n, 'sample')
            if not flat.is_contiguous():
                flat = flat.contiguous()
        wires = sorted(_wire_list(wires, n, 'sample')) if wires is not None else None
        u = torch.rand(flat.shape[0], shots, dtype=torch.float64, device=flat.device, generator=generator)
        if den_mat:       # the diagonal already holds the probabilities: the contract in torch, no kernel
            idx = backend._sample_indices_double(flat.clamp_min(0), u)
        else:
            idx = backend.sample_indices(flat, u)
        if wires is not None and len(wires) != n:
            k = len(wires)
            val = torch.zeros_like(idx)
            for j, w in enumerate(wires):
                val |= ((idx >> (n - 1 - w)) & 1) << (k - 1 - j)
            idx = val
    return idx[0] if single else idx


def _measure_inverse_cdf(state, shots, with_prob, wires, den_mat):
    """``measure`` drawing with :func:`sample`: the dict(s) of ``measure``, the outcomes counted on the device."""
    if den_mat:
        assert is_density_matrix(state), 'Please input density matrices'
        dim = state.shape[-1]
        single = state.ndim == 2
    else:
        single = state.ndim == 1 or (state.ndim == 2 and state.shape[-1] == 1)
        dim = state.numel() if single else state[0].numel()
    assert is_power_of_two(dim), 'The length of the quantum state is not in the form of 2^n'
    n = dim.bit_length() - 1
    if isinstance(wires, int):
        wires = [wires]
    wires = sorted(wires) if wires else None
    part = wires is not None and len(wires) != n
    nbits = len(wires) if wires else n
    outcomes = sample(state, n, shots=shots, wires=wires, den_mat=den_mat)
    outcomes = outcomes.reshape(1, -1) if single else outcomes
    probs = None
    if with_prob:
        with torch.no_grad():
            if den_mat:
                probs = torch.abs(_density_diagonal(state, n, 'measure')[0])
                if part:
                    axes = [w + 1 for w in wires]
                    pm = [0] + axes + [i for i in range(1, n + 1) if i not in axes]
                    probs = probs.reshape([-1] + [2] * n).permute(pm).reshape(probs.shape[0], 2 ** len(wires), -1).sum(-1)
            else:
                flat = _state_batch(state, n, 'measure')[0]
                flat = flat if flat.is_contiguous() else flat.contiguous()
                if part:       # one read of the state whatever the number of wires (dq_marginal_*)
                    probs = backend.marginal(flat, [n - 1 - w for w in wires]).to(flat.real.dtype)
    results = []
    for i in range(outcomes.shape[0]):
        keys, counts = torch.unique(outcomes[i], return_counts=True)
        res = {bin(k)[2:].zfill(nbits): v for k, v in zip(keys.tolist(), counts.tolist(), strict=True)}
        if with_prob:
            if probs is not None:
                pk = probs[i][keys]
            else:              # all wires of a state vector: |psi[idx]|^2 of the distinct outcomes only
                a = flat[i][keys]
                pk = a.real * a.real + a.imag * a.imag
            for j, k in enumerate(res):
                res[k] = res[k], pk[j]
        results.append(res)
    return results[0] if len(results) == 1 else results      # (a batch of one gives a dict, as on the default route)


def expectation(state: torch.Tensor, observable: 'Observable', den_mat: bool = False, chi: int | None = None) -> torch.Tensor:
    """``Re <psi| O |psi>`` for a Pauli-string observable (reference: qmath.py:830-860), computed in a
    single pass over the state by the Pauli-expectation kernel."""
    if isinstance(state, list):
        raise NotImplementedError('matrix product states are outside the accelerated path')
    if den_mat:
        # Tr(P rho) = sum_j P[j ^ x, j] rho[j, j ^ x]: only 2^n of the 4^n entries of rho are needed
        # (the reference multiplies the full 2^n x 2^n observable into rho, qmath.py:855)
        single = state.ndim == 2
        rho = state.reshape(1 if single else state.shape[0], -1)
        xmask, zmask = observable.pauli_masks()
        dim = int(round(rho.shape[-1] ** 0.5))
        j = torch.arange(dim, device=rho.device)
        entries = rho[:, j * dim + (j ^ xmask)]
        sign = (1 - 2 * _parity(j & zmask)).to(rho.real.dtype)
        val = (entries * sign).sum(-1) * (1j) ** bin(xmask & zmask).count('1')
        out = val.real
        return out.squeeze(0) if single else out
    single = state.ndim == 2
    flat = state.reshape(1 if single else state.shape[0], -1)
    xmask, zmask = observable.pauli_masks()
    out = ops.expect_pauli(flat, xmask, zmask)
    return out.squeeze(0) if single else out


def sample2expval(sample: dict) -> torch.Tensor:
    """Parity expectation from measurement counts (reference: qmath.py:863-871)."""
    total = sum(sample.values())
    acc = sum(cnt * (-1) ** (bits.count('1') % 2) for bits, cnt in sample.items())
    return torch.tensor([acc / total])


def _entangle_input(state_tsr: torch.Tensor, what: str) -> tuple[torch.Tensor, int]:
    """(batch, 2, ..., 2) -> the flat (batch, 2**n) state and n = ndim - 1."""
    from .state import DistributedQubitState

    if isinstance(state_tsr, DistributedQubitState):
        raise NotImplementedError(f'{what}: sharded states are not supported (the coherences of the global wires need a '
                                  'pairwise exchange)')
    if not isinstance(state_tsr, torch.Tensor) or state_tsr.ndim < 2:
        raise ValueError(f'{what}: input must have the shape (batch, 2, ..., 2), got '
                         f'{tuple(getattr(state_tsr, "shape", ()))}')
    if any(d != 2 for d in state_tsr.shape[1:]):
        raise ValueError(f'{what}: every non-batch dimension must be 2, got shape {tuple(state_tsr.shape)}')
    if not state_tsr.is_complex():
        state_tsr = state_tsr.to(torch.complex64 if state_tsr.dtype != torch.float64 else torch.complex128)
    n = state_tsr.ndim - 1
    return state_tsr.reshape(state_tsr.shape[0], 1 << n), n


def _rdm1(state_tsr: torch.Tensor, what: str) -> tuple[torch.Tensor, int, torch.dtype]:
    flat, n = _entangle_input(state_tsr, what)
    return ops.rdm1_cross(flat, flat), n, flat.real.dtype


def single_qubit_rdms(state_tsr: torch.Tensor) -> torch.Tensor:
    """Reduced density matrix of every wire, ``rho_k = Tr_{others} |psi><psi|``: (batch, n, 2, 2) in the state's dtype
    for an input of shape (batch, 2, ..., 2) -- what ``partial_trace(psi psi^dagger, n, all but k)`` returns for each
    k, from a fixed number of reads of the state instead of a 4^n matrix.  Not normalised."""
    t, _n, _rd = _rdm1(state_tsr, 'single_qubit_rdms')
    return t.transpose(-1, -2).to(state_tsr.dtype if state_tsr.is_complex() else t.dtype)


def meyer_wallach_measure(state_tsr: torch.Tensor) -> torch.Tensor:
    """Meyer-Wallach entanglement measure (reference: qmath.py:874-890), ``(4 / n) sum_k (p0 p1 - |c|^2)`` with
    ``p0, p1, c`` the entries of the reduced density matrix of wire k: (batch,) real.  No normalisation is applied,
    as in the reference.  Differentiable to any order."""
    t, n, rdt = _rdm1(state_tsr, 'meyer_wallach_measure')
    p0, p1, c = t[..., 0, 0].real, t[..., 1, 1].real, t[..., 0, 1]
    val = (p0 * p1 - (c.real * c.real + c.imag * c.imag)).sum(-1) * (4.0 / n)
    return val.to(rdt)


def meyer_wallach_measure_brennen(state_tsr: torch.Tensor) -> torch.Tensor:
    """Brennen's form of the Meyer-Wallach measure (reference: qmath.py:941-965), ``2 (1 - (1/n) sum_k Tr rho_k^2)``:
    (batch,) real.  The reference builds the 4^n density matrix; here it is the same one-body reduction as
    :func:`meyer_wallach_measure`."""
    t, n, rdt = _rdm1(state_tsr, 'meyer_wallach_measure_brennen')
    p0, p1, c = t[..., 0, 0].real, t[..., 1, 1].real, t[..., 0, 1]
    purity = p0 * p0 + p1 * p1 + 2.0 * (c.real * c.real + c.imag * c.imag)
    return (2.0 * (1.0 - purity.sum(-1) / n)).to(rdt)


def linear_map_mw(state_tsr: torch.Tensor, j: int, b: int) -> torch.Tensor:
    """Project wire ``j`` of a (batch, 2, ..., 2) state onto |b> (reference: qmath.py:893-918): a view of shape
    (batch, 2, ..., 2) with that wire removed, not normalised."""
    if b not in (0, 1):
        raise ValueError('b must be 0 or 1')
    if not 0 <= j < state_tsr.ndim - 1:
        raise ValueError(f'wire {j} out of range for {state_tsr.ndim - 1} qubits')
    return state_tsr.select(j + 1, b)


def generalized_distance(state1: torch.Tensor, state2: torch.Tensor) -> torch.Tensor:
    """``<s1|s1> <s2|s2> - |<s1|s2>|^2`` of (batch, 2^n, 1) inputs, shape (batch, 1, 1) real (reference:
    qmath.py:921-938)."""
    overlap = state1.mH @ state2
    norms = (state1.mH @ state1).real * (state2.mH @ state2).real
    return norms - (overlap.real * overlap.real + overlap.imag * overlap.imag)


RDM_MAX_WIRES = 10      # the k-wire reduction of dq_rdmk_cross_* (k <= 2: dq_gate_grad_*)


def _state_batch(state: torch.Tensor, nqubit: int, what: str) -> tuple[torch.Tensor, bool]:
    """A state vector in any accepted form -> the flat complex (B, 2**n) tensor and whether it was a single state
    (``ndim == 1`` or ``(ndim == 2 and shape[-1] == 1)``, the rule of :func:`measure`)."""
    from .state import DistributedQubitState

    if isinstance(state, DistributedQubitState):
        raise NotImplementedError(f'{what}: sharded states are not supported (kept wires that are global in the '
                                  'placement need a remap)')
    if not isinstance(state, torch.Tensor):
        raise ValueError(f'{what}: state must be a tensor, got {type(state).__name__}')
    n = int(nqubit)
    if n < 1 or n > 40:
        raise ValueError(f'{what}: nqubit={nqubit} out of range')
    dim = 1 << n
    single = state.ndim == 1 or (state.ndim == 2 and state.shape[-1] == 1)
    if single:
        ok = state.numel() == dim
    else:
        ok = state.ndim >= 2 and tuple(state.shape[1:]) in ((dim,), (dim, 1), (2,) * n)
    if not ok:
        raise ValueError(f'{what}: a state of {n} qubits must have the shape (2**n,), (2**n, 1), (B, 2**n), '
                         f'(B, 2**n, 1) or (B, 2, ..., 2); got {tuple(state.shape)}')
    if not state.is_complex():
        state = state.to(torch.complex128 if state.dtype == torch.float64 else torch.complex64)
    return state.reshape(1 if single else state.shape[0], dim), single


def _wire_list(wires: Any, nqubit: int, what: str) -> list[int]:
    if isinstance(wires, int):
        wires = [wires]
    try:
        wires = [int(w) for w in wires]
    except TypeError:
        raise ValueError(f'{what}: wires must be an int or a list of ints, got {wires!r}') from None
    if not wires or len(set(wires)) != len(wires) or any(w < 0 or w >= nqubit for w in wires):
        raise ValueError(f'{what}: wires must be distinct and in [0, {nqubit}), got {wires}')
    return wires


def _rdm_flat(flat: torch.Tensor, nqubit: int, wires: list[int]) -> torch.Tensor:
    """(B, 2**n) -> complex128 (B, 2**k, 2**k): rho[b] = Tr_{other wires} |psi_b><psi_b|, ``wires[0]`` = matrix MSB.
    The same tensor on both sides of ``ops.gate_grad``: the Hermitian route of the kernel, differentiable to any
    order through the node's rules."""
    return ops.gate_grad(flat, flat, [nqubit - 1 - w for w in wires])


def reduced_density_matrix(state: torch.Tensor, nqubit: int, wires: int | list[int]) -> torch.Tensor:
    """Reduced density matrix ``rho_A = Tr_B |psi><psi|`` of the wires ``A = wires`` (1 to 10 of them; all n gives
    psi psi^dagger): (2**k, 2**k) for a single state, (B, 2**k, 2**k) for a batch, in the state's complex dtype.

    ``state`` is (2**n,), (2**n, 1), (B, 2**n), (B, 2**n, 1) or (B, 2, ..., 2).  The order of ``wires`` is the matrix
    index order (``wires[0]`` is the most significant bit); for sorted wires the result equals
    ``partial_trace(psi psi^dagger, n, complement)``.  Not normalised: ``Tr rho_A = <psi|psi>``.  The state is read
    without the 4**n matrix (a Gram reduction on the matrix cores, ``dq_rdmk_cross_*``); differentiable to any order,
    and usable under ``torch.vmap`` / ``torch.func`` and graph capture."""
    flat, single = _state_batch(state, nqubit, 'reduced_density_matrix')
    wires = _wire_list(wires, int(nqubit), 'reduced_density_matrix')
    if len(wires) > RDM_MAX_WIRES:
        raise ValueError(f'reduced_density_matrix: {len(wires)} wires, at most {RDM_MAX_WIRES}')
    rho = _rdm_flat(flat, int(nqubit), wires).to(flat.dtype)
    return rho.squeeze(0) if single else rho


def _cost_table(cost: Any, k: int, what: str) -> torch.Tensor:
    if not isinstance(cost, torch.Tensor):
        cost = torch.tensor(cost, dtype=torch.float)
    if cost.is_complex() or not cost.is_floating_point():
        raise ValueError(f'{what}: the cost table must be real floating point, got {cost.dtype}')
    if cost.shape != (1 << k,):
        raise ValueError(f'{what}: a cost over {k} wires has shape ({1 << k},), got {tuple(cost.shape)}')
    return cost


def expectation_cost(state: torch.Tensor, nqubit: int, cost: torch.Tensor, wires: int | list[int] | None = None) -> torch.Tensor:
    """``<C> = sum_i cost[sub(i)] |psi_i|^2`` for a classical cost given as a real table of 2^k entries over ``wires``
    (``wires[0]`` the most significant bit of the entry index; all n wires by default): (B,) real in the state's
    precision, or 0-d for a single state.  ``state`` in the forms of :func:`reduced_density_matrix`.  One read of the
    state, accumulated in double (``dq_cost_cross_*``); differentiable to any order in the state (the table is a
    constant).  Not normalised: a state of norm r gives r^2 <C>."""
    flat, single = _state_batch(state, nqubit, 'expectation_cost')
    n = int(nqubit)
    wires = list(range(n)) if wires is None else _wire_list(wires, n, 'expectation_cost')
    cost = _cost_table(cost, len(wires), 'expectation_cost')
    val = ops.cost_cross(flat, flat, cost, [n - 1 - w for w in wires]).real.to(flat.real.dtype)
    return val.squeeze(0) if single else val


def _pauli_sum(H: Any, nqubit: int, what: str):
    from .pauli_sum import PauliSum

    if not isinstance(H, PauliSum):
        H = PauliSum(H, nqubit)
    if H.nqubit != int(nqubit):
        raise ValueError(f'{what}: the PauliSum is for {H.nqubit} qubits, the state has {int(nqubit)}')
    return H


def expectation_pauli_sum(state: torch.Tensor, nqubit: int, H: Any) -> torch.Tensor:
    """``Re <psi|H|psi>`` for a sum of Pauli strings ``H`` -- a :class:`PauliSum`, or the list form it is built from,
    ``[[0.5, 'x0y1'], [-1, 'z3y1'], [0.25, '']]`` (build the ``PauliSum`` once where the call repeats): (B,) real in the
    state's precision, or 0-d for a single state.  ``state`` in the forms of :func:`reduced_density_matrix`.  One launch
    for the whole sum, one read of the state per distinct flip mask, accumulated in double (``dq_psum_cross_*``);
    differentiable to any order in the state (the coefficients are constants).  Not normalised."""
    flat, single = _state_batch(state, nqubit, 'expectation_pauli_sum')
    val = ops.psum_cross(flat, flat, _pauli_sum(H, nqubit, 'expectation_pauli_sum')).real.to(flat.real.dtype)
    return val.squeeze(0) if single else val


def apply_pauli_sum(state: torch.Tensor, nqubit: int, H: Any) -> torch.Tensor:
    """``H|psi>`` for a sum of Pauli strings ``H`` (as in :func:`expectation_pauli_sum`), with the shape of ``state`` and
    in its complex dtype: what variance, Krylov and imaginary-time steps are made of.  One launch for the whole sum
    (``dq_apply_psum_axpby_*``); differentiable to any order in the state."""
    flat, _ = _state_batch(state, nqubit, 'apply_pauli_sum')
    zero = torch.zeros(flat.shape[0], dtype=torch.complex128, device=flat.device)      # (made on the device: legal under capture)
    out = ops.psum_axpby(flat, zero, torch.ones_like(zero), _pauli_sum(H, nqubit, 'apply_pauli_sum'))
    return out.reshape(state.shape)


def evolve_pauli_sum(state: torch.Tensor, H: Any, t: Any, nqubit: int | None = None, tol: float | None = None,
                     bounds: tuple[float, float] | None = None) -> torch.Tensor:
    """``exp(-i t H)|psi>`` for a sum of Pauli strings ``H`` (as in :func:`expectation_pauli_sum`) and a real ``t``, one
    value or one per sample, with the shape of ``state`` and in its complex dtype: a Chebyshev expansion in H, accurate to
    ``tol`` (default 1e-6 for complex64, 1e-12 for complex128) for any ``t`` and any strings -- nothing has to commute --
    in about ``H.norm_bound * |t|`` plus a few dozen launches (``ops.psum_evolve``).  ``t`` is read on the host, so the call
    cannot be captured into a graph.  Differentiable to any order in the state and in ``t``.  ``nqubit`` may be left out
    where ``H`` is a ``PauliSum``, or where the state is (2**n,) or (B, 2**n).  ``bounds=(lo, hi)``: an interval that holds
    the spectrum of H, e.g. ``H.spectral_bounds()``, in place of the rigorous and loose ``constant -+ norm_bound``: about
    as many launches fewer as the interval is narrower (``None``: today's path, bit for bit)."""
    from .pauli_sum import PauliSum

    if nqubit is None:
        if isinstance(H, PauliSum):
            nqubit = H.nqubit
        elif state.ndim in (1, 2) and state.shape[-1] > 1:
            nqubit = state.shape[-1].bit_length() - 1
        else:
            raise ValueError('evolve_pauli_sum: pass nqubit (the state is neither (2**n,) nor (B, 2**n), and H is a list)')
    flat, _ = _state_batch(state, nqubit, 'evolve_pauli_sum')
    H = _pauli_sum(H, nqubit, 'evolve_pauli_sum')
    if bounds is None:
        return ops.psum_evolve(flat, t, H, tol).reshape(state.shape)
    return ops.psum_evolve(flat, t, H, tol, bounds).reshape(state.shape)


def _gram_states(state: torch.Tensor, what: str) -> torch.Tensor:
    """A batch of state vectors -- (M, 2**n), (M, 2**n, 1), or a single (2**n, 1) / (2**n,) -- as the flat (M, 2**n)
    tensor of :func:`_state_batch`, n taken from the shape."""
    if not isinstance(state, torch.Tensor):
        raise ValueError(f'{what}: states must be a tensor, got {type(state).__name__}')
    single = state.ndim == 1 or (state.ndim == 2 and state.shape[-1] == 1)
    dim = state.numel() if single else (state.shape[1] if state.ndim >= 2 else 0)
    n = max(int(dim).bit_length() - 1, 0)
    if state.ndim > 3 or dim != 1 << n or n < 1:
        raise ValueError(f'{what}: states must have the shape (M, 2**n), (M, 2**n, 1) or (2**n, 1) with n >= 1; '
                         f'got {tuple(state.shape)}')
    return _state_batch(state, n, what)[0]


def gram_matrix(a: torch.Tensor, b: torch.Tensor | None = None) -> torch.Tensor:
    """The overlaps ``G[i, j] = <a_i|b_j>`` of every state of ``a`` with every state of ``b``: complex128 (M, N).  ``a`` and
    ``b`` are (M, 2**n), (M, 2**n, 1) or a single (2**n, 1), of one dtype.  ``b=None`` is the self-Gram ``<a_i|a_j>``: half
    the reads, exactly Hermitian, a real diagonal.  One launch on the matrix cores, every state read once up to 32 x 32
    rows (``dq_gram_*``; the tiling beyond that: :func:`backend.gram`); complex64 sums at most a few hundred real terms in
    float32, everything else in double.  Differentiable to any order in both batches; not under ``torch.vmap``."""
    fa = _gram_states(a, 'gram_matrix')
    return ops.gram(fa, fa if b is None else _gram_states(b, 'gram_matrix'))


def fidelity_kernel(a: torch.Tensor, b: torch.Tensor | None = None) -> torch.Tensor:
    """The fidelity kernel ``K[i, j] = |<a_i|b_j>|^2`` of quantum kernel methods: real float64 (M, N);
    ``|gram_matrix(a, b)|^2``, symmetric with ``b=None``."""
    g = gram_matrix(a, b)
    return g.real * g.real + g.imag * g.imag


def linear_combination(states: torch.Tensor, coef: torch.Tensor) -> torch.Tensor:
    """``out[m] = sum_j coef[m, j] states[j]`` for a complex (M, N) ``coef`` (a 1-D ``coef`` of N entries gives one
    combination): (M, 2**n) in the states' dtype -- Ritz vectors, Gram-Schmidt, a classically summed LCU.  One read of the
    states and one write of the result up to 32 combinations (``dq_combine_*``); ``coef`` is rounded once to the states'
    precision.  Differentiable to any order in both; not under ``torch.vmap``."""
    flat = _gram_states(states, 'linear_combination')
    if not isinstance(coef, torch.Tensor):
        coef = torch.as_tensor(coef)
    if coef.ndim == 1:
        coef = coef.unsqueeze(0)
    return ops.combine(flat, coef.to(flat.device))


def orthonormalize(states: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """An orthonormal basis ``Q`` of the span of the (M, 2**n) ``states`` and the lower-triangular complex128 (M, M) ``L``
    with ``states = L Q`` (row m of ``states`` is ``sum_k L[m, k] Q[k]``): Cholesky-QR applied twice -- ``S = gram(V)``,
    ``S = L1 L1^H``, ``V <- conj(inv(L1)) V`` (the rows are the vectors), then once more, ``L = conj(L1 L2)`` -- so that ``|gram(Q) - 1|`` is at rounding level of
    the states' precision where one pass leaves ``cond(S)`` times that.  Two self-Grams and two combinations on the
    device; the M x M matrices in complex128 through torch.  A numerically dependent batch -- a pivot of the Cholesky
    factorisation below ``M * eps`` of the largest squared norm -- is refused by name of the pivot.  Differentiable."""
    what = 'orthonormalize'
    v = _gram_states(states, what)
    m = v.shape[0]
    eps = torch.finfo(v.real.dtype).eps
    total = None
    for sweep in range(2):
        s = ops.gram(v, v).cpu()                        # (M x M: the factorisation runs on the host)
        chol, info = torch.linalg.cholesky_ex(s)
        floor = m * eps * float(s.detach().diagonal().real.max())
        pivots = chol.detach().diagonal().real ** 2
        low = torch.nonzero(~(pivots > floor)).flatten()
        if int(info) != 0 or low.numel():
            k = int(info) - 1 if int(info) != 0 else int(low[0])
            raise ValueError(f'{what}: the states are numerically dependent: pivot {k} of the Cholesky factorisation of their '
                             f'Gram matrix (pass {sweep + 1}) is not above {floor:.3e} -- state {k} lies in the span of the '
                             'states before it')
        eye = torch.eye(m, dtype=torch.complex128, device=chol.device)
        v = ops.combine(v, torch.linalg.solve_triangular(chol, eye, upper=False).conj().to(v.device))
        total = chol if total is None else total @ chol
    return v, total.conj().resolve_conj().to(v.device)


class ExtremalResult(NamedTuple):
    """What :func:`pauli_sum_extremal` returns: ``value`` float64, ``vector`` (unit, in ``dtype``; ``None`` with
    ``vector=False``), ``residual`` -- the Lanczos estimate of ``|H y - value y|`` --, ``steps`` and ``converged``; one entry
    per start vector, (B,) and (B, 2**n), or 0-d and (2**n,) for a single start."""
    value: torch.Tensor
    vector: torch.Tensor | None
    residual: torch.Tensor
    steps: torch.Tensor
    converged: torch.Tensor


def pauli_sum_extremal(H: Any, nqubit: int | None = None, which: str = 'lowest', tol: float | None = None,
                       max_steps: int | None = None, start: torch.Tensor | None = None, vector: bool = True,
                       dtype: torch.dtype = torch.complex64, device: Any = None, seed: int = 0) -> ExtremalResult:
    """The lowest (``which='lowest'``) or highest (``'highest'``) eigenvalue of a sum of Pauli strings ``H`` -- a
    :class:`PauliSum` or the list form -- and its eigenvector: the exact ground energy and ground state a variational energy
    is judged against, by Lanczos steps of two launches each on the device (:func:`backend.psum_lanczos`), to a residual of
    ``tol * H.norm_bound`` (``tol``: 1e-6 for complex64, 1e-12 for complex128 by default).  ``start``: (2**n,) or (B, 2**n)
    complex, never written, not necessarily normalised -- one eigenpair per start vector; ``None``: one Gaussian random vector
    from ``seed`` in ``dtype`` on ``device`` (default: the GPU).  ``vector=False`` leaves the second pass out: half the launches.
    The result is detached: the coefficients of a ``PauliSum`` carry no gradient, so neither does this.

    What this is not.  Not several eigenpairs.  In a degenerate extremal eigenspace the value is right and the vector
    returned depends on the start.  complex64 stalls near a residual of 1e-7 * norm_bound: ask complex128 for more.  The
    host reads two numbers after every launch, so the call cannot be captured into a graph."""
    from .pauli_sum import PauliSum

    what = 'pauli_sum_extremal'
    if nqubit is None:
        if isinstance(H, PauliSum):
            nqubit = H.nqubit
        elif start is not None and start.ndim in (1, 2) and start.shape[-1] > 1:
            nqubit = start.shape[-1].bit_length() - 1
        else:
            raise ValueError(f'{what}: pass nqubit (H is a list and there is no start vector to take it from)')
    H = _pauli_sum(H, nqubit, what)
    n = H.nqubit
    single = start is None or start.ndim == 1
    if start is None:
        if dtype not in (torch.complex64, torch.complex128):
            raise ValueError(f'{what}: dtype must be torch.complex64 or torch.complex128, got {dtype}')
        device = torch.device('cuda' if device is None and backend.get_test_backend() is None else device or 'cpu')
        g = torch.Generator().manual_seed(int(seed))
        flat = torch.randn(1, 1 << n, dtype=torch.complex128, generator=g).to(device=device, dtype=dtype)
    else:
        if not isinstance(start, torch.Tensor) or start.ndim not in (1, 2) or start.shape[-1] != 1 << n:
            raise ValueError(f'{what}: start must be a tensor of shape ({1 << n},) or (B, {1 << n})')
        flat = start.detach().reshape(-1, 1 << n).contiguous()
    got = backend.psum_lanczos(H.table, flat, which, tol, max_steps, vector)
    vec = got.vector
    if single:
        return ExtremalResult(got.value[0], None if vec is None else vec[0], got.residual[0], got.steps[0], got.converged[0])
    return ExtremalResult(got.value, vec, got.residual, got.steps, got.converged)


def ising_cost(nqubit: int, terms: list, dtype: torch.dtype | None = None, device: Any = None) -> torch.Tensor:
    """The table ``c[i] = sum_j w_j (-1)^popcount(i & zmask_j)`` over all ``nqubit`` wires of the Ising polynomial
    ``terms = [(weight, [wires...]), ...]`` (a term's sign is the product of Z eigenvalues of its wires in basis state i,
    wire 0 the most significant bit): real (2**nqubit,), built on ``device`` by the Z-string kernel
    (``dq_scale_zsigns_*`` on a vector of ones, 32 terms per pass).  ``dtype``: torch.float32 (default) or float64."""
    n = int(nqubit)
    if n < 1 or n > 40:
        raise ValueError(f'ising_cost: nqubit={nqubit} out of range')
    dtype = torch.float32 if dtype is None else dtype
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f'ising_cost: dtype must be torch.float32 or torch.float64, got {dtype}')
    zmasks, weights = [], []
    try:
        for w, wires in terms:
            weights.append(float(w))
            wires = [wires] if isinstance(wires, int) else list(wires)
            zmasks.append(sum(1 << (n - 1 - q) for q in _wire_list(wires, n, 'ising_cost')) if wires else 0)
    except TypeError:
        raise ValueError('ising_cost: terms must be a list of (weight, [wires...]) pairs') from None
    if not zmasks:
        raise ValueError('ising_cost: no terms')
    cdtype = torch.complex64 if dtype == torch.float32 else torch.complex128
    ones = torch.ones(1, 1 << n, dtype=cdtype, device=device)
    coef = torch.tensor([weights], dtype=torch.float64, device=device)
    return backend.scale_z_signs(ones, zmasks, coef).real.reshape(-1).contiguous()


def _entropy_of(rho: torch.Tensor, alpha: float, base: float | None, tau: float) -> torch.Tensor:
    """Entropy of (B, D, D) Hermitian matrices, normalised by their trace first: (B,) float64."""
    rho = rho.to(torch.complex128)
    tr = rho.diagonal(dim1=-2, dim2=-1).sum(-1).real
    rho = rho / tr[:, None, None]
    if alpha == 2:
        # -log Tr rho^2 = -log ||rho||_F^2 (Hermitian): no eigensolver
        val = -torch.log((rho.real * rho.real + rho.imag * rho.imag).sum((-2, -1)))
    else:
        lam = torch.linalg.eigvalsh(rho)
        keep = lam > tau
        lam = torch.where(keep, lam, torch.ones_like(lam))       # (dropped terms: no value, no gradient)
        if alpha == 1:
            val = -(torch.where(keep, lam * torch.log(lam), torch.zeros_like(lam))).sum(-1)
        else:
            val = torch.log(torch.where(keep, lam**alpha, torch.zeros_like(lam)).sum(-1)) / (1.0 - alpha)
    if base is not None:
        val = val / math.log(base)
    return val


def entanglement_entropy(state: torch.Tensor, nqubit: int, wires: int | list[int], alpha: float = 1.0,
                         base: float | None = None) -> torch.Tensor:
    """Entanglement entropy across the cut ``wires | rest`` of a pure state: the entropy of ``rho_A / Tr rho_A``.
    (B,) real, or a 0-d tensor for a single state (input forms as :func:`reduced_density_matrix`).

    ``alpha == 1``: von Neumann, ``-sum lambda log lambda`` (eigenvalues from ``torch.linalg.eigvalsh`` in complex128);
    ``alpha == 2``: ``-log Tr rho^2``, from the Frobenius norm without an eigensolver; any other ``alpha > 0``: Renyi,
    ``log sum lambda**alpha / (1 - alpha)``.  Eigenvalues at or below tau contribute nothing and carry no gradient:
    tau = 1e-12 for complex128 states, 1e-6 for complex64.  ``base=None``: natural log.  A pure state has
    ``S(A) = S(B)``, so the smaller side of the cut is reduced: either side may hold up to 10 wires; a cut with more
    than 10 on both sides raises ``ValueError``."""
    flat, single = _state_batch(state, nqubit, 'entanglement_entropy')
    n = int(nqubit)
    wires = _wire_list(wires, n, 'entanglement_entropy')
    alpha = float(alpha)
    if not alpha > 0:
        raise ValueError(f'entanglement_entropy: alpha must be > 0, got {alpha}')
    if base is not None and (base <= 0 or base == 1):
        raise ValueError(f'entanglement_entropy: base must be > 0 and != 1, got {base}')
    rest = [w for w in range(n) if w not in wires]
    side = sorted(wires) if len(wires) <= len(rest) else rest
    if len(side) > RDM_MAX_WIRES:
        raise ValueError(f'entanglement_entropy: both sides of the cut exceed {RDM_MAX_WIRES} wires '
                         f'({len(wires)} | {len(rest)})')
    rdt = flat.real.dtype
    if not side:                      # the whole state: pure, no entropy
        val = torch.zeros(flat.shape[0], dtype=rdt, device=flat.device)
    else:
        tau = 1e-12 if flat.dtype == torch.complex128 else 1e-6
        val = _entropy_of(_rdm_flat(flat, n, side), alpha, base, tau).to(rdt)
    return val.squeeze(0) if single else val


def density_matrix_rdm(rho: torch.Tensor, nqubit: int, wires: list[int]) -> torch.Tensor:
    """Reduced density matrix of the wires ``wires`` (in that matrix order) of (B, 2**n, 2**n) or (2**n, 2**n) density
    matrices: ``partial_trace`` over the rest, permuted to the order of ``wires``."""
    n = int(nqubit)
    wires = _wire_list(wires, n, 'reduced_density_matrix')
    single = rho.ndim == 2
    rest = [w for w in range(n) if w not in wires]
    red = partial_trace(rho if rho.ndim == 3 else rho.unsqueeze(0), n, rest)
    k = len(wires)
    red = red.reshape(-1, 1 << k, 1 << k)
    order = sorted(wires)
    if order != wires:
        perm = [order.index(w) for w in wires]
        b = red.shape[0]
        red = red.reshape([b] + [2] * (2 * k)).permute([0] + [1 + p for p in perm] + [1 + k + p for p in perm])
        red = red.reshape(b, 1 << k, 1 << k)
    return red.squeeze(0) if single else red
