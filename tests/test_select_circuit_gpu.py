"""SelectPauli, ``cir.block_encode`` and ``cir.qubitization_walk`` inside circuits on the GPU: SELECT between fused stretches
against the dense matrix and against an independent route through existing kernels (one controlled ``pauli_rot(pi)`` per
string between X flips and a diagonal of the phases), undone by ``cir.inverse()``; the block-encoding identities in both
precisions for three placements of the select wires; one block encoding under a control.  Tolerances are the project's
parity criteria: 1e-4 relative to the largest amplitude in complex64, 1e-10 in complex128."""

import math

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from _select_ref import dense_select, factors, pauli_sum_matrix, random_state

pytestmark = pytest.mark.gpu

PRECISIONS = [pytest.param(torch.complex64, 1e-4, id='c64'), pytest.param(torch.complex128, 1e-10, id='c128')]

N, SELECT, SYSTEM = 6, [4, 1], [0, 2, 3, 5]
STRINGS, PHASES = ['x0y2', 'z1z3', 'y0y1y2y3'], [1, 2, 3]                     # (the fourth entry is the identity)
PI = torch.tensor(math.pi, dtype=torch.float64)         # (a float32 pi would leave 4e-8 in exp(-i pi/2 P) = -i P)


def finish(cir, dtype):
    cir.to('cuda')
    if dtype == torch.complex128:
        cir.to(torch.double)
    return cir


def build(route, dtype):
    """Fused stretches with SELECT between them: as one gate, as the dense matrix, or as the loop over the strings."""
    torch.manual_seed(7)
    cir = dq.QubitCircuit(N)
    cir.rylayer()
    cir.rxlayer()
    cir.cnot_ring()
    if route == 'select':
        cir.select_pauli(STRINGS, wires=SELECT, system_wires=SYSTEM, phases=PHASES)
    elif route == 'dense':
        cir.any(torch.from_numpy(dense_select(N, SELECT, SYSTEM, STRINGS, PHASES)).to(torch.complex64), wires=list(range(N)))
    else:
        k = len(SELECT)
        for s, string in enumerate(STRINGS):
            zeros = [w for j, w in enumerate(SELECT) if not (s >> (k - 1 - j)) & 1]
            for w in zeros:
                cir.x(w)
            letters = {w: p for p, w in factors(string)}
            cir.pauli_rot(''.join(letters[w] for w in sorted(letters)), wires=[SYSTEM[w] for w in sorted(letters)], inputs=PI,
                          controls=SELECT)                                      # exp(-i pi/2 P) = -i P
            for w in zeros:
                cir.x(w)
        cir.diagonal(torch.tensor([1j ** (PHASES[s] + 1) if s < len(STRINGS) else 1 for s in range(1 << k)]), wires=SELECT)
    cir.rylayer()
    cir.cnot_ring(reverse=True)
    cir.rzlayer()
    return finish(cir, dtype)


@pytest.mark.parametrize('dtype,tol', PRECISIONS)
def test_select_between_fused_stretches_against_the_dense_matrix_and_the_loop(dtype, tol):
    new, dense, loop = build('select', dtype), build('dense', dtype), build('loop', dtype)
    for p, q, r in zip(new.parameters(), dense.parameters(), loop.parameters(), strict=True):
        assert torch.equal(p, q) and torch.equal(p, r)
    x = torch.from_numpy(random_state(np.random.default_rng(1), 3, N, np.complex128)).to(dtype)
    x = (x / x.norm(dim=-1, keepdim=True)).cuda().reshape(3, -1, 1)
    with torch.no_grad():
        a, b, c = new(state=x), dense(state=x), loop(state=x)
        scale = a.abs().max().item()
        assert a.dtype == dtype and (a - b).abs().max().item() < tol * scale and (a - c).abs().max().item() < tol * scale
        a0 = new()
        assert (a0 - dense()).abs().max().item() < tol * a0.abs().max().item()
        back = new.inverse()(state=a)
        assert (back - x).abs().max().item() < tol * x.abs().max().item()
    assert sum(isinstance(op, dq.SelectPauli) for op in new.inverse().operators) == 1


def test_unitary_inverse_and_refusals():
    gate = dq.SelectPauli(STRINGS, nqubit=N, wires=SELECT, system_wires=SYSTEM, phases=PHASES, controls=None).to('cuda')
    u = gate.get_unitary()
    assert u.is_cuda and torch.equal(u @ u.mH, torch.eye(1 << N, dtype=u.dtype, device='cuda'))
    np.testing.assert_array_equal(u.cpu().numpy(), dense_select(N, SELECT, SYSTEM, STRINGS, PHASES).astype(np.complex64))
    assert torch.equal(gate.inverse().get_unitary(), u.mH.contiguous())
    with pytest.raises(NotImplementedError, match='den_mat'):
        dq.QubitCircuit(N, den_mat=True).select_pauli(STRINGS, wires=SELECT)
    with pytest.raises(NotImplementedError, match='DistributedQubitCircuit'):
        gate.op_dist_state(None)
    with pytest.raises(NotImplementedError, match='DistributedQubitCircuit'):
        gate.prims()


TERMS = [[0.7, 'x0y2'], [-1.3, 'z1'], [0.4, 'y0y1'], [-0.6, ''], [0.9, 'z0x2']]            # 5 strings on 3 wires
PLACEMENTS = [pytest.param([0, 1, 2], [3, 4, 5], id='first'), pytest.param([3, 4, 5], [0, 1, 2], id='last'),
              pytest.param([4, 0, 2], [5, 1, 3], id='interleaved')]


def system_index(n, system):
    m = len(system)
    return [sum(((r >> (m - 1 - a)) & 1) << (n - 1 - system[a]) for a in range(m)) for r in range(1 << m)]


@pytest.mark.parametrize('select,system', PLACEMENTS)
@pytest.mark.parametrize('dtype,tol', PRECISIONS)
def test_block_encoding_identities(dtype, tol, select, system):
    n, m = 6, 3
    hmat = pauli_sum_matrix(TERMS, m)
    cir = dq.QubitCircuit(n)
    lam = cir.block_encode(dq.PauliSum(TERMS, m), wires=select, system_wires=system)
    assert lam == pytest.approx(sum(abs(h) for h, _ in TERMS), rel=1e-15)
    u = finish(cir, dtype).get_unitary()
    assert u.is_cuda and u.dtype == dtype
    u = u.cpu().numpy().astype(np.complex128)
    assert np.abs(u @ u - np.eye(1 << n)).max() < tol
    idx = system_index(n, system)
    assert np.abs(u[np.ix_(idx, idx)] - hmat / lam).max() < tol * np.abs(hmat / lam).max()
    walk = dq.QubitCircuit(n)
    assert walk.qubitization_walk(TERMS, wires=select, system_wires=system) == lam
    finish(walk, dtype)
    energies, vectors = np.linalg.eigh(hmat)
    start = np.zeros((2, 1 << n), dtype=np.complex128)
    start[0, idx], start[1, idx] = vectors[:, 0], vectors[:, 5]
    first = torch.from_numpy(start).to(dtype).cuda()
    v = first.reshape(2, -1, 1)
    with torch.no_grad():
        for j in range(1, 5):
            v = walk(state=v)
            got = (first.conj() * v.reshape(2, -1)).sum(-1).cpu().numpy()
            want = np.cos(j * np.arccos(energies[[0, 5]] / lam))
            assert np.abs(got - want).max() < tol, (j, got, want)


@pytest.mark.parametrize('dtype,tol', PRECISIONS)
def test_block_encoding_under_a_control(dtype, tol):
    """Only SELECT takes the control: with the control at 0 PREPARE and its reversed copy still run and cancel to rounding."""
    n, m = 7, 3
    select, system = [1, 2, 3], [4, 5, 6]
    free = dq.QubitCircuit(n - 1)
    lam = free.block_encode(TERMS, wires=[0, 1, 2], system_wires=[3, 4, 5])
    u = finish(free, dtype).get_unitary()
    cir = dq.QubitCircuit(n)
    assert cir.block_encode(TERMS, wires=select, system_wires=system, controls=[0]) == lam
    finish(cir, dtype)
    x = torch.from_numpy(random_state(np.random.default_rng(3), 2, n, np.complex128)).to(dtype).cuda()
    x = x / x.norm(dim=-1, keepdim=True)
    with torch.no_grad():
        y = cir(state=x.reshape(2, -1, 1)).reshape(2, 2, -1)
    halves = x.reshape(2, 2, -1)
    scale = x.abs().max().item()
    assert (y[:, 0] - halves[:, 0]).abs().max().item() < tol * scale
    assert (y[:, 1] - halves[:, 1] @ u.T).abs().max().item() < tol * scale
