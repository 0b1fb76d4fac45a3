"""``cir.mid_measure`` and ``qmath.collapse_state`` on the GPU: teleportation with spectator wires, the three-qubit bit-flip
code with a look-up decoder and reset ancillas, and the dropped layout against ``slice_state_vector``.  1e-5 in complex64,
1e-12 in complex128."""

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import qmath

pytestmark = pytest.mark.gpu

PRECISIONS = [pytest.param(torch.complex64, 1e-5, id='c64'), pytest.param(torch.complex128, 1e-12, id='c128')]


def finish(cir, dtype):
    cir.to('cuda')
    if dtype == torch.complex128:
        cir.to(torch.double)
    return cir


def qubits(rng, batch, dtype):
    a = rng.standard_normal((batch, 2)) + 1j * rng.standard_normal((batch, 2))
    return torch.from_numpy(a / np.linalg.norm(a, axis=1, keepdims=True)).to(dtype).cuda()


def on_wire_zero(a, n):
    state = torch.zeros(a.shape[0], 1 << n, dtype=a.dtype, device=a.device)
    state[:, 0], state[:, 1 << (n - 1)] = a[:, 0], a[:, 1]
    return state.reshape(a.shape[0], -1, 1)


@pytest.mark.parametrize('n', [3, 12])
@pytest.mark.parametrize('dtype,tol', PRECISIONS)
def test_teleportation_with_spectators(dtype, tol, n):
    torch.manual_seed(n)
    a = qubits(np.random.default_rng(n), 8, dtype)
    target = n - 1
    cir = dq.QubitCircuit(n)
    for w in range(2, target):
        cir.ry(w)                                        # spectators: random angles
    cir.h(1)
    cir.cnot(1, target)
    cir.cnot(0, 1)
    cir.h(0)
    cir.mid_measure([0, 1], correct={'00': '', '01': f'x{target}', '10': f'z{target}', '11': f'x{target}z{target}'})
    with torch.no_grad():
        out = finish(cir, dtype)(state=on_wire_zero(a, n))
    (o,), (p,) = cir.outcomes, cir.outcome_probs
    assert o.is_cuda and o.dtype == torch.int64 and o.shape == (8,) and p.dtype == torch.float64
    assert (p - 0.25).abs().max().item() < tol
    rho = qmath.reduced_density_matrix(out, n, [target])
    want = a[:, :, None] * a[:, None, :].conj()
    assert (rho - want).abs().max().item() < tol


@pytest.mark.parametrize('flipped', [None, 0, 1, 2])
@pytest.mark.parametrize('dtype,tol', PRECISIONS)
def test_bit_flip_code_with_a_lookup_decoder(dtype, tol, flipped):
    a = qubits(np.random.default_rng(3), 4, dtype)
    cir = dq.QubitCircuit(5)
    cir.cnot(0, 1)
    cir.cnot(0, 2)
    if flipped is not None:
        cir.x(flipped)
    for data, anc in ((0, 3), (1, 3), (1, 4), (2, 4)):
        cir.cnot(data, anc)
    cir.mid_measure([3, 4], correct=lambda s: {0: None, 2: 'x0', 3: 'x1', 1: 'x2'}[s], reset=True)
    with torch.no_grad():
        out = finish(cir, dtype)(state=on_wire_zero(a, 5)).reshape(4, 32)
    encoded = torch.zeros_like(out)
    encoded[:, 0], encoded[:, 0b11100] = a[:, 0], a[:, 1]                # a|000>|00> + b|111>|00>
    assert ((encoded.conj() * out).sum(-1).abs() - 1).abs().max().item() < tol
    assert cir.outcomes[0].tolist() == [{None: 0, 0: 2, 1: 3, 2: 1}[flipped]] * 4
    assert out.reshape(4, 8, 4)[:, :, 1:].abs().max().item() == 0        # the ancillas are in |00>


@pytest.mark.parametrize('dtype,tol', PRECISIONS)
def test_dropped_collapse_is_the_slice(dtype, tol):
    rng = np.random.default_rng(0)
    n, wires = 12, [9, 2, 11]
    x = torch.from_numpy(rng.standard_normal((3, 1 << n)) + 1j * rng.standard_normal((3, 1 << n))).to(dtype).cuda()
    x = x / x.norm(dim=-1, keepdim=True)
    got, o, p = qmath.collapse_state(x, n, wires, outcome='101', drop=True)
    want = qmath.slice_state_vector(x, n, sorted(wires), '101')
    assert got.shape == (3, 1 << (n - 3)) and o.tolist() == [5, 5, 5]
    assert (got - want).abs().max().item() < tol * want.abs().max().item()
