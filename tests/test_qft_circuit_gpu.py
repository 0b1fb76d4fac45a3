"""``cir.qft`` / ``QuantumFourierTransform(native=True)`` inside circuits on the GPU against the replayed gate sequence of
the same circuit, in complex128 at 1e-10: states, unitaries, first and second derivatives, ``vmap``.

The gate sequence keeps its angles and the Hadamard matrix as float32 numbers (pi / 2^d and 1 / sqrt 2 rounded: 4e-8
off), which ``.to(torch.double)`` widens but cannot restore -- measured, the converted sequence is 1.5e-8 from the DFT
matrix that the native gate meets to 1e-10.  ``exact_angles`` sets every controlled phase of the reference back to
pi / 2^d and every Hadamard to 1 / sqrt 2 in double, so that the reference is good to the bar it is held to."""

import math

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import ops
from _qft_ref import dft_matrix

pytestmark = pytest.mark.gpu

BAR = 1e-10


def exact_angles(cir):
    for op in cir.operators:
        if isinstance(op, dq.PhaseShift):
            t = float(op.theta)
            op.init_para(torch.tensor(math.copysign(math.pi / 2 ** round(math.log2(math.pi / abs(t))), t), dtype=torch.float64))
        elif isinstance(op, dq.Hadamard):
            op.register_buffer('matrix', torch.tensor([[1, 1], [1, -1]], dtype=torch.complex128) / math.sqrt(2))
    return cir


def pair(n, minmax, reverse, inverse):
    out = []
    for native in (False, True):
        cir = dq.QuantumFourierTransform(n, minmax=minmax, reverse=reverse, native=native)
        cir = cir.inverse() if inverse else cir
        cir.to(torch.double)
        out.append((cir if native else exact_angles(cir)).to('cuda'))
    return out


@pytest.mark.parametrize('inverse', [False, True])
@pytest.mark.parametrize('reverse', [False, True])
@pytest.mark.parametrize('n,minmax', [(6, [1, 4]), (5, [0, 4])])
def test_native_ansatz_against_the_gate_sequence(n, minmax, reverse, inverse):
    gates, native = pair(n, minmax, reverse, inverse)
    assert len(native.operators) == 1 and len(gates.operators) > 4
    want = gates.get_unitary()
    assert want.dtype == torch.complex128 and (native.get_unitary() - want).abs().max().item() < BAR
    # the same on a state that other gates prepared, and through cir.qft
    prep, direct = dq.QubitCircuit(n), dq.QubitCircuit(n)
    for cir in (prep, direct):
        cir.hlayer()
        cir.rylayer(inputs=[0.1 * (k + 1) for k in range(n)])
    direct.qft(minmax=minmax, swaps=not reverse, inverse=inverse)
    for cir in (prep, direct):
        cir.to(torch.double).to('cuda')
    with torch.no_grad():
        psi = prep()
        want = gates(state=psi).reshape(-1)
        assert (native(state=psi).reshape(-1) - want).abs().max().item() < BAR
        assert (direct().reshape(-1) - want).abs().max().item() < BAR


def test_unitary_of_a_gate_is_the_dft_matrix():
    u = dq.QFTGate(nqubit=4, wires=[0, 1, 2, 3]).double().to('cuda').get_unitary().cpu().numpy()
    assert np.abs(u - dft_matrix(4)).max() < BAR


def expectation(native, data):
    n = 5
    cir = dq.QubitCircuit(n)
    cir.rxlayer(encode=True)
    if native:
        cir.qft(wires=[3, 0, 4, 1])
    else:
        wires, m = [3, 0, 4, 1], 4
        for i, w in enumerate(wires):
            cir.h(w)
            for d in range(1, m - i):
                cir.cp(wires[i + d], w, torch.tensor(math.pi / 2**d, dtype=torch.float64))
        cir.swap([3, 1])
        cir.swap([0, 4])
    cir.observable(0)
    exact_angles(cir.to(torch.double)).to('cuda')
    cir(data=data)
    return cir.expectation().sum()


def test_first_and_second_derivatives_against_the_gate_sequence():
    base = torch.tensor([0.3, -0.7, 1.1, 0.5, -0.2], dtype=torch.float64, device='cuda')
    grads = []
    for native in (False, True):
        data = base.clone().requires_grad_(True)
        (g,) = torch.autograd.grad(expectation(native, data), data, create_graph=True)
        (h,) = torch.autograd.grad(g.sum(), data)
        grads.append((g.detach(), h))
    assert grads[0][0].abs().max() > 1e-3
    assert (grads[0][0] - grads[1][0]).abs().max().item() < BAR and (grads[0][1] - grads[1][1]).abs().max().item() < BAR


def test_vmap():
    x = torch.randn(3, 2, 64, dtype=torch.complex128, device='cuda')
    got = torch.vmap(lambda s: ops.qft(s, (4, 1, 2)))(x)
    assert torch.equal(got, ops.qft(x.reshape(6, 64), (4, 1, 2)).reshape(3, 2, 64))
