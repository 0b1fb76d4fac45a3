"""``cir.expectation_pauli_sum`` on the MI355X: a 6-wire circuit of rx, cnot, pauli_rot and single_excitation, the energy of
a Pauli sum in one launch against the dense matrix (value) and against the same energy written string by string through
``cir.observable`` and ``expectation()`` (gradient), a batch of data, and a replay under ``dq.CapturedGraph``."""

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import qmath
from _psum_ref import dense_psum, energy_per_string

pytestmark = pytest.mark.gpu

N = 6
HAM = [[0.5, 'x0y1'], [-1, 'z3y1'], [0.25, ''], [0.7, 'z0z5'], [0.3, 'y0y2y4'], [-0.4, 'x1x2x3'], [0.2, 'y0y1y3x5'], [1.5, 'y2'],
       [0.6, 'x5'], [-0.9, 'z1z2z3z4'], [0.35, 'x0x1x2x3x4x5'], [-0.45, 'z4']]
DATA = [0.3, -0.8, 1.1, 0.45, -0.2, 0.9, 1.7, -1.4, 0.65]


def build(double):
    cir = dq.QubitCircuit(N)
    cir.hlayer()
    cir.rxlayer(encode=True)
    cir.cnot(0, 1)
    cir.pauli_rot('xyz', wires=[0, 2, 5], encode=True)
    cir.single_excitation([1, 4], encode=True)
    cir.cnot(3, 5)
    cir.rx(2, encode=True)
    cir.to('cuda')
    if double:
        cir.to(torch.double)
    return cir


@pytest.mark.parametrize('double', [False, True], ids=['c64', 'c128'])
def test_value_gradient_and_batch(double):
    real = torch.float64 if double else torch.float32
    tol = 1e-10 if double else 1e-4
    H = dq.PauliSum(HAM, N)
    size = sum(abs(h) for h, _ in HAM)
    data = torch.tensor(DATA, dtype=real, device='cuda', requires_grad=True)
    cir = build(double)
    psi = cir(data)
    e = cir.expectation_pauli_sum(H)
    assert e.shape == () and e.dtype == real
    ev = float(e.detach())
    pr = psi.detach().reshape(-1).cpu().numpy().astype(np.complex128)
    assert abs(ev - (pr.conj() @ dense_psum(N, HAM) @ pr).real) <= tol * size
    (g_new,) = torch.autograd.grad(e, data)
    other = data.detach().clone().requires_grad_()
    e_old = energy_per_string(build(double), other, HAM)
    (g_old,) = torch.autograd.grad(e_old, other)
    assert abs(ev - float(e_old.detach())) <= tol * size
    assert (g_new - g_old).abs().max().item() <= tol * size and g_new.abs().max().item() > 1e-2
    assert abs(float(cir.expectation_pauli_sum(HAM).detach()) - ev) <= tol * size           # the list form
    # a batch of data: every row is the single run
    batch = torch.stack([data.detach(), data.detach().flip(0), 0.5 * data.detach()]).requires_grad_()
    cir(batch)
    eb = cir.expectation_pauli_sum(H)
    assert eb.shape == (3,) and abs(float(eb[0].detach()) - ev) <= tol * size
    (gb,) = torch.autograd.grad(eb.sum(), batch)
    assert (gb[0] - g_new).abs().max().item() <= tol * size
    for b in (1, 2):
        one = batch.detach()[b].clone().requires_grad_()
        cir(one)
        eo = cir.expectation_pauli_sum(H)
        assert abs(float(eo.detach()) - float(eb[b].detach())) <= tol * size
        assert (torch.autograd.grad(eo, one)[0] - gb[b]).abs().max().item() <= tol * size


def test_captured_graph_replays_the_eager_value():
    n = 14
    g = torch.Generator().manual_seed(6)
    psi = torch.randn(4, 1 << n, dtype=torch.complex128, generator=g).to(torch.complex64).cuda()
    H = dq.PauliSum([[0.5, 'x0y13'], [-1, 'z3y1'], [0.25, ''], [0.7, 'z0z5'], [0.3, 'y2y12'], [0.6, 'x13'], [-0.2, 'x2z7x13']], n)
    eager = (qmath.expectation_pauli_sum(psi, n, H), qmath.apply_pauli_sum(psi, n, H))
    graph = dq.CapturedGraph(lambda: (qmath.expectation_pauli_sum(psi, n, H), qmath.apply_pauli_sum(psi, n, H)))
    for _ in range(2):
        out = graph.replay()
        torch.testing.assert_close(out[0], eager[0], rtol=0, atol=0)
        torch.testing.assert_close(out[1], eager[1], rtol=0, atol=0)
