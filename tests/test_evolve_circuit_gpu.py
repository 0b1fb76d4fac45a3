"""``cir.pauli_sum_evolution`` inside circuits on the MI355X: a 6-wire circuit with ordinary gates on both sides of the new
gate against the dense exponential and against ``cir.hamiltonian`` with the same list."""

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from _psum_ref import dense_psum

pytestmark = pytest.mark.gpu

N = 6
# (coefficients that float32 holds exactly: HamiltonianGate keeps its list in the default precision)
HAM = [[0.5, 'x0y1'], [-0.625, 'z3y1'], [0.25, ''], [0.75, 'z0z5'], [0.375, 'y0y2y4'], [-0.5, 'x1x2x3'], [0.875, 'y2'], [0.5, 'x4x5'],
       [-0.25, 'z4']]
TOL = {False: 1e-4, True: 1e-10}


def front(cir):
    cir.hlayer()
    cir.ry(2)
    cir.cnot(0, 3)
    cir.rx(5, inputs=0.3)


def back(cir):
    cir.ry(1)
    cir.cnot(4, 1)
    cir.rz(0, inputs=-0.7)


def of_type(cir, name):
    return [op for op in cir.operators if type(op).__name__ == name]


def build(kind, double, t=None, encode=False):
    cir = dq.QubitCircuit(N)
    front(cir)
    getattr(cir, kind)(HAM, t=t, encode=encode)
    back(cir)
    cir.observable(0)
    cir.observable([1, 4], 'xz')
    cir.to('cuda')
    if double:
        cir.to(torch.double)
    return cir


@pytest.mark.parametrize('double', [False, True], ids=['c64', 'c128'])
def test_value_and_gradient_against_the_dense_routes(double):
    torch.manual_seed(4)
    new = build('pauli_sum_evolution', double)
    old = build('hamiltonian', double)
    (gate,) = of_type(new, 'PauliSumEvolution')
    assert isinstance(gate.t, torch.nn.Parameter) and len(list(new.parameters())) == len(list(old.parameters())) == 3
    with torch.no_grad():
        for p, q in zip(new.parameters(), old.parameters()):
            q.copy_(p)
    s_new, s_old = new().reshape(-1), old().reshape(-1)
    assert (s_new - s_old).abs().max().item() < TOL[double]
    # against the dense exponential itself: the gates in front, the matrix, the gates behind
    t = float(gate.t)
    u = torch.linalg.matrix_exp(-1j * t * torch.from_numpy(dense_psum(N, HAM))).cuda().to(s_new.dtype)
    pre = dq.QubitCircuit(N)
    front(pre)
    post = dq.QubitCircuit(N)
    back(post)
    for cir in (pre, post):
        cir.to('cuda')
        if double:
            cir.to(torch.double)
    with torch.no_grad():
        of_type(pre, 'Ry')[0].theta.copy_(of_type(new, 'Ry')[0].theta)
        of_type(post, 'Ry')[0].theta.copy_(of_type(new, 'Ry')[1].theta)
        mid = u @ pre().reshape(-1)
        want = post(state=mid.reshape(-1, 1)).reshape(-1)
    assert (s_new.detach() - want).abs().max().item() < TOL[double]
    # the gradient of an expectation with respect to t and the two neighbouring ry angles
    g_new = torch.autograd.grad(new.expectation().sum(), list(new.parameters()))
    g_old = torch.autograd.grad(old.expectation().sum(), list(old.parameters()))
    for a, b in zip(g_new, g_old):
        assert (a - b).abs().max().item() < TOL[double]
    assert all(g.abs().max().item() > 1e-3 for g in g_new)


@pytest.mark.parametrize('double', [False, True], ids=['c64', 'c128'])
def test_encoded_batch_of_t(double):
    torch.manual_seed(5)
    new = build('pauli_sum_evolution', double, encode=True)
    assert new.ndata == 1 and len(list(new.parameters())) == 2
    data = torch.tensor([[0.4], [-1.1], [0.0]], dtype=torch.float64 if double else torch.float32, device='cuda')
    states = new(data).reshape(3, -1)
    dense = torch.from_numpy(dense_psum(N, HAM))
    pre = dq.QubitCircuit(N)
    front(pre)
    post = dq.QubitCircuit(N)
    back(post)
    for cir in (pre, post):
        cir.to('cuda')
        if double:
            cir.to(torch.double)
    with torch.no_grad():
        of_type(pre, 'Ry')[0].theta.copy_(of_type(new, 'Ry')[0].theta)
        of_type(post, 'Ry')[0].theta.copy_(of_type(new, 'Ry')[1].theta)
        psi = pre().reshape(-1)
        for s in range(3):
            u = torch.linalg.matrix_exp(-1j * float(data[s, 0]) * dense).cuda().to(psi.dtype)
            want = post(state=(u @ psi).reshape(-1, 1)).reshape(-1)
            assert (states[s] - want).abs().max().item() < TOL[double], s
    assert np.isfinite(new.expectation().detach().cpu().numpy()).all()
