"""DiagonalGate / CostPhase inside circuits on the MI355X: a QAOA layer by two routes, Grover's closed form, the unitary
and the inverse of a circuit that contains them, encoded batches, and what is refused."""

import math

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import qmath

pytestmark = pytest.mark.gpu

PREC = {'c64': (torch.float32, 1e-4), 'c128': (torch.float64, 1e-10)}


def k6_edges():
    return [(i, j) for i in range(6) for j in range(i + 1, 6)]


def qaoa(route, dt, t0=0.37, beta0=0.61):
    """One QAOA layer on K_6 with unit weights.  Route A: one Rzz(2 t) per edge (Rzz(theta) = exp(-i theta/2 ZZ));
    route B: exp(-i t C) with the table C = sum_edges Z_i Z_j.  Both hold exactly the same angles."""
    n = 6
    real, _ = PREC[dt]
    cir = dq.QubitCircuit(n)
    cir.hlayer()
    if route == 'A':
        for e in k6_edges():
            cir.rzz(list(e), inputs=2 * t0)
    else:
        cir.cost_phase(qmath.ising_cost(n, [(1.0, list(e)) for e in k6_edges()], dtype=real, device='cuda'), inputs=t0)
    cir.rxlayer(inputs=[2 * beta0] * n)
    cir.to('cuda')
    if real == torch.float64:
        cir.to(torch.double)
    return cir


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_qaoa_layer_by_two_routes(dt):
    real, tol = PREC[dt]
    n = 6
    table = qmath.ising_cost(n, [(1.0, list(e)) for e in k6_edges()], dtype=real, device='cuda')
    states, grads, costs = {}, {}, {}
    for route in 'AB':
        cir = qaoa(route, dt)
        gamma = torch.tensor(0.37, dtype=real, device='cuda', requires_grad=True)
        beta = torch.tensor(0.61, dtype=real, device='cuda', requires_grad=True)
        # the same two leaves feed every gate of the layer: d<C>/dt and d<C>/dbeta come out of one backward()
        for op in cir.operators:
            if isinstance(op, dq.Rzz):
                op.init_para(2 * gamma)
            elif isinstance(op, dq.CostPhase):
                op.init_para(gamma)
            elif isinstance(op, dq.Rx):
                op.init_para(2 * beta)
        state = cir()
        cost = cir.expectation_cost(table)
        cost.backward()
        states[route], costs[route], grads[route] = state.detach(), cost.detach(), (gamma.grad.item(), beta.grad.item())
        if route == 'B':
            for e in k6_edges():
                cir.observable(list(e))
            zz = cir.expectation().detach().sum()
            print(f'{dt}: <C> table {cost.item():+.9f}, sum of 15 <ZZ> {zz.item():+.9f}')
            assert abs(cost.item() - zz.item()) <= tol * 15
    err = (states['A'] - states['B']).abs().max().item()
    print(f'{dt}: routes differ by {err:.3e} (largest amplitude {states["A"].abs().max().item():.3e}); '
          f'grads A {grads["A"]}, B {grads["B"]}')
    assert err <= tol * states['A'].abs().max().item()
    assert abs(costs['A'].item() - costs['B'].item()) <= tol * 15
    gtol = 1e-3 if dt == 'c64' else 1e-9            # (gradients of <C> ~ 15 terms through 30 gates of float32 / float64 angles)
    assert abs(grads['A'][0] - grads['B'][0]) <= gtol * max(1.0, abs(grads['A'][0]))
    assert abs(grads['A'][1] - grads['B'][1]) <= gtol * max(1.0, abs(grads['A'][1]))
    assert abs(grads['B'][0]) > 1e-2 and abs(grads['B'][1]) > 1e-2


def test_grover_closed_form():
    n, marked, iters = 10, 0b1011001110, 25
    assert iters == math.floor(math.pi / 4 * math.sqrt(1 << n))
    oracle = torch.ones(1 << n, dtype=torch.complex64)
    oracle[marked] = -1
    about_zero = -torch.ones(1 << n, dtype=torch.complex64)
    about_zero[0] = 1                                   # 2 |0><0| - 1
    cir = dq.QubitCircuit(n)
    cir.hlayer()
    for _ in range(iters):
        cir.diagonal(oracle)
        cir.hlayer()
        cir.diagonal(about_zero)
        cir.hlayer()
    cir.to('cuda')
    with torch.no_grad():
        state = cir().reshape(-1)
    p = (state[marked].abs() ** 2).item()
    want = math.sin((2 * iters + 1) * math.asin(1 / 32)) ** 2
    print(f'grover: p(marked) = {p:.6f}, closed form {want:.6f}, norm {state.norm().item():.7f}')
    assert abs(p - want) < 1e-3
    assert int(state.abs().argmax()) == marked


def test_get_unitary_and_inverse():
    n = 3
    g = torch.Generator().manual_seed(2)
    c = torch.randn(4, dtype=torch.float64, generator=g)
    d = torch.exp(1j * torch.randn(8, dtype=torch.float64, generator=g))
    cir = dq.QubitCircuit(n)
    cir.h(0)
    cir.cost_phase(c, wires=[2, 0], inputs=0.4)
    cir.diagonal(d)
    cir.to('cuda').to(torch.double)
    t = float(cir.operators[1].t)
    h = torch.tensor([[1, 1], [1, -1]], dtype=torch.complex64).div(2**0.5).to(torch.complex128)     # (as the library rounds it)
    eye = torch.eye(2, dtype=torch.complex128)
    u_h = torch.kron(torch.kron(h, eye), eye)
    i = np.arange(8)
    sub = (((i >> 0) & 1) << 1) | ((i >> 2) & 1)        # wires [2, 0] = bits [0, 2], wires[0] the MSB
    u_c = torch.diag(torch.exp(-1j * t * c[sub]))
    ref = torch.diag(d) @ u_c @ u_h
    got = cir.get_unitary().cpu()
    assert (got - ref).abs().max().item() < 1e-10
    both = cir + cir.inverse()
    assert (both.get_unitary().cpu() - torch.eye(8, dtype=torch.complex128)).abs().max().item() < 1e-7
    x = torch.randn(8, 1, dtype=torch.complex128, generator=g).cuda()
    with torch.no_grad():
        back = cir.inverse()(state=cir(state=x))
    assert (back - x).abs().max().item() < 1e-7       # (H H = 1 to the float32 rounding of 1/sqrt(2))


def test_encoded_batch_equals_single_runs():
    n = 4
    c = torch.randn(1 << n, dtype=torch.float64, generator=torch.Generator().manual_seed(4)).cuda()
    cir = dq.QubitCircuit(n)
    cir.hlayer()
    cir.cost_phase(c, encode=True)
    cir.rxlayer(inputs=[0.3] * n)
    cir.to('cuda').to(torch.double)
    assert cir.ndata == 1 and cir.encoders == [cir.operators[n]]
    data = torch.tensor([[0.1], [0.7], [-1.3]], dtype=torch.float64, device='cuda', requires_grad=True)
    batch = cir(data)
    assert batch.shape == (3, 1 << n, 1)
    cir.expectation_cost(c).sum().backward()
    singles, grads = [], []
    for b in range(3):
        one = data.detach()[b].clone().requires_grad_()
        singles.append(cir(one).detach())
        cir.expectation_cost(c).backward()
        grads.append(one.grad)
    assert (batch.detach() - torch.stack(singles)).abs().max().item() < 1e-12
    assert (data.grad - torch.stack(grads)).abs().max().item() < 1e-10
    assert data.grad.abs().min().item() > 1e-3


def test_refusals():
    c = torch.randn(4)
    makers = {'CostPhase': lambda **kw: dq.CostPhase(c, nqubit=2, **kw),
              'DiagonalGate': lambda **kw: dq.DiagonalGate(torch.ones(4, dtype=torch.complex64), nqubit=2, **kw)}
    for name, make in makers.items():
        with pytest.raises(NotImplementedError, match=name):
            make(den_mat=True)
        dm = dq.QubitCircuit(2, den_mat=True)
        with pytest.raises(NotImplementedError, match=name):
            if name == 'CostPhase':
                dm.cost_phase(c)
            else:
                dm.diagonal(torch.ones(4, dtype=torch.complex64))
        with pytest.raises(NotImplementedError, match=name):
            make().op_dist_state(None)
        with pytest.raises(NotImplementedError, match=name):
            from deepquantum_amd.distributed import dist_run

            dist_run(None, [make()])
        cir = dq.QubitCircuit(2)
        cir.add(make())
        with pytest.raises(NotImplementedError, match=name):
            cir.qasm()
