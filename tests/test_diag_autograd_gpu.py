"""Autograd through the diagonal kernels on the MI355X, complex128, n = 4 and 5: the three operations that differentiate
into one another (ops.cost_phase / cost_cross / cost_scale), the read-out built on them, and ``torch.func``."""

import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import ops, qmath

pytestmark = pytest.mark.gpu


def state(batch, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, 1 << n, dtype=torch.complex128, generator=g).cuda()


def table(k, seed):
    return torch.randn(1 << k, dtype=torch.float64, generator=torch.Generator().manual_seed(seed)).cuda()


@pytest.mark.parametrize('n', [4, 5])
def test_cost_phase_gradcheck_with_a_control_and_a_gathered_table(n):
    bits, controls = (0, n - 1), (2,)
    c = table(2, n)
    x = state(2, n, 1).requires_grad_()
    t = torch.tensor([0.3, -0.8], dtype=torch.float64, device='cuda', requires_grad=True)
    f = lambda a, b: ops.cost_phase(a, c, b, bits, controls)  # noqa: E731
    assert torch.autograd.gradcheck(f, (x, t))
    assert torch.autograd.gradgradcheck(f, (x, t))


@pytest.mark.parametrize('n', [4, 5])
def test_cost_cross_gradcheck(n):
    bits, controls = (0, n - 1), (2,)
    c = table(2, n)
    x, y = state(2, n, 2).requires_grad_(), state(2, n, 3).requires_grad_()
    f = lambda a, b: ops.cost_cross(a, b, c, bits, controls)  # noqa: E731
    assert torch.autograd.gradcheck(f, (x, y))
    assert torch.autograd.gradgradcheck(f, (x, y))
    full = tuple(range(n - 1, -1, -1))
    cn = table(n, 7)
    assert torch.autograd.gradcheck(lambda a, b: ops.cost_cross(a, b, cn, full), (x, y))


@pytest.mark.parametrize('n', [4, 5])
def test_expectation_cost_gradcheck(n):
    cn = table(n, 5)
    x = state(2, n, 4).requires_grad_()
    assert torch.autograd.gradcheck(lambda a: qmath.expectation_cost(a, n, cn), (x,))
    assert torch.autograd.gradgradcheck(lambda a: qmath.expectation_cost(a, n, cn), (x,))
    c2 = table(2, 6)
    assert torch.autograd.gradcheck(lambda a: qmath.expectation_cost(a, n, c2, [n - 1, 1]), (x,))


def test_vmap_and_func_grad_through_a_circuit():
    """The circuit object itself under the transforms: a per-sample loop equals ``torch.vmap`` over ``cir`` with ``t`` fed as
    data, ``torch.func.grad`` through it matches finite differences, and ``vmap(grad)`` equals the loop of gradients.
    That is ``_run_operators`` flushing a fused stretch, ``CostPhase.apply_flat`` with a wrapped ``t``, and a new stretch
    with the zero-state shortcut off."""
    n = 4
    c = qmath.ising_cost(n, [(1.0, [i, j]) for i in range(n) for j in range(i + 1, n)] + [(0.5, [2])],
                         dtype=torch.float64, device='cuda')
    cir = dq.QubitCircuit(n)
    cir.hlayer()
    cir.cost_phase(c, encode=True)
    cir.rxlayer(inputs=[0.4, -0.9, 1.3, 0.2])
    cir.to('cuda').to(torch.double)
    gate = cir.operators[n]
    assert isinstance(gate, dq.CostPhase) and cir.encoders == [gate]

    def f(th):
        return qmath.expectation_cost(cir(th.reshape(1)), n, c)

    ts = torch.tensor([0.1, 0.5, -2.0], dtype=torch.float64, device='cuda')
    loop = torch.stack([f(th) for th in ts])
    assert loop.std().item() > 1e-2
    assert torch.allclose(torch.vmap(f)(ts), loop, atol=1e-12)
    eps = 1e-6
    fd = torch.stack([(f(th + eps) - f(th - eps)) / (2 * eps) for th in ts])
    g = torch.stack([torch.func.grad(f)(th) for th in ts])
    assert torch.allclose(g, fd, atol=1e-7) and g.abs().min().item() > 1e-3
    assert torch.allclose(torch.vmap(torch.func.grad(f))(ts), g, atol=1e-12)
    # the parameter set by hand under the transform, and the same three values through eager runs
    def h(th):
        gate.init_para(th)
        return qmath.expectation_cost(cir(), n, c)

    assert torch.allclose(torch.vmap(h)(ts), loop, atol=1e-12)
    for th, want in zip(ts, loop):
        gate.init_para(th)
        cir()
        assert abs(float(cir.expectation_cost(c)) - float(want)) < 1e-12


def test_a_table_that_requires_grad_is_refused():
    x = state(1, 3, 1)
    c = table(3, 1).requires_grad_()
    t = torch.tensor(0.2, dtype=torch.float64, device='cuda')
    full = (2, 1, 0)
    for call in (lambda: ops.cost_phase(x, c, t, full), lambda: ops.cost_cross(x, x, c, full),
                 lambda: ops.cost_scale(x, c, t + 0j, full), lambda: qmath.expectation_cost(x, 3, c),
                 lambda: ops.diag_mul(x, torch.exp(1j * c), full), lambda: dq.CostPhase(c, nqubit=3)):
        with pytest.raises(ValueError, match='constant'):
            call()
