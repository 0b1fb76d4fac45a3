"""Autograd through the Pauli-string kernels on the MI355X, complex128, n = 4 and 5: the operations that differentiate
into one another (ops.pauli_axpby / pauli_cross), the rotation node on top of them (ops.pauli_rot), the gates' parameters
inside circuits, and ``torch.func``."""

import math

import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import ops

pytestmark = pytest.mark.gpu


def state(batch, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, 1 << n, dtype=torch.complex128, generator=g).cuda()


def masks(n):
    """x on bits n-1 and 1, y on bit 0, z on bit 3 -- with a control on bit 2."""
    return 1 << (n - 1) | 0b11, 0b1001, (2,)


@pytest.mark.parametrize('mode', ['gate', 'map'])
@pytest.mark.parametrize('n', [4, 5])
def test_pauli_axpby_gradcheck_with_a_control_and_a_y(n, mode):
    xmask, zmask, controls = masks(n)
    x = state(2, n, 1).requires_grad_()
    a = torch.tensor([0.3 - 0.2j, 1.1j], dtype=torch.complex128, device='cuda', requires_grad=True)
    c = torch.tensor([-0.6 + 0.1j, 0.4], dtype=torch.complex128, device='cuda', requires_grad=True)
    f = lambda s, p, q: ops.pauli_axpby(s, xmask, zmask, p, q, controls, mode)  # noqa: E731
    assert torch.autograd.gradcheck(f, (x, a, c))
    assert torch.autograd.gradgradcheck(f, (x, a, c))


@pytest.mark.parametrize('n', [4, 5])
def test_pauli_cross_gradcheck(n):
    xmask, zmask, controls = masks(n)
    x, y = state(2, n, 2).requires_grad_(), state(2, n, 3).requires_grad_()
    f = lambda u, v: ops.pauli_cross(u, v, xmask, zmask, controls)  # noqa: E731
    assert torch.autograd.gradcheck(f, (x, y))
    assert torch.autograd.gradgradcheck(f, (x, y))
    assert torch.autograd.gradcheck(lambda u: ops.pauli_cross(u, u, xmask, zmask), (x,))       # bra is ket: one read
    assert torch.autograd.gradcheck(lambda u, v: ops.pauli_cross(u, v, 0, 0, controls), (x, y))  # the plain inner product


@pytest.mark.parametrize('n', [4, 5])
def test_pauli_rot_gradcheck_with_a_per_sample_angle(n):
    xmask, zmask, controls = masks(n)
    x = state(2, n, 4).requires_grad_()
    th = torch.tensor([0.3, -0.8], dtype=torch.float64, device='cuda', requires_grad=True)
    one = torch.tensor(0.45, dtype=torch.float64, device='cuda', requires_grad=True)
    f = lambda s, p: ops.pauli_rot(s, xmask, zmask, p, controls)  # noqa: E731
    assert torch.autograd.gradcheck(f, (x, th))
    assert torch.autograd.gradgradcheck(f, (x, th))
    assert torch.autograd.gradcheck(f, (x, one))                            # a shared angle: the sum of the samples' gradients
    assert torch.autograd.gradcheck(f, (x, th), check_forward_ad=True, check_backward_ad=False)
    assert torch.autograd.gradcheck(lambda s, p: ops.pauli_rot(s, 0, 0b110, p), (x, th))       # a Z string: no partner


def z0_circuit(n, theta=None):
    cir = dq.QubitCircuit(n)
    cir.hlayer()
    cir.rylayer(inputs=[0.3 * (i + 1) for i in range(n)])
    cir.cnot_ring()
    cir.pauli_rot('yzx', wires=[0, 2, 3], inputs=theta)
    cir.rxlayer(inputs=[-0.2 * (i + 1) for i in range(n)])
    cir.observable(0)
    return cir.to('cuda').to(torch.double)


def test_trainable_angle_against_the_parameter_shift_rule():
    """d<Z0>/dtheta of a circuit with a trainable PauliRot = (f(theta + pi/2) - f(theta - pi/2)) / 2."""
    n = 4
    cir = z0_circuit(n)
    gate = cir.operators[2 * n + n]
    assert isinstance(gate, dq.PauliRot) and isinstance(gate.theta, torch.nn.Parameter)
    cir()
    cir.expectation().sum().backward()
    grad = float(gate.theta.grad)
    th = float(gate.theta.detach())

    def f(value):
        with torch.no_grad():
            fixed = z0_circuit(n, theta=torch.tensor(value, dtype=torch.float64))
            fixed()
            return float(fixed.expectation().sum())

    shift = (f(th + math.pi / 2) - f(th - math.pi / 2)) / 2
    assert abs(shift) > 1e-3 and abs(grad - shift) < 1e-10


def test_evolution_time_against_finite_differences():
    n = 4
    ham = [[0.8, 'x0z2'], [-0.6, 'y2'], [0.3, 'z0y1x3'], [0.5, 'x1x2']]
    x = state(1, n, 6)
    x = x / x.norm()
    zmask = 1 << (n - 1)

    def f(t, steps, order):
        y = dq.PauliEvolution(ham, t=t, nqubit=n, steps=steps, order=order).apply_flat(x)
        return ops.pauli_cross(y, y, 0, zmask).real.sum()

    for steps, order in ((1, 1), (2, 2)):
        t = torch.tensor(0.37, dtype=torch.float64, device='cuda', requires_grad=True)
        (g,) = torch.autograd.grad(f(t, steps, order), t)
        eps = 1e-6
        with torch.no_grad():
            fd = (f(t + eps, steps, order) - f(t - eps, steps, order)) / (2 * eps)
        assert abs(float(fd)) > 1e-3 and abs(float(g) - float(fd)) < 1e-7
        assert torch.autograd.gradcheck(lambda v: f(v, steps, order), (t,))


def test_vmap_and_func_grad_through_a_circuit():
    """The circuit object itself under the transforms: a per-sample loop equals ``torch.vmap`` over ``cir`` with ``theta``
    fed as data, ``torch.func.grad`` through it matches finite differences, and ``vmap(grad)`` equals the loop of
    gradients."""
    n = 4
    cir = dq.QubitCircuit(n)
    cir.hlayer()
    cir.pauli_rot('xyx', wires=[3, 0, 1], encode=True, controls=[2])
    cir.rxlayer(inputs=[0.4, -0.9, 1.3, 0.2])
    cir.pauli_evolution([[0.7, 'z0z1'], [0.4, 'x1y3']], t=0.3, steps=2, order=2)
    cir.to('cuda').to(torch.double)
    gate = cir.operators[n]
    assert isinstance(gate, dq.PauliRot) and cir.encoders == [gate]
    zmask = 1 << (n - 1)

    def f(th):
        psi = cir(th.reshape(1)).reshape(1, -1)
        return ops.pauli_cross(psi, psi, 0, zmask).real.sum()

    ts = torch.tensor([0.1, 0.5, -2.0], dtype=torch.float64, device='cuda')
    loop = torch.stack([f(th) for th in ts])
    assert loop.std().item() > 1e-2
    assert torch.allclose(torch.vmap(f)(ts), loop, atol=1e-12)
    eps = 1e-6
    fd = torch.stack([(f(th + eps) - f(th - eps)) / (2 * eps) for th in ts])
    g = torch.stack([torch.func.grad(f)(th) for th in ts])
    assert torch.allclose(g, fd, atol=1e-7) and g.abs().min().item() > 1e-3
    assert torch.allclose(torch.vmap(torch.func.grad(f))(ts), g, atol=1e-12)
