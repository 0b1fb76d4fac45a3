"""The autograd rules of ops.mux_axpby / mux_cross / mux_rot on the GPU: gradcheck and gradgradcheck in complex128 at a
small n, the first derivatives of ``mux_rot`` in the state and in the angles at kernel-path shapes in both precisions
against the closed forms  gx = rot(gy; -theta),  gtheta[b, s] = Im cross(gx, x)[b, s] / 2  evaluated by the numpy
reference (tests/_muxgrad_ref.py), and the Hessian in the angles at k = 2 against the dense oracle.  The first derivatives of
all three nodes at kernel-path shapes -- reverse and forward mode, ``vmap``, the layouts autograd hands a node, both
precisions, judged bin by bin -- are the family 'muxgrad' of tests/_stream_grad_cases.py (test_stream_autograd_gpu.py).

Kernel-path shapes (csrc/dq_muxgrad.hip): P = 10 + (1 for complex64 with target != 0) pair bits of a unit; n = P + 1 is one
unit, n = P + 3 eight units, with selects and a control on both sides of the unit boundary."""

import numpy as np
import pytest
import torch

from deepquantum_amd import ops
from _mux_ref import random_state
from _muxgrad_ref import dense_mux_rot, mux_rot_grads_ref

pytestmark = pytest.mark.gpu

SMALL = dict(n=4, target=1, bits=(3, 0), controls=(2,))


def cuda(a):
    return torch.from_numpy(np.asarray(a)).cuda()


def coef(shape, seed):
    rng = np.random.default_rng(seed)
    return cuda(rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).requires_grad_()


def state(batch, n, seed):
    return cuda(random_state(batch, n, seed, np.complex128)).requires_grad_()


@pytest.mark.parametrize('axis', ['x', 'y', 'z'])
def test_mux_rot_gradcheck(axis):
    target, bits, controls = SMALL['target'], SMALL['bits'], SMALL['controls']
    f = lambda s, t: ops.mux_rot(s, t, axis, target, bits, controls)  # noqa: E731
    for shape in ((4,), (2, 4)):
        theta = cuda(np.random.default_rng(5).uniform(-3, 3, shape)).requires_grad_()
        x = state(2, SMALL['n'], 1)
        assert torch.autograd.gradcheck(f, (x, theta))
        assert torch.autograd.gradgradcheck(f, (x, theta))


@pytest.mark.parametrize('mode', ['gate', 'map'])
@pytest.mark.parametrize('axis', ['i', 'x', 'y', 'z'])
def test_mux_axpby_gradcheck(axis, mode):
    target, bits, controls = SMALL['target'], SMALL['bits'], SMALL['controls']
    f = lambda s, a, c: ops.mux_axpby(s, a, c, axis, target, bits, controls, mode)  # noqa: E731
    x, a, c = state(2, SMALL['n'], 3), coef((4,), 6), coef((4,), 7)
    assert torch.autograd.gradcheck(f, (x, a, c))
    assert torch.autograd.gradgradcheck(f, (x, a, c))


@pytest.mark.parametrize('axis', ['i', 'x', 'y', 'z'])
def test_mux_cross_gradcheck(axis):
    target, bits, controls = SMALL['target'], SMALL['bits'], SMALL['controls']
    f = lambda u, v: ops.mux_cross(u, v, axis, target, bits, controls)  # noqa: E731
    u, v = state(2, SMALL['n'], 4), state(2, SMALL['n'], 5)
    assert torch.autograd.gradcheck(f, (u, v))
    assert torch.autograd.gradgradcheck(f, (u, v))
    assert torch.autograd.gradcheck(lambda s: f(s, s), (v,))


# (n, target, bits, controls) per precision: one unit, and eight units with selects and a control on both sides of it
PATHS = {
    'c64': [(12, 4, (0, 11, 7, 2), (9,)), (11, 0, (10, 1, 5), (3,)), (14, 4, (13, 0, 12, 11, 6), (2, 10)), (14, 13, (12, 3, 0), (11,))],
    'c128': [(11, 4, (0, 10, 7, 2), (9,)), (13, 4, (12, 0, 11, 10, 6), (2, 9)), (13, 12, (11, 3, 0), (10,))],
}


@pytest.mark.parametrize('dt,tol', [('c64', 1e-4), ('c128', 1e-10)])
@pytest.mark.parametrize('axis', ['x', 'y', 'z'])
def test_mux_rot_first_derivatives_at_kernel_path_shapes(axis, dt, tol):
    dtype = torch.complex64 if dt == 'c64' else torch.complex128
    for j, (n, target, bits, controls) in enumerate(PATHS[dt]):
        batch = 1 + j % 2 * 2
        xr = random_state(batch, n, 10 + j, np.complex64 if dt == 'c64' else np.complex128)
        gr = random_state(batch, n, 20 + j, np.complex64 if dt == 'c64' else np.complex128)
        th = np.random.default_rng(30 + j).uniform(-6, 6, 1 << len(bits))
        x = cuda(xr).to(dtype).requires_grad_()
        theta = cuda(th).requires_grad_()
        y = ops.mux_rot(x, theta, axis, target, bits, controls)
        gx, gt = torch.autograd.grad(y, (x, theta), cuda(gr).to(dtype))
        wx, wt = mux_rot_grads_ref(xr, th, gr, axis, target, bits, controls)
        wt = wt.sum(0)                                  # (shared angles: the sum over the batch)
        ex = np.abs(gx.cpu().numpy() - wx).max() / np.abs(wx).max()
        et = np.abs(gt.cpu().numpy() - wt).max() / np.abs(wt).max()
        print(f'mux_rot {axis} {dt} n={n} target={target}: state {ex:.2e} angles {et:.2e} (tol {tol})')
        assert gx.dtype == dtype and gt.dtype == torch.float64 and ex <= tol and et <= tol, (n, target, bits, controls, ex, et)
        # per-sample angles: the rows of the cross itself
        if batch > 1:
            thb = np.random.default_rng(40 + j).uniform(-6, 6, (batch, 1 << len(bits)))
            thetab = cuda(thb).requires_grad_()
            (gtb,) = torch.autograd.grad(ops.mux_rot(x, thetab, axis, target, bits, controls), thetab, cuda(gr).to(dtype))
            _, wtb = mux_rot_grads_ref(xr, thb, gr, axis, target, bits, controls)
            assert np.abs(gtb.cpu().numpy() - wtb).max() <= tol * np.abs(wtb).max()


@pytest.mark.parametrize('axis', ['x', 'y', 'z'])
def test_hessian_in_the_angles_against_the_dense_oracle(axis):
    n, target, bits, controls = 5, 2, (4, 0), (3,)
    x = cuda(random_state(1, n, 3, np.complex128))
    x = x / x.norm()
    w = torch.arange(1 << n, dtype=torch.float64)
    v = torch.from_numpy(random_state(1, n, 4, np.complex128)).reshape(-1)        # (a phase-sensitive term: Rz moves no modulus)
    theta = torch.from_numpy(np.random.default_rng(8).uniform(-3, 3, 4))

    def loss(t):
        y = ops.mux_rot(x, t, axis, target, bits, controls).reshape(-1)
        return ((y.abs() ** 2) * w.cuda()).sum() + (v.cuda().conj() * y).sum().real

    def oracle(t):
        y = dense_mux_rot(t, axis, n, target, bits, controls) @ x.cpu().reshape(-1)
        return ((y.abs() ** 2) * w).sum() + (v.conj() * y).sum().real

    got = torch.autograd.functional.hessian(loss, theta.cuda()).cpu()
    want = torch.autograd.functional.hessian(oracle, theta)
    assert got.shape == (4, 4) and want.abs().max() > 1e-3
    assert (got - want).abs().max() <= 1e-10 * want.abs().max()
    g1 = torch.autograd.functional.jacobian(loss, theta.cuda()).cpu()
    g2 = torch.autograd.functional.jacobian(oracle, theta)
    assert (g1 - g2).abs().max() <= 1e-10 * g2.abs().max()
