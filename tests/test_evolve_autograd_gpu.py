"""Derivatives of ``ops.psum_evolve`` on the MI355X at kernel-path shapes: n = 13 (complex64) / 12 (complex128), a
Hamiltonian with flips at bit 0 and at the unit boundary, ``f(x, t) = |<phi|exp(-i t H)|x>|^2`` for unit states.  The
reference is the same function through the complex128 host route of ``backend`` (CPU tensors under the test double) at
tol = 1e-12.  Bounds: 1e-10 (complex128) / 1e-4 (complex64) of the largest component of the reference, and never more than
that in absolute terms."""

import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import ops
from _psum_ref import hamiltonian_of

pytestmark = pytest.mark.gpu

DTYPES = {'c64': torch.complex64, 'c128': torch.complex128}
BOUND = {'c64': 1e-4, 'c128': 1e-10}


def case(dt):
    n = {'c64': 13, 'c128': 12}[dt]
    ub = {'c64': 11, 'c128': 10}[dt]                    # the first bit above a unit of 1024 vectors
    terms = [(0.2, 0, 0), (0.3, 0, 1 << (n - 1)), (0.7, 1, 0), (-0.4, 1, 1 | 1 << 5), (0.5, 1 << ub, 1 << 3),
             (0.6, 1 << ub | 1, 1 << ub), (-0.35, 1 << (ub - 1), 1 << ub)]
    H = dq.PauliSum(hamiltonian_of(n, terms), n)
    g = torch.Generator().manual_seed(21)
    x, phi = (torch.randn(2, 1 << n, dtype=torch.complex128, generator=g) for _ in range(2))
    x, phi = (v / v.norm(dim=-1, keepdim=True) for v in (x, phi))
    # (overlapping states, so that f and its derivatives are of order 1, not 2^-n)
    phi = (phi + 2 * x) / (phi + 2 * x).norm(dim=-1, keepdim=True)
    t = torch.tensor([0.8, -1.3], dtype=torch.float64)
    return n, H, x.to(DTYPES[dt]), phi.to(DTYPES[dt]), t


def derivatives(H, x, phi, t, tol):
    """f, df/dx, df/dt and d2f/dt2, each sample's own."""
    x = x.clone().requires_grad_()
    t = t.clone().requires_grad_()
    y = ops.psum_evolve(x, t, H, tol)
    amp = (phi.conj() * y).sum(-1)
    f = amp.real ** 2 + amp.imag ** 2
    gx, gt = torch.autograd.grad(f.sum(), (x, t), create_graph=True)
    (gtt,) = torch.autograd.grad(gt.sum(), t)
    return [v.detach().cpu() for v in (f, gx, gt, gtt)]


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_first_and_second_derivatives_against_the_host_route(dt, cpu_backend):
    n, H, x, phi, t = case(dt)
    want = derivatives(H, x.to(torch.complex128), phi.to(torch.complex128), t, 1e-12)
    got = derivatives(H, x.cuda(), phi.cuda(), t.cuda(), None)
    assert got[1].dtype == DTYPES[dt] and got[2].dtype == torch.float64
    for name, g, w in zip(('f', 'gx', 'gt', 'd2f/dt2'), got, want):
        scale = min(1.0, w.abs().max().item())
        err = (g.to(w.dtype) - w).abs().max().item()
        print(f'{name} n={n} {dt}: err {err:.3e}, largest component {w.abs().max().item():.3e}, err / (bound * scale) = '
              f'{err / (BOUND[dt] * scale):.3e}')
        assert w.abs().max().item() > 1e-3                # (something to compare)
        assert err <= BOUND[dt] * scale, name
