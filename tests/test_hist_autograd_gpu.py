"""Autograd through the histogram kernels on the MI355X: ops.cost_hist and ops.apply_binned differentiate into one another
(complex128 gradcheck / gradgradcheck at n = 6 .. 8, with a control and a gathered table as in
test_diag_autograd_gpu.py), and one complex64 first-order case against the complex128 gradient."""

import pytest
import torch

from deepquantum_amd import backend, ops

pytestmark = pytest.mark.gpu

NBINS = 5


def state(batch, n, seed, dtype=torch.complex128):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, 1 << n, dtype=torch.complex128, generator=g).to(dtype).cuda()


def bins(k, like, seed):
    return backend.bin_table(torch.randint(0, NBINS, (1 << k,), generator=torch.Generator().manual_seed(seed)), like, NBINS)


@pytest.mark.parametrize('n', [6, 7, 8])
def test_cost_hist_gradcheck(n):
    bits, controls = (0, n - 1, 3), (2,)
    x, y = state(2, n, 2).requires_grad_(), state(2, n, 3).requires_grad_()
    tab = bins(3, x, n)
    f = lambda a, b: ops.cost_hist(a, b, tab, NBINS, bits, controls)  # noqa: E731
    assert torch.autograd.gradcheck(f, (x, y))
    assert torch.autograd.gradgradcheck(f, (x, y))
    full = tuple(range(n - 1, -1, -1))
    tn = bins(n, x, n + 1)
    assert torch.autograd.gradcheck(lambda a: ops.cost_hist(a, a, tn, NBINS, full).real, (x,))


@pytest.mark.parametrize('n', [6, 7, 8])
def test_apply_binned_gradcheck(n):
    bits, controls = (0, n - 1, 3), (2,)
    x = state(2, n, 4).requires_grad_()
    g = torch.randn(2, NBINS, dtype=torch.complex128, generator=torch.Generator().manual_seed(n)).cuda().requires_grad_()
    tab = bins(3, x, n)
    f = lambda a, b: ops.apply_binned(a, b, tab, bits, controls)  # noqa: E731
    assert torch.autograd.gradcheck(f, (x, g))
    assert torch.autograd.gradgradcheck(f, (x, g))


def test_complex64_gradient_against_complex128():
    n, bits, controls = 12, (11, 0, 5, 3), (7,)
    x128 = state(2, n, 9, torch.complex64).to(torch.complex128)
    tab = bins(4, x128, 1)
    w = torch.randn(2, NBINS, dtype=torch.float64, generator=torch.Generator().manual_seed(2)).cuda()
    grads = []
    for x in (x128.to(torch.complex64), x128):
        x = x.clone().requires_grad_()
        (ops.cost_hist(x, x, tab, NBINS, bits, controls).real * w).sum().backward()
        grads.append(x.grad.to(torch.complex128))
    assert (grads[0] - grads[1]).abs().max() <= 1e-4 * grads[1].abs().max() and grads[1].abs().max() > 0

