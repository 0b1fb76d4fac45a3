"""The derivatives of ``ops.gram`` and ``ops.combine`` on the MI355X at kernel-path shapes: the smallest n at which a Gram
launch has more than one workgroup per tile pair (one column past a unit of ``backend.gram_geometry``: n = 9 in complex128)
and row counts that straddle the edge of a block of 16 (3 x 17: one block against two, a partial second block).

``gradcheck`` / ``gradgradcheck`` in complex128 run with ``fast_mode`` there (random projections instead of the whole
Jacobian of 20 x 512 complex inputs) and in full at n = 2; complex64 first derivatives are held to the complex128 ones at
1e-4 of their largest entry; the fidelity kernel of a small circuit is differentiated in its parameters and its data against
finite differences."""

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import backend, ops
import _gram_ref as ref

pytestmark = pytest.mark.gpu

DEVICE = 'cuda'
ROWS_A, ROWS_B = 3, 17


def kernel_n():
    return ref.log2(backend.gram_geometry(torch.complex128).unit_cols) + 1


def dev(a, grad=True):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEVICE).requires_grad_(grad)


def inputs(n, dt='c128', seed=0):
    rng = np.random.default_rng([n, seed])
    a, b = ref.gaussian_rows(rng, ROWS_A, n, dt), ref.gaussian_rows(rng, ROWS_B, n, dt)
    coef = ref.gaussian_coefs(rng, ROWS_A, ROWS_B)
    return a, b, coef


@pytest.mark.parametrize('small', [True, False], ids=['n2-full', 'kernel-path-fast'])
def test_gradcheck_and_gradgradcheck_of_gram(small):
    n = 2 if small else kernel_n()
    a, b, _ = inputs(n)
    a, b = dev(a), dev(b)
    kw = dict(nondet_tol=0, fast_mode=not small)
    assert torch.autograd.gradcheck(ops.gram, (a, b), **kw)
    assert torch.autograd.gradgradcheck(ops.gram, (a, b), **kw)
    assert torch.autograd.gradcheck(ops.gram, (a, b), check_forward_ad=True, check_backward_ad=False, **kw)
    assert torch.autograd.gradcheck(lambda x: ops.gram(x, x), (b,), **kw)
    assert torch.autograd.gradgradcheck(lambda x: ops.gram(x, x), (b,), **kw)


@pytest.mark.parametrize('small', [True, False], ids=['n2-full', 'kernel-path-fast'])
def test_gradcheck_and_gradgradcheck_of_combine(small):
    n = 2 if small else kernel_n()
    _, b, coef = inputs(n)
    s, c = dev(b), dev(coef)
    kw = dict(nondet_tol=0, fast_mode=not small)
    assert torch.autograd.gradcheck(ops.combine, (s, c), **kw)
    assert torch.autograd.gradgradcheck(ops.combine, (s, c), **kw)
    assert torch.autograd.gradcheck(ops.combine, (s, c), check_forward_ad=True, check_backward_ad=False, **kw)


def test_first_derivatives_in_complex64_against_complex128():
    n = kernel_n() + 1                                   # (one column past a unit of complex64 vectors as well)
    a, b, coef = inputs(n, 'c64', seed=1)
    rng = np.random.default_rng(7)
    gbar, ybar = ref.gaussian_coefs(rng, ROWS_A, ROWS_B), ref.gaussian_rows(rng, ROWS_A, n, 'c64')
    got, want = [], []
    for cast, out in ((np.complex64, got), (np.complex128, want)):
        da, db, dc = dev(a.astype(cast)), dev(b.astype(cast)), dev(coef)
        out += torch.autograd.grad(ops.gram(da, db), (da, db), dev(gbar, False))
        out += torch.autograd.grad(ops.combine(db, dc), (db, dc), dev(ybar.astype(cast), False))
        out += torch.autograd.grad(ops.gram(db, db), (db,), dev(ref.gaussian_coefs(np.random.default_rng(8), ROWS_B, ROWS_B), False))
    # and the complex128 ones against the formulas
    np.testing.assert_allclose(want[0].cpu().numpy(), gbar.conj() @ b.astype(np.complex128), rtol=0, atol=1e-10)
    np.testing.assert_allclose(want[1].cpu().numpy(), gbar.T @ a.astype(np.complex128), rtol=0, atol=1e-10)
    np.testing.assert_allclose(want[2].cpu().numpy(), coef.conj().T @ ybar.astype(np.complex128), rtol=0, atol=1e-10)
    np.testing.assert_allclose(want[3].cpu().numpy(), ref.gram_ref(b, ybar).T, rtol=0, atol=1e-9)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == (torch.complex64 if g.shape[-1] == 1 << n else torch.complex128)
        err = (g.to(torch.complex128) - w).abs().max().item()
        assert err <= ref.TOL['c64'] * w.abs().max().item(), (err, w.abs().max().item())


def encoder_circuit(n):
    cir = dq.QubitCircuit(n)
    cir.rxlayer(encode=True)
    cir.cnot_ring()
    cir.rylayer()
    cir.rzlayer(encode=True)
    cir.cnot_ring()
    cir.to(torch.double)
    return cir.to(DEVICE)


def test_kernel_matrix_gradient_through_a_circuit():
    torch.manual_seed(5)
    n = 4
    cir = encoder_circuit(n)
    x1 = torch.randn(5, 2 * n, dtype=torch.float64, device=DEVICE)
    x2 = torch.randn(3, 2 * n, dtype=torch.float64, device=DEVICE, requires_grad=True)
    weight = torch.randn(5, 3, dtype=torch.float64, device=DEVICE)
    params = [p for p in cir.parameters() if p.requires_grad]
    assert params

    def loss():
        return (weight * cir.kernel_matrix(x1, x2)).sum()

    k = cir.kernel_matrix(x1)
    assert k.dtype == torch.float64 and torch.equal(k, k.T) and (k.diagonal() - 1).abs().max() < 1e-12
    with torch.no_grad():
        s1 = cir(x1).reshape(5, -1).clone()
        want = torch.stack([backend.inner(s1[i:i + 1].expand(5, -1).contiguous(), s1).abs() ** 2 for i in range(5)])
    assert (k.detach() - want).abs().max() < 1e-12
    grads = torch.autograd.grad(loss(), params + [x2])
    eps = 1e-6
    for p, g in zip(params + [x2], grads):
        flat = p.data.view(-1)
        for i in range(0, p.numel(), max(1, p.numel() // 4)):               # (a handful of entries of each)
            old = flat[i].item()
            flat[i] = old + eps
            up = loss().item()
            flat[i] = old - eps
            fd = (up - loss().item()) / (2 * eps)
            flat[i] = old
            assert abs(g.reshape(-1)[i].item() - fd) < 1e-7, (i, g.reshape(-1)[i].item(), fd)
