"""The autograd rules of ``ops.permute_basis`` on the GPU (n = 6, complex128): every rule is the differentiable function
itself -- the backward with the two tables swapped, the jvp and the vmap rule with them as they are -- so derivatives of
any order exist; the operator moves amplitudes without arithmetic, so its backward and its jvp are exact."""

import numpy as np
import pytest
import torch

from deepquantum_amd import ops
from _perm_ref import inverse_of, permute_ref, random_bijection, random_state, same_bits

pytestmark = pytest.mark.gpu

N, BITS, CONTROLS = 6, (4, 0, 2), (3,)


@pytest.fixture(scope='module')
def setup():
    perm = random_bijection(len(BITS), 17)
    x = random_state(2, N, 1, np.complex128)
    return perm, torch.from_numpy(perm).cuda(), x


def f_of(perm_dev):
    return lambda s: ops.permute_basis(s, perm_dev, BITS, CONTROLS)


def test_gradcheck_and_gradgradcheck(setup):
    perm, perm_dev, x = setup
    s = torch.from_numpy(x).cuda().requires_grad_()
    assert torch.autograd.gradcheck(f_of(perm_dev), (s,))
    assert torch.autograd.gradgradcheck(f_of(perm_dev), (s,))
    assert torch.autograd.gradcheck(f_of(perm_dev), (s,), check_forward_ad=True, check_backward_ad=False)


def test_backward_is_the_permutation_by_the_inverse_table(setup):
    perm, perm_dev, x = setup
    s = torch.from_numpy(x).cuda().requires_grad_()
    gy = random_state(2, N, 2, np.complex128)
    y = f_of(perm_dev)(s)
    assert same_bits(y.detach().cpu().numpy(), permute_ref(x, perm, BITS, CONTROLS))
    (gx,) = torch.autograd.grad(y, s, torch.from_numpy(gy).cuda())
    want = permute_ref(gy, inverse_of(perm), BITS, CONTROLS)
    np.testing.assert_array_equal(gx.cpu().numpy(), want)
    assert same_bits(gx.cpu().numpy(), want)


def test_jvp_is_the_same_permutation_of_the_tangent(setup):
    perm, perm_dev, x = setup
    t = random_state(2, N, 3, np.complex128)
    y, yt = torch.func.jvp(f_of(perm_dev), (torch.from_numpy(x).cuda(),), (torch.from_numpy(t).cuda(),))
    assert same_bits(y.cpu().numpy(), permute_ref(x, perm, BITS, CONTROLS))
    assert same_bits(yt.cpu().numpy(), permute_ref(t, perm, BITS, CONTROLS))


def test_vmap_over_a_batch_of_states(setup):
    perm, perm_dev, _ = setup
    xs = random_state(6, N, 4, np.complex128)
    want = permute_ref(xs, perm, BITS, CONTROLS)
    dev = torch.from_numpy(xs).cuda().reshape(3, 2, -1)
    got = torch.vmap(f_of(perm_dev))(dev)
    assert got.shape == (3, 2, 1 << N) and same_bits(got.cpu().numpy().reshape(6, -1), want)
    got = torch.vmap(f_of(perm_dev), in_dims=1, out_dims=1)(dev.transpose(0, 1).contiguous())
    assert same_bits(got.transpose(0, 1).contiguous().cpu().numpy().reshape(6, -1), want)
    # per-sample gradients through the vmapped rule: the gradient of Re <w, P x> is P^T w for every sample
    w = torch.from_numpy(random_state(2, N, 5, np.complex128)).cuda()
    g = torch.vmap(torch.func.grad(lambda s: (w.conj() * f_of(perm_dev)(s)).sum().real))(dev)
    want_g = permute_ref(w.cpu().numpy(), inverse_of(perm), BITS, CONTROLS)
    for b in range(3):
        np.testing.assert_array_equal(g[b].cpu().numpy(), want_g)
