"""Autograd through the excitation kernels on the MI355X, complex128, n = 4 and 5, batch 2: the excitation side of the
generator nodes that Pauli strings and excitations share (``ops._GenAxpby / _GenCross / _GenRot`` with s = -1, r = 1 and
the two-kernel inner product ``ops._excite_inner``) -- the twin of test_pauli_autograd_gpu.py at node level."""

import pytest
import torch

from deepquantum_amd import backend, ops

pytestmark = pytest.mark.gpu

gradcheck, gradgradcheck = torch.autograd.gradcheck, torch.autograd.gradgradcheck
FORWARD = dict(check_forward_ad=True, check_backward_ad=False)


def state(batch, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, 1 << n, dtype=torch.complex128, generator=g).cuda()


def specs(n):
    """Pairs on index bits n - 1 and 0 with a string bit (1), negate = 1 and a control on bit 2; the same without the
    control; a weight-1 excitation on bit 0 (the pair is two neighbouring amplitudes) with a string bit."""
    x = 1 << (n - 1) | 1
    return {'controlled': (x, 1 << (n - 1), 0b10, 1, (2,)), 'free': (x, 1 << (n - 1), 0b10, 1), 'bit0': (1, 0, 0b100, 0)}


def coefs():
    a = torch.tensor([0.3 - 0.2j, 1.1j], dtype=torch.complex128, device='cuda', requires_grad=True)
    c = torch.tensor([-0.6 + 0.1j, 0.4], dtype=torch.complex128, device='cuda', requires_grad=True)
    return a, c


@pytest.mark.parametrize('mode', ['gate', 'map'])
@pytest.mark.parametrize('which', ['controlled', 'bit0'])
@pytest.mark.parametrize('n', [4, 5])
def test_excite_axpby_gradcheck(n, which, mode):
    spec = specs(n)[which]
    x = state(2, n, 1).requires_grad_()
    a, c = coefs()
    f = lambda s, p, q: ops.excite_axpby(s, spec, p, q, mode)  # noqa: E731
    assert gradcheck(f, (x, a, c))
    assert gradgradcheck(f, (x, a, c))
    assert gradcheck(f, (x, a, c), **FORWARD)


@pytest.mark.parametrize('which', ['controlled', 'free', 'bit0'])
@pytest.mark.parametrize('n', [4, 5])
def test_excite_cross_gradcheck(n, which):
    spec = specs(n)[which]
    x, y = state(2, n, 2).requires_grad_(), state(2, n, 3).requires_grad_()
    f = lambda u, v: ops.excite_cross(u, v, spec)  # noqa: E731
    assert gradcheck(f, (x, y))
    assert gradgradcheck(f, (x, y))
    assert gradcheck(lambda u: ops.excite_cross(u, u, spec), (x,))                        # bra is ket: each pair read once
    assert gradcheck(f, (x, y), **FORWARD)


@pytest.mark.parametrize('which', ['controlled', 'bit0'])
@pytest.mark.parametrize('n', [4, 5])
def test_excite_rot_gradcheck_with_a_per_sample_and_a_shared_angle(n, which):
    spec = specs(n)[which]
    x = state(2, n, 4).requires_grad_()
    th = torch.tensor([0.3, -3.8], dtype=torch.float64, device='cuda', requires_grad=True)
    one = torch.tensor(0.45, dtype=torch.float64, device='cuda', requires_grad=True)
    f = lambda s, p: ops.excite_rot(s, spec, p)  # noqa: E731
    assert gradcheck(f, (x, th))
    assert gradgradcheck(f, (x, th))
    assert gradcheck(f, (x, one))                                           # a shared angle: the sum of the samples' gradients
    assert gradcheck(f, (x, th), **FORWARD)
    assert gradcheck(f, (x, one), **FORWARD)


@pytest.mark.parametrize('n', [4, 5])
def test_the_backward_of_the_rotation_is_the_rotation_back_exactly(n):
    x = state(2, n, 5).requires_grad_()
    gy = state(2, n, 6)
    th = torch.tensor([0.3, -3.8], dtype=torch.float64, device='cuda')
    for spec in specs(n).values():
        (gx,) = torch.autograd.grad(ops.excite_rot(x, spec, th), x, gy)
        assert torch.equal(gx, backend.apply_excite_rot(gy, spec, -th))
