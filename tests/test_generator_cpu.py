"""The autograd contract of the generator nodes (``ops._GenAxpby / _GenCross / _GenRot``) without a GPU, asserted alike for
the two families that share them -- Pauli strings and excitations -- through the plain-torch complex128 stand-ins of
``backend`` under the CPU test double."""

import pytest
import torch

from deepquantum_amd import backend, ops


def rand_state(batch, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, 1 << n, dtype=torch.complex128, generator=g)


class Pauli:
    """Z Y . X on index bits 3 2 . 0 with a control on bit 1; ``free``: the same string without the control; ``shared``
    (the spec that takes one angle for all samples): YY."""
    spec, free, shared = (0b0101, 0b1100, (1,)), (0b0101, 0b1100, ()), (0b0011, 0b0011, ())
    axpby = staticmethod(lambda s, spec, a, c, mode='gate': ops.pauli_axpby(s, spec[0], spec[1], a, c, spec[2], mode))
    cross = staticmethod(lambda u, v, spec: ops.pauli_cross(u, v, *spec))
    rot = staticmethod(lambda s, spec, th: ops.pauli_rot(s, spec[0], spec[1], th, spec[2]))
    backend_rot = staticmethod(lambda s, spec, th: backend.apply_pauli_rot(s, spec[0], spec[1], th, spec[2]))
    backend_cross = staticmethod(lambda u, v, spec: backend.pauli_cross(u, v, *spec))


class Excite:
    """Pairs on index bits 2 and 0 with a string bit (1), a sign and a control on bit 3; ``free`` and ``shared``: the same
    without the control."""
    spec = (0b0101, 0b0100, 0b0010, 1, (3,))
    free = shared = spec[:4]
    axpby = staticmethod(lambda s, spec, a, c, mode='gate': ops.excite_axpby(s, spec, a, c, mode))
    cross = staticmethod(lambda u, v, spec: ops.excite_cross(u, v, spec))
    rot = staticmethod(lambda s, spec, th: ops.excite_rot(s, spec, th))
    backend_rot = staticmethod(lambda s, spec, th: backend.apply_excite_rot(s, spec, th))
    backend_cross = staticmethod(lambda u, v, spec: backend.excite_cross(u, v, spec))


@pytest.mark.parametrize('fam', [Pauli, Excite], ids=['pauli', 'excite'])
def test_autograd_closure_through_the_stand_ins(cpu_backend, fam):
    """gradcheck / gradgradcheck / forward AD at n = 4, complex128, batch 2 of the operations that differentiate into one
    another, with a control, a Y or a string bit, a per-sample angle and a shared one; the backward of the rotation is
    the rotation back, exactly; vmap folds into the batch of the backend call, exactly; torch.func.grad goes through."""
    n, spec = 4, fam.spec
    x = rand_state(2, n, 1).requires_grad_()
    y = rand_state(2, n, 2).requires_grad_()
    a = torch.tensor([0.3 - 0.2j, 1.1j], dtype=torch.complex128, requires_grad=True)
    c = torch.tensor([-0.6 + 0.1j, 0.4], dtype=torch.complex128, requires_grad=True)
    th = torch.tensor([0.3, -3.8], dtype=torch.float64, requires_grad=True)
    one = torch.tensor(0.45, dtype=torch.float64, requires_grad=True)
    gc, ggc = torch.autograd.gradcheck, torch.autograd.gradgradcheck
    forward = dict(check_forward_ad=True, check_backward_ad=False)
    for mode in ('gate', 'map'):
        f = lambda s, p, q: fam.axpby(s, spec, p, q, mode)  # noqa: E731
        assert gc(f, (x, a, c))
        assert ggc(f, (x, a, c))
    assert gc(lambda u, v: fam.cross(u, v, spec), (x, y))
    assert ggc(lambda u, v: fam.cross(u, v, spec), (x, y))
    assert gc(lambda u: fam.cross(u, u, spec), (x,))                           # the same tensor in both slots
    assert gc(lambda u: fam.cross(u, u, fam.free), (x,))
    assert gc(lambda s, p: fam.rot(s, spec, p), (x, th))
    assert ggc(lambda s, p: fam.rot(s, spec, p), (x, th))
    assert gc(lambda s, p: fam.rot(s, fam.shared, p), (x, one))                # a shared angle: the sum of the samples' gradients
    assert gc(lambda s, p: fam.rot(s, spec, p), (x, th), **forward)
    assert gc(lambda s, p, q: fam.axpby(s, spec, p, q), (x, a, c), **forward)
    assert gc(lambda u, v: fam.cross(u, v, spec), (x, y), **forward)
    # the backward of the rotation is the rotation back, exactly, and vmap folds into the batch
    gy = rand_state(2, n, 3)
    (gx,) = torch.autograd.grad(fam.rot(x, spec, th.detach()), x, gy)
    assert torch.equal(gx, fam.backend_rot(gy, spec, -th.detach()))
    xs = rand_state(6, n, 4).reshape(3, 2, -1)
    ths = torch.linspace(-1, 1, 6, dtype=torch.float64).reshape(3, 2)
    want = fam.backend_rot(xs.reshape(6, -1), spec, ths.reshape(-1))
    assert torch.equal(torch.vmap(lambda s, p: fam.rot(s, spec, p))(xs, ths).reshape(6, -1), want)
    want = fam.backend_cross(xs.reshape(6, -1), xs.flip(0).reshape(6, -1).contiguous(), spec)
    got = torch.vmap(lambda u, v: fam.cross(u, v, spec))(xs, xs.flip(0))
    assert torch.equal(got.reshape(-1), want)
    g = torch.func.grad(lambda p: fam.rot(x.detach(), spec, p)[:, 3].abs().pow(2).sum())(th.detach())
    assert g.shape == (2,) and torch.isfinite(g).all()
