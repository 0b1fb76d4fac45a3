"""The autograd rules of ``ops.mux_apply`` on the GPU (n = 6, complex128): every rule is the differentiable function itself
-- the backward with ``dagger`` toggled, the jvp and the vmap rule with it as it is -- so derivatives of any order in the
state exist; the backward is compared with the kernel's own dagger map bit for bit and with the reference to 1e-10."""

import numpy as np
import pytest
import torch

from deepquantum_amd import backend, ops
from _mux_ref import mux_ref, random_cs, random_state, random_unitaries, ry_blocks

pytestmark = pytest.mark.gpu

N, TARGET, BITS, CONTROLS = 6, 2, (4, 0, 5), (3,)
KINDS = [pytest.param('u', False, id='u'), pytest.param('u', True, id='u-dagger'), pytest.param('ry', False, id='ry'),
         pytest.param('ry', True, id='ry-dagger')]


@pytest.fixture(scope='module')
def tables():
    u, cs = random_unitaries(len(BITS), 17), random_cs(len(BITS), 18)
    return {'u': (u, torch.from_numpy(u).cuda()), 'ry': (ry_blocks(cs), torch.from_numpy(cs).cuda())}


def f_of(table, kind, dagger):
    return lambda s: ops.mux_apply(s, table, kind, TARGET, BITS, CONTROLS, dagger=dagger)


def close(got, want):
    return np.abs(got.cpu().numpy() - want).max() <= 1e-10 * np.abs(want).max()


@pytest.mark.parametrize('kind,dagger', KINDS)
def test_gradcheck_and_gradgradcheck(tables, kind, dagger):
    f = f_of(tables[kind][1], kind, dagger)
    s = torch.from_numpy(random_state(2, N, 1, np.complex128)).cuda().requires_grad_()
    assert torch.autograd.gradcheck(f, (s,))
    assert torch.autograd.gradgradcheck(f, (s,))
    assert torch.autograd.gradcheck(f, (s,), check_forward_ad=True, check_backward_ad=False)


@pytest.mark.parametrize('kind,dagger', KINDS)
def test_backward_is_the_dagger_map_exactly(tables, kind, dagger):
    blocks, table = tables[kind]
    x, gy = random_state(2, N, 1, np.complex128), random_state(2, N, 2, np.complex128)
    s = torch.from_numpy(x).cuda().requires_grad_()
    y = f_of(table, kind, dagger)(s)
    assert close(y.detach(), mux_ref(x, blocks, TARGET, BITS, CONTROLS, dagger))
    gyd = torch.from_numpy(gy).cuda()
    (gx,) = torch.autograd.grad(y, s, gyd)
    assert torch.equal(gx, backend.apply_mux(gyd, table, kind, TARGET, BITS, CONTROLS, dagger=not dagger))
    assert close(gx, mux_ref(gy, blocks, TARGET, BITS, CONTROLS, not dagger))


@pytest.mark.parametrize('kind,dagger', KINDS)
def test_jvp_is_the_same_map_of_the_tangent(tables, kind, dagger):
    blocks, table = tables[kind]
    x, t = random_state(2, N, 1, np.complex128), random_state(2, N, 3, np.complex128)
    y, yt = torch.func.jvp(f_of(table, kind, dagger), (torch.from_numpy(x).cuda(),), (torch.from_numpy(t).cuda(),))
    assert close(y, mux_ref(x, blocks, TARGET, BITS, CONTROLS, dagger))
    assert close(yt, mux_ref(t, blocks, TARGET, BITS, CONTROLS, dagger))
    assert torch.equal(yt, backend.apply_mux(torch.from_numpy(t).cuda(), table, kind, TARGET, BITS, CONTROLS, dagger=dagger))


@pytest.mark.parametrize('kind,dagger', KINDS)
def test_vmap_over_a_batch_of_states(tables, kind, dagger):
    blocks, table = tables[kind]
    f = f_of(table, kind, dagger)
    xs = random_state(6, N, 4, np.complex128)
    want = mux_ref(xs, blocks, TARGET, BITS, CONTROLS, dagger)
    dev = torch.from_numpy(xs).cuda().reshape(3, 2, -1)
    got = torch.vmap(f)(dev)
    assert got.shape == (3, 2, 1 << N) and close(got.reshape(6, -1), want)
    got = torch.vmap(f, in_dims=1, out_dims=1)(dev.transpose(0, 1).contiguous())
    assert close(got.transpose(0, 1).contiguous().reshape(6, -1), want)
    # per-sample gradients through the vmapped rule: the gradient of Re <w, M x> is M^+ w for every sample
    w = random_state(2, N, 5, np.complex128)
    wd = torch.from_numpy(w).cuda()
    g = torch.vmap(torch.func.grad(lambda s: (wd.conj() * f(s)).sum().real))(dev)
    want_g = mux_ref(w, blocks, TARGET, BITS, CONTROLS, not dagger)
    for b in range(3):
        assert close(g[b], want_g)
