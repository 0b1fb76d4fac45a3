"""The autograd rules of ``ops.select_pauli`` on the GPU: every rule is the differentiable function itself -- the backward
with the two tables swapped, the jvp and the vmap rule with them as they are -- so derivatives of any order exist; the
operator gathers amplitudes and multiplies them by powers of i exactly, so its backward and its jvp are exact.
``gradcheck`` / ``gradgradcheck`` run in full at n = 4 and with ``fast_mode`` (random projections instead of the whole
Jacobian, which would be some twenty thousand launches) at n = u + 1, where the select bits straddle the unit."""

import numpy as np
import pytest
import torch

from deepquantum_amd import backend, ops
from _select_ref import random_entries, random_state, select_ref, words

pytestmark = pytest.mark.gpu


def case(n, bits, controls, seed):
    free = [p for p in range(n) if p not in bits and p not in controls]
    entries = random_entries(np.random.default_rng(seed), (1 << len(bits)) - 1, free)
    return backend.SelectTable(n, entries + [(0, 0, 0)]), words(entries, k=len(bits)), words(entries, dagger=True, k=len(bits))


def unit_bits(dtype):
    return backend.select_pauli_unit_bits(dtype)


@pytest.mark.parametrize('small', [True, False], ids=['n4', 'n_u_plus_1'])
def test_gradcheck_and_gradgradcheck(small):
    u = unit_bits(torch.complex128)
    n, bits, controls = (4, (2, 0), (3,)) if small else (u + 1, (u, u - 1, 0), (4,))
    table, _, _ = case(n, bits, controls, 1)
    f = lambda s: ops.select_pauli(s, table, bits, controls)
    s = torch.from_numpy(random_state(np.random.default_rng(2), 2 if small else 1, n, np.complex128)).cuda().requires_grad_()
    assert torch.autograd.gradcheck(f, (s,), nondet_tol=0, fast_mode=not small)
    assert torch.autograd.gradgradcheck(f, (s,), nondet_tol=0, fast_mode=not small)
    assert torch.autograd.gradcheck(f, (s,), nondet_tol=0, fast_mode=not small, check_forward_ad=True, check_backward_ad=False)


@pytest.mark.parametrize('dtype', [np.complex64, np.complex128], ids=['c64', 'c128'])
def test_cotangent_is_the_adjoint_table_applied_to_the_upstream_gradient(dtype):
    u = unit_bits(torch.complex128 if dtype == np.complex128 else torch.complex64)
    n, bits, controls = u + 1, (u, 3, 0), (5,)
    table, forward, dagger = case(n, bits, controls, 3)
    x, gy = random_state(np.random.default_rng(4), 2, n, dtype), random_state(np.random.default_rng(5), 2, n, dtype)
    s = torch.from_numpy(x).cuda().requires_grad_()
    y = ops.select_pauli(s, table, bits, controls)
    np.testing.assert_array_equal(y.detach().cpu().numpy(), select_ref(x, forward, bits, controls))
    (gx,) = torch.autograd.grad(y, s, torch.from_numpy(gy).cuda())
    np.testing.assert_array_equal(gx.cpu().numpy(), select_ref(gy, dagger, bits, controls))
    # dagger=True swaps the roles
    y = ops.select_pauli(s, table, bits, controls, dagger=True)
    np.testing.assert_array_equal(y.detach().cpu().numpy(), select_ref(x, dagger, bits, controls))
    (gx,) = torch.autograd.grad(y, s, torch.from_numpy(gy).cuda())
    np.testing.assert_array_equal(gx.cpu().numpy(), select_ref(gy, forward, bits, controls))


def test_jvp_and_vmap_go_through_the_node():
    n, bits, controls = 6, (4, 0), (3,)
    table, forward, dagger = case(n, bits, controls, 6)
    f = lambda s: ops.select_pauli(s, table, bits, controls)
    x, t = random_state(np.random.default_rng(7), 2, n, np.complex128), random_state(np.random.default_rng(8), 2, n, np.complex128)
    y, yt = torch.func.jvp(f, (torch.from_numpy(x).cuda(),), (torch.from_numpy(t).cuda(),))
    np.testing.assert_array_equal(y.cpu().numpy(), select_ref(x, forward, bits, controls))
    np.testing.assert_array_equal(yt.cpu().numpy(), select_ref(t, forward, bits, controls))
    xs = random_state(np.random.default_rng(9), 6, n, np.complex128)
    dev = torch.from_numpy(xs).cuda().reshape(3, 2, -1)
    got = torch.vmap(f)(dev)
    assert got.shape == (3, 2, 1 << n)
    np.testing.assert_array_equal(got.cpu().numpy().reshape(6, -1), select_ref(xs, forward, bits, controls))
    # per-sample gradients through the vmapped rule: the gradient of Re <w, S x> is S^dagger w for every sample
    w = torch.from_numpy(random_state(np.random.default_rng(10), 2, n, np.complex128)).cuda()
    g = torch.vmap(torch.func.grad(lambda s: (w.conj() * f(s)).sum().real))(dev)
    want = select_ref(w.cpu().numpy(), dagger, bits, controls)
    for b in range(3):
        np.testing.assert_array_equal(g[b].cpu().numpy(), want)
