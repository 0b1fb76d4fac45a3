"""The derivatives of ``ops.psum_axpby`` and ``ops.psum_cross`` on the MI355X at kernel-path shapes -- n = 12 and 13 with a
flip at bit 11 (above and inside a unit of complex64 vectors, above it for complex128) and one at bit 0 (inside a complex64
vector), complex64 and complex128 -- against closed forms in numpy complex128 built from tests/_psum_ref.py alone.

First derivatives: the checks of tests/_stream_grad_cases.py (reverse and forward mode, and at n = 12 the state and cotangent
layouts autograd hands a node) with the Pauli sums as a third family of tests/_stream_grad_ref.py.  Second derivatives: the
rules in the comment above ``ops._Generator`` applied twice, written out below; a reduction through H is held to tol * |u| |v| sum_t |h_t|, the bound of |<u, H v>|."""

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import ops
import _stream_grad_cases as cases
import _stream_grad_ref as ref
from _psum_ref import PauliSums, hamiltonian_of, psum_apply_ref

pytestmark = pytest.mark.gpu

DEVICE = 'cuda'


def terms_of(n):
    top = 1 << (n - 1)
    return [(0.5, 0, 0), (-0.75, 0, 1 << 11 | 1 << 3), (1.25, 1 << 11, 1 << 11 | 1 << 5), (0.5, 1 << 11, 1), (-1.0, 1, 1 | top),
            (0.25, 1, 1 << 10), (0.75, 1 << 11 | 1, 1 << 11 | 1 | 1 << 6), (-0.5, top | 1 << 4, top | 1 << 4 | 1 << 11)]


def family(n):
    terms = terms_of(n)
    H = dq.PauliSum(hamiltonian_of(n, terms), n)
    assert {bin(x & z).count('1') % 4 for _, x, z in terms} == {0, 1, 2}
    return PauliSums(n, terms), H, sum(abs(h) for h, _, _ in terms)


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('n', [12, 13])
def test_vjp_and_jvp_against_the_closed_forms(n, dt):
    fam, H, _ = family(n)
    nodes = cases.generator_nodes(f'psum n={n} {dt}', fam, lambda s, a, c, mode: ops.psum_axpby(s, a, c, H),
                                  lambda u, v: ops.psum_cross(u, v, H), None, 2, False, dt, np.random.default_rng(n))
    for node in nodes[:-1]:                              # (the last is the rotation, which this family does not have)
        cases.check_forward(node, dt, DEVICE)
        cases.check_vjp(node, dt, DEVICE)
        cases.check_jvp(node, dt, DEVICE)


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_cotangent_and_state_layouts(dt):
    """The states at element offset 1 (a complex64 pointer at 8 mod 16) and an expanded, a strided and an offset cotangent."""
    n = 12
    fam, H, _ = family(n)
    nodes = cases.generator_nodes(f'psum n={n} {dt}', fam, lambda s, a, c, mode: ops.psum_axpby(s, a, c, H),
                                  lambda u, v: ops.psum_cross(u, v, H), None, 2, False, dt, np.random.default_rng(n))
    for node in nodes[:-1]:
        cases.check_layouts(node, dt, DEVICE)


def dev(pair):
    return pair[0].to(DEVICE).requires_grad_(), pair[1]


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('n', [12, 13])
def test_second_derivatives_of_axpby(n, dt):
    """y = a x + c H x with the cotangent gy:  gx = conj(a) gy + conj(c) H gy,  ga = <x, gy>,  gc = <H x, gy> = cross(x, gy).
    Their VJP with cotangents (v, wa, wc):
        g_gy = a v + c H v + wa x + wc H x          g_x = conj(wa) gy + conj(wc) H gy
        g_a  = conj(sum conj(gy) v) = <v, gy>       g_c = conj(sum conj(H gy) v) = <v, H gy>"""
    fam, H, hsum = family(n)
    rng = np.random.default_rng(100 + n)
    size = (2, 1 << n)
    (x, xr), (gy, gyr) = dev(cases.gauss(rng, size, cases.DTYPES[dt])), dev(cases.gauss(rng, size, cases.DTYPES[dt]))
    v, vr = cases.gauss(rng, size, cases.DTYPES[dt])
    a, c = (torch.tensor(p[:2], device=DEVICE, requires_grad=True) for p in (cases.A, cases.C))
    ar, cr = cases.A[:2], cases.C[:2]
    wa, wc = (torch.tensor(p, device=DEVICE) for p in (np.array([0.4 - 0.9j, -1.2 + 0.3j]), np.array([0.7j, 0.5 - 0.2j])))
    war, wcr = cases.host(wa), cases.host(wc)
    gx, ga, gc = torch.autograd.grad(ops.psum_axpby(x, a, c, H), (x, a, c), gy, create_graph=True)
    g_gy, g_a, g_c, g_x = torch.autograd.grad((gx, ga, gc), (gy, a, c, x), (v.to(DEVICE), wa, wc))
    hv, hx, hgy = (psum_apply_ref(t, fam.terms) for t in (vr, xr, gyr))
    col = lambda p: p.reshape(-1, 1)  # noqa: E731
    what = f'psum axpby n={n} {dt}, second order'
    cases.close_state(g_gy, col(ar) * vr + col(cr) * hv + col(war) * xr + col(wcr) * hx, dt, what + ': gy')
    cases.close_state(g_x, col(war.conj()) * gyr + col(wcr.conj()) * hgy, dt, what + ': x')
    scale = cases.norms(vr) * cases.norms(gyr)
    cases.close_reduction(g_a, (vr.conj() * gyr).sum(-1), scale, dt, what + ': a')
    cases.close_reduction(g_c, (vr.conj() * hgy).sum(-1), scale * hsum, dt, what + ': c')
    # and the same through the closed forms of the family, one level down
    want_gx, want_ga, want_gc = ref.axpby_vjp(fam, xr, ar, cr, 'gate', gyr)
    cases.close_state(gx, want_gx, dt, what + ': the first-order gx it differentiates')
    cases.close_reduction(ga, want_ga, cases.norms(xr) * cases.norms(gyr), dt, what + ': ga')
    cases.close_reduction(gc, want_gc, cases.norms(xr) * cases.norms(gyr) * hsum, dt, what + ': gc')


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('same', [False, True], ids=['cross', 'expect'])
@pytest.mark.parametrize('n', [12, 13])
def test_second_derivatives_of_cross(n, same, dt):
    """z = <u, H x> with the cotangent gz:  g_u = conj(gz) H x,  g_x = gz H u.  Their VJP with cotangents (tu, tx):
        g_gz = <tu, H x> + <H u, tx>        g_u = conj(gz) H tx        g_x = gz H tu
    (``same``: u is x, one tensor in both slots -- the two gradients add up)."""
    fam, H, hsum = family(n)
    rng = np.random.default_rng(200 + n)
    size = (2, 1 << n)
    x, xr = dev(cases.gauss(rng, size, cases.DTYPES[dt]))
    u, ur = (x, xr) if same else dev(cases.gauss(rng, size, cases.DTYPES[dt]))
    (tu, tur), (tx, txr) = cases.gauss(rng, size, cases.DTYPES[dt]), cases.gauss(rng, size, cases.DTYPES[dt])
    gz = torch.tensor(np.array([0.8 - 0.3j, -0.4 + 1.1j]), device=DEVICE, requires_grad=True)
    gzr = cases.host(gz).reshape(-1, 1)
    z = ops.psum_cross(u, x, H)
    what = f'psum cross n={n} {dt} {"expect" if same else "cross"}, second order'
    htu, htx, hx, hu = (psum_apply_ref(t, fam.terms) for t in (tur, txr, xr, ur))
    if same:
        (g1,) = torch.autograd.grad(z, (x,), gz, create_graph=True)             # = conj(gz) H x + gz H x
        g_gz, g_x = torch.autograd.grad(g1, (gz, x), tx.to(DEVICE))
        cases.close_state(g1, (gzr.conj() + gzr) * hx, dt, what + ': the first-order gradient it differentiates')
        cases.close_state(g_x, (gzr + gzr.conj()) * htx, dt, what + ': x')
        want = (txr.conj() * hx).sum(-1) + (hx.conj() * txr).sum(-1)
        cases.close_reduction(g_gz, want, 2 * cases.norms(txr) * cases.norms(xr) * hsum, dt, what + ': gz')
        return
    g_u, g_x = torch.autograd.grad(z, (u, x), gz, create_graph=True)
    gg_gz, gg_u, gg_x = torch.autograd.grad((g_u, g_x), (gz, u, x), (tu.to(DEVICE), tx.to(DEVICE)))
    want_u, want_x = ref.cross_vjp(fam, ur, xr, gzr.reshape(-1))
    cases.close_state(g_u, want_u, dt, what + ': the first-order g_u it differentiates')
    cases.close_state(g_x, want_x, dt, what + ': the first-order g_x it differentiates')
    cases.close_state(gg_u, gzr.conj() * htx, dt, what + ': u')
    cases.close_state(gg_x, gzr * htu, dt, what + ': x')
    want = (tur.conj() * hx).sum(-1) + (hu.conj() * txr).sum(-1)
    scale = (cases.norms(tur) * cases.norms(xr) + cases.norms(ur) * cases.norms(txr)) * hsum
    cases.close_reduction(gg_gz, want, scale, dt, what + ': gz')


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_vmap_folds_into_the_batch_bit_for_bit(dt):
    from deepquantum_amd import backend

    n = 12
    _, H, _ = family(n)
    xs = cases.gauss(np.random.default_rng(5), (6, 1 << n), cases.DTYPES[dt])[0].to(DEVICE).reshape(3, 2, -1)
    ones = torch.ones(6, dtype=torch.complex128, device=DEVICE)
    want = backend.apply_psum_axpby(xs.reshape(6, -1), H.table, 0.5 * ones, 2 * ones)
    assert cases.bitwise_equal(torch.vmap(lambda s: ops.psum_axpby(s, 0.5, 2.0, H))(xs).reshape(6, -1), want)
    want = backend.psum_cross(xs.reshape(6, -1), xs.flip(0).reshape(6, -1).contiguous(), H.table)
    assert torch.equal(torch.vmap(lambda p, q: ops.psum_cross(p, q, H))(xs, xs.flip(0)).reshape(-1), want)
