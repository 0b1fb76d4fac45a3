"""The Chebyshev step kernel (dq_pauli_sum_cheb_step_*) and the evolution built on it (backend.apply_psum_evolve) on the
MI355X, against numpy complex128 (tests/_evolve_ref.py).

ONE step: the gather is that of dq_apply_psum_axpby_* (tests/test_psum_gpu.py describes its geometry, and its Hamiltonians
per class of flip are reused here): n = 1 .. 13 takes the flips across bit 0 (the complex64 element swap), inside a lane's
vectors, inside a unit, and across bit 11 / 10 (the unit size) and above.  prev, next and acc are touched at the lane's
own vectors only, so what is new is the aliasing -- next is prev, or a buffer of its own -- and that nothing else moves.

Exact rows: Gaussian integers in [-4, 4], weights from test_psum_gpu.HS, alpha, beta, gamma from {+-1, +-2, +-1/2, 0} and
delta from test_pauli_gpu.COEFS: every partial sum is a multiple of 1/8 far below 2^21, exact in float32 in any order.
Gaussian rows: 1e-4 / 1e-10 of the largest amplitude of the reference.

The whole evolution, for unit states: complex128 at tol = 1e-12 within 1e-10 and complex64 at tol = 1e-6 within 1e-4, in the
2-norm."""

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import _lib, backend
from _evolve_ref import apply_product, cheb_step_ref, product_evolution
from _psum_ref import hamiltonian_of, psum_apply_ref
from test_pauli_gpu import COEFS, TOL, bitwise_equal, gaussian, host, integer_state
from test_psum_gpu import built, hamiltonians

pytestmark = pytest.mark.gpu

DTYPES = {'c64': torch.complex64, 'c128': torch.complex128}
REALS = np.array([1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 0.0])
EVOLVE_TOL = {'c64': (1e-6, 1e-4), 'c128': (1e-12, 1e-10)}      # (the tolerance asked for, the bound on the 2-norm error)


def step_coefs(batch, seed, exact=True):
    """(device [B][5], alpha, beta, gamma, delta): dyadic for the exact rows, Gaussian otherwise; alpha never 0."""
    rng = np.random.default_rng(seed)
    if exact:
        alpha, beta, gamma = REALS[rng.integers(0, 6, batch)], REALS[rng.integers(0, 7, batch)], REALS[rng.integers(0, 7, batch)]
        delta = COEFS[rng.integers(1, len(COEFS), batch)]
    else:
        alpha, beta, gamma = rng.standard_normal(batch), rng.standard_normal(batch), rng.standard_normal(batch)
        delta = rng.standard_normal(batch) + 1j * rng.standard_normal(batch)
    rows = np.stack([alpha, beta, gamma, delta.real, delta.imag], axis=1)
    return torch.from_numpy(rows).contiguous().cuda(), alpha, beta, gamma, delta


def launch(cur, prev, nxt, acc, coef, H):
    n = cur.shape[-1].bit_length() - 1
    ptrs = [backend._ptr(t) for t in H.device_table('cuda')]
    backend._call('dq_pauli_sum_cheb_step', cur, backend._ptr(cur), backend._ptr(prev), backend._ptr(nxt), backend._ptr(acc),
                  backend._ptr(coef), *ptrs, H.ngroups, H.nterms, n, cur.shape[0])


def run_both_ways(cur, prev, acc, coef, H):
    """The step with next a buffer of its own and with next = prev: [(next, acc), (next, acc)], the inputs checked."""
    outs = []
    for separate in (True, False):
        p, a = prev.clone(), acc.clone()
        nxt = torch.full_like(cur, 7.0) if separate else p
        keep = cur.clone()
        launch(cur, p, nxt, a, coef, H)
        assert bitwise_equal(cur, keep)
        if separate:
            assert bitwise_equal(p, prev)
        outs.append((nxt, a))
    return outs


# ---- one step --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('n', range(1, 14))
def test_step_exact(n, dt):
    cur, cr = integer_state(n, 1, dt)
    prev, pr = integer_state(n, 1, dt, seed=5)
    acc, ar = integer_state(n, 1, dt, seed=9)
    seen_groups, seen_counts = set(), set()
    for k, name in enumerate(hamiltonians(n)):
        H, terms = built(n, name)
        seen_groups.add(H.ngroups)
        seen_counts |= {sum(1 for t in terms if t[1] == xm) for xm in {t[1] for t in terms}}
        coef, alpha, beta, gamma, delta = step_coefs(1, 1000 * n + k)
        want_next, want_acc = cheb_step_ref(cr, pr, ar, terms, alpha, beta, gamma, delta)
        for way, (nxt, a) in zip(('own buffer', 'next is prev'), run_both_ways(cur, prev, acc, coef, H)):
            assert np.array_equal(host(nxt), want_next), (n, dt, name, way, 'next')
            assert np.array_equal(host(a), want_acc), (n, dt, name, way, 'acc')
    if n >= 9:
        assert {1, 2, 40} <= seen_groups and {1, 2, 17} <= seen_counts
    assert 'x=0x0 T=17' in hamiltonians(n)                          # (a diagonal H: no flip at all)
    assert np.array_equal(host(cur), cr) and np.array_equal(host(prev), pr) and np.array_equal(host(acc), ar)


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('n', range(1, 14))
def test_step_gaussian(n, dt):
    cur, cr = gaussian(n, 2, dt)
    prev, pr = gaussian(n, 2, dt, seed=5)
    acc, ar = gaussian(n, 2, dt, seed=9)
    names = ['all classes', f'G={min(40, 1 << n)}', f'x={(1 << n) - 1:#x} T=17', 'x=0x0 T=17', 'x=0x1 T=2']
    for k, name in enumerate(names):
        H, terms = built(n, name, exact=False)
        coef, alpha, beta, gamma, delta = step_coefs(2, 77 * n + k, exact=False)
        want_next, want_acc = cheb_step_ref(cr, pr, ar, terms, alpha, beta, gamma, delta)
        for way, (nxt, a) in zip(('own buffer', 'next is prev'), run_both_ways(cur, prev, acc, coef, H)):
            for what, got, want in (('next', nxt, want_next), ('acc', a, want_acc)):
                ratio = np.abs(host(got) - want).max() / (TOL[dt] * np.abs(want).max())
                print(f'step n={n} {name} {way} {what} {dt}: err / (tol * max|ref|) = {ratio:.3e}')
                assert ratio <= 1.0, (n, dt, name, way, what)


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_step_batch_of_three_with_per_sample_coefficients(dt):
    n = 12
    cur, cr = integer_state(n, 3, dt, seed=1)
    prev, pr = integer_state(n, 3, dt, seed=6)
    acc, ar = integer_state(n, 3, dt, seed=8)
    for name in ('all classes', 'G=40', 'x=0x800 T=17'):
        H, terms = built(n, name)
        coef, alpha, beta, gamma, delta = step_coefs(3, 17 + len(terms))
        assert len({tuple(r) for r in coef.cpu().tolist()}) > 1                   # the samples' coefficients differ
        want_next, want_acc = cheb_step_ref(cr, pr, ar, terms, alpha, beta, gamma, delta)
        for nxt, a in run_both_ways(cur, prev, acc, coef, H):
            assert np.array_equal(host(nxt), want_next) and np.array_equal(host(a), want_acc)


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_step_second_grid_stride_iteration(dt):
    """More than 2048 units of 1024 vectors per sample: flips at bit 0 and at the top bit, the top z bit meeting the unit's
    index (the Hamiltonian of test_psum_gpu.test_second_grid_stride_iteration)."""
    n = {'c64': 23, 'c128': 22}[dt]
    top = 1 << (n - 1)
    terms = [(0.75, 0, 0), (-1.5, 0, top | 1 << 10 | 1), (0.6, 1, 1 << 12), (1.25, 1, 1 | top), (-0.8, top, top | 1 << 11),
             (0.4, top, 1 << 3)]
    H = dq.PauliSum(hamiltonian_of(n, terms), n)
    cur, cr = gaussian.__wrapped__(n, 1, dt)                         # (not kept: 2^23 amplitudes)
    prev, pr = gaussian.__wrapped__(n, 1, dt, seed=5)
    acc, ar = gaussian.__wrapped__(n, 1, dt, seed=9)
    coef, alpha, beta, gamma, delta = step_coefs(1, 5, exact=False)
    want_next, want_acc = cheb_step_ref(cr, pr, ar, terms, alpha, beta, gamma, delta)
    launch(cur, prev, prev, acc, coef, H)                            # next is prev: the normal case
    for got, want in ((prev, want_next), (acc, want_acc)):
        assert np.abs(host(got) - want).max() <= TOL[dt] * np.abs(want).max()
    assert np.array_equal(host(cur), cr)


# ---- the whole evolution -----------------------------------------------------------------------------------------------------
def unit_state(n, batch, dt, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, 1 << n, dtype=torch.complex128, generator=g)
    x = (x / x.norm(dim=-1, keepdim=True)).to(DTYPES[dt])
    return x.cuda(), x.to(torch.complex128)


def worst_error(got, want):
    return (got.cpu().to(torch.complex128) - want).norm(dim=-1).max().item()


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_chain_against_the_dense_exponential(dt):
    n, t = 10, 1.6
    rng = np.random.default_rng(3)
    ham = [[0.4, '']]
    for w in range(n - 1):
        ham += [[float(rng.uniform(0.6, 1.2)), f'{p}{w}{p}{w + 1}'] for p in 'xyz']
    ham += [[float(rng.uniform(-0.6, 0.6)), f'{p}{w}'] for w in range(n) for p in 'xz'[w % 2]]
    H = dq.PauliSum(ham, n)
    tol, bound = EVOLVE_TOL[dt]
    order = H.chebyshev_order(t, tol)
    assert order > 40
    dense = torch.from_numpy(psum_apply_ref(np.eye(1 << n), H.terms).T.copy())
    x, xr = unit_state(n, 3, dt, 11)
    keep = x.clone()
    for tt in (t, -t):
        got = backend.apply_psum_evolve(x, H.table, tt, tol)
        err = worst_error(got, xr @ torch.linalg.matrix_exp(-1j * tt * dense).T)
        print(f'chain n={n} t={tt} K={order} {dt}: 2-norm error {err:.3e}')
        assert err <= bound
    assert bitwise_equal(x, keep)                                    # the input is never written
    back = backend.apply_psum_evolve(backend.apply_psum_evolve(x, H.table, t, tol), H.table, -t, tol)
    err = worst_error(back, xr)
    print(f'chain there and back {dt}: {err:.3e}')
    assert err <= bound
    # t = 0 is the input bit for bit; one t per sample is every sample alone, bit for bit
    assert bitwise_equal(backend.apply_psum_evolve(x, H.table, 0.0, tol), x)
    ts = torch.tensor([t, 0.0, -0.3], dtype=torch.float64, device='cuda')
    many = backend.apply_psum_evolve(x, H.table, ts, tol)
    assert bitwise_equal(many[1], x[1])
    for s in range(3):
        alone = backend.apply_psum_evolve(x[s:s + 1], H.table, float(ts[s]), tol)
        assert bitwise_equal(many[s:s + 1], alone), s
    buf = torch.empty_like(x)
    assert backend.apply_psum_evolve(x, H.table, ts, tol, out=buf) is buf and bitwise_equal(buf, many)


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_product_hamiltonian_against_its_closed_form(dt):
    """H = sum_w (u_w X_w + v_w Z_w) + c: one group per wire, flips on both sides of the unit boundary, and
    exp(-i t H) a tensor product of 2x2 exponentials, exact at any n."""
    n = {'c64': 13, 'c128': 12}[dt]
    rng = np.random.default_rng(8)
    u, v, c, t = rng.uniform(0.3, 1.0, n), rng.uniform(-1.0, 1.0, n), -0.35, 1.9
    ham = [[c, '']] + [[float(u[w]), f'x{w}'] for w in range(n)] + [[float(v[w]), f'z{w}'] for w in range(n)]
    H = dq.PauliSum(ham, n)
    assert H.ngroups == n + 1
    tol, bound = EVOLVE_TOL[dt]
    x, xr = unit_state(n, 2, dt, 12)
    got = backend.apply_psum_evolve(x, H.table, t, tol)
    want = torch.from_numpy(apply_product(xr.numpy(), *product_evolution(n, u, v, c, t)))
    err = worst_error(got, want)
    print(f'product n={n} K={H.chebyshev_order(t, tol)} {dt}: 2-norm error {err:.3e}')
    assert err <= bound
    err = worst_error(backend.apply_psum_evolve(got, H.table, -t, tol), xr)
    print(f'product there and back {dt}: {err:.3e}')
    assert err <= bound


# ---- argument checks ---------------------------------------------------------------------------------------------------------
def test_library_error_returns():
    """DQ_ERR_ARG (-1) from the C entry point for real device buffers: nothing is launched."""
    lib = _lib.load()
    H, _ = built(5, 'all classes')
    cur, prev, nxt, acc = (torch.zeros(1, 32, dtype=torch.complex64, device='cuda') for _ in range(4))
    coef = torch.ones(5, dtype=torch.float64, device='cuda')
    tb = [t.data_ptr() for t in H.device_table('cuda')]
    torch.cuda.synchronize()
    cp, pp, np_, ap, fp = (v.data_ptr() for v in (cur, prev, nxt, acc, coef))
    g, t, n = H.ngroups, H.nterms, 5
    f = lib.dq_pauli_sum_cheb_step_c64
    for args, word in (((cp, pp, cp, ap), b'cur and next overlap'), ((cp, pp, np_, cp), b'acc and cur overlap'),
                       ((cp, pp, pp, pp), b'acc and prev overlap'), ((cp, pp, np_, np_ + 16), b'acc and next overlap'),
                       ((cp, pp, pp + 16, ap), b'without being equal'), ((cp, pp, np_ + 8, ap), b'aligned'),
                       ((cp, None, np_, ap), b'null')):
        assert f(*args, fp, *tb, g, t, n, 1, None) == -1 and word in lib.dq_last_error(), lib.dq_last_error()
    assert f(cp, pp, np_, ap, None, *tb, g, t, n, 1, None) == -1
    assert f(cp, pp, np_, ap, fp, *tb, 0, t, n, 1, None) == -1
    assert f(cp, pp, np_, ap, fp, *tb, g, t, 41, 1, None) == -1
    assert f(cp, pp, np_, ap, fp, tb[0], None, tb[2], tb[3], g, t, n, 1, None) == -1
    torch.cuda.synchronize()
    assert not cur.any() and not prev.any() and not nxt.any() and not acc.any()
    x = torch.zeros(1, 32, dtype=torch.complex64, device='cuda')
    with pytest.raises(ValueError, match='out of place'):
        backend.apply_psum_evolve(x, H.table, 0.3, 1e-6, out=x)
