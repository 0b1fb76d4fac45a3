"""The two kernels of a Lanczos step (dq_pauli_sum_lanczos_step_*, dq_lanczos_update_*) and the solver built on them
(backend.psum_lanczos, PauliSum.extremal) on the MI355X, against numpy complex128.

The step kernel shares the gather of dq_pauli_sum_cheb_step_* (tests/test_evolve_gpu.py, tests/test_psum_gpu.py describe its
geometry; their Hamiltonians per class of flip are reused): n = 1 .. 13 takes the lanes beyond a small sample (n < 12 / 11),
which must add nothing to either sum, and the flips across bit 0, inside a lane, inside a unit and across the unit size;
n = 23 / 22 a second grid-stride iteration.  The update kernel is a plain stream on the same geometry.

Exact rows: Gaussian integers in [-4, 4], weights from test_psum_gpu.HS, coefficients from {+-1, +-2, +-1/2, 0}: every
amplitude written is a multiple of 1/8 far below 2^21, and every term of either sum a multiple of 1/64 with the sum of their
absolute values below 2^53 / 64 (asserted here, on the host): exact in double in ANY order, so both numbers of `out` must EQUAL
the reference's.  Gaussian rows: the amplitudes within 1e-4 / 1e-10 of the largest of the reference; `out` against sums
formed on the host in extended precision from the kernel's OWN stored vectors -- both sides add the same numbers -- within
2^n 2^-52 sum |terms|, the worst case of a double sum of 2 * 2^n terms taken in another order.

The solver: |theta - E| and |H y - theta y| (formed in complex128 on the host) within bound * norm_bound and | |y| - 1 |
within bound for (tol, bound) = test_evolve_gpu.EVOLVE_TOL, in at most 150 steps."""

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import _lib, backend
from _evolve_ref import cheb_step_ref
from _psum_ref import hamiltonian_of, psum_apply_ref
from test_evolve_gpu import DTYPES, EVOLVE_TOL, REALS
from test_pauli_gpu import TOL, bitwise_equal, gaussian, host, integer_state
from test_psum_gpu import built, hamiltonians

pytestmark = pytest.mark.gpu

MAX_STEPS_SEEN = 150


def workspace(n, batch, dt):
    nbytes = _lib.load().dq_psum_cross_ws_bytes(n, batch, int(dt == 'c128'), 0)
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device='cuda'), nbytes


def launch_step(cur, prev, nxt, coef, H):
    """out (B, 2) on the host"""
    n, batch = cur.shape[-1].bit_length() - 1, cur.shape[0]
    ws, nbytes = workspace(n, batch, 'c128' if cur.dtype == torch.complex128 else 'c64')
    out = torch.full((batch, 2), 7.0, dtype=torch.float64, device='cuda')
    ptrs = [backend._ptr(t) for t in H.device_table('cuda')]
    backend._call('dq_pauli_sum_lanczos_step', cur, backend._ptr(cur), backend._ptr(prev), backend._ptr(nxt), backend._ptr(coef),
                  *ptrs, H.ngroups, H.nterms, n, batch, backend._ptr(out), backend._ptr(ws), nbytes)
    return out.cpu().numpy()


def launch_update(v, w, acc, coef):
    n, batch = v.shape[-1].bit_length() - 1, v.shape[0]
    ws, nbytes = workspace(n, batch, 'c128' if v.dtype == torch.complex128 else 'c64')
    out = torch.full((batch, 2), 7.0, dtype=torch.float64, device='cuda')
    backend._call('dq_lanczos_update', v, backend._ptr(v), backend._ptr(w), backend._ptr(acc), backend._ptr(coef), n, batch,
                  backend._ptr(out), backend._ptr(ws), nbytes)
    return out.cpu().numpy()


def real_coefs(batch, width, seed, exact=True):
    """(device [B][width], host (B, width)): dyadic for the exact rows, Gaussian otherwise; the first never 0."""
    rng = np.random.default_rng(seed)
    if exact:
        rows = np.stack([REALS[rng.integers(0, 6 if k == 0 else 7, batch)] for k in range(width)], axis=1)
    else:
        rows = rng.standard_normal((batch, width))
    return torch.from_numpy(rows).contiguous().cuda(), rows


def step_both_ways(cur, prev, coef, H):
    """The step with next a buffer of its own and with next = prev: [(next, out), (next, out)], the inputs checked."""
    outs = []
    for separate in (True, False):
        p = prev.clone()
        nxt = torch.full_like(cur, 7.0) if separate else p
        keep = cur.clone()
        out = launch_step(cur, p, nxt, coef, H)
        assert bitwise_equal(cur, keep)
        if separate:
            assert bitwise_equal(p, prev)
        outs.append((nxt, out))
    return outs


def exact_in_any_order(terms):
    """Every term a multiple of 1/64 and the sum of their absolute values below 2^53 / 64."""
    scaled = np.asarray(terms, dtype=np.float64) * 64.0
    return bool(np.all(scaled == np.rint(scaled))) and float(np.abs(scaled).sum()) < 2.0**53


def sum_terms(a, b):
    """The terms of sum_i Re conj(a_i) b_i per sample, (B, 2 * 2^n), in extended precision."""
    a, b = np.asarray(a), np.asarray(b)
    return np.concatenate([a.real.astype(np.longdouble) * b.real.astype(np.longdouble),
                           a.imag.astype(np.longdouble) * b.imag.astype(np.longdouble)], axis=-1)


def check_sums_exact(out, pairs, where):
    for col, (a, b) in enumerate(pairs):
        terms = sum_terms(a, b)
        assert exact_in_any_order(terms), where
        assert np.array_equal(out[:, col], terms.sum(-1).astype(np.float64)), (where, col, out[:, col], terms.sum(-1))


def check_sums_close(out, pairs, n, where):
    """Against extended-precision sums of the same numbers: within 2^n 2^-52 sum |terms|."""
    for col, (a, b) in enumerate(pairs):
        terms = sum_terms(a, b)
        want, size = terms.sum(-1), np.abs(terms).sum(-1)
        err = np.abs(out[:, col].astype(np.longdouble) - want)
        bound = (2.0**n * 2.0**-52) * size
        print(f'{where} sum {col}: err / bound = {float((err / bound).max()):.3e}')
        assert np.all(err <= bound), (where, col)


# ---- the step kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('n', range(1, 14))
def test_step_exact(n, dt):
    cur, cr = integer_state(n, 1, dt)
    prev, pr = integer_state(n, 1, dt, seed=5)
    for k, name in enumerate(hamiltonians(n)):
        H, terms = built(n, name)
        coef, rows = real_coefs(1, 3, 1000 * n + k)
        want, _ = cheb_step_ref(cr, pr, np.zeros_like(cr), terms, rows[:, 0], rows[:, 1], rows[:, 2], np.zeros(1))
        for way, (nxt, out) in zip(('own buffer', 'next is prev'), step_both_ways(cur, prev, coef, H)):
            assert np.array_equal(host(nxt), want), (n, dt, name, way, 'next')
            check_sums_exact(out, ((cr, want), (want, want)), (n, dt, name, way))
    assert np.array_equal(host(cur), cr) and np.array_equal(host(prev), pr)


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('n', range(1, 14))
def test_step_gaussian(n, dt):
    cur, cr = gaussian(n, 2, dt)
    prev, pr = gaussian(n, 2, dt, seed=5)
    names = ['all classes', f'G={min(40, 1 << n)}', f'x={(1 << n) - 1:#x} T=17', 'x=0x0 T=17', 'x=0x1 T=2']
    for k, name in enumerate(names):
        H, terms = built(n, name, exact=False)
        coef, rows = real_coefs(2, 3, 77 * n + k, exact=False)
        want, _ = cheb_step_ref(cr, pr, np.zeros_like(cr), terms, rows[:, 0], rows[:, 1], rows[:, 2], np.zeros(2))
        for way, (nxt, out) in zip(('own buffer', 'next is prev'), step_both_ways(cur, prev, coef, H)):
            got = host(nxt)
            ratio = np.abs(got - want).max() / (TOL[dt] * np.abs(want).max())
            print(f'lanczos step n={n} {name} {way} {dt}: err / (tol * max|ref|) = {ratio:.3e}')
            assert ratio <= 1.0, (n, dt, name, way)
            check_sums_close(out, ((cr, got), (got, got)), n, f'n={n} {dt} {name} {way}')


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_step_batch_of_three_and_identical_launches(dt):
    n = 12
    cur, cr = integer_state(n, 3, dt, seed=1)
    prev, pr = integer_state(n, 3, dt, seed=6)
    for name in ('all classes', 'G=40', 'x=0x800 T=17'):
        H, terms = built(n, name)
        coef, rows = real_coefs(3, 3, 17 + len(terms))
        assert len({tuple(r) for r in rows.tolist()}) > 1                         # the samples' coefficients differ
        want, _ = cheb_step_ref(cr, pr, np.zeros_like(cr), terms, rows[:, 0], rows[:, 1], rows[:, 2], np.zeros(3))
        for nxt, out in step_both_ways(cur, prev, coef, H):
            assert np.array_equal(host(nxt), want)
            check_sums_exact(out, ((cr, want), (want, want)), (dt, name))
    # two identical launches: identical bits in next and out
    g, _ = gaussian(n, 3, dt)
    gp, _ = gaussian(n, 3, dt, seed=5)
    H, _ = built(n, 'all classes', exact=False)
    coef, _ = real_coefs(3, 3, 5, exact=False)
    (n1, o1), _ = step_both_ways(g, gp, coef, H)
    (n2, o2), _ = step_both_ways(g, gp, coef, H)
    assert bitwise_equal(n1, n2) and np.array_equal(o1.view(np.int64), o2.view(np.int64))


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_step_second_grid_stride_iteration(dt):
    """More than 2048 units of 1024 vectors per sample (the Hamiltonian of test_evolve_gpu.test_step_second_grid_stride_iteration)."""
    n = {'c64': 23, 'c128': 22}[dt]
    top = 1 << (n - 1)
    terms = [(0.75, 0, 0), (-1.5, 0, top | 1 << 10 | 1), (0.6, 1, 1 << 12), (1.25, 1, 1 | top), (-0.8, top, top | 1 << 11),
             (0.4, top, 1 << 3)]
    H = dq.PauliSum(hamiltonian_of(n, terms), n)
    cur, cr = gaussian.__wrapped__(n, 1, dt)                         # (not kept: 2^23 amplitudes)
    prev, pr = gaussian.__wrapped__(n, 1, dt, seed=5)
    coef, rows = real_coefs(1, 3, 5, exact=False)
    want, _ = cheb_step_ref(cr, pr, np.zeros_like(cr), terms, rows[:, 0], rows[:, 1], rows[:, 2], np.zeros(1))
    out = launch_step(cur, prev, prev, coef, H)                      # next is prev: the normal case
    got = host(prev)
    assert np.abs(got - want).max() <= TOL[dt] * np.abs(want).max()
    assert np.array_equal(host(cur), cr)
    check_sums_close(out, ((cr, got), (got, got)), n, f'n={n} {dt}')


# ---- the update kernel -------------------------------------------------------------------------------------------------------
def update_both_ways(v, w, acc, coef):
    """With acc and with a null acc: [(w, acc or None, out), ...]; v checked."""
    outs = []
    for with_acc in (True, False):
        ww, aa, keep = w.clone(), (acc.clone() if with_acc else None), v.clone()
        out = launch_update(v, ww, aa, coef)
        assert bitwise_equal(v, keep)
        outs.append((ww, aa, out))
    return outs


def update_ref(vr, wr, ar, rows):
    return wr + rows[:, 0:1] * vr, ar + rows[:, 1:2] * vr


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('n', range(1, 14))
def test_update_exact_and_gaussian(n, dt):
    for exact, make in ((True, integer_state), (False, gaussian)):
        v, vr = make(n, 2, dt)
        w, wr = make(n, 2, dt, seed=5)
        acc, ar = make(n, 2, dt, seed=9)
        coef, rows = real_coefs(2, 2, 31 * n, exact)
        want_w, want_acc = update_ref(vr, wr, ar, rows)
        for ww, aa, out in update_both_ways(v, w, acc, coef):
            got = host(ww)
            where = f'update n={n} {dt} {"exact" if exact else "gaussian"} acc={aa is not None}'
            if exact:
                assert np.array_equal(got, want_w), where
                assert aa is None or np.array_equal(host(aa), want_acc), where
                check_sums_exact(out, ((want_w, want_w), (vr, want_w)), where)
            else:
                assert np.abs(got - want_w).max() <= TOL[dt] * np.abs(want_w).max(), where
                assert aa is None or np.abs(host(aa) - want_acc).max() <= TOL[dt] * np.abs(want_acc).max(), where
                check_sums_close(out, ((got, got), (vr, got)), n, where)
        assert np.array_equal(host(v), vr) and np.array_equal(host(w), wr) and np.array_equal(host(acc), ar)     # the shared inputs


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_update_batch_of_three_and_the_second_grid_stride_iteration(dt):
    v, vr = integer_state(12, 3, dt, seed=1)
    w, wr = integer_state(12, 3, dt, seed=6)
    acc, ar = integer_state(12, 3, dt, seed=8)
    coef, rows = real_coefs(3, 2, 4)
    assert len({tuple(r) for r in rows.tolist()}) > 1
    want_w, want_acc = update_ref(vr, wr, ar, rows)
    for ww, aa, out in update_both_ways(v, w, acc, coef):
        assert np.array_equal(host(ww), want_w) and (aa is None or np.array_equal(host(aa), want_acc))
        check_sums_exact(out, ((want_w, want_w), (vr, want_w)), dt)
    n = {'c64': 23, 'c128': 22}[dt]
    v, vr = gaussian.__wrapped__(n, 1, dt)
    w, wr = gaussian.__wrapped__(n, 1, dt, seed=5)
    acc, ar = gaussian.__wrapped__(n, 1, dt, seed=9)
    coef, rows = real_coefs(1, 2, 6, exact=False)
    want_w, want_acc = update_ref(vr, wr, ar, rows)
    out = launch_update(v, w, acc, coef)
    got = host(w)
    assert np.abs(got - want_w).max() <= TOL[dt] * np.abs(want_w).max()
    assert np.abs(host(acc) - want_acc).max() <= TOL[dt] * np.abs(want_acc).max()
    assert np.array_equal(host(v), vr)
    check_sums_close(out, ((got, got), (vr, got)), n, f'update n={n} {dt}')


# ---- the solver ----------------------------------------------------------------------------------------------------------------
def chain_hamiltonian(n=10):
    """The Hamiltonian of test_evolve_gpu.test_chain_against_the_dense_exponential."""
    rng = np.random.default_rng(3)
    ham = [[0.4, '']]
    for w in range(n - 1):
        ham += [[float(rng.uniform(0.6, 1.2)), f'{p}{w}{p}{w + 1}'] for p in 'xyz']
    ham += [[float(rng.uniform(-0.6, 0.6)), f'{p}{w}'] for w in range(n) for p in 'xz'[w % 2]]
    return dq.PauliSum(ham, n)


def check_eigenpair(H, got, exact, dt, where):
    """The criteria of the module's docstring; returns y in complex128 on the host."""
    _tol, bound = EVOLVE_TOL[dt]
    nb = H.norm_bound
    theta = float(got.value)
    y = got.vector.cpu().numpy().astype(np.complex128)
    res = np.linalg.norm(psum_apply_ref(y[None], H.terms)[0] - theta * y)
    print(f'{where} {dt}: steps {int(got.steps)}, |theta - E| / nb = {abs(theta - exact) / nb:.3e}, |H y - theta y| / nb = {res / nb:.3e}, '
          f'estimate / nb = {float(got.residual) / nb:.3e}, | |y| - 1 | = {abs(np.linalg.norm(y) - 1):.3e}')
    assert got.vector.dtype == DTYPES[dt] and got.vector.is_cuda
    assert abs(theta - exact) <= bound * nb
    assert res <= bound * nb
    assert abs(np.linalg.norm(y) - 1.0) <= bound
    assert bool(got.converged)
    assert int(got.steps) <= MAX_STEPS_SEEN
    return y


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_solver_chain_against_eigh(dt):
    H = chain_hamiltonian()
    n = H.nqubit
    vals = np.linalg.eigvalsh(psum_apply_ref(np.eye(1 << n), H.terms).T)
    assert abs(vals[0] - (-15.2372491)) < 1e-6 and abs(vals[-1] - 10.9047643) < 1e-6 and vals[1] - vals[0] > 1.0
    for which, exact in (('lowest', vals[0]), ('highest', vals[-1])):
        got = H.extremal(which, dtype=DTYPES[dt], device='cuda')
        check_eigenpair(H, got, exact, dt, f'chain {which}')
        again = H.extremal(which, dtype=DTYPES[dt], device='cuda')                 # the same seed: the same bits
        assert bitwise_equal(again.vector, got.vector) and float(again.value) == float(got.value)
        value_only = H.extremal(which, dtype=DTYPES[dt], device='cuda', vector=False)
        assert value_only.vector is None and float(value_only.value) == float(got.value)


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_solver_product_hamiltonian_against_its_closed_form(dt):
    """H = sum_w (u_w X_w + v_w Z_w) + c (test_evolve_gpu.test_product_hamiltonian_against_its_closed_form): one group per
    wire on both sides of the unit boundary, E = c -+ sum_w r_w with r_w = sqrt(u_w^2 + v_w^2), a product eigenvector and
    the gap 2 min r_w: sin(angle between y and the eigenvector) <= residual / gap."""
    n = {'c64': 13, 'c128': 12}[dt]
    rng = np.random.default_rng(8)
    u, v, c = rng.uniform(0.3, 1.0, n), rng.uniform(-1.0, 1.0, n), -0.35
    ham = [[c, '']] + [[float(u[w]), f'x{w}'] for w in range(n)] + [[float(v[w]), f'z{w}'] for w in range(n)]
    H = dq.PauliSum(ham, n)
    assert H.ngroups == n + 1
    r = np.hypot(u, v)
    gap = 2.0 * r.min()
    _tol, bound = EVOLVE_TOL[dt]
    for which, sign in (('lowest', -1.0), ('highest', 1.0)):
        got = H.extremal(which, dtype=DTYPES[dt], device='cuda')
        y = check_eigenpair(H, got, c + sign * r.sum(), dt, f'product n={n} {which}')
        exact = np.ones(1)
        for w in range(n):                              # the eigenvector of [[v, u], [u, -v]] for sign * r, wire 0 the top bit
            vec = np.array([u[w], sign * r[w] - v[w]])
            exact = np.kron(exact, vec / np.linalg.norm(vec))
        phase = np.vdot(exact, y)
        dist = np.linalg.norm(y - exact * phase / abs(phase))
        print(f'product {which} {dt}: distance from the product eigenvector {dist:.3e}, bound {bound * H.norm_bound / gap:.3e}')
        assert dist <= bound * H.norm_bound / gap


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_solver_batch_of_three_is_three_single_runs(dt):
    H = chain_hamiltonian()
    g = torch.Generator().manual_seed(21)
    x = (torch.randn(3, 1 << H.nqubit, dtype=torch.complex128, generator=g) * 3.0).to(DTYPES[dt]).cuda()
    keep = x.clone()
    many = backend.psum_lanczos(H.table, x, 'lowest')
    assert bitwise_equal(x, keep) and many.converged.all() and int(many.steps.max()) <= MAX_STEPS_SEEN
    for s in range(3):
        alone = backend.psum_lanczos(H.table, x[s:s + 1].clone(), 'lowest')
        assert bitwise_equal(alone.vector, many.vector[s:s + 1]), s
        assert torch.equal(alone.value, many.value[s:s + 1]) and torch.equal(alone.steps, many.steps[s:s + 1])
        assert alone.alphas[0] == many.alphas[s] and alone.betas[0] == many.betas[s]


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_solver_one_wire_ends_at_its_second_step_and_leaves_the_start_alone(dt):
    """n = 1: the Krylov space has two dimensions, so the second pass ends while the start vector still is one of the two
    buffers of the recurrence; it must come back bit for bit, its negative zeros included."""
    H = dq.PauliSum([[0.7, 'x0'], [-0.4, 'z0'], [0.1, '']], 1)
    x = torch.tensor([[complex(1.0, -0.0), complex(-0.0, 0.5)]], dtype=DTYPES[dt]).cuda()
    keep = x.clone()
    _tol, bound = EVOLVE_TOL[dt]
    for which, sign in (('lowest', -1.0), ('highest', 1.0)):
        got = backend.psum_lanczos(H.table, x, which)
        assert bitwise_equal(x, keep)
        assert got.steps.tolist() == [2] and got.converged.all()
        assert abs(float(got.value[0]) - (0.1 + sign * np.hypot(0.7, 0.4))) <= bound * H.norm_bound
        y = host(got.vector)[0]
        dense = np.array([[0.1 - 0.4, 0.7], [0.7, 0.1 + 0.4]])
        assert np.linalg.norm(dense @ y - float(got.value[0]) * y) <= bound * H.norm_bound and abs(np.linalg.norm(y) - 1) <= bound


# ---- sharp bounds for the evolution ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_chain_evolution_with_spectral_bounds(dt):
    H = chain_hamiltonian()
    n, (tol, bound) = H.nqubit, EVOLVE_TOL[dt]
    dense = torch.from_numpy(psum_apply_ref(np.eye(1 << n), H.terms).T.copy())
    vals = np.linalg.eigvalsh(dense.numpy())
    lo, hi = H.spectral_bounds(device='cuda')
    assert H.constant - H.norm_bound <= lo < vals[0] and vals[-1] < hi <= H.constant + H.norm_bound
    g = torch.Generator().manual_seed(11)
    xr = torch.randn(3, 1 << n, dtype=torch.complex128, generator=g)
    xr = (xr / xr.norm(dim=-1, keepdim=True)).to(DTYPES[dt])
    x, xr = xr.cuda(), xr.to(torch.complex128)
    for t in (1.6, -1.6):
        sharp, loose = H.chebyshev_order(t, tol, bounds=(lo, hi)), H.chebyshev_order(t, tol)
        got = backend.apply_psum_evolve(x, H.table, t, tol, bounds=(lo, hi))
        err = (got.cpu().to(torch.complex128) - xr @ torch.linalg.matrix_exp(-1j * t * dense).T).norm(dim=-1).max().item()
        print(f'chain t={t} {dt}: bounds ({lo:.3f}, {hi:.3f}) for [{vals[0]:.3f}, {vals[-1]:.3f}], K {loose} -> {sharp}, 2-norm error {err:.3e}')
        assert err <= bound and sharp < loose
        assert bitwise_equal(dq.evolve_pauli_sum(x, H, t, tol=tol, bounds=(lo, hi)), got)
        plain = backend.apply_psum_evolve(x, H.table, t, tol)
        assert bitwise_equal(backend.apply_psum_evolve(x, H.table, t, tol, bounds=None), plain)
        assert bitwise_equal(dq.evolve_pauli_sum(x, H, t, tol=tol, bounds=None), plain)


# ---- argument checks ---------------------------------------------------------------------------------------------------------
def test_library_error_returns():
    """DQ_ERR_ARG (-1) from the C entry points for real device buffers: nothing is launched, nothing written."""
    lib = _lib.load()
    H, _ = built(5, 'all classes')
    cur, prev, nxt, acc = (torch.zeros(1, 32, dtype=torch.complex64, device='cuda') for _ in range(4))
    coef = torch.ones(3, dtype=torch.float64, device='cuda')
    out = torch.zeros(1, 2, dtype=torch.float64, device='cuda')
    ws, nbytes = workspace(5, 1, 'c64')
    ws.zero_()
    tb = [t.data_ptr() for t in H.device_table('cuda')]
    torch.cuda.synchronize()
    cp, pp, np_, ap, fp, op, wp = (v.data_ptr() for v in (cur, prev, nxt, acc, coef, out, ws))
    g, t, n = H.ngroups, H.nterms, 5
    f = lib.dq_pauli_sum_lanczos_step_c64
    for args, word in (((cp, pp, cp), b'cur and next overlap'), ((cp, pp, pp + 16), b'without being equal'),
                       ((cp, pp, np_ + 8), b'aligned'), ((cp, None, np_), b'null')):
        assert f(*args, fp, *tb, g, t, n, 1, op, wp, nbytes, None) == -1 and word in lib.dq_last_error(), lib.dq_last_error()
    assert f(cp, pp, np_, None, *tb, g, t, n, 1, op, wp, nbytes, None) == -1
    assert f(cp, pp, np_, fp, *tb, 0, t, n, 1, op, wp, nbytes, None) == -1
    assert f(cp, pp, np_, fp, *tb, g, t, 41, 1, op, wp, nbytes, None) == -1
    assert f(cp, pp, np_, fp, tb[0], None, tb[2], tb[3], g, t, n, 1, op, wp, nbytes, None) == -1
    assert f(cp, pp, np_, fp, *tb, g, t, n, 1, None, wp, nbytes, None) == -1 and b'null' in lib.dq_last_error()
    assert f(cp, pp, np_, fp, *tb, g, t, n, 1, op, None, nbytes, None) == -1 and b'null' in lib.dq_last_error()
    assert f(cp, pp, np_, fp, *tb, g, t, n, 1, op, wp, nbytes - 1, None) == -1 and b'workspace' in lib.dq_last_error()
    f = lib.dq_lanczos_update_c64
    for args, word in (((cp, cp, ap), b'v and w overlap'), ((cp, np_, cp), b'acc and v overlap'), ((cp, np_, np_ + 16), b'acc and w overlap'),
                       ((cp, np_ + 8, ap), b'aligned'), ((None, np_, ap), b'null'), ((cp, cp + 16, None), b'v and w overlap')):
        assert f(*args, fp, n, 1, op, wp, nbytes, None) == -1 and word in lib.dq_last_error(), lib.dq_last_error()
    assert f(cp, np_, ap, None, n, 1, op, wp, nbytes, None) == -1
    assert f(cp, np_, ap, fp, 0, 1, op, wp, nbytes, None) == -1
    assert f(cp, np_, None, fp, n, 1, op, wp, nbytes - 1, None) == -1 and b'workspace' in lib.dq_last_error()
    assert f(cp, np_, None, fp, n, 1, None, wp, nbytes, None) == -1 and b'null' in lib.dq_last_error()
    torch.cuda.synchronize()
    assert not cur.any() and not prev.any() and not nxt.any() and not acc.any() and not out.any() and not ws.any()
    x = torch.zeros(1, 32, dtype=torch.complex64, device='cuda')
    with pytest.raises(ValueError, match='zero'):
        backend.psum_lanczos(H.table, x)
