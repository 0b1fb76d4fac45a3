"""Host logic of the extremal-eigenpair solver (backend.psum_lanczos, qmath.pauli_sum_extremal, PauliSum.ground_state /
extremal) without a GPU: the library's argument checks of both kernels through never-dereferenced pointers, the complex128
host route against numpy.linalg.eigh of the dense matrix, the special cases, batch independence and the capture refusal."""

import os
import re

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import _lib, backend, qmath
from _psum_ref import dense_psum
from test_evolve_cpu import HAMS, rand_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('dq_pauli_sum_lanczos_step_c64', 'dq_pauli_sum_lanczos_step_c128', 'dq_lanczos_update_c64', 'dq_lanczos_update_c128')
TOL = 1e-10


def chain(n, seed=3):
    rng = np.random.default_rng(seed)
    ham = [[0.4, '']]
    for w in range(n - 1):
        ham += [[float(rng.uniform(0.6, 1.2)), f'{p}{w}{p}{w + 1}'] for p in 'xyz']
    ham += [[float(rng.uniform(-0.6, 0.6)), f'{p}{w}'] for w in range(n) for p in 'xz'[w % 2]]
    return ham


def test_library_exports_both_kernels_and_still_reports_abi_30():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 30 and lib.dq_abi_version() == 30
    text = open(os.path.join(ROOT, 'include', 'dq_hip.h')).read()
    assert re.search(r'#define DQ_ABI_VERSION 30\b', text)
    declared = re.findall(r'^\s*(?:int|int64_t)\s+(dq_\w+)\s*\(', text, flags=re.M)
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.exported_symbols() and name in declared
    for mod, names in ((backend, ('psum_lanczos', 'LanczosResult')), (qmath, ('pauli_sum_extremal',)), (dq, ('pauli_sum_extremal',)),
                       (dq.PauliSum, ('ground_state', 'extremal'))):
        for name in names:
            assert hasattr(mod, name)


def refused(lib, rc, *words):
    text = lib.dq_last_error().decode()
    assert rc == -1 and all(w in text for w in words), text


def test_host_side_argument_checks_of_the_step():
    """DQ_ERR_ARG with a text, before any HIP call (no device is touched: the pointers are never dereferenced)."""
    lib = _lib.load()
    cur, prev, nxt, cf = 1 << 20, 1 << 22, 1 << 24, 1 << 28             # aligned non-null "pointers", far apart
    xm, bd, zm, wt, out, ws = 1 << 32, 1 << 33, 1 << 34, 1 << 35, 1 << 36, 1 << 37
    # f(cur, prev, next, coef, xmasks, bounds, zmasks, weights, ngroups, nterms, n, batch, out, ws, ws_bytes, stream)
    for f, amp, c128 in ((lib.dq_pauli_sum_lanczos_step_c64, 8, 0), (lib.dq_pauli_sum_lanczos_step_c128, 16, 1)):
        need = lib.dq_psum_cross_ws_bytes(5, 1, c128, 0)
        assert need > 0
        good = [cur, prev, nxt, cf, xm, bd, zm, wt, 2, 3, 5, 1, out, ws, need]
        for slot in (0, 1, 2, 3, 4, 5, 6, 7, 12, 13):
            refused(lib, f(*[None if i == slot else v for i, v in enumerate(good)], None), 'null')
        for slot, off in ((0, 8), (1, 8), (2, 8), (3, 4), (4, 4), (5, 2), (6, 4), (7, 4), (12, 4), (13, 8)):
            refused(lib, f(*[v + off if i == slot else v for i, v in enumerate(good)], None), 'aligned')
        head, tail = [cf, xm, bd, zm, wt], [out, ws, need]
        refused(lib, f(cur, prev, nxt, *head, 2, 3, 0, 1, *tail, None), 'n=0')
        refused(lib, f(cur, prev, nxt, *head, 2, 3, 41, 1, *tail, None), 'n=41')
        refused(lib, f(cur, prev, nxt, *head, 0, 3, 5, 1, *tail, None), 'ngroups=0')
        refused(lib, f(cur, prev, nxt, *head, 2, 0, 5, 1, *tail, None), 'nterms=0')
        refused(lib, f(cur, prev, nxt, *head, 2, 3, 5, 0, *tail, None), 'batch')
        refused(lib, f(cur, prev, nxt, *head, 2, 3, 5, 65536, *tail, None), 'batch')
        refused(lib, f(cur, prev, nxt, *head, 2, 3, 5, 1, out, ws, need - 1, None), 'workspace', 'dq_psum_cross_ws_bytes')
        refused(lib, f(cur, prev, nxt, *head, 2, 3, 5, 3, out, ws, need, None), 'workspace')          # sized for one sample
        size = 32 * amp                                                 # one sample at n = 5
        for shift in (0, 16, size - 16):                                # equal, shifted, the last vector
            refused(lib, f(cur, prev, cur + shift, *head, 2, 3, 5, 1, *tail, None), 'cur and next overlap')
            refused(lib, f(cur, cur, cur + shift, *head, 2, 3, 5, 1, *tail, None), 'cur and next overlap')
        for shift in (16, size - 16):
            refused(lib, f(cur, prev, prev + shift, *head, 2, 3, 5, 1, *tail, None), 'next and prev overlap', 'without being equal')
            refused(lib, f(cur, prev + shift, prev, *head, 2, 3, 5, 1, *tail, None), 'next and prev overlap', 'without being equal')
        need3 = lib.dq_psum_cross_ws_bytes(5, 3, c128, 0)
        refused(lib, f(cur + 3 * size - 16, prev, cur, *head, 2, 3, 5, 3, out, ws, need3, None), 'cur and next overlap')   # a batch of 3
        refused(lib, f(cur, prev, cur + size, *head, 2, 3, 5, 3, out, ws, need3, None), 'cur and next overlap')


def test_host_side_argument_checks_of_the_update():
    lib = _lib.load()
    v, w, acc, cf, out, ws = 1 << 20, 1 << 22, 1 << 24, 1 << 28, 1 << 36, 1 << 37
    # f(v, w, acc, coef, n, batch, out, ws, ws_bytes, stream)
    for f, amp, c128 in ((lib.dq_lanczos_update_c64, 8, 0), (lib.dq_lanczos_update_c128, 16, 1)):
        need = lib.dq_psum_cross_ws_bytes(5, 1, c128, 0)
        good = [v, w, acc, cf, 5, 1, out, ws, need]
        for slot in (0, 1, 3, 6, 7):                                    # (a null acc is no error: see the end)
            refused(lib, f(*[None if i == slot else x for i, x in enumerate(good)], None), 'null')
        for slot, off in ((0, 8), (1, 8), (2, 8), (3, 4), (6, 4), (7, 8)):
            refused(lib, f(*[x + off if i == slot else x for i, x in enumerate(good)], None), 'aligned')
        refused(lib, f(v, w, acc, cf, 0, 1, out, ws, need, None), 'n=0')
        refused(lib, f(v, w, acc, cf, 41, 1, out, ws, need, None), 'n=41')
        refused(lib, f(v, w, acc, cf, 5, 0, out, ws, need, None), 'batch')
        refused(lib, f(v, w, acc, cf, 5, 65536, out, ws, need, None), 'batch')
        refused(lib, f(v, w, acc, cf, 5, 1, out, ws, need - 1, None), 'workspace')
        size = 32 * amp
        for shift in (0, 16, size - 16):
            refused(lib, f(v, v + shift, acc, cf, 5, 1, out, ws, need, None), 'v and w overlap')
            refused(lib, f(v, v + shift, None, cf, 5, 1, out, ws, need, None), 'v and w overlap')
            refused(lib, f(v, w, v + shift, cf, 5, 1, out, ws, need, None), 'acc and v overlap')
            refused(lib, f(v, w, w + shift, cf, 5, 1, out, ws, need, None), 'acc and w overlap')
            refused(lib, f(v + shift, w, v, cf, 5, 1, out, ws, need, None), 'acc and v overlap')
        need3 = lib.dq_psum_cross_ws_bytes(5, 3, c128, 0)
        refused(lib, f(v, v + 3 * size - 16, acc, cf, 5, 3, out, ws, need3, None), 'v and w overlap')
        # a null acc passes every check up to the launch: the next refusal down the list is the one reported
        refused(lib, f(v, w, None, cf, 5, 1, out, ws, need - 1, None), 'workspace')
        refused(lib, f(v, w, None, cf, 5, 1, None, ws, need, None), 'null pointer (out, ws)')


def dense_pairs(n, ham):
    vals, vecs = np.linalg.eigh(dense_psum(n, ham))
    return vals, vecs


def check_pair(H, dense, got, b, want, tol):
    """value within tol * norm_bound, |H y - theta y| <= 2 tol * norm_bound, |y| = 1"""
    nb = H.norm_bound
    theta, y = float(got.value[b]), got.vector[b].to(torch.complex128).numpy()
    assert abs(theta - want) <= tol * nb, (theta, want)
    assert abs(np.linalg.norm(y) - 1.0) <= 1e-9
    assert np.linalg.norm(dense @ y - theta * y) <= 2 * tol * nb
    assert bool(got.converged[b]) and float(got.residual[b]) <= tol * nb


@pytest.mark.parametrize('kind', sorted(HAMS))
def test_host_route_against_eigh(cpu_backend, kind):
    for n in range(1, 7):
        ham = HAMS[kind](n)
        H = dq.PauliSum(ham, n)
        if kind == 'one_group':
            assert H.ngroups == 1
        dense = dense_psum(n, ham)
        vals = np.linalg.eigvalsh(dense)
        x = rand_state(2, n, 20 + n, unit=False)
        keep = x.clone()
        for which, want in (('lowest', vals[0]), ('highest', vals[-1])):
            got = backend.psum_lanczos(H.table, x, which, TOL)
            assert got.value.dtype == torch.float64 and got.vector.shape == x.shape and got.vector.dtype == x.dtype
            for b in range(2):
                check_pair(H, dense, got, b, want, TOL)
                assert int(got.steps[b]) == len(got.alphas[b]) == len(got.betas[b]) <= 4 << n
            none = backend.psum_lanczos(H.table, x, which, TOL, vector=False)
            assert none.vector is None and torch.equal(none.value, got.value) and torch.equal(none.steps, got.steps)
        assert torch.equal(x, keep)
        # complex64 states on the host route, at their own default tolerance
        got32 = backend.psum_lanczos(H.table, x.to(torch.complex64), 'lowest')
        assert got32.vector.dtype == torch.complex64 and abs(float(got32.value[0]) - vals[0]) <= 1e-6 * H.norm_bound


def test_special_cases(cpu_backend):
    x = rand_state(2, 3, 5, unit=False)
    # H a constant: norm_bound == 0, no step, the start normalised
    C = dq.PauliSum([[1.5, '']], 3)
    got = backend.psum_lanczos(C.table, x, 'highest')
    assert got.value.tolist() == [1.5, 1.5] and got.steps.tolist() == [0, 0] and got.converged.all()
    assert torch.allclose(got.vector, x / x.norm(dim=-1, keepdim=True), atol=1e-15)
    # a diagonal H with a degenerate ground level: -z0 z1 - z1 z2 has the ground space span(|000>, |111>)
    D = dq.PauliSum([[-1.0, 'z0z1'], [-1.0, 'z1z2'], [0.25, '']], 3)
    got = backend.psum_lanczos(D.table, x, 'lowest', TOL)
    assert got.converged.all() and (got.value - (-1.75)).abs().max() <= TOL * D.norm_bound
    y = got.vector
    assert (y.norm(dim=-1) - 1).abs().max() <= 1e-9 and y[:, 1:7].abs().max() <= 2 * TOL * D.norm_bound
    # a start that is an eigenvector: one step
    ham = HAMS['constant_and_mixed'](4)
    H = dq.PauliSum(ham, 4)
    vals, vecs = np.linalg.eigh(dense_psum(4, ham))
    for k, which in ((0, 'lowest'), (-1, 'highest'), (5, 'lowest')):
        e = torch.from_numpy(3.0 * vecs[:, k].copy()).reshape(1, -1)
        got = backend.psum_lanczos(H.table, e, which, TOL)
        assert got.steps.tolist() == [1] and got.converged.all() and abs(float(got.value[0]) - vals[k]) <= TOL * H.norm_bound
        assert (got.vector - e / 3.0).norm() <= 1e-9
    # one wire
    H1 = dq.PauliSum([[0.7, 'x0'], [-0.4, 'z0'], [0.1, '']], 1)
    got = backend.psum_lanczos(H1.table, rand_state(1, 1, 2), 'lowest', TOL)
    assert got.converged.all() and abs(float(got.value[0]) - (0.1 - np.hypot(0.7, 0.4))) <= TOL * H1.norm_bound
    # max_steps reached: the best pair so far, no exception
    ham = chain(6)
    H6 = dq.PauliSum(ham, 6)
    got = backend.psum_lanczos(H6.table, rand_state(1, 6, 7), 'lowest', TOL, max_steps=2)
    assert got.steps.tolist() == [2] and got.converged.tolist() == [False] and float(got.residual[0]) > TOL * H6.norm_bound
    vals = np.linalg.eigvalsh(dense_psum(6, ham))
    y = got.vector[0].numpy()
    rayleigh = float(np.real(np.vdot(y, dense_psum(6, ham) @ y)))
    assert vals[0] < float(got.value[0]) < vals[-1] and abs(np.linalg.norm(y) - 1) <= 1e-9 and abs(rayleigh - float(got.value[0])) <= 1e-9
    # refusals
    with pytest.raises(ValueError, match='which'):
        backend.psum_lanczos(H6.table, rand_state(1, 6, 7), 'middle')
    with pytest.raises(ValueError, match='tol'):
        backend.psum_lanczos(H6.table, rand_state(1, 6, 7), tol=0.0)
    with pytest.raises(ValueError, match='max_steps'):
        backend.psum_lanczos(H6.table, rand_state(1, 6, 7), max_steps=0)
    with pytest.raises(ValueError, match='zero'):
        backend.psum_lanczos(H6.table, torch.zeros(1, 64, dtype=torch.complex128))
    with pytest.raises(ValueError, match='qubits'):
        backend.psum_lanczos(H6.table, rand_state(1, 5, 7))
    with pytest.raises(ValueError, match='PsumTable'):
        backend.psum_lanczos(H6, rand_state(1, 6, 7))


def test_a_batch_is_three_single_runs_bit_for_bit(cpu_backend):
    ham = chain(6)
    H = dq.PauliSum(ham, 6)
    x = rand_state(3, 6, 9, unit=False)
    x[1] = torch.from_numpy(np.linalg.eigh(dense_psum(6, ham))[1][:, 0].copy())      # one sample stops at its first step
    keep = x.clone()
    many = backend.psum_lanczos(H.table, x, 'lowest', TOL)
    assert torch.equal(x, keep) and len(set(many.steps.tolist())) > 1
    for b in range(3):
        alone = backend.psum_lanczos(H.table, x[b:b + 1].clone(), 'lowest', TOL)
        assert torch.equal(alone.value, many.value[b:b + 1]) and torch.equal(alone.vector, many.vector[b:b + 1])
        assert torch.equal(alone.residual, many.residual[b:b + 1]) and torch.equal(alone.steps, many.steps[b:b + 1])
        assert alone.alphas[0] == many.alphas[b] and alone.betas[0] == many.betas[b]


def test_public_surface_and_seed(cpu_backend):
    n = 5
    ham = chain(n)
    H = dq.PauliSum(ham, n)
    vals = np.linalg.eigvalsh(dense_psum(n, ham))
    a = H.ground_state(dtype=torch.complex128, tol=TOL)
    b = dq.pauli_sum_extremal(ham, n, dtype=torch.complex128, tol=TOL)
    assert isinstance(a, qmath.ExtremalResult) and a.value.ndim == 0 and a.vector.shape == (1 << n,)
    assert torch.equal(a.value, b.value) and torch.equal(a.vector, b.vector) and int(a.steps) == int(b.steps)
    assert abs(float(a.value) - vals[0]) <= TOL * H.norm_bound and bool(a.converged) and not a.vector.requires_grad
    other = H.ground_state(dtype=torch.complex128, tol=TOL, seed=1)
    assert not torch.equal(other.vector, a.vector) and abs(float(other.value) - vals[0]) <= TOL * H.norm_bound
    top = H.extremal('highest', dtype=torch.complex128, tol=TOL, vector=False)
    assert top.vector is None and abs(float(top.value) - vals[-1]) <= TOL * H.norm_bound
    starts = rand_state(2, n, 3).requires_grad_()
    got = qmath.pauli_sum_extremal(H, start=starts, tol=TOL)
    assert got.value.shape == (2,) and got.vector.shape == (2, 1 << n) and not got.vector.requires_grad
    assert float(H.ground_state(start=starts[0], tol=TOL).value) == float(got.value[0])
    with pytest.raises(ValueError, match='nqubit'):
        qmath.pauli_sum_extremal(ham)
    with pytest.raises(ValueError, match='start'):
        qmath.pauli_sum_extremal(H, start=torch.zeros(3, dtype=torch.complex128))
    with pytest.raises(ValueError, match='dtype'):
        qmath.pauli_sum_extremal(H, dtype=torch.float32)


# ---- sharp bounds for the evolution ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', sorted(HAMS))
def test_spectral_bounds_and_the_evolution_with_them(cpu_backend, kind):
    tol = 1e-12
    for n in range(1, 7):
        ham = HAMS[kind](n)
        H = dq.PauliSum(ham, n)
        dense = dense_psum(n, ham)
        vals = np.linalg.eigvalsh(dense)
        lo, hi = H.spectral_bounds(dtype=torch.complex128)
        assert lo < vals[0] and vals[-1] < hi, (n, lo, hi, vals[0], vals[-1])
        assert H.constant - H.norm_bound <= lo and hi <= H.constant + H.norm_bound
        assert H.spectral_bounds(dtype=torch.complex128) is H.spectral_bounds(dtype=torch.complex128)       # cached
        x = rand_state(3, n, 10 + n)
        for t in (-2.0, 0.05, 3.0):
            got = qmath.evolve_pauli_sum(x, H, t, tol=tol, bounds=(lo, hi))
            want = x @ torch.linalg.matrix_exp(-1j * t * torch.from_numpy(dense)).T
            assert (got - want).norm(dim=-1).max().item() <= 2 * tol, (n, t)
            sharp, loose = H.chebyshev_order(t, tol, bounds=(lo, hi)), H.chebyshev_order(t, tol)
            print(f'{kind} n={n} t={t}: K = {loose} -> {sharp}')
            # the order is an integer: at a |t| far below 1 (t = 0.05: K = 6 .. 8) a width 0.7 times as large may round to the
            # same one; where a |t| is a few units it must be smaller
            assert sharp < loose if abs(t) >= 2.0 else sharp <= loose, (n, t, sharp, loose)
        # None is the call without the keyword, bit for bit, on every layer
        for t in (0.05, 3.0):
            assert torch.equal(qmath.evolve_pauli_sum(x, H, t, tol=tol, bounds=None), qmath.evolve_pauli_sum(x, H, t, tol=tol))
            assert torch.equal(backend.apply_psum_evolve(x, H.table, t, tol, bounds=None), backend.apply_psum_evolve(x, H.table, t, tol))
            assert torch.equal(dq.ops.psum_evolve(x, t, H, tol, None), dq.ops.psum_evolve(x, t, H, tol))


def test_bounds_gradcheck_gate_and_refusals(cpu_backend):
    n = 3
    ham = [[0.5, 'x0y1'], [-0.6, 'z2y1'], [0.25, ''], [0.7, 'z0z2'], [0.3, 'y0y2'], [-0.4, 'x0x1x2'], [0.8, 'y2']]
    H = dq.PauliSum(ham, n)
    bounds = H.spectral_bounds(dtype=torch.complex128)
    vals = np.linalg.eigvalsh(dense_psum(n, ham))
    assert bounds[0] < vals[0] and vals[-1] < bounds[1] and bounds[1] - bounds[0] < 2 * H.norm_bound
    x = rand_state(2, n, 1, unit=False).requires_grad_()
    t = torch.tensor([0.37, -0.81], dtype=torch.float64, requires_grad=True)
    f = lambda s, p: dq.ops.psum_evolve(s, p, H, None, bounds)  # noqa: E731
    assert torch.autograd.gradcheck(f, (x, t)) and torch.autograd.gradgradcheck(f, (x, t))
    dense = torch.from_numpy(dense_psum(n, ham))
    want = x.detach()[0] @ torch.linalg.matrix_exp(-0.37j * dense).T
    # the gate and the circuit method carry the keyword; the inverse keeps it
    g = dq.PauliSumEvolution(ham, t=torch.tensor(0.37, dtype=torch.float64), nqubit=n, tol=1e-13, bounds=bounds)
    assert g.bounds == bounds and 'bounds=' in g.extra_repr() and g.inverse().bounds == bounds
    assert (g.apply_flat(x.detach()[:1])[0] - want).norm().item() <= 1e-12
    assert torch.allclose(g.inverse().get_unitary(), g.get_unitary().mH, atol=1e-12)
    assert 'bounds' not in dq.PauliSumEvolution(ham, t=0.1, nqubit=n).extra_repr()
    cir = dq.QubitCircuit(n)
    cir.pauli_sum_evolution(H, t=0.37, bounds=bounds)
    assert cir.operators[-1].bounds == bounds
    # refusals, by name, on every layer
    for bad in ((1.0, 1.0), (2.0, -2.0), (float('-inf'), 1.0), (0.0, float('nan')), (1.0,), 'ab', 3.0):
        with pytest.raises(ValueError, match='bounds'):
            backend.apply_psum_evolve(x.detach(), H.table, 0.3, 1e-9, bounds=bad)
        with pytest.raises(ValueError, match='psum_evolve.*bounds'):
            dq.ops.psum_evolve(x.detach(), 0.3, H, bounds=bad)
        with pytest.raises(ValueError, match='bounds'):
            qmath.evolve_pauli_sum(x.detach(), H, 0.3, bounds=bad)
        with pytest.raises(ValueError, match='PauliSumEvolution.*bounds'):
            dq.PauliSumEvolution(ham, t=0.1, nqubit=n, bounds=bad)
        with pytest.raises(ValueError, match='chebyshev_order.*bounds'):
            H.chebyshev_order(0.3, 1e-9, bounds=bad)
    with pytest.raises(ValueError, match='margin'):
        H.spectral_bounds(margin=-1.0, dtype=torch.complex128)
    assert dq.PauliSum([[1.5, '']], 2).spectral_bounds() == (1.5, 1.5)


def test_refused_under_capture(cpu_backend, monkeypatch):
    H = dq.PauliSum(chain(4), 4)
    x = rand_state(1, 4, 1)
    calls = []
    monkeypatch.setattr(backend, '_psum_apply_double', lambda *a: calls.append(1))
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    with pytest.raises(RuntimeError, match='psum_lanczos under stream capture'):
        backend.psum_lanczos(H.table, x)
    with pytest.raises(RuntimeError, match='capture'):
        H.ground_state(start=x)
    assert calls == []
