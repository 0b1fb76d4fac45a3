"""Host logic of the Pauli-sum evolution (backend.apply_psum_evolve, ops.psum_evolve, qmath.evolve_pauli_sum,
dq.PauliSumEvolution, cir.pauli_sum_evolution) without a GPU: the library's argument checks through never-dereferenced
pointers, the Bessel helper and the order rule, the complex128 host route against dense exponentials, the autograd rules
and the public surface."""

import os
import pickle
import re

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import _lib, backend, ops, qmath
from _evolve_ref import bessel_integral, evolve_ref, smallest_order
from _psum_ref import dense_psum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('dq_pauli_sum_cheb_step_c64', 'dq_pauli_sum_cheb_step_c128')
ZS = (0.0, 0.3, 5.0, 37.5, 200.0)


def rand_state(batch, n, seed, unit=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, 1 << n, dtype=torch.complex128, generator=g)
    return x / x.norm(dim=-1, keepdim=True) if unit else x


def dense_u(n, ham, t):
    return torch.linalg.matrix_exp(-1j * float(t) * torch.from_numpy(dense_psum(n, ham)))


def test_library_exports_the_step_and_still_reports_abi_30():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 30 and lib.dq_abi_version() == 30
    text = open(os.path.join(ROOT, 'include', 'dq_hip.h')).read()
    assert re.search(r'#define DQ_ABI_VERSION 30\b', text)
    declared = re.findall(r'^\s*(?:int|int64_t)\s+(dq_\w+)\s*\(', text, flags=re.M)
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.exported_symbols() and name in declared
    for mod, names in ((ops, ('psum_evolve',)), (backend, ('apply_psum_evolve', 'bessel_j', 'chebyshev_order')),
                       (qmath, ('evolve_pauli_sum',)), (dq, ('PauliSumEvolution', 'evolve_pauli_sum'))):
        for name in names:
            assert hasattr(mod, name)
    assert hasattr(dq.QubitCircuit, 'pauli_sum_evolution')


def test_host_side_argument_checks_of_the_step():
    """DQ_ERR_ARG with a text, before any HIP call (no device is touched: the pointers are never dereferenced)."""
    lib = _lib.load()
    cur, prev, nxt, acc, cf = 1 << 20, 1 << 22, 1 << 24, 1 << 26, 1 << 28      # aligned non-null "pointers", far apart
    xm, bd, zm, wt = 1 << 32, 1 << 33, 1 << 34, 1 << 35

    def refused(rc, *words):
        text = lib.dq_last_error().decode()
        assert rc == -1 and all(w in text for w in words), text

    # f(cur, prev, next, acc, coef, xmasks, bounds, zmasks, weights, ngroups, nterms, n, batch, stream)
    for f, amp in ((lib.dq_pauli_sum_cheb_step_c64, 8), (lib.dq_pauli_sum_cheb_step_c128, 16)):
        good = [cur, prev, nxt, acc, cf, xm, bd, zm, wt, 2, 3, 5, 1]
        for slot in range(9):
            refused(f(*[None if i == slot else v for i, v in enumerate(good)], None), 'null')
        for slot, off in ((0, 8), (1, 8), (2, 8), (3, 8), (4, 4), (5, 4), (6, 2), (7, 4), (8, 4)):
            refused(f(*[v + off if i == slot else v for i, v in enumerate(good)], None), 'aligned')
        tail = [cf, xm, bd, zm, wt]
        refused(f(cur, prev, nxt, acc, *tail, 2, 3, 0, 1, None), 'n=0')
        refused(f(cur, prev, nxt, acc, *tail, 2, 3, 41, 1, None), 'n=41')
        refused(f(cur, prev, nxt, acc, *tail, 0, 3, 5, 1, None), 'ngroups=0')
        refused(f(cur, prev, nxt, acc, *tail, 2, 0, 5, 1, None), 'nterms=0')
        refused(f(cur, prev, nxt, acc, *tail, 2, 3, 5, 0, None), 'batch')
        refused(f(cur, prev, nxt, acc, *tail, 2, 3, 5, 65536, None), 'batch')
        size = 32 * amp                                                 # one sample at n = 5
        for shift in (0, 16, size - 16):                                # equal, shifted, the last vector
            refused(f(cur, prev, cur + shift, acc, *tail, 2, 3, 5, 1, None), 'cur and next overlap')
            refused(f(cur, prev, nxt, cur + shift, *tail, 2, 3, 5, 1, None), 'acc and cur overlap')
            refused(f(cur, prev, nxt, prev + shift, *tail, 2, 3, 5, 1, None), 'acc and prev overlap')
            refused(f(cur, prev, nxt, nxt + shift, *tail, 2, 3, 5, 1, None), 'acc and next overlap')
            refused(f(cur, prev, prev, prev + shift, *tail, 2, 3, 5, 1, None), 'acc and prev overlap')
        for shift in (16, size - 16):
            refused(f(cur, prev, prev + shift, acc, *tail, 2, 3, 5, 1, None), 'next and prev overlap', 'without being equal')
            refused(f(cur, prev + shift, prev, acc, *tail, 2, 3, 5, 1, None), 'next and prev overlap', 'without being equal')
        refused(f(cur + 3 * size - 16, prev, cur, acc, *tail, 2, 3, 5, 3, None), 'cur and next overlap')     # a batch of 3
        refused(f(cur, prev, cur + size, acc, *tail, 2, 3, 5, 3, None), 'cur and next overlap')


def test_bessel_helper_against_the_integral():
    """J_k(z) = (1/N) sum_m cos(k tau_m - z sin tau_m): the trapezoid rule is spectrally exact at N = 4096 for these z and k."""
    for z in ZS:
        kmax = int(z + 60)
        want = bessel_integral(z, kmax)
        got = np.array(backend.bessel_j(z, kmax))
        print(f'z = {z}: max |J_k - integral| = {np.abs(got - want).max():.2e} over k <= {kmax}')
        assert got.shape == want.shape and np.abs(got - want).max() <= 2e-14
    assert backend.bessel_j(0.0, 3) == [1.0, 0.0, 0.0, 0.0]
    assert backend.bessel_j(2.0, 500)[200:] == [0.0] * 301 or max(map(abs, backend.bessel_j(2.0, 500)[200:])) < 1e-300
    with pytest.raises(ValueError, match='bessel_j'):
        backend.bessel_j(-1.0)


def test_chebyshev_order_is_the_smallest_with_the_tail_below_tol():
    H = dq.PauliSum([[0.5, 'x0'], [-1.5, 'z1y0'], [0.25, ''], [2.0, 'z1']], 2)
    assert H.norm_bound >= 4.0 and H.norm_bound - 4.0 < 1e-14 and H.constant == 0.25
    assert dq.PauliSum([[3.0, '']], 2).norm_bound == 0.0
    for z in ZS:
        values = bessel_integral(z, int(z + 10 * z ** (1 / 3)) + 110)
        for tol in (1e-6, 1e-12):
            want = smallest_order(values, tol)
            got = backend.chebyshev_order(z, tol)
            print(f'z = {z}, tol = {tol}: K = {got}')
            assert got == want == backend.chebyshev_order(-z, tol)
            if z:
                assert H.chebyshev_order(z / H.norm_bound, tol) in (got - 1, got, got + 1)
    assert H.chebyshev_order(1.0, 1e-6) == backend.chebyshev_order(H.norm_bound, 1e-6)
    for bad in (0.0, -1e-6, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='tol'):
            backend.chebyshev_order(1.0, bad)


HAMS = {
    'constant_and_mixed': lambda n: [[0.25, ''], [0.7, 'x0'], [-0.4, 'z0']] + [[0.5, f'x{w}x{w + 1}'] for w in range(n - 1)]
    + [[-0.3, f'z{w}z{w + 1}'] for w in range(n - 1)],
    'y_strings': lambda n: [[0.6, 'y0'], [-0.8, 'z0']] + [[0.45, f'y{w}x{w + 1}'] for w in range(n - 1)]
    + [[0.35, f'y{w}y{w + 1}'] for w in range(n - 1)],
    'one_group': lambda n: [[0.9, 'x0' + ''.join(f'z{w}' for w in range(1, n))], [-0.5, 'y0'], [0.3, 'x0']],
}


@pytest.mark.parametrize('kind', sorted(HAMS))
def test_host_route_against_the_dense_exponential(cpu_backend, kind):
    tol = 1e-12
    for n in range(1, 7):
        ham = HAMS[kind](n)
        H = dq.PauliSum(ham, n)
        if kind == 'one_group':
            assert H.ngroups == 1
        x = rand_state(4, n, 10 + n)
        ts = [-2.0, 0.0, 0.05, 3.0]
        for t in ts:
            got = backend.apply_psum_evolve(x, H.table, t, tol)
            want = x @ dense_u(n, ham, t).T
            err = (got - want).norm(dim=-1).max().item()
            assert err <= 2 * tol, (n, t, err)
            if t == 0.0:
                assert torch.equal(got, x)
        # one t per sample: every sample as it would come out alone
        tt = torch.tensor(ts, dtype=torch.float64)
        got = backend.apply_psum_evolve(x, H.table, tt, tol)
        for s, t in enumerate(ts):
            assert torch.equal(got[s:s + 1], backend.apply_psum_evolve(x[s:s + 1], H.table, t, tol))
            assert (got[s] - dense_u(n, ham, t) @ x[s]).norm().item() <= 2 * tol
        # the reference expansion at the order the host chose, and complex64 states at their own tolerance
        order = H.chebyshev_order(3.0, tol)
        assert np.abs(evolve_ref(x.numpy(), H.terms, 3.0, order) - backend.apply_psum_evolve(x, H.table, 3.0, tol).numpy()).max() < 1e-12
        got32 = backend.apply_psum_evolve(x.to(torch.complex64), H.table, 3.0, 1e-6)
        assert got32.dtype == torch.complex64 and (got32.to(torch.complex128) - x @ dense_u(n, ham, 3.0).T).norm(dim=-1).max() < 1e-5


def test_backend_refusals_and_out(cpu_backend, monkeypatch):
    H = dq.PauliSum(HAMS['constant_and_mixed'](3), 3)
    x = rand_state(2, 3, 1)
    with pytest.raises(ValueError, match='tol'):
        backend.apply_psum_evolve(x, H.table, 0.3, 0.0)
    with pytest.raises(ValueError, match='real'):
        backend.apply_psum_evolve(x, H.table, 0.3j, 1e-9)
    with pytest.raises(ValueError, match='one per sample'):
        backend.apply_psum_evolve(x, H.table, [0.1, 0.2, 0.3], 1e-9)
    with pytest.raises(ValueError, match='finite'):
        backend.apply_psum_evolve(x, H.table, float('inf'), 1e-9)
    with pytest.raises(ValueError, match='out of place'):
        backend.apply_psum_evolve(x, H.table, 0.3, 1e-9, out=x)
    with pytest.raises(ValueError, match='qubits'):
        backend.apply_psum_evolve(rand_state(1, 4, 1), H.table, 0.3, 1e-9)
    with pytest.raises(ValueError, match='PsumTable'):
        backend.apply_psum_evolve(x, H, 0.3, 1e-9)
    with pytest.raises(ValueError, match='PauliSum'):
        ops.psum_evolve(x, 0.3, HAMS['y_strings'](3))
    with pytest.raises(ValueError, match='tol'):
        ops.psum_evolve(x, 0.3, H, tol=-1.0)
    buf = torch.empty_like(x)
    before = x.clone()
    assert backend.apply_psum_evolve(x, H.table, 0.3, 1e-9, out=buf) is buf and torch.equal(x, before)
    # a Hamiltonian that is a constant: a phase
    C = dq.PauliSum([[1.5, '']], 3)
    assert torch.allclose(backend.apply_psum_evolve(x, C.table, 0.4, 1e-12), np.exp(-0.6j) * x, atol=1e-15)
    # under capture the call is refused by name before anything runs
    calls = []
    monkeypatch.setattr(backend, '_psum_apply_double', lambda *a: calls.append(1))
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    with pytest.raises(RuntimeError, match='apply_psum_evolve under stream capture'):
        backend.apply_psum_evolve(x, H.table, 0.3, 1e-9)
    with pytest.raises(RuntimeError, match='capture'):
        qmath.evolve_pauli_sum(x, H, 0.3)
    assert calls == []


def test_node_gradcheck_jvp_and_vmap(cpu_backend):
    n = 3
    ham = [[0.5, 'x0y1'], [-0.6, 'z2y1'], [0.25, ''], [0.7, 'z0z2'], [0.3, 'y0y2'], [-0.4, 'x0x1x2'], [0.8, 'y2']]
    H = dq.PauliSum(ham, n)
    x = rand_state(2, n, 1, unit=False).requires_grad_()
    t = torch.tensor([0.37, -0.81], dtype=torch.float64, requires_grad=True)
    shared = torch.tensor(0.53, dtype=torch.float64, requires_grad=True)
    gc, ggc = torch.autograd.gradcheck, torch.autograd.gradgradcheck
    f = lambda s, p: ops.psum_evolve(s, p, H)  # noqa: E731
    assert gc(f, (x, t)) and gc(f, (x, shared))
    assert ggc(f, (x, t)) and ggc(f, (x, shared))
    assert gc(f, (x, t), check_forward_ad=True, check_backward_ad=False)
    assert gc(f, (x, shared), check_forward_ad=True, check_backward_ad=False)
    # d/dt exp(-i t H) x = -i H exp(-i t H) x, through jvp
    xd, td = x.detach(), t.detach()
    out, tangent = torch.func.jvp(lambda p: ops.psum_evolve(xd, p, H), (td,), (torch.ones_like(td),))
    dense = torch.from_numpy(dense_psum(n, ham))
    assert (tangent - (-1j) * out @ dense.T).abs().max().item() < 1e-11
    # vmap over a batch of states folds into the batch of one backend call, exactly
    xs = rand_state(6, n, 4).reshape(3, 2, -1)
    want = backend.apply_psum_evolve(xs.reshape(6, -1), H.table, 0.4, 1e-12)
    assert torch.equal(torch.vmap(lambda s: ops.psum_evolve(s, 0.4, H))(xs).reshape(6, -1), want)
    tv = torch.tensor([0.1, 0.2, 0.3], dtype=torch.float64)
    got = torch.vmap(lambda s, p: ops.psum_evolve(s, p, H))(xs, tv)
    for j in range(3):
        assert torch.equal(got[j], backend.apply_psum_evolve(xs[j].contiguous(), H.table, float(tv[j]), 1e-12))
    # the default tolerance follows the precision
    x32 = xd.to(torch.complex64)
    assert torch.equal(ops.psum_evolve(x32, 0.4, H), backend.apply_psum_evolve(x32, H.table, 0.4, 1e-6))
    assert torch.equal(ops.psum_evolve(xd, 0.4, H), backend.apply_psum_evolve(xd, H.table, 0.4, 1e-12))


def test_the_other_generator_families_are_unchanged(cpu_backend):
    x = rand_state(2, 4, 3, unit=False).requires_grad_()
    th = torch.tensor([0.3, -0.8], dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda s, p: ops.pauli_rot(s, 0b1010, 0b0110, p, (0,)), (x, th))
    spec = (0b0110, 0b0010, 0b0001, 1, ())
    assert torch.autograd.gradcheck(lambda s, p: ops.excite_rot(s, spec, p), (x, th))
    assert ops._PAULI_STRINGS.rot_tail(spec) == () and ops._EXCITATIONS.rot_tail(spec) == ()


def test_gate_against_the_dense_hamiltonian_gate(cpu_backend):
    n = 4
    # (coefficients that float32 holds exactly: HamiltonianGate keeps its list in the default precision)
    ham = [[0.5, 'x0y1'], [-0.625, 'z3y1'], [0.25, ''], [0.75, 'z0z2'], [0.375, 'y0y2'], [-0.5, 'x1x2x3'], [0.875, 'y2']]

    def energy(kind, t):
        cir = dq.QubitCircuit(n)
        cir.hlayer()
        cir.ry(1, inputs=0.4)
        getattr(cir, kind)(ham, t=t)
        cir.cnot(0, 2)
        cir.observable(0)
        cir.observable([1, 3], 'xz')
        cir.to(torch.double)
        cir()
        return cir.expectation().sum(), cir

    t_new = torch.tensor(0.83, dtype=torch.float64, requires_grad=True)
    t_old = torch.tensor(0.83, dtype=torch.float64, requires_grad=True)
    e_new, cir_new = energy('pauli_sum_evolution', t_new)
    e_old, cir_old = energy('hamiltonian', t_old)
    assert (cir_new.state - cir_old.state).abs().max().item() < 1e-11 and abs(float(e_new) - float(e_old)) < 1e-11
    # a trainable t
    cir = dq.QubitCircuit(n)
    cir.hlayer()
    cir.pauli_sum_evolution(ham)
    cir.observable(0)
    cir.to(torch.double)
    gate = cir.operators[-1]
    assert isinstance(gate, dq.PauliSumEvolution) and isinstance(gate.t, torch.nn.Parameter) and cir.npara == 1
    ref = dq.QubitCircuit(n)
    ref.hlayer()
    ref.hamiltonian(ham, t=gate.t.detach().clone())
    ref.operators[-1].t.requires_grad_()
    ref.observable(0)
    ref.to(torch.double)
    cir()
    ref()
    (g_new,) = torch.autograd.grad(cir.expectation().sum(), gate.t)
    (g_old,) = torch.autograd.grad(ref.expectation().sum(), ref.operators[-1].t)
    assert abs(float(g_new) - float(g_old)) < 1e-10 and abs(float(g_new)) > 1e-3
    # the unitary, its inverse, pickling and the repr
    g = dq.PauliSumEvolution(ham, t=torch.tensor(0.37, dtype=torch.float64), nqubit=n, tol=1e-13)
    u = g.get_unitary()
    assert torch.allclose(u, dense_u(n, ham, 0.37), atol=1e-12)
    assert torch.allclose(g.inverse().get_unitary(), u.mH, atol=1e-12)
    assert g.wires == [0, 1, 2, 3] and g.npara == 1 and g.tol == 1e-13
    assert 'terms=7' in g.extra_repr() and 'tol=1e-13' in g.extra_repr() and 't=0.37' in g.extra_repr()
    back = pickle.loads(pickle.dumps(g))
    assert torch.equal(back.get_unitary(), u) and back.hamiltonian.table._devices == {}
    assert dq.PauliSumEvolution(dq.PauliSum(ham, n), t=0.1, nqubit=n).hamiltonian.nterms == 7
    # qmath, in the forms of the other Pauli-sum functions
    x = rand_state(2, n, 9)
    want = x @ dense_u(n, ham, -0.6).T
    assert (qmath.evolve_pauli_sum(x, ham, -0.6) - want).abs().max().item() < 1e-12
    assert (dq.evolve_pauli_sum(x[0], dq.PauliSum(ham, n), -0.6) - want[0]).abs().max().item() < 1e-12
    assert qmath.evolve_pauli_sum(x[:1].reshape(1, -1, 1), ham, -0.6, nqubit=n).shape == (1, 16, 1)
    # encode=True: t from the data, one per sample
    enc = dq.QubitCircuit(n)
    enc.hlayer()
    enc.pauli_sum_evolution(ham, encode=True)
    enc.to(torch.double)
    assert (enc.npara, enc.ndata) == (0, 1)
    data = torch.tensor([[0.2], [-0.9]], dtype=torch.float64)
    states = enc(data).reshape(2, -1)
    plus = torch.full((16,), 0.25, dtype=torch.complex128)
    for s in range(2):
        assert (states[s] - dense_u(n, ham, float(data[s, 0])) @ plus).abs().max().item() < 1e-6


def test_gate_refusals(cpu_backend):
    for bad in ([[1j, 'x0']], [[0.5 + 0.1j, 'x0y1']]):
        with pytest.raises(ValueError, match='PauliSumEvolution.*real'):
            dq.PauliSumEvolution(bad, nqubit=2)
    for kw in (dict(hamiltonian=[]), dict(hamiltonian='x0'), dict(hamiltonian=[[1.0, 'x0y0']]), dict(hamiltonian=[[1.0, 'x4']]),
               dict(tol=0.0), dict(tol=float('nan')), dict(hamiltonian=dq.PauliSum([[1.0, 'x0']], 3))):
        args = dict(hamiltonian=[[1.0, 'x0y1']], nqubit=2)
        args.update(kw)
        with pytest.raises(ValueError, match='PauliSumEvolution'):
            dq.PauliSumEvolution(**args)
    make = lambda **kw: dq.PauliSumEvolution([[1.0, 'x0y1'], [0.5, '']], t=0.3, nqubit=2, **kw)  # noqa: E731
    name = 'PauliSumEvolution'
    with pytest.raises(NotImplementedError, match=name):
        make(den_mat=True)
    with pytest.raises(NotImplementedError, match=name):
        make().op_dist_state(None)
    with pytest.raises(NotImplementedError, match=name):
        make().prims()
    dm = dq.QubitCircuit(2, den_mat=True)
    with pytest.raises(NotImplementedError, match=name):
        dm.pauli_sum_evolution([[1.0, 'x0y1']])
    cir = dq.QubitCircuit(2)
    cir.add(make())
    with pytest.raises(NotImplementedError, match=name):
        cir.qasm()
