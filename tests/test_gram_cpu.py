"""Gram matrices and linear combinations of state batches without a GPU: shapes, dtypes and every refusal by name, the
library's host-side checks (no device is touched: the pointers are never dereferenced), the public wrappers against numpy,
and the derivatives of ``ops.gram`` / ``ops.combine`` through the plain-torch complex128 stand-ins of ``backend`` under the
CPU test double."""

import os
import re

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import _lib, backend, ops, qmath
import _gram_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('dq_gram_geometry', 'dq_gram_ws_bytes', 'dq_gram_c64', 'dq_gram_c128', 'dq_combine_c64', 'dq_combine_c128')


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rows(seed, m, n, dt='c128', kind='gauss'):
    rng = np.random.default_rng(seed)
    return (ref.gaussian_rows if kind == 'gauss' else ref.integer_rows)(rng, m, n, dt)


# ---- the library and its header -------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, 'include', 'dq_hip.h')).read()
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name) and re.search(rf'\b{name}\(', text) and name in _lib.exported_symbols()
    assert lib.dq_abi_version() == 30
    for name in ('gram_matrix', 'fidelity_kernel', 'linear_combination', 'orthonormalize'):
        assert getattr(dq, name) is getattr(qmath, name)
    assert hasattr(dq.QubitCircuit, 'kernel_matrix') and hasattr(dq.PauliSum, 'subspace_matrices')


def test_geometry_and_workspace_exports():
    lib = _lib.load()
    for dtype, c128 in ((torch.complex64, 0), (torch.complex128, 1)):
        g = backend.gram_geometry(dtype)
        per_vec = 1 if c128 else 2
        assert g.tile_rows == 32 and g.lane_cols == 4 * per_vec and g.wave_cols == 4 * g.lane_cols
        assert g.unit_cols % g.wave_cols == 0 and g.max_blocks >= 256
        assert (0 < g.chain <= 512) if not c128 else g.chain == 0
        tile = 32 * 32 * 16
        nmin = 0 if c128 else 1
        assert lib.dq_gram_ws_bytes(nmin, 1, 1, c128) == tile and lib.dq_gram_ws_bytes(nmin, 32, 32, c128) == tile
        assert lib.dq_gram_ws_bytes(nmin, 33, 32, c128) == 2 * tile and lib.dq_gram_ws_bytes(nmin, 33, 65, c128) == 6 * tile
        unit = ref.log2(g.unit_cols)
        assert lib.dq_gram_ws_bytes(unit + 2, 5, 7, c128) == 4 * tile                  # four units, a workgroup each
        assert lib.dq_gram_ws_bytes(40, 32, 32, c128) == g.max_blocks * tile           # never more than max_blocks per pair
        assert lib.dq_gram_ws_bytes(40, 64, 64, c128) == g.max_blocks * tile           # ... shared among the pairs
        assert lib.dq_gram_ws_bytes(12, 1024, 1024, c128) == 1024 * tile               # a thousand pairs: one workgroup each
        for bad in ((nmin - 1, 1, 1), (41, 1, 1), (5, 0, 1), (5, 1, 0), (5, 65535 * 32 + 1, 1)):
            assert lib.dq_gram_ws_bytes(*bad, c128) == -1
    null = _lib.C.POINTER(_lib.C.c_int)()
    one = _lib.C.c_int()
    assert lib.dq_gram_geometry(0, null, one, one, one, one, one) < 0 and b'null pointer' in lib.dq_last_error()


def refused(lib, rc, *words):
    text = lib.dq_last_error().decode()
    assert rc < 0 and all(w in text for w in words), text


def test_host_side_argument_checks():
    lib = _lib.load()
    a, b, out, ws, coef = 1 << 20, 1 << 24, 1 << 28, 1 << 30, 1 << 32                 # aligned non-null "pointers", far apart
    for dt, c128 in (('c64', 0), ('c128', 1)):
        gram, combine = getattr(lib, f'dq_gram_{dt}'), getattr(lib, f'dq_combine_{dt}')
        need = lib.dq_gram_ws_bytes(5, 3, 4, c128)
        good = [a, b, 5, 3, 4, out, ws, need]
        for slot in (0, 1, 5, 6):
            args = list(good)
            args[slot] = None
            refused(lib, gram(*args, None), f'dq_gram_{dt}', 'null pointer')
        for slot in (0, 1, 6):
            args = list(good)
            args[slot] += 8
            refused(lib, gram(*args, None), '16-byte aligned')
        refused(lib, gram(a, b, 5, 3, 4, out + 4, ws, need, None), 'aligned')
        refused(lib, gram(a, b, 5, 3, 4, out, ws, need - 1, None), 'workspace', str(need), 'dq_gram_ws_bytes')
        refused(lib, gram(a, b, 41, 3, 4, out, ws, need, None), 'n=41 out of range')
        refused(lib, gram(a, b, -c128, 3, 4, out, ws, need, None), 'out of range')
        refused(lib, gram(a, b, 5, 0, 4, out, ws, need, None), 'rows')
        refused(lib, gram(a, b, 5, 3, 65535 * 32 + 1, out, ws, need, None), 'rows')
        row = 32 * (16 if c128 else 8)
        refused(lib, gram(a, b, 5, 3, 4, a + 2 * row, ws, need, None), 'overlap')      # out inside a
        refused(lib, gram(a, b, 5, 3, 4, out, b + 3 * row, need, None), 'overlap')     # ws inside b
        refused(lib, gram(a, b, 5, 3, 4, out, out + 16, need, None), 'overlap')        # ws inside out
        good = [a, coef, b, 5, 3, 4]
        for slot in (0, 1, 2):
            args = list(good)
            args[slot] = None
            refused(lib, combine(*args, None), f'dq_combine_{dt}', 'null pointer')
        refused(lib, combine(a + 8, coef, b, 5, 3, 4, None), 'in and out', '16-byte aligned')
        refused(lib, combine(a, coef, b + 8, 5, 3, 4, None), 'in and out', '16-byte aligned')
        refused(lib, combine(a, coef + 8, b, 5, 3, 4, None), 'coef', '16-byte aligned')
        refused(lib, combine(a, coef, b, 41, 3, 4, None), 'n=41 out of range')
        refused(lib, combine(a, coef, b, 5, 0, 4, None), 'rows')
        refused(lib, combine(a, coef, a, 5, 4, 4, None), 'in and out overlap', 'out of place only')
        refused(lib, combine(a, coef, a + 4 * row - 16, 5, 1, 4, None), 'in and out overlap')     # the last vector of `in`
        refused(lib, combine(a, coef, a - 3 * row + 16, 5, 3, 4, None), 'in and out overlap')     # the last vector of `out`
        refused(lib, combine(a, coef, coef + 16, 5, 3, 4, None), 'coef and out overlap')


# ---- backend: shapes, dtypes, refusals ------------------------------------------------------------------------------------
def test_backend_shapes_dtypes_and_refusals(cpu_backend):
    a, b = tt(rows(1, 3, 4)), tt(rows(2, 5, 4))
    g = backend.gram(a, b)
    assert g.dtype == torch.complex128 and g.shape == (3, 5) and not g.requires_grad
    np.testing.assert_allclose(g.numpy(), ref.gram_ref(a.numpy(), b.numpy()), rtol=0, atol=1e-14)
    assert backend.gram(a.to(torch.complex64), b.to(torch.complex64)).dtype == torch.complex128
    one = backend.gram(torch.ones(2, 1, dtype=torch.complex128), torch.ones(1, 1, dtype=torch.complex128))     # n = 0
    assert one.shape == (2, 1)
    coef = tt(ref.gaussian_coefs(np.random.default_rng(3), 2, 5))
    y = backend.combine(b, coef)
    assert y.dtype == b.dtype and y.shape == (2, 16)
    np.testing.assert_allclose(y.numpy(), ref.combine_ref(coef.numpy(), b.numpy()), rtol=0, atol=1e-14)
    y32 = backend.combine(b.to(torch.complex64), coef)
    assert y32.dtype == torch.complex64
    out = torch.empty(2, 16, dtype=torch.complex128)
    assert backend.combine(b, coef, out=out) is out and torch.equal(out, y)
    # a non-contiguous state
    with pytest.raises(ValueError, match='contiguous'):
        backend.gram(a, torch.cat([b, b], 1)[:, :16])
    with pytest.raises(ValueError, match='contiguous'):
        backend.gram(torch.cat([a, a], 1)[:, :16], b)
    with pytest.raises(ValueError, match='contiguous'):
        backend.combine(torch.cat([b, b], 1)[:, :16], coef)
    # a pending conj bit (the double refuses what `_ptr` refuses)
    with pytest.raises(ValueError, match='pending conjugation'):
        backend.gram(a.conj(), b)
    with pytest.raises(ValueError, match='pending conjugation'):
        backend.combine(b.conj(), coef)
    # mismatched n, dtype
    with pytest.raises(ValueError, match='one n, dtype'):
        backend.gram(a, tt(rows(4, 5, 3)))
    with pytest.raises(ValueError, match='one n, dtype'):
        backend.gram(a.to(torch.complex64), b)
    with pytest.raises(ValueError, match='2\\*\\*n'):
        backend.gram(a[:, :12].contiguous(), b[:, :12].contiguous())
    with pytest.raises(ValueError, match='at least two amplitudes'):
        backend.gram(torch.ones(2, 1, dtype=torch.complex64), torch.ones(2, 1, dtype=torch.complex64))
    with pytest.raises(TypeError, match='complex64 or complex128'):
        backend.gram(a.real.contiguous(), a.real.contiguous())
    # a wrong coef shape
    for bad in (coef.T.contiguous(), coef[0], coef[:, :4]):
        with pytest.raises(ValueError, match=r'coef must have shape \(M, 5\)'):
            backend.combine(b, bad)
    # a coef with requires_grad reaching backend
    with pytest.raises(ValueError, match='constant'):
        backend.combine(b, coef.clone().requires_grad_())
    # out: overlapping, wrong shape
    pool = torch.zeros(8, 16, dtype=torch.complex128)
    with pytest.raises(ValueError, match='out of place only'):
        backend.combine(pool[:5], coef, out=pool[4:6])
    with pytest.raises(ValueError, match='out of place only'):
        backend.combine(pool[:5], torch.ones(5, 5, dtype=torch.complex128), out=pool[:5])
    with pytest.raises(ValueError, match='out of place only'):
        backend.combine(pool[:5], torch.ones(5, 5, dtype=torch.complex128), out=pool[1:6])
    with pytest.raises(ValueError, match='out must be'):
        backend.combine(b, coef, out=torch.empty(3, 16, dtype=torch.complex128))
    with pytest.raises(ValueError, match='out must be'):
        backend.combine(b, coef, out=torch.empty(2, 16, dtype=torch.complex64))
    assert backend.combine(pool[:5], coef, out=pool[5:7]).data_ptr() == pool[5].data_ptr()


def test_no_cpu_fallback():
    a = tt(rows(1, 2, 3))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        backend.gram(a, a)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        backend.combine(a, torch.ones(1, 2, dtype=torch.complex128))


def test_vmap_is_refused(cpu_backend):
    xs = tt(rows(5, 6, 3)).reshape(2, 3, 8)
    with pytest.raises(RuntimeError, match='gram under torch.vmap is not supported'):
        torch.vmap(lambda s: ops.gram(s, s))(xs)
    with pytest.raises(RuntimeError, match='gram under torch.vmap is not supported'):
        torch.vmap(lambda s: ops.gram(xs[0], s))(xs)
    with pytest.raises(RuntimeError, match='combine under torch.vmap is not supported'):
        torch.vmap(lambda s: ops.combine(s, torch.ones(2, 3, dtype=torch.complex128)))(xs)
    with pytest.raises(RuntimeError, match='combine under torch.vmap is not supported'):
        torch.vmap(lambda c: ops.combine(xs[0], c))(torch.ones(4, 2, 3, dtype=torch.complex128))
    with pytest.raises(RuntimeError, match='under torch.vmap is not supported'):
        torch.vmap(qmath.gram_matrix)(xs)


# ---- derivatives ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m', [1, 3])
@pytest.mark.parametrize('k', [1, 3])
def test_gradcheck_of_gram(cpu_backend, m, k):
    a, b = tt(rows(10 + m, m, 2)).requires_grad_(), tt(rows(20 + k, k, 2)).requires_grad_()
    assert torch.autograd.gradcheck(ops.gram, (a, b))
    assert torch.autograd.gradgradcheck(ops.gram, (a, b))
    assert torch.autograd.gradcheck(ops.gram, (a, b), check_forward_ad=True, check_backward_ad=False)


@pytest.mark.parametrize('m', [1, 3])
def test_gradcheck_of_the_self_gram(cpu_backend, m):
    a = tt(rows(30 + m, m, 2)).requires_grad_()
    assert torch.autograd.gradcheck(lambda x: ops.gram(x, x), (a,))
    assert torch.autograd.gradgradcheck(lambda x: ops.gram(x, x), (a,))


@pytest.mark.parametrize('m', [1, 3])
@pytest.mark.parametrize('k', [1, 3])
def test_gradcheck_of_combine(cpu_backend, m, k):
    s = tt(rows(40 + k, k, 2)).requires_grad_()
    coef = tt(ref.gaussian_coefs(np.random.default_rng(50 + m), m, k)).requires_grad_()
    assert torch.autograd.gradcheck(ops.combine, (s, coef))
    assert torch.autograd.gradgradcheck(ops.combine, (s, coef))
    assert torch.autograd.gradcheck(ops.combine, (s, coef), check_forward_ad=True, check_backward_ad=False)


def test_gradients_against_the_formulas(cpu_backend):
    """Abar = conj(Gbar) B, Bbar = Gbar^T A; Sbar = C^H Ybar, Cbar = gram(S, Ybar)^T -- in numpy."""
    a, b = tt(rows(1, 3, 3)).requires_grad_(), tt(rows(2, 2, 3)).requires_grad_()
    gbar = tt(ref.gaussian_coefs(np.random.default_rng(3), 3, 2))
    ga, gb = torch.autograd.grad(ops.gram(a, b), (a, b), gbar)
    np.testing.assert_allclose(ga.numpy(), gbar.numpy().conj() @ b.detach().numpy(), atol=1e-14)
    np.testing.assert_allclose(gb.numpy(), gbar.numpy().T @ a.detach().numpy(), atol=1e-14)
    coef = tt(ref.gaussian_coefs(np.random.default_rng(4), 2, 3)).requires_grad_()
    ybar = tt(rows(5, 2, 3))
    gs, gc = torch.autograd.grad(ops.combine(a, coef), (a, coef), ybar)
    np.testing.assert_allclose(gs.numpy(), coef.detach().numpy().conj().T @ ybar.numpy(), atol=1e-14)
    np.testing.assert_allclose(gc.numpy(), ref.gram_ref(a.detach().numpy(), ybar.numpy()).T, atol=1e-14)


# ---- the public wrappers --------------------------------------------------------------------------------------------------
def test_public_wrappers_against_the_reference(cpu_backend):
    a, b = rows(1, 4, 3), rows(2, 3, 3)
    want = ref.gram_ref(a, b)
    for fa, fb in ((tt(a), tt(b)), (tt(a).unsqueeze(-1), tt(b).unsqueeze(-1)), (tt(a), tt(b)[1].reshape(8, 1))):
        got = qmath.gram_matrix(fa, fb)
        assert got.dtype == torch.complex128
        np.testing.assert_allclose(got.numpy(), want if got.shape == want.shape else want[:, 1:2], rtol=0, atol=1e-14)
    self_gram = qmath.gram_matrix(tt(a))
    np.testing.assert_allclose(self_gram.numpy(), ref.gram_ref(a, a), rtol=0, atol=1e-14)
    k = qmath.fidelity_kernel(tt(a), tt(b))
    assert k.dtype == torch.float64 and k.shape == (4, 3)
    np.testing.assert_allclose(k.numpy(), np.abs(want) ** 2, rtol=1e-14, atol=1e-14)
    np.testing.assert_allclose(qmath.fidelity_kernel(tt(a)).numpy(), np.abs(ref.gram_ref(a, a)) ** 2, rtol=1e-14, atol=0)
    assert qmath.gram_matrix(tt(a).to(torch.complex64)).dtype == torch.complex128
    coef = ref.gaussian_coefs(np.random.default_rng(3), 2, 4)
    y = qmath.linear_combination(tt(a), tt(coef))
    assert y.shape == (2, 8) and y.dtype == torch.complex128
    np.testing.assert_allclose(y.numpy(), ref.combine_ref(coef, a), rtol=0, atol=1e-14)
    np.testing.assert_allclose(qmath.linear_combination(tt(a), tt(coef[0])).numpy(), ref.combine_ref(coef[:1], a), atol=1e-14)
    assert qmath.linear_combination(tt(a).to(torch.complex64), tt(coef.real.copy())).dtype == torch.complex64
    for bad in (torch.ones(2, 3, dtype=torch.complex128), torch.ones(2, 2, 2, 2, dtype=torch.complex128), 'x'):
        with pytest.raises(ValueError, match='gram_matrix'):
            qmath.gram_matrix(bad)
    with pytest.raises(ValueError, match='one number of qubits'):
        qmath.gram_matrix(tt(a), tt(rows(3, 2, 2)))
    with pytest.raises(ValueError, match='one dtype'):
        qmath.gram_matrix(tt(a), tt(b).to(torch.complex64))
    with pytest.raises(ValueError, match=r'coef must have shape \(M, 4\)'):
        qmath.linear_combination(tt(a), torch.ones(2, 3, dtype=torch.complex128))


def test_orthonormalize(cpu_backend):
    v = rows(7, 5, 4)
    v[3] = v[2] + 1e-5 * v[3]                            # nearly dependent: cond(S) ~ 1e10, one pass would leave 1e-6
    q, low = qmath.orthonormalize(tt(v))
    assert q.shape == (5, 16) and q.dtype == torch.complex128 and low.shape == (5, 5) and low.dtype == torch.complex128
    assert (qmath.gram_matrix(q) - torch.eye(5)).abs().max() < 1e-12
    assert torch.equal(low, torch.tril(low)) and (low.diagonal().imag == 0).all() and (low.diagonal().real > 0).all()
    np.testing.assert_allclose((low @ q).numpy(), v, rtol=0, atol=1e-10)
    q32, _ = qmath.orthonormalize(tt(rows(8, 3, 4, 'c64')))
    assert q32.dtype == torch.complex64 and (qmath.gram_matrix(q32) - torch.eye(3)).abs().max() < 1e-5
    dep = tt(np.concatenate([v[:2], (2 * v[0] - 1j * v[1])[None]]))
    with pytest.raises(ValueError, match='numerically dependent: pivot 2'):
        qmath.orthonormalize(dep)
    with pytest.raises(ValueError, match='numerically dependent: pivot 1'):
        qmath.orthonormalize(tt(np.stack([v[0], 3j * v[0], v[1]])))
    # differentiable: d/dv of a function of the orthonormal basis
    x = tt(rows(9, 2, 2)).requires_grad_()
    assert torch.autograd.gradcheck(lambda s: qmath.orthonormalize(s)[0], (x,))


def dense_of(H, n):
    """The matrix of a PauliSum from its action on the basis states (row b of the batch is H|b>)."""
    return qmath.apply_pauli_sum(torch.eye(1 << n, dtype=torch.complex128), n, H).numpy().T


def test_subspace_matrices_of_a_krylov_basis(cpu_backend):
    """The generalised eigenproblem Hs c = E S c of a 4-vector Krylov basis of a 5-site chain against the dense
    diagonalisation of H restricted to the same subspace."""
    n = 5
    terms = [[1.0, f'x{i}x{i + 1}'] for i in range(n - 1)] + [[1.0, f'y{i}y{i + 1}'] for i in range(n - 1)]
    terms += [[0.7, f'z{i}z{i + 1}'] for i in range(n - 1)] + [[0.3, f'z{i}'] for i in range(n)] + [[0.25, '']]
    H = dq.PauliSum(terms, n)
    dense = dense_of(H, n)
    assert np.allclose(dense, dense.conj().T)
    basis = [rows(11, 1, n)[0]]
    basis[0] /= np.linalg.norm(basis[0])
    for _ in range(3):
        basis.append(dense @ basis[-1])
    v = np.stack(basis)
    hs, s = H.subspace_matrices(tt(v))
    assert hs.dtype == torch.complex128 and hs.shape == (4, 4) and s.shape == (4, 4)
    np.testing.assert_allclose(s.numpy(), ref.gram_ref(v, v), rtol=1e-13, atol=0)
    np.testing.assert_allclose(hs.numpy(), v.conj() @ dense @ v.T, rtol=1e-12, atol=1e-12)
    assert torch.equal(s, s.mH.resolve_conj())
    low = np.linalg.cholesky(s.numpy())
    inv = np.linalg.inv(low)
    ritz = np.linalg.eigvalsh(inv @ hs.numpy() @ inv.conj().T)
    q, _ = np.linalg.qr(v.T)                             # columns: an orthonormal basis of the span
    want = np.linalg.eigvalsh(q.conj().T @ dense @ q)
    np.testing.assert_allclose(ritz, want, rtol=0, atol=1e-9 * np.abs(want).max())
    exact = np.linalg.eigvalsh(dense)
    assert exact[0] - 1e-9 <= ritz[0] and ritz[-1] <= exact[-1] + 1e-9
    with pytest.raises(ValueError, match='5 qubits'):
        H.subspace_matrices(tt(rows(1, 2, 4)))


def encoder_circuit(n=3):
    cir = dq.QubitCircuit(n)
    cir.rxlayer(encode=True)
    cir.cnot_ring()
    cir.rylayer()
    cir.rzlayer(encode=True)
    cir.cnot_ring()
    cir.to(torch.double)
    return cir


def test_kernel_matrix_against_the_loop_of_inner(cpu_backend):
    torch.manual_seed(3)
    cir = encoder_circuit()
    x1 = torch.randn(4, 6, dtype=torch.float64)
    x2 = torch.randn(3, 6, dtype=torch.float64)
    got = cir.kernel_matrix(x1, x2)
    assert got.dtype == torch.float64 and got.shape == (4, 3)
    with torch.no_grad():
        s1, s2 = cir(x1).reshape(4, -1).clone(), cir(x2).reshape(3, -1).clone()
        want = torch.stack([torch.stack([backend.inner(s1[i:i + 1], s2[j:j + 1])[0].abs() ** 2 for j in range(3)]) for i in range(4)])
    assert (got.detach() - want).abs().max() < 1e-13
    sym = cir.kernel_matrix(x1)
    assert torch.equal(sym, sym.T) and (sym.diagonal() - 1).abs().max() < 1e-13
    assert (cir.kernel_matrix(x1, x1).detach() - sym.detach()).abs().max() < 1e-13
    assert cir.kernel_matrix(x1[0], x2).shape == (1, 3)


def test_kernel_matrix_gradients_against_finite_differences(cpu_backend):
    torch.manual_seed(4)
    cir = encoder_circuit()
    x1 = torch.randn(3, 6, dtype=torch.float64)
    x2 = torch.randn(2, 6, dtype=torch.float64, requires_grad=True)
    weight = torch.randn(3, 2, dtype=torch.float64)
    params = [p for p in cir.parameters() if p.requires_grad]
    assert params

    def loss():
        return (weight * cir.kernel_matrix(x1, x2)).sum()

    grads = torch.autograd.grad(loss(), params + [x2])
    eps = 1e-6
    for p, g in zip(params + [x2], grads):
        flat, fd = p.data.view(-1), torch.zeros(p.numel(), dtype=torch.float64)
        for i in range(p.numel()):
            old = flat[i].item()
            flat[i] = old + eps
            up = loss().item()
            flat[i] = old - eps
            fd[i] = (up - loss().item()) / (2 * eps)
            flat[i] = old
        assert (g.reshape(-1) - fd).abs().max() < 1e-7, (g.reshape(-1), fd)


def test_kernel_matrix_refusals(cpu_backend):
    with pytest.raises(NotImplementedError, match='den_mat=True'):
        dq.QubitCircuit(2, den_mat=True).kernel_matrix(torch.zeros(2, 2))
    plain = dq.QubitCircuit(2)
    plain.rxlayer()
    with pytest.raises(ValueError, match='no encoders'):
        plain.kernel_matrix(torch.zeros(2, 2))
    with pytest.raises(NotImplementedError, match='sharded states are not supported'):
        dq.DistributedQubitCircuit.kernel_matrix(object.__new__(dq.DistributedQubitCircuit), torch.zeros(2, 2))
    with pytest.raises(ValueError, match='data must be'):
        encoder_circuit().kernel_matrix(torch.zeros(2, 2, 6))
