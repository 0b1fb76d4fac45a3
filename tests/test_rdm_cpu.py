"""k-wire reduced density matrices and entanglement entropy, host side (no GPU): input forms and shapes, wire order,
equality with ``partial_trace(psi psi^dagger)``, the error paths, entropies against numpy eigenvalues, the density-
matrix circuit route and the reference fixture's self-consistency -- on the oracle-backed CPU double, whose
``gate_grad`` handles any k."""

import math
import os
import sys

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import qmath
from deepquantum_amd.state import DistributedQubitState

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
from make_golden_rdm import SIZES, WIRE_SETS, wires_key  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_rdm.npz')


def rand_state(b, n, dtype=torch.complex128, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.view_as_complex(torch.randn(b, 1 << n, 2, generator=g, dtype=torch.float64))
    return (x / x.norm(dim=-1, keepdim=True)).to(dtype)


def ptrace_ref(psi, n, wires):
    """partial_trace(psi psi^dagger, n, complement) for sorted wires: (B, 2^k, 2^k) complex128."""
    psi = psi.to(torch.complex128)
    rho = psi.reshape(psi.shape[0], -1, 1) @ psi.conj().reshape(psi.shape[0], 1, -1)
    red = qmath.partial_trace(rho, n, [w for w in range(n) if w not in wires])
    k = len(wires)
    return red.reshape(-1, 1 << k, 1 << k)


def np_entropy(rho, alpha=1.0):
    lam = np.linalg.eigvalsh(rho / np.trace(rho).real)
    lam = lam[lam > 1e-12]
    if alpha == 1:
        return float(-(lam * np.log(lam)).sum())
    return float(np.log((lam**alpha).sum()) / (1 - alpha))


def test_shapes_for_every_input_form(cpu_backend):
    n = 5
    psi = rand_state(3, n)
    ref = ptrace_ref(psi, n, [1, 3])
    for st, single in ((psi[0], True), (psi[0].reshape(-1, 1), True), (psi, False), (psi.reshape(3, -1, 1), False),
                       (psi.reshape([3] + [2] * n), False)):
        got = qmath.reduced_density_matrix(st, n, [1, 3])
        if single:
            assert got.shape == (4, 4)
            torch.testing.assert_close(got, ref[0], rtol=0, atol=1e-12)
        else:
            assert got.shape == (3, 4, 4)
            torch.testing.assert_close(got, ref, rtol=0, atol=1e-12)
        assert got.dtype == torch.complex128
    got = qmath.reduced_density_matrix(psi.to(torch.complex64), n, 2)
    assert got.shape == (3, 2, 2) and got.dtype == torch.complex64
    s = qmath.entanglement_entropy(psi[0], n, [0, 1])
    assert s.ndim == 0 and s.dtype == torch.float64
    s = qmath.entanglement_entropy(psi.to(torch.complex64), n, [0, 1])
    assert s.shape == (3,) and s.dtype == torch.float32


@pytest.mark.parametrize('k', [1, 2, 3, 4, 6])
def test_equals_partial_trace_and_follows_wire_order(cpu_backend, k):
    n = 7
    psi = rand_state(2, n, seed=k)
    wires = sorted(np.random.default_rng(k).choice(n, k, replace=False).tolist())
    rho = qmath.reduced_density_matrix(psi, n, wires)
    torch.testing.assert_close(rho, ptrace_ref(psi, n, wires), rtol=0, atol=1e-12)
    torch.testing.assert_close(rho.diagonal(dim1=-2, dim2=-1).sum(-1).real, torch.ones(2, dtype=torch.float64))
    perm = np.random.default_rng(10 + k).permutation(k).tolist()
    got = qmath.reduced_density_matrix(psi, n, [wires[p] for p in perm])
    want = rho.reshape([2] + [2] * (2 * k)).permute([0] + [1 + p for p in perm] + [1 + k + p for p in perm])
    torch.testing.assert_close(got, want.reshape(2, 1 << k, 1 << k), rtol=0, atol=1e-12)


def test_whole_register_gives_the_projector(cpu_backend):
    n = 3
    psi = rand_state(1, n, seed=2)
    rho = qmath.reduced_density_matrix(psi[0] * 2, n, [0, 1, 2])
    torch.testing.assert_close(rho, 4 * psi[0][:, None] * psi[0].conj()[None, :], rtol=0, atol=1e-12)
    assert abs(qmath.entanglement_entropy(psi[0], n, [0, 1, 2]).item()) == 0.0


def test_errors(cpu_backend):
    psi = rand_state(2, 4)
    for wires in ([], [0, 0], [4], [-1], 'x'):
        with pytest.raises(ValueError):
            qmath.reduced_density_matrix(psi, 4, wires)
    with pytest.raises(ValueError):
        qmath.reduced_density_matrix(rand_state(1, 11)[0], 11, list(range(11)))
    with pytest.raises(ValueError):
        qmath.reduced_density_matrix(psi, 5, [0])
    with pytest.raises(ValueError):
        qmath.reduced_density_matrix(psi.reshape(2, 4, 4), 4, [0])
    with pytest.raises(ValueError):
        qmath.entanglement_entropy(rand_state(1, 22)[0], 22, list(range(11)))
    with pytest.raises(ValueError):
        qmath.entanglement_entropy(psi, 4, [0], alpha=0)
    shard = DistributedQubitState.__new__(DistributedQubitState)
    with pytest.raises(NotImplementedError):
        qmath.reduced_density_matrix(shard, 4, [0])
    with pytest.raises(NotImplementedError):
        qmath.entanglement_entropy(shard, 4, [0])


def test_cpu_tensor_without_backend_has_no_fallback():
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        qmath.reduced_density_matrix(rand_state(1, 4), 4, [0, 1, 2])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        qmath.entanglement_entropy(rand_state(1, 4), 4, [0, 1])


def test_entropies_against_numpy(cpu_backend):
    n = 8
    psi = rand_state(3, n, seed=4)
    for wires in ([0], [1, 5], [0, 2, 3], [0, 1, 2, 3, 4, 5]):
        side = wires if len(wires) <= n - len(wires) else [w for w in range(n) if w not in wires]
        rhos = ptrace_ref(psi, n, sorted(side)).numpy()
        for alpha in (1.0, 2.0, 0.5, 3.0):
            got = qmath.entanglement_entropy(psi, n, wires, alpha=alpha)
            ref = [np_entropy(r, alpha) for r in rhos]
            np.testing.assert_allclose(got.numpy(), ref, rtol=1e-9, atol=1e-12)
        # the complement trick: both sides of the cut agree with the direct eigenvalues of the other side
        comp = [w for w in range(n) if w not in wires]
        direct = [np_entropy(r) for r in ptrace_ref(psi, n, sorted(wires)).numpy()]
        np.testing.assert_allclose(qmath.entanglement_entropy(psi, n, comp).numpy(), direct, rtol=1e-9, atol=1e-12)
        # alpha = 2 by the Frobenius norm equals the eigenvalue form
        lam2 = [-math.log(np.sum(np.linalg.eigvalsh(r / np.trace(r).real) ** 2)) for r in rhos]
        np.testing.assert_allclose(qmath.entanglement_entropy(psi, n, wires, alpha=2).numpy(), lam2, rtol=1e-9)
        np.testing.assert_allclose(qmath.entanglement_entropy(psi, n, wires, base=2).numpy(),
                                   np.asarray(direct) / math.log(2), rtol=1e-9, atol=1e-12)
    # un-normalised input: the entropy of rho / Tr rho
    np.testing.assert_allclose(qmath.entanglement_entropy(psi * 3, n, [1, 2]).numpy(),
                               qmath.entanglement_entropy(psi, n, [1, 2]).numpy(), rtol=1e-9)


def test_circuit_methods(cpu_backend):
    n = 5
    cir = dq.QubitCircuit(n)
    cir.hlayer()
    cir.rylayer()
    cir.cnot_ring()
    cir()
    psi = cir.state.reshape(1, -1)
    torch.testing.assert_close(cir.reduced_density_matrix([3, 0]), qmath.reduced_density_matrix(psi, n, [3, 0])[0])
    s = cir.entanglement_entropy([0, 1])
    assert s.ndim == 0 and abs(s.item() - qmath.entanglement_entropy(psi, n, [0, 1])[0].item()) < 1e-12
    # the density-matrix route: partial_trace permuted to the order of the wires, no complement
    dm = dq.QubitCircuit(n, den_mat=True)
    dm.hlayer()
    dm.rylayer()
    dm.cnot_ring()
    for w in range(n):
        dm.rx(w, 0.3)
    dm()
    rho = dm.state
    red = qmath.partial_trace(rho, n, [1, 2, 4])
    got = dm.reduced_density_matrix([3, 0])
    want = red.reshape(2, 2, 2, 2).permute(1, 0, 3, 2).reshape(4, 4)
    torch.testing.assert_close(got, want)
    ref = np_entropy(red.detach().numpy())
    assert abs(dm.entanglement_entropy([0, 3]).item() - ref) < 1e-5
    with pytest.raises(NotImplementedError):
        dq.DistributedQubitCircuit.reduced_density_matrix(None, [0])
    with pytest.raises(NotImplementedError):
        dq.DistributedQubitCircuit.entanglement_entropy(None, [0])


def test_fixture_is_consistent():
    z = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 300 * 1024
    for n in SIZES:
        for prec in ('c64', 'c128'):
            st = z[f'{n}/{prec}/state'].astype(np.complex128)
            assert st.shape == (1, 1 << n)
            np.testing.assert_allclose(z[f'{n}/{prec}/norm'], [np.vdot(st[0], st[0]).real], rtol=1e-6)
            for wires in WIRE_SETS[n]:
                rho = z[f'{n}/{prec}/rdm/{wires_key(wires)}'][0]
                k = len(wires)
                assert rho.shape == (1 << k, 1 << k)
                np.testing.assert_allclose(rho, rho.conj().T, atol=1e-6)
                np.testing.assert_allclose(np.trace(rho).real, z[f'{n}/{prec}/norm'][0], rtol=1e-5)
                ref = ptrace_ref(torch.from_numpy(st), n, wires)[0].numpy()
                np.testing.assert_allclose(rho, ref, atol=1e-5 if prec == 'c64' else 1e-12)
