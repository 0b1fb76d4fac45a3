"""k-wire reduced density matrices and entanglement entropy on the MI355X (``dq_rdmk_cross_*``): the kernel against an
explicit complex128 einsum over wire sets, controls and both routes (also element by element against tau * S, the
criterion of test_rdmk_paths_gpu.py, which takes the kernel path by path), exact Hermiticity and reproducibility, the
reference's fixtures, known answers at 26 qubits, derivatives, the routing of ``backend.gate_grad`` and its GEMM
fallback above ten wires, memory and graph capture."""

import math
import os
import random
import sys

import numpy as np
import pytest
import torch

import _grid_refs as R
import deepquantum_amd as dq
from _rdmk_cases import TAU_C64, TAU_SUM
from deepquantum_amd import backend, ops, qmath

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
from make_golden_entanglement import circuit_data, entangling_circuit  # noqa: E402
from make_golden_rdm import SIZES, WIRE_SETS, wires_key  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, 'golden', 'golden_rdm.npz')
TOL = {torch.complex64: 1e-5, torch.complex128: 1e-10}
DEV = 'cuda'


def explicit_cross(x, gy, targets, controls=()):
    """sum over the controlled groups of gy[a] conj(x[c]) in complex128 (matrix MSB = targets[0]), by an index gather."""
    b, dim = x.shape
    n = dim.bit_length() - 1
    k = len(targets)
    rest = [p for p in range(n) if p not in targets and p not in controls]

    def dep(v, bits):          # bit i of v (MSB first over `bits`) -> index bit bits[i]
        out = torch.zeros_like(v)
        for i, p in enumerate(bits):
            out |= ((v >> (len(bits) - 1 - i)) & 1) << p
        return out

    cm = sum(1 << c for c in controls)
    a = dep(torch.arange(1 << k, device=x.device), list(targets))
    r = dep(torch.arange(1 << len(rest), device=x.device), rest[::-1])
    idx = (a[:, None] | r[None, :] | cm).reshape(-1)

    def mat(t):
        return t.to(torch.complex128)[:, idx].reshape(b, 1 << k, -1)

    return mat(gy) @ mat(x).mH


def rand_state(b, n, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.view_as_complex(torch.randn(b, 1 << n, 2, generator=g, device=DEV, dtype=torch.float64))
    return (x / x.norm(dim=-1, keepdim=True)).to(dtype)


def wire_sets(n, k, rng):
    """The lowest bits, the highest bits, a scattered set holding bit 0, and an unsorted one (as target bit lists)."""
    sets = [list(range(k - 1, -1, -1)), list(range(n - 1, n - 1 - k, -1))]
    if n > k:
        s = sorted(rng.sample(range(1, n), k - 1) + [0], reverse=True)
        sets.append(s)
        u = rng.sample(range(n), k)
        sets.append(u)
    return sets


def _cases():
    rng = random.Random(5)
    out = []
    for k in range(3, 11):
        for n in sorted({k, k + 1, 12, 20}):
            if n < k:
                continue
            for tg in wire_sets(n, k, rng):
                free = [p for p in range(n) if p not in tg]
                nc = min(len(free), rng.choice((0, 1, 2)))
                out.append((n, tg, rng.sample(free, nc), rng.choice((1, 3)), rng.random() < 0.5))
    return out


def _check(got, ref, dtype, x, gy, what):
    scale = (x.abs().pow(2).sum(-1).sqrt() * gy.abs().pow(2).sum(-1).sqrt()).max().item()
    err = (got - ref).abs().max().item()
    assert err <= TOL[dtype] * max(scale, 1e-30), f'{what}: error {err:.3e} (scale {scale:.3e})'


def _check_elementwise(got, x, gy, tg, ctl, dtype, what):
    """|got - ref| <= tau * S element by element, S the same sum over |gy| |x| (the criterion of test_rdmk_paths_gpu.py,
    whose _rdmk_cases.py derives the complex64 figure)."""
    ref, s = R.cross(x, gy, tg, ctl)
    tau = TAU_C64 if dtype == torch.complex64 else TAU_SUM
    err = (got - ref).abs()
    assert (err <= tau * s).all(), f'{what}: max |got - ref| / S = {float((err / s).max()):.3e} (tau {tau:.0e})'
    return float((err / s).max())


@pytest.mark.parametrize('dtype', [torch.complex64, torch.complex128])
def test_kernel_against_explicit_einsum(dtype):
    for i, (n, tg, ctl, b, same) in enumerate(_cases()):
        x = rand_state(b, n, dtype, seed=10 + i)
        gy = x if same else rand_state(b, n, dtype, seed=1000 + i)
        got = backend.rdmk_cross(x, gy, tg, ctl)
        assert got.dtype == torch.complex128 and got.shape == (b, 1 << len(tg), 1 << len(tg))
        what = f'n={n} targets={tg} controls={ctl} b={b} same={same}'
        _check(got, explicit_cross(x, gy, tg, ctl), dtype, x, gy, what)
        _check_elementwise(got, x, gy, tg, ctl, dtype, what)


def test_hermitian_exact_and_reproducible():
    n, k = 20, 6
    psi = rand_state(2, n, torch.complex64, seed=2)
    tg = [19, 3, 0, 11, 7, 14]
    a = backend.rdmk_cross(psi, psi, tg)
    b = backend.rdmk_cross(psi, psi, tg)
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(a.mH.resolve_conj()))
    gy = rand_state(2, n, torch.complex64, seed=3)
    c = backend.rdmk_cross(psi, gy, tg, [5])
    d = backend.rdmk_cross(psi, gy, tg, [5])
    assert torch.equal(torch.view_as_real(c), torch.view_as_real(d))
    rho = qmath.reduced_density_matrix(psi.reshape([2] + [2] * n), n, [0, 5, 13])
    assert torch.equal(torch.view_as_real(rho), torch.view_as_real(rho.mH.resolve_conj()))
    assert rho.shape == (2, 8, 8) and rho.dtype == torch.complex64


def test_reference_fixtures():
    z = np.load(GOLDEN)
    for n in SIZES:
        for prec in ('c64', 'c128'):
            dtype = torch.complex128 if prec == 'c128' else torch.complex64
            st = torch.from_numpy(z[f'{n}/{prec}/state']).to(DEV)
            tr = float(z[f'{n}/{prec}/norm'][0])
            for wires in WIRE_SETS[n]:
                ref = z[f'{n}/{prec}/rdm/{wires_key(wires)}'][0]
                got = qmath.reduced_density_matrix(st, n, wires)
                assert got.dtype == dtype and got.shape == (1,) + ref.shape
                got = got[0]
                tol = TOL[dtype] * 10 if dtype == torch.complex64 else 1e-9
                np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=0, atol=tol * tr)
                np.testing.assert_allclose(np.trace(got.cpu().numpy()).real, tr, rtol=tol)


def test_known_answers_at_26_qubits():
    n = 26
    ghz = torch.zeros(1 << n, dtype=torch.complex64, device=DEV)
    ghz[0] = ghz[-1] = 1 / math.sqrt(2)
    for k in (3, 10):
        wires = list(range(5, 5 + k))
        rho = qmath.reduced_density_matrix(ghz, n, wires)
        ref = torch.zeros(1 << k, 1 << k, dtype=torch.complex64, device=DEV)
        ref[0, 0] = ref[-1, -1] = 0.5
        torch.testing.assert_close(rho, ref, rtol=0, atol=1e-6)
        s = qmath.entanglement_entropy(ghz, n, wires)
        assert s.ndim == 0 and abs(s.item() - math.log(2)) < 1e-5
    del ghz
    # a product state: no entanglement across any cut
    g = torch.Generator().manual_seed(4)
    qs = [torch.view_as_complex(torch.randn(2, 2, generator=g, dtype=torch.float64)) for _ in range(n)]
    prod = qs[0] / qs[0].norm()
    for q in qs[1:]:
        prod = torch.kron(prod, q / q.norm())
    prod = prod.to(torch.complex64).to(DEV)
    for wires in ([0, 1, 2], [3, 9, 17, 25], list(range(8, 18))):
        assert abs(qmath.entanglement_entropy(prod, n, wires).item()) < 1e-4
    del prod
    # m Bell pairs straddling the cut of 8 wires
    m, a = 3, [0, 2, 4, 6, 8, 10, 12, 14]
    cir = dq.QubitCircuit(n)
    for i in range(m):
        cir.h(a[i])
        cir.cnot(a[i], 20 + i)
    cir.cnot(a[5], a[6])          # entanglement inside A adds nothing
    cir.to(DEV)
    with torch.no_grad():
        cir()
    s = cir.entanglement_entropy(a)
    assert abs(s.item() - m * math.log(2)) < 1e-4
    assert abs(cir.entanglement_entropy(a, base=2).item() - m) < 1e-4
    assert abs(cir.entanglement_entropy(a, alpha=2).item() - m * math.log(2)) < 1e-4


def test_derivatives():
    for k in (3, 4):
        psi = rand_state(1, 6, torch.complex128, seed=k).requires_grad_(True)
        wires = [4, 1, 2, 5][:k]
        f = lambda p: qmath.reduced_density_matrix(p, 6, wires)      # noqa: E731
        assert torch.autograd.gradcheck(f, (psi,), eps=1e-6, atol=1e-7)
        assert torch.autograd.gradgradcheck(f, (psi,), eps=1e-6, atol=1e-6)
    # d S / d (circuit inputs) against central differences, n = 8
    n, wires = 8, [0, 3, 5]
    cir = entangling_circuit(dq, n)
    cir.to(DEV)
    cir.to(torch.double)
    data = circuit_data(n, 1, seed=9).to(DEV)
    x = data.clone().requires_grad_(True)
    s = qmath.entanglement_entropy(cir(data=x), n, wires)
    (g,) = torch.autograd.grad(s.sum(), x)
    h = 1e-5
    with torch.no_grad():
        for j in (0, 5, 11, 15):
            d1, d2 = data.clone(), data.clone()
            d1[0, j] += h
            d2[0, j] -= h
            fd = (qmath.entanglement_entropy(cir(data=d1), n, wires) - qmath.entanglement_entropy(cir(data=d2), n, wires)) / (2 * h)
            assert abs(fd.item() - g[0, j].item()) < 1e-6, (j, fd.item(), g[0, j].item())
    # torch.func over the circuit
    xs = circuit_data(n, 3, seed=1).to(DEV)

    def fs(v):
        return qmath.entanglement_entropy(cir(data=v.unsqueeze(0)), n, wires)[0]

    xb = xs.clone().requires_grad_(True)
    batched = qmath.entanglement_entropy(cir(data=xb), n, wires)
    (gb,) = torch.autograd.grad(batched.sum(), xb)
    torch.testing.assert_close(torch.vmap(fs)(xs), batched.detach(), rtol=1e-9, atol=1e-11)
    torch.testing.assert_close(torch.func.jacrev(fs)(xs[0]), gb[0], rtol=1e-8, atol=1e-10)
    rv = torch.vmap(lambda v: qmath.reduced_density_matrix(cir(data=v.unsqueeze(0)), n, [1, 6, 2])[0])(xs)
    torch.testing.assert_close(rv, qmath.reduced_density_matrix(cir(data=xs), n, [1, 6, 2]), rtol=1e-10, atol=1e-12)


def test_routing_never_needs_the_gemm_fallback(monkeypatch):
    n = 13
    x = rand_state(2, n, torch.complex64, seed=21)
    gy = rand_state(2, n, torch.complex64, seed=22)
    refs = {}
    for k in range(3, 11):
        tg = list(range(n - 1, n - 1 - k, -1))[::-1]
        ctl = [0] if k < 10 else []
        refs[k] = (tg, ctl, backend._gate_grad_gemm(x, gy, n, tg, ctl))

    def refuse(*a, **kw):
        raise AssertionError('the GEMM fallback ran')

    monkeypatch.setattr(backend, '_gate_grad_gemm', refuse)
    for k, (tg, ctl, ref) in refs.items():
        got = backend.gate_grad(x, gy, tg, ctl)
        _check(got, ref.to(torch.complex128), torch.complex64, x, gy, f'gate_grad k={k}')
        wires = [n - 1 - t for t in tg]
        rho = qmath.reduced_density_matrix(x, n, wires)
        _check(rho.to(torch.complex128), explicit_cross(x, x, tg), torch.complex64, x, x, f'rdm k={k}')


@pytest.mark.parametrize('dtype', [torch.complex64, torch.complex128])
def test_gemm_fallback_above_ten_wires(dtype, monkeypatch):
    """k = 11 with a control at n = 14: ``backend.gate_grad`` hands it to ``_gate_grad_gemm`` (asserted), which is held to
    the reference and the criteria of the matrix-core route.  K = 4: a complex64 GEMM of four terms rounds at a few 2^-24
    of S, inside TAU_C64."""
    n, tg, ctl = 14, [13, 2, 7, 0, 11, 4, 9, 1, 12, 6, 3], [8]
    x, gy = rand_state(2, n, dtype, seed=31), rand_state(2, n, dtype, seed=32)
    calls, gemm = [], backend._gate_grad_gemm
    monkeypatch.setattr(backend, '_gate_grad_gemm', lambda *a: calls.append(1) or gemm(*a))
    got = backend.gate_grad(x, gy, tg, ctl)
    assert calls == [1] and got.dtype == torch.complex128 and got.shape == (2, 2048, 2048)
    _check(got, explicit_cross(x, gy, tg, ctl), dtype, x, gy, f'gemm fallback {dtype}')
    worst = _check_elementwise(got, x, gy, tg, ctl, dtype, f'gemm fallback {dtype}')
    print(f'gemm fallback, k = 11, {dtype}: worst |got - ref| / S = {worst:.3e}')


def test_workspace_budget_at_26_qubits():
    n = 26
    psi = rand_state(1, n, torch.complex64, seed=7)
    state_bytes = psi.numel() * psi.element_size()
    for k, same in ((4, True), (10, True), (10, False)):
        gy = psi if same else psi.clone()
        tg = list(range(3, 3 + k))
        out_bytes = 16 << (2 * k)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        backend.rdmk_cross(psi, gy, tg)
        torch.cuda.synchronize()
        grew = torch.cuda.max_memory_allocated() - before
        assert grew < 0.01 * state_bytes + 2 * out_bytes, (k, same, grew)
        del gy


def test_captured_graph_replays_the_eager_value():
    n = 14
    psi = rand_state(4, n, torch.complex64, seed=6).reshape([4] + [2] * n)
    eager = qmath.reduced_density_matrix(psi, n, [2, 7, 0, 11])
    graph = dq.CapturedGraph(lambda: qmath.reduced_density_matrix(psi, n, [2, 7, 0, 11]))
    for _ in range(2):
        out = graph.replay()
        torch.testing.assert_close(out, eager, rtol=0, atol=0)
