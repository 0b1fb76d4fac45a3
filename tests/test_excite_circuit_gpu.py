"""ExcitationGate / UCCSD inside circuits on the MI355X: against ``cir.pauli_evolution`` of the Pauli strings that the
dense Jordan-Wigner K projects onto, the unitary against the dense closed form, a UCCSD layer (exact zeros outside the
particle-number sector, the dense product, the gradient against central differences), ``torch.vmap`` / ``torch.func.grad``
over the angle, and a trainable gate between two fused stretches."""

import functools

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import ops
from deepquantum_amd.gate import excitation_masks
from _excite_ref import dense_k, dense_u, index_rot, pauli_terms, random_state

pytestmark = pytest.mark.gpu

PREC = {'c64': (torch.float32, torch.complex64, 1e-4), 'c128': (torch.float64, torch.complex128, 1e-10)}


def finish(cir, dt):
    cir.to('cuda')
    if dt == 'c128':
        cir.to(torch.double)
    return cir


def close(got, ref, tol, what=''):
    got, ref = np.asarray(got, dtype=np.complex128), np.asarray(ref, dtype=np.complex128)
    err = np.abs(got - ref).max()
    print(f'{what}: err / (tol * max|ref|) = {err / (tol * np.abs(ref).max()):.3e}')
    assert err <= tol * np.abs(ref).max(), f'{what}: {err:.3e} against {tol} * {np.abs(ref).max():.3e}'


@functools.lru_cache(maxsize=None)
def strings_of(create, annihilate, shift):
    """K = E - E^dagger on the wires of a 6-qubit register as a Hamiltonian for ``pauli_evolution``, its wires shifted by
    ``shift``: K = sum_j c_j P_j with imaginary c_j, so exp(theta K) = exp(-i H theta) for H = sum_j -Im(c_j) P_j (the
    strings commute: one slice is exact)."""
    terms = pauli_terms(dense_k(6, list(create), list(annihilate)), 6)
    assert len(terms) == 2 ** (2 * len(create) - 1) and all(abs(c.real) < 1e-15 for c, _ in terms)
    return [[-c.imag, ''.join(f'{ch}{l + shift}' for l, ch in enumerate(s) if ch != 'i')] for c, s in terms]


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('create,annihilate', [((3, 5), (0, 1)), ((0, 4), (5, 2)), ((4,), (0,)), ((1,), (5,))])
def test_against_pauli_evolution_of_the_projected_strings(create, annihilate, dt):
    n, shift, theta = 10, 2, 0.77
    real, cplx, tol = PREC[dt]
    x = torch.from_numpy(random_state(2, n, 5)).to(cplx).cuda().reshape(2, -1, 1)
    one, many = dq.QubitCircuit(n), dq.QubitCircuit(n)
    one.excitation([w + shift for w in create], [w + shift for w in annihilate], inputs=torch.tensor(theta, dtype=real))
    many.pauli_evolution(strings_of(create, annihilate, shift), t=torch.tensor(theta, dtype=real))
    finish(one, dt)
    finish(many, dt)
    with torch.no_grad():
        got, want = one(state=x), many(state=x)
    close(got.cpu().numpy(), want.cpu().numpy(), tol, f'{create} <- {annihilate} {dt}')
    spec = excitation_masks(n, [w + shift for w in create], [w + shift for w in annihilate])
    ref = index_rot(x.reshape(2, -1).cpu().numpy(), spec, theta if dt == 'c128' else float(np.float32(theta)))
    close(got.reshape(2, -1).cpu().numpy(), ref, tol, f'{create} <- {annihilate} {dt} against the pair formula')


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_unitary_against_the_dense_builder(dt):
    real, _, tol = PREC[dt]
    theta = float(np.float32(-2.1))
    for create, annihilate, controls in (([3, 5], [0, 1], []), ([4], [1], [2]), ([0, 4, 3], [5, 2, 1], [])):
        g = dq.ExcitationGate(create, annihilate, nqubit=6, inputs=torch.tensor(theta, dtype=real), controls=controls)
        finish(g, dt)
        want = dense_u(6, create, annihilate, theta, True, controls)
        close(g.get_unitary().cpu().numpy(), want, tol, f'{create} <- {annihilate} | {controls} {dt}')
        close(g.inverse().get_unitary().cpu().numpy(), want.T, tol, f'{create} <- {annihilate} | {controls} {dt} inverse')


def uccsd_dense(uc, angles):
    n = uc.nqubit
    psi = np.zeros(1 << n)
    psi[((1 << len(uc.doubles[0][:2])) - 1) << (n - 2)] = 1.0
    for wires, th in zip(uc.singles + uc.doubles, angles):
        h = len(wires) // 2
        psi = dense_u(n, wires[h:], wires[:h], th) @ psi
    return psi


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_uccsd_keeps_the_particle_number_exactly_and_matches_the_dense_product(dt):
    real, _, tol = PREC[dt]
    angles = np.random.default_rng(11).uniform(-2.5, 2.5, 14).astype(np.float32).astype(np.float64)
    uc = finish(dq.UCCSD(6, 2, inputs=torch.tensor(angles, dtype=real)), dt)
    assert uc.nparam == 14
    with torch.no_grad():
        got = uc().reshape(-1).cpu().numpy()
    weight = np.array([bin(i).count('1') for i in range(64)])
    assert np.all(got[weight != 2] == 0), 'an amplitude outside the two-particle sector is not exactly 0'
    close(got, uccsd_dense(uc, angles), tol, f'UCCSD(6, 2) {dt}')


def test_uccsd_gradient_against_central_differences():
    angles = np.random.default_rng(12).uniform(-1.5, 1.5, 14)
    uc = dq.UCCSD(6, 2)
    uc.observable(0)
    finish(uc, 'c128')
    params = list(uc.parameters())
    assert len(params) == 14

    def value(vals):
        with torch.no_grad():
            for p, v in zip(params, vals):
                p.copy_(torch.tensor(v, dtype=torch.float64))
            uc()
            return float(uc.expectation().sum())

    with torch.no_grad():
        for p, v in zip(params, angles):
            p.copy_(torch.tensor(v, dtype=torch.float64))
    uc()
    uc.expectation().sum().backward()
    grad = np.array([float(p.grad) for p in params])
    # <Z_0> is the dense expectation as well
    psi = uccsd_dense(uc, angles)
    z0 = np.array([1.0 - 2.0 * ((i >> 5) & 1) for i in range(64)])
    assert abs(value(angles) - float(psi @ (z0 * psi))) < 1e-12
    h = 1e-4
    for k in range(14):
        up, down = angles.copy(), angles.copy()
        up[k] += h
        down[k] -= h
        fd = (value(up) - value(down)) / (2 * h)
        print(f'theta[{k}]: backward {grad[k]:+.9f}, central difference {fd:+.9f}')
        assert abs(grad[k] - fd) <= 1e-6


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_vmap_and_func_grad_over_the_angle(dt):
    real, cplx, tol = PREC[dt]
    n = 8
    spec = (*excitation_masks(n, [6, 2], [0, 5], True, [3]), (n - 1 - 3,))
    x = torch.from_numpy(random_state(2, n, 9)).to(cplx).cuda()
    thetas = torch.tensor([[0.3, -0.9], [1.7, 0.2], [-2.8, 3.6]], dtype=torch.float64, device='cuda')
    got = torch.vmap(lambda p: ops.excite_rot(x, spec, p))(thetas)
    for v in range(3):
        ref = index_rot(x.cpu().numpy(), spec, thetas[v].cpu().numpy().reshape(-1, 1))
        close(got[v].cpu().numpy(), ref, tol, f'vmap row {v} {dt}')

    def loss(p):
        return (ops.excite_rot(x, spec, p)[:, 5::7].abs() ** 2).sum()

    g = torch.func.grad(loss)(thetas[0])
    h = 1e-3 if dt == 'c64' else 1e-5
    for b in range(2):
        e = torch.zeros(2, dtype=torch.float64, device='cuda')
        e[b] = h
        fd = float(loss(thetas[0] + e) - loss(thetas[0] - e)) / (2 * h)
        assert abs(float(g[b]) - fd) <= (2e-3 if dt == 'c64' else 1e-8), (float(g[b]), fd)
    rows = torch.vmap(torch.func.grad(loss))(thetas)
    assert torch.allclose(rows[0], g, atol=1e-5 if dt == 'c64' else 1e-12)


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_a_trainable_gate_between_two_fused_stretches(dt):
    real, cplx, tol = PREC[dt]
    n = 7
    rng = np.random.default_rng(21)
    before, after = rng.uniform(-2, 2, n).astype(np.float32), rng.uniform(-2, 2, n).astype(np.float32)
    theta = float(np.float32(0.61))

    def build(middle):
        cir = dq.QubitCircuit(n)
        cir.rylayer(inputs=torch.tensor(before))
        cir.cnot_ring()
        middle(cir)
        cir.rxlayer(inputs=torch.tensor(after))
        cir.cnot_ring()
        cir.observable(0)
        return finish(cir, dt)

    cir = build(lambda c: c.double_excitation([1, 4, 2, 6]))
    (gate,) = [op for op in cir.operators if isinstance(op, dq.ExcitationGate)]
    assert isinstance(gate.theta, torch.nn.Parameter)
    with torch.no_grad():
        gate.theta.copy_(torch.tensor(theta, dtype=real))
    state = cir()
    cir.expectation().sum().backward()
    assert gate.theta.grad is not None and torch.isfinite(gate.theta.grad).all()
    # the same circuit with the gate as a dense matrix on the state between the stretches
    first, second = dq.QubitCircuit(n), dq.QubitCircuit(n)
    first.rylayer(inputs=torch.tensor(before))
    first.cnot_ring()
    second.rxlayer(inputs=torch.tensor(after))
    second.cnot_ring()
    finish(first, dt)
    finish(second, dt)
    with torch.no_grad():
        mid = first().reshape(-1).cpu().numpy().astype(np.complex128)
        mid = dense_u(n, [2, 6], [1, 4], theta) @ mid
        want = second(state=torch.from_numpy(mid).to(cplx).cuda().reshape(1, -1, 1)).reshape(-1).cpu().numpy()
    close(state.detach().reshape(-1).cpu().numpy(), want, tol, f'between fused stretches {dt}')
    # the angle's gradient against a central difference of the expectation value
    def value(t):
        with torch.no_grad():
            gate.theta.copy_(torch.tensor(t, dtype=real))
            cir()
            return float(cir.expectation().sum())

    h = 1e-2 if dt == 'c64' else 1e-5
    fd = (value(theta + h) - value(theta - h)) / (2 * h)
    assert abs(float(gate.theta.grad) - fd) <= (1e-3 if dt == 'c64' else 1e-8), (float(gate.theta.grad), fd)
