"""PauliRot / PauliEvolution inside circuits on the MI355X: against fixtures made with the reference's HamiltonianGate,
against this package's HamiltonianGate and the hand decomposition (basis change, CNOT ladder, rz), the unitary and the
inverse, encoded batches, a string no dense route reaches, the Trotter products, and what is refused."""

import os
import sys

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from _pauli_ref import dense_pauli, masks_of, rot_ref

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
from make_golden_entanglement import entangling_circuit  # noqa: E402
from make_golden_pauli import SIZES, VARIANTS, gates_of  # noqa: E402

pytestmark = pytest.mark.gpu

PREC = {'c64': (torch.float32, 1e-4), 'c128': (torch.float64, 1e-10)}
GOLDEN = np.load(os.path.join(HERE, 'golden', 'golden_pauli.npz'))


def split(s):
    """'x0y13z5' -> ('xyz', [0, 13, 5])"""
    import re

    pairs = re.findall(r'([xyz])(\d+)', s)
    return ''.join(p for p, _ in pairs), [int(w) for _, w in pairs]


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


def rotations(n, variant, route):
    """The three gates of a fixture as a circuit of this package: ``route`` 'pauli' (cir.pauli_rot) or 'dense'
    (HamiltonianGate with t = theta / 2, a dense matrix on the string's span)."""
    rots = dq.QubitCircuit(n)
    for s, theta, controls in gates_of(n, 'ctrl' if variant == 'ctrl' else 'plain'):
        if route == 'pauli':
            letters, wires = split(s)
            rots.pauli_rot(letters, wires=wires, inputs=theta, controls=controls)
        else:
            rots.hamiltonian([[1.0, s]], t=theta / 2, controls=controls)
    return rots.inverse() if variant == 'inv' else rots


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('n', SIZES)
def test_pauli_rot_against_the_reference_fixture_and_the_dense_route(n, variant, dt):
    real, tol = PREC[dt]
    data = torch.from_numpy(GOLDEN[f'{n}/{dt}/data']).to(real).cuda()
    states = {}
    for route in ('pauli', 'dense'):
        cir = entangling_circuit(dq, n)
        cir += rotations(n, variant, route)
        finish(cir, dt)
        with torch.no_grad():
            states[route] = cir(data=data).reshape(-1).cpu().numpy()
    close(states['pauli'], GOLDEN[f'{n}/{dt}/{variant}'].reshape(-1), tol, f'fixture n={n} {variant} {dt}')
    close(states['pauli'], states['dense'], tol, f'HamiltonianGate n={n} {variant} {dt}')


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_against_the_hand_decomposition(dt):
    """exp(-i theta/2 P) = B^dagger L^dagger rz(theta) L B with B the basis change (h for x, sdg then h for y) and L the CNOT
    ladder onto the last wire of the string."""
    n, theta, tol = 10, 0.9375, PREC[dt][1]
    letters, wires = 'xyzyx', [1, 4, 5, 7, 8]

    def prefix():
        cir = dq.QubitCircuit(n)
        cir.hlayer()
        cir.rylayer(inputs=[0.2 * (i + 1) for i in range(n)])
        cir.cnot_ring()
        return cir

    by_hand = prefix()
    for ch, w in zip(letters, wires):
        if ch == 'y':
            by_hand.sdg(w)
        if ch in 'xy':
            by_hand.h(w)
    for a, b in zip(wires[:-1], wires[1:]):
        by_hand.cnot(a, b)
    by_hand.rz(wires[-1], inputs=theta)
    for a, b in reversed(list(zip(wires[:-1], wires[1:]))):
        by_hand.cnot(a, b)
    for ch, w in zip(letters, wires):
        if ch in 'xy':
            by_hand.h(w)
        if ch == 'y':
            by_hand.s(w)
    one_pass = prefix()
    one_pass.pauli_rot(letters, wires=wires, inputs=theta)
    with torch.no_grad():
        a = finish(by_hand, dt)().reshape(-1).cpu().numpy()
        b = finish(one_pass, dt)().reshape(-1).cpu().numpy()
    # (h is float32-rounded in the library: four h h pairs of the hand route are 1 to 1e-7 only)
    close(b, a, max(tol, 1e-6), f'hand decomposition {dt}')


def test_get_unitary_against_the_dense_matrix():
    n, theta = 4, 0.9375
    for letters, wires, controls in (('yzx', [2, 0, 3], None), ('xy', [3, 1], [0]), ('z', [2], None)):
        cir = dq.QubitCircuit(n)
        cir.pauli_rot(letters, wires=wires, inputs=theta, controls=controls)
        finish(cir, 'c128')
        p = dense_pauli(n, letters, wires)
        dense = np.cos(theta / 2) * np.eye(1 << n) - 1j * np.sin(theta / 2) * p
        if controls:
            on = ((np.arange(1 << n) >> (n - 1 - controls[0])) & 1) == 1
            dense = np.where(on[:, None], dense, np.eye(1 << n))
        close(cir.get_unitary().cpu().numpy(), dense, 1e-10, f'unitary {letters}')
        close(cir.operators[0].get_unitary().cpu().numpy(), dense, 1e-10, f'gate unitary {letters}')
        close(cir.operators[0].inverse().get_unitary().cpu().numpy(), dense.conj().T, 1e-10, f'inverse unitary {letters}')


def test_inverse_composes_to_the_identity():
    n = 5
    cir = dq.QubitCircuit(n)
    cir.pauli_rot('xyz', wires=[4, 0, 2], inputs=0.7)
    cir.pauli_rot('yy', wires=[1, 3], inputs=-1.9, controls=[0])
    cir.pauli_evolution([[0.8, 'x0z2'], [-0.6, 'y2'], [0.3, 'z0y1x3']], t=0.4, steps=2, order=1)
    cir.pauli_evolution([[0.8, 'x0z2'], [-0.6, 'y2'], [0.3, 'z0y1x4']], t=-0.7, steps=2, order=2)
    finish(cir, 'c128')
    both = cir + cir.inverse()
    close(both.get_unitary().cpu().numpy(), np.eye(1 << n), 1e-10, 'circuit + inverse')
    x = torch.randn(1 << n, 1, dtype=torch.complex128, generator=torch.Generator().manual_seed(3)).cuda()
    with torch.no_grad():
        back = cir.inverse()(state=cir(state=x))
    close(back.cpu().numpy(), x.cpu().numpy(), 1e-10, 'inverse(state)')


def test_encoded_batch_equals_single_runs():
    n = 4
    cir = dq.QubitCircuit(n)
    cir.hlayer()
    cir.pauli_rot('xyx', wires=[3, 0, 1], encode=True)
    cir.rxlayer(inputs=[0.3] * n)
    cir.observable(0)
    finish(cir, 'c128')
    assert cir.ndata == 1 and cir.encoders == [cir.operators[n]]
    data = torch.tensor([[0.1], [0.7], [-1.3]], dtype=torch.float64, device='cuda', requires_grad=True)
    batch = cir(data)
    assert batch.shape == (3, 1 << n, 1)
    cir.expectation().sum().backward()
    singles, grads = [], []
    for b in range(3):
        one = data.detach()[b].clone().requires_grad_()
        singles.append(cir(one).detach())
        cir.expectation().sum().backward()
        grads.append(one.grad)
    assert (batch.detach() - torch.stack(singles)).abs().max().item() < 1e-12
    assert (data.grad - torch.stack(grads)).abs().max().item() < 1e-10
    assert data.grad.abs().min().item() > 1e-3


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_weight_20_string_on_22_qubits(dt):
    """What no dense route reaches: the rotation applied by the numpy formula to the state in front of it."""
    n, theta = 22, 0.8125
    wires = [w for w in range(n) if w not in (3, 17)]
    letters = ('xyzzyx' * 4)[:20]
    front = dq.QubitCircuit(n)
    front.hlayer()
    front.rylayer(inputs=[0.1 * (i + 1) for i in range(n)])
    front.cnot_ring()
    whole = dq.QubitCircuit(n)
    whole += front
    whole.pauli_rot(letters, wires=wires, inputs=theta, controls=[17])
    with torch.no_grad():
        before = finish(front, dt)().reshape(1, -1).cpu().numpy()
        after = finish(whole, dt)().reshape(1, -1).cpu().numpy()
    xmask, zmask = masks_of(n, letters, wires)
    assert bin(xmask | zmask).count('1') == 20
    ref = rot_ref(before, xmask, zmask, theta, controls=(n - 1 - 17,))
    assert np.abs(ref - before).max() > 1e-4
    close(after, ref, PREC[dt][1], f'weight 20 on 22 qubits {dt}')


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_pauli_evolution(dt):
    n, tol = 5, PREC[dt][1]
    t = 0.4375

    def run(tail):
        cir = dq.QubitCircuit(n)
        cir.hlayer()
        cir.rylayer(inputs=[0.3 * (i + 1) for i in range(n)])
        cir.cnot_ring()
        front = dq.QubitCircuit(n)
        front += cir
        tail(cir)
        with torch.no_grad():
            return finish(front, dt)().reshape(1, -1).cpu().numpy(), finish(cir, dt)().reshape(-1).cpu().numpy()

    # commuting terms: equal to exp(-i H t) of the dense route at any steps and order
    commuting = [[0.5, 'x0x1'], [-0.25, 'y0y1'], [0.75, 'z0z1'], [1.5, 'z3']]
    _, exact = run(lambda cir: cir.hamiltonian(commuting, t=t))
    for steps, order in ((1, 1), (3, 1), (2, 2)):
        _, got = run(lambda cir: cir.pauli_evolution(commuting, t=t, steps=steps, order=order))
        close(got, exact, tol, f'commuting steps={steps} order={order} {dt}')
    # non-commuting terms: the same product formula in numpy, slice by slice
    ham = [[0.8, 'x0z2'], [-0.6, 'y2'], [0.3, 'z0y1x4'], [0.5, 'x1x2']]
    for steps in (1, 3):
        for order in (1, 2):
            before, got = run(lambda cir: cir.pauli_evolution(ham, t=t, steps=steps, order=order))
            ref = before
            seq = list(range(len(ham))) if order == 1 else list(range(len(ham))) + list(range(len(ham) - 1, -1, -1))
            for _ in range(steps):
                for j in seq:
                    letters, wires = split(ham[j][1])
                    ref = rot_ref(ref, *masks_of(n, letters, wires), 2 * ham[j][0] * t / steps / order)
            close(got, ref.reshape(-1), tol, f'product steps={steps} order={order} {dt}')
    # ... and the second order is the more accurate of the two
    p = sum(c * dense_pauli(n, *split(s)) for c, s in ham)
    w, v = np.linalg.eigh(p)
    before, first = run(lambda cir: cir.pauli_evolution(ham, t=t, steps=3, order=1))
    _, second = run(lambda cir: cir.pauli_evolution(ham, t=t, steps=3, order=2))
    exact = (v * np.exp(-1j * t * w)) @ v.conj().T @ before.reshape(-1)
    assert np.abs(second - exact).max() < np.abs(first - exact).max()


def test_refusals():
    makers = {'PauliRot': lambda **kw: dq.PauliRot('xy', nqubit=2, **kw),
              'PauliEvolution': lambda **kw: dq.PauliEvolution([[1.0, 'x0y1']], nqubit=2, **kw)}
    for name, make in makers.items():
        with pytest.raises(NotImplementedError, match=name):
            make(den_mat=True)
        dm = dq.QubitCircuit(2, den_mat=True)
        with pytest.raises(NotImplementedError, match=name):
            if name == 'PauliRot':
                dm.pauli_rot('xy')
            else:
                dm.pauli_evolution([[1.0, 'x0y1']])
        with pytest.raises(NotImplementedError, match=name):
            make().op_dist_state(None)
        with pytest.raises(NotImplementedError, match=name):
            from deepquantum_amd.distributed import dist_run

            dist_run(None, [make()])
        cir = dq.QubitCircuit(2)
        cir.add(make())
        with pytest.raises(NotImplementedError, match=name):
            cir.qasm()
    with pytest.raises(AssertionError):
        dq.PauliRot('xy', nqubit=3, wires=[0, 1], controls=[1])            # a control inside the string
    with pytest.raises(ValueError):
        dq.PauliRot('ii', nqubit=3, wires=[0, 1])                          # the identity is a global phase, not a gate
    with pytest.raises(ValueError):
        dq.PauliEvolution([[1.0, 'x0y0']], nqubit=2)                       # a wire repeated within one string
