"""Trainable multiplexed rotations inside circuits on the GPU: ``cir.ucrx / ucry / ucrz(requires_grad=True)`` on 6 - 8
wires under a control, after and before ordinary gates, with the gradients of the state and of the angles against the
dense oracle -- block_diag(R(theta_s)) built differentiably in torch complex128 and applied as a matrix on the CPU
(tests/_muxgrad_ref.py) -- to 1e-10 (complex128) / 1e-4 (complex64) of the largest gradient entry; constant gates give the
bits they gave before; and the ``ry`` + ``ucry`` ladder of ``prepare_state`` made trainable sits at fidelity 1 with a
vanishing gradient, and climbs back from perturbed angles."""

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import backend
from _mux_ref import random_state
from _muxgrad_ref import dense_mux_rot

pytestmark = pytest.mark.gpu

PRECISIONS = [pytest.param(torch.complex64, 1e-4, id='c64'), pytest.param(torch.complex128, 1e-10, id='c128')]
# axis, n, wires (selects.., target), controls
GATES = [('x', 6, [4, 0, 2], [5]), ('y', 7, [6, 1, 3, 0], [2]), ('z', 8, [2, 7, 5], [0]), ('y', 8, [0, 1, 2, 3, 4, 5, 7], [6])]


def placed(cir, dtype):
    cir.to('cuda')
    if dtype == torch.complex128:
        cir.to(torch.double)
    return cir


def ordinary(n, seed):
    """Ordinary gates with fixed angles: a fused stretch."""
    rng = np.random.default_rng(seed)
    cir = dq.QubitCircuit(n)
    for w in range(n):
        cir.h(w)
        cir.rx(w, inputs=float(rng.uniform(-3, 3)))
    for w in range(n - 1):
        cir.cnot(w, w + 1)
    for w in range(n):
        cir.ry(w, inputs=float(rng.uniform(-3, 3)))
    return cir


@pytest.mark.parametrize('dtype,tol', PRECISIONS)
@pytest.mark.parametrize('axis,n,wires,controls', GATES)
def test_state_and_parameter_gradients_against_the_dense_oracle(axis, n, wires, controls, dtype, tol):
    before, after = ordinary(n, 1), ordinary(n, 2)
    torch.manual_seed(3)
    cir = dq.QubitCircuit(n)
    cir.add(before)
    getattr(cir, 'ucr' + axis)(wires=wires, controls=controls, requires_grad=True)
    assert cir.npara == before.npara + 2 ** (len(wires) - 1)
    cir.add(after)
    placed(cir, dtype)
    (gate,) = [op for op in cir.operators if isinstance(op, dq.MultiplexedRotation)]
    assert [p is gate.angles for p in cir.parameters()] == [True]
    ua = placed(ordinary(n, 1), torch.complex128).get_unitary().cpu()      # (fresh copies: `cir` holds the gates of the others)
    ub = placed(ordinary(n, 2), torch.complex128).get_unitary().cpu()
    xr = random_state(2, n, 4, np.complex128)
    xr /= np.linalg.norm(xr, axis=-1, keepdims=True)
    wr = random_state(2, n, 5, np.complex128)

    x = torch.from_numpy(xr).to(dtype).cuda().requires_grad_()
    y = cir(state=x.reshape(2, -1, 1)).reshape(2, -1)
    loss = (torch.from_numpy(wr).to(dtype).cuda().conj() * y).sum().real + (y.abs() ** 2 * torch.arange(1 << n, device='cuda')).sum() / (1 << n)
    gx, gt = torch.autograd.grad(loss, (x, gate.angles))

    bit = lambda w: n - 1 - w  # noqa: E731
    xo = torch.from_numpy(xr).to(dtype).to(torch.complex128).requires_grad_()
    to = gate.angles.detach().cpu().to(torch.float64).requires_grad_()
    um = dense_mux_rot(to, axis, n, bit(wires[-1]), [bit(w) for w in wires[:-1]], [bit(w) for w in controls])
    yo = (ub @ um @ ua @ xo.T).T
    lo = (torch.from_numpy(wr).to(dtype).to(torch.complex128).conj() * yo).sum().real + (yo.abs() ** 2 * torch.arange(1 << n)).sum() / (1 << n)
    wx, wt = torch.autograd.grad(lo, (xo, to))
    assert (y.detach().cpu().to(torch.complex128) - yo.detach()).abs().max() <= tol
    ex = (gx.cpu().to(torch.complex128) - wx).abs().max() / wx.abs().max()
    et = (gt.cpu().to(torch.float64) - wt).abs().max() / wt.abs().max()
    print(f'ucr{axis} n={n} {dtype}: state {ex:.2e} angles {et:.2e} (tol {tol})')
    assert gx.dtype == dtype and gt.shape == gate.angles.shape and ex <= tol and et <= tol


@pytest.mark.parametrize('dtype,tol', PRECISIONS)
def test_constant_gates_give_the_bits_they_gave_before(dtype, tol):
    n = 7
    x = torch.from_numpy(random_state(3, n, 6, np.complex128)).to(dtype).cuda()
    angles = torch.from_numpy(np.random.default_rng(2).uniform(-6, 6, 8))
    for axis in 'xyz':
        cir = dq.QubitCircuit(n)
        cir.ucr(axis, angles, [5, 0, 3, 1], controls=[6])
        placed(cir, dtype)
        gate = cir.operators[0]
        assert not gate.requires_grad and gate.npara == 0 and not list(cir.parameters())
        with torch.no_grad():
            got = cir(state=x.reshape(3, -1, 1)).reshape(3, -1)
        bit = lambda w: n - 1 - w  # noqa: E731
        table = gate.table(dtype)
        if axis == 'z':
            want = backend.apply_diag(x, table, [bit(w) for w in [5, 0, 3, 1]], [bit(6)])
        else:
            want = backend.apply_mux(x, table, 'ry' if axis == 'y' else 'u', bit(1), [bit(w) for w in [5, 0, 3]], [bit(6)])
        assert torch.equal(torch.view_as_real(got), torch.view_as_real(want)), axis
        # and the trainable gate with the same angles agrees with it to the precision
        tr = dq.QubitCircuit(n)
        tr.ucr(axis, angles, [5, 0, 3, 1], controls=[6], requires_grad=True)
        placed(tr, dtype)
        with torch.no_grad():
            assert (tr(state=x.reshape(3, -1, 1)).reshape(3, -1) - want).abs().max() <= tol * want.abs().max()


def ladder(n, wires, phi):
    """The gates of ``prepare_state`` for a real non-negative vector, with the ucry angles as trainable parameters."""
    ref = dq.QubitCircuit(n)
    ref.prepare_state(phi, wires=wires)
    cir = dq.QubitCircuit(n)
    for op in ref.operators:
        if isinstance(op, dq.MultiplexedRotation):
            cir.ucry(op.angles.clone(), op.wires, requires_grad=True)
        else:
            assert type(op).__name__ == 'Ry'
            cir.ry(op.wires[0], inputs=op.theta.detach().clone())
    return cir


def test_prepare_state_ladder_made_trainable_is_a_stationary_point_and_is_found_again():
    n, wires = 8, [5, 2, 7, 0, 3]
    phi = np.abs(np.random.default_rng(12).standard_normal(32)) + 0.05
    cir = placed(ladder(n, wires, torch.from_numpy(phi)), torch.complex128)
    params = list(cir.parameters())
    assert [tuple(p.shape) for p in params] == [(2,), (4,), (8,), (16,)] and all(p.dtype == torch.float64 for p in params)
    # the vector on `wires` (wires[0] = the most significant bit of its index), |0> on the other wires
    full = np.zeros(1 << n)
    for v in range(32):
        full[sum(((v >> (4 - j)) & 1) << (n - 1 - w) for j, w in enumerate(wires))] = phi[v] / np.linalg.norm(phi)
    target = torch.from_numpy(full).to(torch.complex128).cuda()

    def fidelity():
        return (target.conj() * cir().reshape(-1)).sum().abs() ** 2

    f = fidelity()
    grads = torch.autograd.grad(f, params)
    assert abs(f.item() - 1.0) <= 1e-12
    assert max(g.abs().max().item() for g in grads) <= 1e-8
    torch.manual_seed(5)
    with torch.no_grad():
        for p in params:
            p.add_(0.2 * torch.randn_like(p))
    opt = torch.optim.SGD(params, lr=0.5)
    seen = [fidelity().item()]
    for _ in range(3):
        opt.zero_grad()
        (1.0 - fidelity()).backward()
        opt.step()
        seen.append(fidelity().item())
    print('fidelity:', seen)
    assert seen[0] < 0.999 and seen[-1] > seen[0]
