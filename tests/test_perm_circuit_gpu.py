"""PermutationGate inside circuits on the GPU: between fused stretches against the dense route (``cir.any`` of the 0/1
matrix, which multiplies where the new gate copies: the existing parity tolerances 1e-10 / 1e-4), undone by
``cir.inverse()``, and order finding for N = 15 with ``modmul`` against ``ShorCircuitFor15``."""

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd.ansatz import _qft_steps, _replay
from _perm_ref import perm_matrix, random_bijection, random_state

pytestmark = pytest.mark.gpu

PRECISIONS = [pytest.param(torch.complex64, 1e-4, id='c64'), pytest.param(torch.complex128, 1e-10, id='c128')]


def build(n, dense, dtype):
    """Fused stretches with a permutation between them; ``dense``: the same maps as 0/1 matrices."""
    torch.manual_seed(11)
    cir = dq.QubitCircuit(n)
    cir.rylayer()
    cir.rxlayer()
    cir.cnot_ring()
    for seed, wires, controls in ((1, [6, 0, 3, 8, 2], None), (2, [4, 5], [1]), (3, [7, 1, 0], [3, 8])):
        perm = random_bijection(len(wires), seed)
        if dense:
            cir.any(torch.from_numpy(perm_matrix(perm)).to(torch.complex64), wires=wires, controls=controls)
        else:
            cir.permutation(perm, wires=wires, controls=controls)
        cir.rylayer()
        cir.cnot_ring(reverse=True)
    cir.rzlayer()
    cir.to('cuda')
    if dtype == torch.complex128:
        cir.to(torch.double)
    return cir


@pytest.mark.parametrize('dtype,tol', PRECISIONS)
def test_permutation_between_fused_stretches_against_the_dense_route(dtype, tol):
    n = 9
    new, old = build(n, False, dtype), build(n, True, dtype)
    for p, q in zip(new.parameters(), old.parameters(), strict=True):
        assert torch.equal(p, q)
    x = torch.from_numpy(random_state(3, n, 1, np.complex128)).to(dtype)
    x = (x / x.norm(dim=-1, keepdim=True)).cuda().reshape(3, -1, 1)
    with torch.no_grad():
        a, b = new(state=x), old(state=x)
        assert a.dtype == dtype and (a - b).abs().max().item() < tol
        a0, b0 = new(), old()                           # from |0..0>
        assert (a0 - b0).abs().max().item() < tol
        # cir.inverse() after cir gives back the input
        back = new.inverse()(state=a)
        assert (back - x).abs().max().item() < tol
        both = new + new.inverse()
        assert (both(state=x) - x).abs().max().item() < tol
    assert sum(isinstance(op, dq.PermutationGate) for op in new.inverse().operators) == 3


def test_gradients_flow_through_the_permutation():
    cir = build(9, False, torch.complex128)
    ref = build(9, True, torch.complex128)
    for c in (cir, ref):
        c.observable(0)
        c.observable(4, 'x')
        c()
        c.expectation().sum().backward()
    for p, q in zip(cir.parameters(), ref.parameters(), strict=True):
        assert (p.grad - q.grad).abs().max().item() < 1e-10


def order_finding(ncount, a):
    """ShorCircuitFor15 with its controlled multiplications as one ``modmul`` each.  Its work register counts from its
    first wire as the LEAST significant bit (x -> 2 x mod 15 moves the bit of wire q to wire q + 1): the table's wires run
    the other way round."""
    cir = dq.QubitCircuit(ncount + 4)
    cir.hlayer(list(range(ncount)))
    cir.x(ncount + 3)
    work = [ncount + 3, ncount + 2, ncount + 1, ncount]
    for j, control in enumerate(range(ncount - 1, -1, -1)):
        cir.modmul(pow(a, 2**j, 15), 15, wires=work, controls=[control])
    _replay(cir, _qft_steps(list(range(ncount)), swaps=True), inverse=True)
    return cir


@pytest.mark.parametrize('a', [7, 2, 11])
def test_order_finding_for_15_against_the_hand_made_circuit(a):
    ncount = 4
    ref, new = dq.ShorCircuitFor15(ncount, a).to('cuda'), order_finding(ncount, a).to('cuda')
    assert sum(isinstance(op, dq.PermutationGate) for op in new.operators) == ncount
    with torch.no_grad():
        pr = (ref().reshape(1 << ncount, 16).abs() ** 2).sum(dim=1).cpu()
        pn = (new().reshape(1 << ncount, 16).abs() ** 2).sum(dim=1).cpu()
    assert abs(pr.sum().item() - 1) < 2e-5
    assert (pr - pn).abs().max().item() < 2e-5                          # (the tolerance of the ansatz checks)
    order = {7: 4, 2: 4, 11: 2}[a]
    peaks = sorted(int(i) for i in torch.nonzero(pn > 0.5 / order).reshape(-1))
    assert peaks == [j * (1 << ncount) // order for j in range(order)]
