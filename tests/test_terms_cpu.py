"""Host logic of the per-string Pauli values (backend.pauli_terms_cross, qmath.pauli_term_overlaps / pauli_term_expectations /
pauli_pool_gradients, PauliSum.term_expectations, cir.expectation_pauli_terms / pauli_pool_gradients) without a GPU: the
kernel's stand-in is the complex128 route of ``backend`` under the CPU test double, which leaves what the kernel leaves --
the table's sign bit still on every value -- so the order, the sign and the cuts at the cap are the host's own work."""

import os
import re

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import _lib, backend, qmath
from _terms_ref import term_overlaps_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# negative coefficients, every ny mod 4 (x: 0, y0: 1, y0y1: 2, y0y1y2: 3, y0y1y2y3: 4), several flip masks, a constant
HAM4 = [[0.7, 'x0x1x2x3'], [-1.3, 'y0x1x2x3'], [-0.4, 'y0y1x2x3'], [2.1, 'y0y1y2x3'], [-0.6, 'y0y1y2y3'], [-0.9, 'z0y1x2z3'],
        [-0.8, 'z1z2'], [0.25, ''], [-0.5, 'x1'], [0.3, 'y1'], [1.1, 'z0x1'], [-0.2, 'y3z0'], [0.6, 'y1y3']]


def rand_state(batch, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, 1 << n, dtype=torch.complex128, generator=g)


def test_symbols_follow_the_abi_conventions():
    lib = _lib.load()
    text = open(os.path.join(ROOT, 'include', 'dq_hip.h')).read()
    declared = re.findall(r'^\s*(?:int|int64_t)\s+(dq_\w+)\s*\(', text, flags=re.M)
    mine = ['dq_pauli_terms_cross_c128', 'dq_pauli_terms_cross_c64', 'dq_pauli_terms_max', 'dq_pauli_terms_ws_bytes']
    assert sorted(s for s in _lib.exported_symbols() if 'pauli_terms' in s) == sorted(d for d in declared if 'pauli_terms' in d) == mine
    assert all(hasattr(lib, s) for s in mine) and lib.dq_abi_version() == _lib.ABI_VERSION
    cap, size = lib.dq_pauli_terms_max(), lib.dq_pauli_terms_ws_bytes
    assert cap == backend.pauli_terms_max() == 1024
    # 16 bytes per term, workgroup and sample; a unit is 1024 vectors, at most 1024 workgroups a sample
    assert size(3, 1, 0, 0, 5) == 5 * 16 and size(14, 3, 0, 1, 7) == 3 * 8 * 7 * 16 and size(14, 3, 1, 1, 7) == 3 * 16 * 7 * 16
    assert size(30, 2, 0, 0, cap) == 2 * 1024 * cap * 16
    for bad in ((0, 1, 0, 0, 1), (41, 1, 0, 0, 1), (3, 0, 0, 0, 1), (3, 65536, 0, 0, 1), (3, 1, 0, 0, 0), (3, 1, 0, 0, cap + 1)):
        assert size(*bad) == -1
    # refusals on the host, before any HIP call (the pointers are never dereferenced)
    p, q, o, w, xm, bd, zm, wt, big = 1 << 20, 1 << 30, 1 << 24, 1 << 26, 1 << 32, 1 << 33, 1 << 34, 1 << 35, 1 << 40

    def refused(rc, word):
        assert rc == -1 and word in lib.dq_last_error().decode(), lib.dq_last_error()

    for f in (lib.dq_pauli_terms_cross_c64, lib.dq_pauli_terms_cross_c128):
        good = [p, q, xm, bd, zm, wt, 2, 3, 5, 1, o, w, big]
        for slot in (0, 1, 2, 3, 4, 5, 10, 11):
            refused(f(*[None if i == slot else v for i, v in enumerate(good)], None), 'null')
        for slot, off in ((0, 8), (1, 8), (2, 4), (3, 2), (4, 4), (5, 4), (10, 8), (11, 8)):
            refused(f(*[v + off if i == slot else v for i, v in enumerate(good)], None), 'aligned')
        for slot, value, word in ((8, 0, 'n=0'), (8, 41, 'n=41'), (6, 0, 'ngroups=0'), (7, 0, 'nterms=0'), (7, cap + 1, 'at most'),
                                  (9, 0, 'batch'), (9, 65536, 'batch'), (12, size(5, 1, 0, 1, 3) - 1, 'workspace')):
            refused(f(*[value if i == slot else v for i, v in enumerate(good)], None), word)


@pytest.mark.parametrize('cap', [1024, 3])
def test_order_sign_and_cuts_at_the_cap(cpu_backend, monkeypatch, cap):
    """The values come in the order of ``H.terms`` without sign(h_t), whole or cut at a cap of 3: HAM4 has several groups
    (cut between them, and its group of five terms inside), the second table is ONE group of 7 terms."""
    monkeypatch.setattr(backend, 'pauli_terms_max', lambda: cap)
    n = 4
    bra, ket = rand_state(3, n, 1), rand_state(3, n, 2)
    one_group = [[(-1.0) ** k * (k + 1), s] for k, s in enumerate(['x0', 'x0z1', 'x0z2', 'y0', 'y0z3', 'x0z1z2', 'y0z1z3'])]
    for ham in (HAM4, one_group):
        H = dq.PauliSum(ham, n)
        pieces = backend._terms_pieces(H.table, cap)
        assert sum(p.nterms for p, _ in pieces) == H.nterms and all(p.nterms <= cap for p, _ in pieces)
        assert len(pieces) == (1 if cap == 1024 else 5 if ham is HAM4 else 3)
        want, _ = term_overlaps_ref(bra.numpy(), ket.numpy(), H.terms)
        got = backend.pauli_terms_cross(bra, ket, H.table)
        assert got.shape == (3, H.nterms) and got.dtype == torch.complex128
        assert np.abs(got.numpy() - want).max() < 1e-13 * np.abs(want).max()
        assert np.abs(want).min() > 1e-3                                        # (no value that a lost sign would leave alone)
        # through qmath: single states, the list form, the expectations as the real part with bra = ket
        assert torch.equal(qmath.pauli_term_overlaps(bra, ket, n, H), got)
        assert torch.equal(qmath.pauli_term_overlaps(bra[1], ket[1], n, H), got[1])
        e = qmath.pauli_term_expectations(ket, n, ham)
        assert e.dtype == torch.float64 and e.shape == (3, H.nterms) and torch.equal(H.term_expectations(ket[0]), e[0])
        assert np.abs(e.numpy() - term_overlaps_ref(ket.numpy(), ket.numpy(), H.terms)[0].real).max() < 1e-12
        # sum_t h_t <P_t> is <H>
        h = torch.tensor([t[0] for t in H.terms], dtype=torch.float64)
        assert ((e * h).sum(-1) - qmath.expectation_pauli_sum(ket, n, H)).abs().max().item() < 1e-12


def build_circuit(n, tail=None):
    cir = dq.QubitCircuit(n)
    cir.rylayer(encode=True)
    cir.cnot(0, 1)
    cir.pauli_rot('xyz', wires=[0, 2, 3], encode=True)
    cir.cnot(2, 3)
    cir.cnot(1, 2)
    if tail is not None:
        cir.pauli_rot(tail[0], wires=tail[1], encode=True)
    cir.to(torch.double)
    return cir


def test_pool_gradients_against_a_central_difference(cpu_backend):
    """d<H>/d theta_k at 0 through cir.pauli_rot and <H>.  A step of 1e-4 leaves h^2 / 6 |E'''| <= 1e-8 / 6 * norm_bound
    of truncation and 1e-16 * norm_bound / 1e-4 of rounding: 1e-7 holds both with norm_bound = 10."""
    n, step = 4, 1e-4
    H = dq.PauliSum(HAM4, n)
    pool = [('xy', [0, 1]), ('yx', [0, 1]), ('yzzx', [0, 1, 2, 3]), ('z', [2]), ('xy', [0, 1])]        # (one string twice)
    strings = [''.join(f'{p}{w}' for p, w in zip(*k)) for k in pool]
    data = torch.tensor([0.3, -0.8, 1.1, 0.45, -0.2], dtype=torch.float64)
    with torch.no_grad():
        cir = build_circuit(n)
        cir(data)
        got = cir.pauli_pool_gradients(H, strings)
        assert got.shape == (5,) and got.dtype == torch.float64 and got.abs().min().item() > 1e-2
        for k, tail in enumerate(pool):
            e = [float(qmath.expectation_pauli_sum(build_circuit(n, tail)(torch.cat([data, torch.tensor([s * step])])), n, H))
                 for s in (1.0, -1.0)]
            assert abs(float(got[k]) - (e[0] - e[1]) / (2 * step)) < 1e-7
        # a PauliSum as the pool: the order of its terms, coefficients as 1; a batch of states
        P, order = dq.PauliSum.from_strings(strings, n)
        assert P.nterms == 4 and order[0] == order[4]
        states = cir(torch.stack([data, 0.5 * data]))
        both = qmath.pauli_pool_gradients(states, n, H, dq.PauliSum([[-2.0, s] for s in strings[:4]], n))
        assert both.shape == (2, 4) and (both[0] - got[:4][torch.tensor(order[:4]).argsort()]).abs().max().item() < 1e-12
        assert torch.equal(cir.expectation_pauli_terms(H), qmath.pauli_term_expectations(states, n, H))


def test_refusals(cpu_backend):
    n = 2
    H = dq.PauliSum([[1.0, 'z0'], [0.5, 'x0y1']], n)
    x = rand_state(1, n, 3).requires_grad_()
    for call in (lambda: qmath.pauli_term_overlaps(x, x, n, H), lambda: qmath.pauli_term_expectations(x, n, H),
                 lambda: qmath.pauli_pool_gradients(x, n, H, ['x0']), lambda: H.term_expectations(x)):
        with pytest.raises(NotImplementedError, match='expectation_pauli_sum'):
            call()
    with torch.no_grad():
        assert qmath.pauli_term_expectations(x, n, H).shape == (1, 2)
    cir = dq.QubitCircuit(n)
    cir.hlayer()
    dm = dq.QubitCircuit(n, den_mat=True)
    dm.state = torch.zeros(4, 4)
    for name, args in (('expectation_pauli_terms', (H,)), ('pauli_pool_gradients', (H, ['x0']))):
        with pytest.raises(RuntimeError, match='run the circuit first'):
            getattr(cir, name)(*args)
        with pytest.raises(NotImplementedError, match='den_mat'):
            getattr(dm, name)(*args)
        with pytest.raises(NotImplementedError, match='sharded'):
            getattr(dq.DistributedQubitCircuit, name)(object(), *args)
    with pytest.raises(ValueError, match='qubits'):
        qmath.pauli_term_expectations(x.detach(), n, dq.PauliSum([[1.0, 'z0']], 3))
    with pytest.raises(ValueError, match='PsumTable'):
        backend.pauli_terms_cross(x.detach(), x.detach(), H)
    with pytest.raises(ValueError, match='list of strings'):
        qmath.pauli_pool_gradients(x.detach(), n, H, 'x0')
