"""SELECT over Pauli strings and the block encoding built on it, without a GPU: the reference against the dense definition,
both table constructors, every refusal by name, the library's host-side checks, and the block-encoding identities through
the plain-torch stand-in of the kernel (``backend._apply_select_pauli_double``)."""

import os
import pickle
import re

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import _lib, backend, ops
from _select_ref import dense_select, masks, pauli_sum_matrix, random_state, random_words, select_ref, words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('dq_apply_select_pauli_c64', 'dq_apply_select_pauli_c128', 'dq_select_pauli_unit_bits')


def tt(a):
    return torch.from_numpy(np.asarray(a))


def signed(table):
    return tt(table.view(np.int64))


def test_reference_against_the_dense_definition():
    n, select, system = 5, [3, 0], [1, 2, 4]
    strings, phases = ['x0y2', 'z1', 'y0y1y2'], [1, 2, 3]                     # (the fourth entry is the identity)
    dense = dense_select(n, select, system, strings, phases)
    assert np.allclose(dense @ dense.conj().T, np.eye(1 << n), atol=1e-15)
    entries = [(*masks(s, n, system), q) for s, q in zip(strings, phases)]
    bits = [n - 1 - w for w in select]
    x = random_state(np.random.default_rng(1), 3, n, np.complex128)
    for dagger, matrix in ((False, dense), (True, dense.conj().T)):
        got = select_ref(x, words(entries, dagger), bits)
        np.testing.assert_allclose(got, x @ matrix.T, rtol=0, atol=1e-15)
    # with a control: the identity where it is 0
    dense = dense_select(n, [3], [1, 2], ['x0y1', 'z0'], [0, 1], controls=[4])
    entries = [(*masks('x0y1', n, [1, 2]), 0), (*masks('z0', n, [1, 2]), 1)]
    np.testing.assert_allclose(select_ref(x, words(entries), [1], [0]), x @ dense.T, rtol=0, atol=1e-15)


def test_both_table_constructors():
    n = 5
    entries = [(0b10100, 0b00100, 1), (0, 0b01010, 2), (0b00110, 0b00110, 3), (0, 0, 0)]
    table = backend.SelectTable(n, entries)
    assert table.k == 2 and table.nqubit == n
    forward, dagger = table.on('cpu')
    assert forward.dtype == torch.int64 and forward.shape == (4, 2)
    np.testing.assert_array_equal(forward.numpy().view(np.uint64), words(entries))
    np.testing.assert_array_equal(dagger.numpy().view(np.uint64), words(entries, dagger=True))
    assert table.on('cpu', dagger=True)[0] is dagger
    # q = (q_user + ny) mod 4 forward, (ny - q_user) mod 4 for the adjoint
    assert [int(w) >> 62 & 3 for w in forward[:, 0]] == [2, 2, 1, 0] and [int(w) >> 62 & 3 for w in dagger[:, 0]] == [0, 2, 3, 0]
    again = pickle.loads(pickle.dumps(table))
    assert torch.equal(again.on('cpu')[0], forward) and again._devices == {}
    for bad, word in (([(0, 0, 0)] * 3, '2\\^k entries'), ([(0, 0, 0)], '2\\^k entries'), ([(32, 0, 0), (0, 0, 0)], 'mask'),
                      ([(0, -1, 0), (0, 0, 0)], 'mask'), ([(0, 0, 4), (0, 0, 0)], 'power of i')):
        with pytest.raises(ValueError, match=word):
            backend.SelectTable(n, bad)
    with pytest.raises(ValueError, match='nqubit'):
        backend.SelectTable(41, entries)
    # the gate builds the same table from strings, wire w of a string being system_wires[w]
    gate = dq.SelectPauli(['x0y2', 'z1', 'y0y1y2'], nqubit=n, wires=[3, 0], phases=[1, 2, 3])
    assert gate.system_wires == [1, 2, 4]
    want = [(*masks(s, n, [1, 2, 4]), q) for s, q in zip(['x0y2', 'z1', 'y0y1y2', ''], [1, 2, 3, 0])]
    np.testing.assert_array_equal(gate.table.on('cpu')[0].numpy().view(np.uint64), words(want))
    assert 'wires=[3, 0], strings=3' in repr(gate)
    # from a PauliSum: its merged terms in their order, the signs as phases, the magnitudes ignored
    ham = dq.PauliSum([[0.5, 'x0y2'], [-2.0, 'z1'], [-0.25, ''], [1.5, 'x0y2']], 3)
    gate = dq.SelectPauli(ham, nqubit=n, wires=[3, 0], system_wires=[4, 2, 1])
    want = []
    for h, x, z in ham.terms:
        string = ''.join(('y' if x >> (2 - w) & z >> (2 - w) & 1 else 'x' if x >> (2 - w) & 1 else 'z') + str(w)
                         for w in range(3) if (x | z) >> (2 - w) & 1)
        want.append((*masks(string, n, [4, 2, 1]), 0 if h > 0 else 2))
    assert len(want) == 3 and ham.select_bits == 2
    np.testing.assert_array_equal(gate.table.on('cpu')[0].numpy().view(np.uint64), words(want))
    assert dq.PauliSum([[1.0, 'x0']], 2).select_bits == 1 and dq.PauliSum([[1.0, f'z{w}'] for w in range(5)], 5).select_bits == 3


def test_gate_refusals_by_name():
    ok = dict(paulis=['x0', 'z1'], nqubit=4, wires=[0])
    for bad, word in ((dict(paulis=['x0', 'z1', 'y0']), 'too many strings'),
                      (dict(system_wires=[0, 1]), 'touches a select or control wire'),
                      (dict(system_wires=[1, 2], controls=[2]), 'touches a select or control wire'),
                      (dict(paulis=['x0', 'z3']), 'outside the system register'),
                      (dict(system_wires=[1, 4]), 'outside'),
                      (dict(wires=[0, 0]), 'repeated wires'),
                      (dict(controls=[0]), 'repeated wires'),
                      (dict(system_wires=[1, 1]), 'repeated wires'),
                      (dict(paulis=['x0z0', 'z1']), 'repeated'),
                      (dict(phases=[0, 4]), 'power of i'),
                      (dict(phases=[0, -1]), 'power of i'),
                      (dict(phases=[0]), 'phases for'),
                      (dict(paulis=['q0', 'z1']), 'not a string of factors'),
                      (dict(paulis=dq.PauliSum([[1.0, 'x0']], 2)), 'PauliSum is for 2 qubits'),
                      (dict(wires=None), 'select wires')):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError, match=word):
            dq.SelectPauli(**kw)
    with pytest.raises(NotImplementedError, match='den_mat'):
        dq.SelectPauli(den_mat=True, **ok)
    gate = dq.SelectPauli(**ok)
    with pytest.raises(NotImplementedError, match='qasm'):
        gate.qasm_refusal()
    with pytest.raises(NotImplementedError, match='matrix primitive'):
        gate.prims()
    with pytest.raises(NotImplementedError, match='sharded'):
        gate.op_dist_state(None)
    cir = dq.QubitCircuit(4)
    with pytest.raises(ValueError, match='select wires'):
        cir.block_encode([[1.0, 'x0'], [0.5, 'z1'], [0.25, 'y2']], wires=[0])
    with pytest.raises(ValueError, match='PauliSum is for 2 qubits'):
        cir.block_encode(dq.PauliSum([[1.0, 'x0'], [0.5, 'z1']], 2), wires=[0])
    with pytest.raises(NotImplementedError, match='den_mat'):
        dq.QubitCircuit(4, den_mat=True).select_pauli(['x0', 'z1'], wires=[0])


def test_backend_refusals(cpu_backend):
    x = tt(random_state(np.random.default_rng(2), 2, 4, np.complex128))
    table = backend.SelectTable(4, [(1, 0, 0), (0, 1, 0), (0, 0, 0), (1, 1, 1)]).on('cpu')[0]
    ok = dict(table_words=table, bits=(1, 2), controls=())
    for bad, word in ((dict(bits=(1, 1)), 'distinct'), (dict(bits=(1, 4)), 'distinct'), (dict(controls=(2,)), 'distinct'),
                      (dict(bits=()), 'at least one'), (dict(bits=(1,)), 'shape'), (dict(table_words=table.to(torch.int32)), 'int64'),
                      (dict(out=x), 'overlap'), (dict(out=torch.zeros(2, 8, dtype=x.dtype)), 'shape')):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError, match=word):
            backend.apply_select_pauli(x, **kw)
    with pytest.raises(ValueError, match='SelectTable'):
        ops.select_pauli(x, table, (1, 2))
    with pytest.raises(ValueError, match='select bits'):
        ops.select_pauli(x, backend.SelectTable(4, [(0, 0, 0)] * 4), (1,))


def test_library_exports_the_new_symbols_and_still_reports_abi_30():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 30 and lib.dq_abi_version() == 30
    text = open(os.path.join(ROOT, 'include', 'dq_hip.h')).read()
    assert re.search(r'#define DQ_ABI_VERSION 30\b', text)
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.exported_symbols() and 'psum' not in name
        assert re.search(r'\bint %s\(' % name, text)
    assert lib.dq_select_pauli_unit_bits(0) == 11 and lib.dq_select_pauli_unit_bits(1) == 10
    assert backend.select_pauli_unit_bits(torch.complex64) == 11 and backend.select_pauli_unit_bits(torch.complex128) == 10
    assert hasattr(dq, 'SelectPauli')


def test_host_side_argument_checks_of_the_library():
    """DQ_ERR_ARG with a text, before any HIP call (no device is touched: the pointers are never dereferenced)."""
    lib = _lib.load()
    ia = _lib.int_array
    p, q, t = 1 << 20, 1 << 30, 4096                    # aligned non-null "pointers", far apart

    def refused(rc, word):
        assert rc == -1 and word in lib.dq_last_error().decode(), lib.dq_last_error()

    f64, f128 = lib.dq_apply_select_pauli_c64, lib.dq_apply_select_pauli_c128
    for f in (f64, f128):
        refused(f(None, q, t, 3, ia([0]), 1, ia([]), 0, 1, None), 'null')
        refused(f(p, None, t, 3, ia([0]), 1, ia([]), 0, 1, None), 'null')
        refused(f(p, q, None, 3, ia([0]), 1, ia([]), 0, 1, None), 'null')
        refused(f(p, q, t, 0, ia([0]), 1, ia([]), 0, 1, None), 'n=0')
        refused(f(p, q, t, 41, ia([0]), 1, ia([]), 0, 1, None), 'n=41')
        refused(f(p, q, t, 3, ia([0]), 0, ia([]), 0, 1, None), 'k=0')
        refused(f(p, q, t, 3, ia([0, 1, 2, 3]), 4, ia([]), 0, 1, None), 'k=4')
        refused(f(p, q, t, 40, ia(range(32)), 32, ia([]), 0, 1, None), 'k=32')
        refused(f(p, q, t, 3, ia([3]), 1, ia([]), 0, 1, None), 'out of range')
        refused(f(p, q, t, 3, ia([0]), 1, ia([3]), 1, 1, None), 'out of range')
        refused(f(p, q, t, 3, ia([1, 1]), 2, ia([]), 0, 1, None), 'twice')
        refused(f(p, q, t, 3, ia([0, 1]), 2, ia([1]), 1, 1, None), 'twice')                       # a control among the select bits
        refused(f(p, q, t, 3, ia([0]), 1, ia([]), 0, 0, None), 'batch')
        refused(f(p, q, t, 3, ia([0]), 1, ia([]), 0, 65536, None), 'batch')
        refused(f(p + 8, q, t, 3, ia([0]), 1, ia([]), 0, 1, None), 'aligned')
        refused(f(p, q + 8, t, 3, ia([0]), 1, ia([]), 0, 1, None), 'aligned')
        refused(f(p, q, t + 8, 3, ia([0]), 1, ia([]), 0, 1, None), 'aligned')                     # the table: 16 bytes
        refused(f(p, p, t, 3, ia([0]), 1, ia([]), 0, 1, None), 'overlap')
    # the ranges [in, in + batch * 2^n) and [out, ..): 2 samples of 8 amplitudes are 128 (256) bytes
    refused(f64(p, p + 112, t, 3, ia([0]), 1, ia([]), 0, 2, None), 'overlap')
    refused(f64(p + 112, p, t, 3, ia([0]), 1, ia([]), 0, 2, None), 'overlap')
    refused(f128(p, p + 240, t, 3, ia([0]), 1, ia([]), 0, 2, None), 'overlap')


CASES = [
    # n, bits, controls
    (5, (3, 0), ()),                    # unsorted, bit 0 a select bit
    (5, (2,), ()),                      # k = 1
    (4, (0, 2, 3, 1), ()),              # k = n: every entry a bare phase
    (5, (1, 3), (0,)),                  # one control
    (6, (4, 1, 2), (5, 0)),             # two controls
]


@pytest.mark.parametrize('n,bits,controls', CASES)
def test_stand_in_against_the_reference(cpu_backend, n, bits, controls):
    """The plain-torch stand-in computes in the state's dtype with factors 1, i, -1, -i: exact as well.  The table is drawn
    over ALL index bits: the flip masks are confined to the free bits by the stand-in as by the kernel."""
    rng = np.random.default_rng(n * 7 + len(bits))
    for dtype in (np.complex64, np.complex128):
        x = random_state(rng, 2, n, dtype)
        table = random_words(rng, len(bits), range(n))
        got = backend.apply_select_pauli(tt(x), signed(table), bits, controls).numpy()
        np.testing.assert_array_equal(got, select_ref(x, table, bits, controls))


def test_dagger_table_undoes_the_forward_table(cpu_backend):
    n = 6
    gate = dq.SelectPauli(['x0', 'z1', 'y0y1', '', 'x1'], nqubit=n, wires=[4, 0, 2], phases=[1, 2, 3, 0, 1], controls=[5])
    x = tt(random_state(np.random.default_rng(3), 3, n, np.complex128))
    y = gate.apply_flat(x)
    assert not torch.equal(y, x)
    inv = gate.inverse()
    assert inv.name == 'SelectPauli_dagger' and torch.equal(inv.apply_flat(y), x)
    u = gate.get_unitary()
    assert u.dtype == torch.complex64 and gate.double().get_unitary().dtype == torch.complex128
    assert torch.equal(u @ u.mH, torch.eye(1 << n, dtype=u.dtype)) and torch.equal(inv.get_unitary(), u.mH)
    dense = dense_select(n, [4, 0, 2], [1, 3], ['x0', 'z1', 'y0y1', '', 'x1'], [1, 2, 3, 0, 1], controls=[5])
    np.testing.assert_array_equal(gate.double().get_unitary().numpy(), dense)
    # the autograd node through the stand-in: the cotangent is the dagger table applied to the upstream gradient
    xr = x.clone().requires_grad_(True)
    g = tt(random_state(np.random.default_rng(4), 3, n, np.complex128))
    (gx,) = torch.autograd.grad(gate.double().apply_flat(xr), xr, g)
    assert torch.equal(gx, gate.inverse().apply_flat(g))


TERMS = [[0.7, 'x0y2'], [-1.3, 'z1'], [0.4, 'y0y1'], [-0.6, ''], [0.9, 'z0x2']]            # 5 strings on 3 wires


@pytest.mark.parametrize('select,system', [([0, 1, 2], [3, 4, 5]), ([3, 4, 5], [0, 1, 2]), ([4, 0, 2], [5, 1, 3])])
def test_block_encoding_identities(cpu_backend, select, system):
    n, m = 6, 3
    ham = dq.PauliSum(TERMS, m)
    hmat = pauli_sum_matrix(TERMS, m)
    cir = dq.QubitCircuit(n)
    lam = cir.block_encode(ham, wires=select, system_wires=system)
    assert lam == pytest.approx(sum(abs(h) for h, _ in TERMS), rel=1e-15)
    assert lam == pytest.approx(ham.norm_bound + abs(ham.constant), rel=1e-15)
    cir.to(torch.double)
    u = cir.get_unitary().numpy()
    assert u.dtype == np.complex128
    np.testing.assert_allclose(u @ u, np.eye(1 << n), rtol=0, atol=1e-10)
    np.testing.assert_allclose(u, u.conj().T, rtol=0, atol=1e-10)
    # the block where the select wires are |0>: rows and columns whose select bits are 0, ordered by the system wires
    idx = [sum(((r >> (m - 1 - a)) & 1) << (n - 1 - system[a]) for a in range(m)) for r in range(1 << m)]
    np.testing.assert_allclose(u[np.ix_(idx, idx)], hmat / lam, rtol=0, atol=1e-10)
    # qubitization: <0, psi| W^j |0, psi> = cos(j arccos(E / lam)) on eigenvectors of H
    walk = dq.QubitCircuit(n)
    assert walk.qubitization_walk(TERMS, wires=select, system_wires=system) == lam
    walk.to(torch.double)
    w = walk.get_unitary().numpy()
    energies, vectors = np.linalg.eigh(hmat)
    for e in (0, 5):
        start = np.zeros(1 << n, dtype=np.complex128)
        start[idx] = vectors[:, e]
        v = start
        for j in range(1, 5):
            v = w @ v
            assert abs(np.vdot(start, v) - np.cos(j * np.arccos(energies[e] / lam))) < 1e-10
