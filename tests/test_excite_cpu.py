"""Host logic of the excitation gates (ExcitationGate, UCCSD, ops.excite_*, backend.apply_excite_* / excite_cross)
without a GPU: the kernels' stand-in is the plain-torch complex128 route of ``backend`` under the CPU test double, so what
is checked here is the library's argument checks, the Jordan-Wigner sign and mask builder against the dense definition,
the autograd rules and the bookkeeping."""

import itertools
import os
import re

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import _lib, backend, ops
from deepquantum_amd.gate import excitation_masks
from _excite_ref import (
    dense_k, dense_u, index_axpby, index_cross, index_k, index_rot, outside, pairs, pauli_terms, random_state,
)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('dq_apply_excite_axpby_c64', 'dq_apply_excite_axpby_c128', 'dq_excite_cross_c64', 'dq_excite_cross_c128')


def tt(a):
    return torch.from_numpy(np.asarray(a))


def bits_of(n, wires):
    return tuple(n - 1 - w for w in wires)


def test_library_exports_the_new_symbols_and_still_reports_abi_30():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 30 and lib.dq_abi_version() == 30
    text = open(os.path.join(ROOT, 'include', 'dq_hip.h')).read()
    assert re.search(r'#define DQ_ABI_VERSION 30\b', text)
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.exported_symbols()
        assert re.search(r'\bint %s\(' % name, text)
    assert re.search(r'#define DQ_EXCITE_GATE %d\b' % _lib.EXCITE_GATE, text)
    assert re.search(r'#define DQ_EXCITE_MAP %d\b' % _lib.EXCITE_MAP, text)
    for name in ('ExcitationGate', 'UCCSD'):
        assert hasattr(dq, name)
    # the sizing function agrees with the other cross reductions and refuses what they refuse
    assert lib.dq_excite_cross_ws_bytes(20, 3, 0, 0) == lib.dq_pauli_cross_ws_bytes(20, 3, 0, 0) > 0
    assert lib.dq_excite_cross_ws_bytes(0, 1, 0, 0) == -1 and lib.dq_excite_cross_ws_bytes(3, 0, 1, 0) == -1


def test_host_side_argument_checks_of_the_library():
    """DQ_ERR_ARG with a text, before any HIP call (no device is touched: the pointers are never dereferenced)."""
    lib = _lib.load()
    ia = _lib.int_array
    p, q, t, w = 1 << 20, 1 << 30, 4096, 1 << 16        # aligned non-null "pointers", far apart

    def refused(rc, word):
        assert rc == -1 and word in lib.dq_last_error().decode(), lib.dq_last_error()

    # f(in, out, coef, mode, xmask, amask, zmask, negate, n, controls, nc, batch, stream)
    for f in (lib.dq_apply_excite_axpby_c64, lib.dq_apply_excite_axpby_c128):
        refused(f(None, q, t, 0, 3, 1, 0, 0, 3, ia([]), 0, 1, None), 'null')
        refused(f(p, None, t, 0, 3, 1, 0, 0, 3, ia([]), 0, 1, None), 'null')
        refused(f(p, q, None, 0, 3, 1, 0, 0, 3, ia([]), 0, 1, None), 'coef')
        refused(f(p + 8, q, t, 0, 3, 1, 0, 0, 3, ia([]), 0, 1, None), 'aligned')
        refused(f(p, q + 8, t, 0, 3, 1, 0, 0, 3, ia([]), 0, 1, None), 'aligned')
        refused(f(p, q, t + 4, 0, 3, 1, 0, 0, 3, ia([]), 0, 1, None), 'aligned')
        refused(f(p, q, t, 0, 1, 1, 0, 0, 0, ia([]), 0, 1, None), 'n=0')
        refused(f(p, q, t, 0, 3, 1, 0, 0, 41, ia([]), 0, 1, None), 'n=41')
        refused(f(p, q, t, 2, 3, 1, 0, 0, 3, ia([]), 0, 1, None), 'mode')
        refused(f(p, q, t, -1, 3, 1, 0, 0, 3, ia([]), 0, 1, None), 'mode')
        refused(f(p, q, t, 0, 0, 0, 0, 0, 3, ia([]), 0, 1, None), 'xmask == 0')
        refused(f(p, q, t, 0, 8, 0, 0, 0, 3, ia([]), 0, 1, None), 'at or above n')
        refused(f(p, q, t, 0, 3, 0, 8, 0, 3, ia([]), 0, 1, None), 'at or above n')
        refused(f(p, q, t, 0, 3, 4, 0, 0, 3, ia([]), 0, 1, None), 'not a subset')
        refused(f(p, q, t, 0, 3, 1, 2, 0, 3, ia([]), 0, 1, None), 'share a bit')
        refused(f(p, q, t, 0, 3, 1, 0, 2, 3, ia([]), 0, 1, None), 'negate')
        refused(f(p, q, t, 0, 3, 1, 0, -1, 3, ia([]), 0, 1, None), 'negate')
        refused(f(p, q, t, 0, 3, 1, 0, 0, 3, ia([1]), 1, 1, None), 'control lies inside')
        refused(f(p, q, t, 0, 3, 1, 4, 0, 3, ia([2]), 1, 1, None), 'control lies inside')          # .. inside zmask
        refused(f(p, q, t, 0, 3, 1, 0, 0, 4, ia([2, 2]), 2, 1, None), 'twice')
        refused(f(p, q, t, 0, 3, 1, 0, 0, 4, ia([4]), 1, 1, None), 'out of range')
        refused(f(p, q, t, 0, 3, 1, 0, 0, 4, ia([-1]), 1, 1, None), 'out of range')
        refused(f(p, q, t, 0, 3, 1, 0, 0, 3, ia([]), 0, 0, None), 'batch')
        refused(f(p, q, t, 0, 3, 1, 0, 0, 3, ia([]), 0, 65536, None), 'batch')
    # the ranges [in, in + batch * 2^n) and [out, ..): 2 samples of 8 amplitudes are 128 (256) bytes
    refused(lib.dq_apply_excite_axpby_c64(p, p + 112, t, 0, 3, 1, 0, 0, 3, ia([]), 0, 2, None), 'overlap')
    refused(lib.dq_apply_excite_axpby_c64(p + 112, p, t, 0, 3, 1, 0, 0, 3, ia([]), 0, 2, None), 'overlap')
    refused(lib.dq_apply_excite_axpby_c128(p, p + 240, t, 0, 3, 1, 0, 0, 3, ia([]), 0, 2, None), 'overlap')
    # g(bra, ket, xmask, amask, zmask, negate, n, controls, nc, batch, out, ws, ws_bytes, stream)
    for g, c128 in ((lib.dq_excite_cross_c64, 0), (lib.dq_excite_cross_c128, 1)):
        need = lib.dq_excite_cross_ws_bytes(3, 1, c128, 1)
        assert need == 16
        refused(g(None, q, 3, 1, 0, 0, 3, ia([]), 0, 1, t, w, need, None), 'null')
        refused(g(p, None, 3, 1, 0, 0, 3, ia([]), 0, 1, t, w, need, None), 'null')
        refused(g(p, q, 3, 1, 0, 0, 3, ia([]), 0, 1, None, w, need, None), 'null')
        refused(g(p, q, 3, 1, 0, 0, 3, ia([]), 0, 1, t, None, need, None), 'null')
        refused(g(p + 8, q, 3, 1, 0, 0, 3, ia([]), 0, 1, t, w, need, None), 'aligned')
        refused(g(p, q + 8, 3, 1, 0, 0, 3, ia([]), 0, 1, t, w, need, None), 'aligned')
        refused(g(p, q, 3, 1, 0, 0, 3, ia([]), 0, 1, t + 4, w, need, None), 'aligned')
        refused(g(p, q, 3, 1, 0, 0, 3, ia([]), 0, 1, t, w + 8, need, None), 'aligned')
        refused(g(p, q, 3, 1, 0, 0, 3, ia([]), 0, 1, t, w, need - 1, None), 'workspace')
        refused(g(p, q, 3, 1, 0, 0, 0, ia([]), 0, 1, t, w, need, None), 'n=0')
        refused(g(p, q, 3, 1, 0, 0, 41, ia([]), 0, 1, t, w, need, None), 'n=41')
        refused(g(p, q, 0, 0, 0, 0, 3, ia([]), 0, 1, t, w, need, None), 'xmask == 0')
        refused(g(p, q, 3, 4, 0, 0, 3, ia([]), 0, 1, t, w, need, None), 'not a subset')
        refused(g(p, q, 3, 1, 1, 0, 3, ia([]), 0, 1, t, w, need, None), 'share a bit')
        refused(g(p, q, 3, 1, 0, 0, 3, ia([0]), 1, 1, t, w, need, None), 'control lies inside')
        refused(g(p, q, 3, 1, 0, 0, 4, ia([3, 3]), 2, 1, t, w, need, None), 'twice')
        refused(g(p, q, 3, 1, 0, 0, 4, ia([7]), 1, 1, t, w, need, None), 'out of range')
        refused(g(p, q, 3, 1, 0, 0, 3, ia([]), 0, 0, t, w, need, None), 'batch')
        refused(g(p, q, 3, 1, 0, 0, 3, ia([]), 0, 65536, t, w, need, None), 'batch')


# ---- the spec builder against the definition --------------------------------------------------------------------------
def check_masks(n, create, annihilate, fermionic=True, controls=()):
    spec = excitation_masks(n, create, annihilate, fermionic, controls)
    k = index_k(n, (*spec, bits_of(n, controls)))
    assert np.array_equal(k, dense_k(n, create, annihilate, fermionic, controls)), (n, create, annihilate, fermionic, controls)
    return spec


def test_the_two_references_agree_and_singles_match_the_definition_for_every_ordered_pair():
    for n in (2, 3, 5, 6):
        for p, q in itertools.permutations(range(n), 2):
            xmask, amask, zmask, negate = check_masks(n, [q], [p])
            assert xmask == (1 << (n - 1 - p)) | (1 << (n - 1 - q)) and amask == 1 << (n - 1 - p)
            assert negate == 0 and zmask == sum(1 << (n - 1 - l) for l in range(min(p, q) + 1, max(p, q)))
            assert check_masks(n, [q], [p], fermionic=False)[2:] == (0, 0)
    # U from the closed form is orthogonal and equals the index formula applied to the identity
    n, theta = 5, 0.73
    spec = excitation_masks(n, [3], [0])
    u = dense_u(n, [3], [0], theta)
    assert np.abs(u.T @ u - np.eye(1 << n)).max() < 1e-14
    assert np.abs(index_rot(np.eye(1 << n), spec, theta).T - u).max() < 1e-15


DOUBLES = ([(c, a) for c in itertools.permutations((2, 3)) for a in itertools.permutations((0, 1))]                # contiguous
           + [(c, a) for c in itertools.permutations((1, 4)) for a in itertools.permutations((0, 5))]             # nested
           + [(c, a) for c in itertools.permutations((1, 3)) for a in itertools.permutations((0, 2))]             # interleaved
           + [(c, a) for c in itertools.permutations((0, 4)) for a in itertools.permutations((2, 5))]             # interleaved
           + [(c, a) for c in itertools.permutations((0, 1)) for a in itertools.permutations((4, 5))]             # downward
           + [(c, a) for c in itertools.permutations((2, 5)) for a in itertools.permutations((1, 3))]
           + [(c, a) for c in itertools.permutations((0, 3)) for a in itertools.permutations((1, 5))])


def test_doubles_and_a_triple_match_the_definition_in_every_sampled_ordering():
    assert len(DOUBLES) >= 24
    seen = set()
    for create, annihilate in DOUBLES:
        spec = check_masks(6, list(create), list(annihilate))
        seen.add(spec[3])
        assert check_masks(6, list(create), list(annihilate), fermionic=False)[2:] == (0, 0)
        # swapping two operators of one kind flips the sign of E
        other = check_masks(6, list(create)[::-1], list(annihilate))
        assert other[:3] == spec[:3] and other[3] == 1 - spec[3]
    assert seen == {0, 1}
    check_masks(6, [1, 4, 2], [5, 0, 3])
    check_masks(6, [5, 3, 0], [1, 2, 4], fermionic=False)
    # controls: inside the string they are folded into the sign, outside they only restrict
    for controls in ((2,), (5,), (2, 4), (0, 2)):
        spec = check_masks(6, [3], [1], controls=controls)
        assert not spec[2] & sum(1 << (5 - c) for c in controls)
    assert check_masks(6, [3], [1], controls=(2,))[3] == 1 and check_masks(6, [3], [1], controls=(0,))[3] == 0
    check_masks(6, [4, 0], [1, 5], controls=(2, 3))


def test_k_projects_onto_exactly_two_and_eight_pauli_strings():
    single = pauli_terms(dense_k(4, [3], [0]), 4)
    assert sorted(s for _, s in single) == ['xzzy', 'yzzx']
    assert all(abs(abs(c) - 0.5) < 1e-15 and abs(c.real) < 1e-15 for c, _ in single)
    double = pauli_terms(dense_k(6, [3, 5], [0, 1]), 6)
    assert len(double) == 8 and all(abs(abs(c) - 0.125) < 1e-15 and abs(c.real) < 1e-15 for c, _ in double)
    # an odd number of Y on the four wires, the string between the second pair of listed wires
    assert all(sum(ch == 'y' for ch in s) % 2 == 1 and s[2] == 'i' and s[4] == 'z' for _, s in double)
    assert len(pauli_terms(dense_k(4, [2], [1], fermionic=False), 4)) == 2
    assert len(pauli_terms(dense_k(4, [2, 3], [0, 1], fermionic=False), 4)) == 8


# ---- the stand-ins, the gate, the circuit, the ansatz -----------------------------------------------------------------
CASES = [
    # n, create, annihilate, controls (wires)
    (2, [1], [0], ()),
    (4, [2, 3], [0, 1], ()),
    (5, [4], [1], (2,)),
    (6, [0, 4], [5, 2], (3, 1)),
    (6, [1, 4, 2], [5, 0, 3], ()),
]


@pytest.mark.parametrize('n,create,annihilate,controls', CASES)
def test_stand_ins_against_the_definition(cpu_backend, n, create, annihilate, controls):
    spec = (*excitation_masks(n, create, annihilate, True, controls), bits_of(n, controls))
    k = dense_k(n, create, annihilate, True, controls)
    a, c = np.array([0.3 - 0.2j, 1.1j]), np.array([-0.6 + 0.1j, 0.4])
    th = np.array([0.7, -3.9])
    for dtype, tol in ((np.complex64, 1e-6), (np.complex128, 1e-14)):
        x, y = random_state(2, n, 3, dtype), random_state(2, n, 4, dtype)
        xd = x.astype(np.complex128)
        want = a[:, None] * xd + c[:, None] * (xd @ k.T)
        got = backend.apply_excite_axpby(tt(x), spec, tt(a), tt(c), 'gate').numpy()
        out = outside(n, spec)
        assert got.dtype == dtype and np.array_equal(got[:, out], x[:, out])
        got[:, out] = want[:, out]
        assert np.abs(got - want).max() <= tol
        assert np.abs(index_axpby(x, spec, a, c) [:, np.setdiff1d(np.arange(1 << n), out)]
                      - want[:, np.setdiff1d(np.arange(1 << n), out)]).max() < 1e-14
        got = backend.apply_excite_axpby(tt(x), spec, tt(a), tt(c), 'map').numpy()
        assert np.all(got[:, out] == 0)
        assert np.abs(got - index_axpby(x, spec, a, c, 'map')).max() <= tol
        # the rotation is the closed form of the definition, per sample
        got = backend.apply_excite_rot(tt(x), spec, tt(th)).numpy()
        for b in range(2):
            assert np.abs(got[b] - dense_u(n, create, annihilate, th[b], True, controls) @ xd[b]).max() <= tol
        # in place: the same bits; 'map' in place too
        z = tt(x.copy())
        assert backend.apply_excite_rot(z, spec, tt(th), out=z) is z and np.array_equal(z.numpy(), got)
        z = tt(x.copy())
        backend.apply_excite_axpby(z, spec, tt(a), tt(c), 'map', out=z)
        assert np.array_equal(z.numpy(), backend.apply_excite_axpby(tt(x), spec, tt(a), tt(c), 'map').numpy())
        # the cross
        want = np.einsum('bi,ij,bj->b', y.astype(np.complex128).conj(), k, xd)
        assert np.abs(backend.excite_cross(tt(y), tt(x), spec).numpy() - want).max() <= tol
        assert np.abs(index_cross(y, x, spec) - want).max() < 1e-14
        same = backend.excite_cross(tt(x), tt(x), spec).numpy()
        assert np.abs(same.real).max() <= tol and np.abs(same - index_cross(x, x, spec)).max() <= tol


def test_backend_refusals(cpu_backend):
    x = tt(random_state(2, 4, 1))
    ok = (0b0110, 0b0100, 0b0001, 0)
    for spec, word in (((0, 0, 0, 0), 'xmask'), ((16, 0, 0, 0), 'xmask'), ((6, 1, 0, 0), 'subset'), ((6, 4, 2, 0), 'share a bit'),
                       ((6, 4, 0, 2), 'negate'), ((6, 4, 0, 0, (1,)), 'disjoint'), ((6, 4, 1, 0, (0,)), 'disjoint'),
                       ((6, 4, 0, 0, (3, 3)), 'distinct'), ((6, 4, 0, 0, (4,)), 'distinct'), ((6, 4, 0), 'spec'), (6, 'spec')):
        with pytest.raises(ValueError, match=word):
            backend.apply_excite_axpby(x, spec, 1.0, 0.5)
        with pytest.raises(ValueError, match=word):
            backend.excite_cross(x, x, spec)
    with pytest.raises(ValueError, match='mode'):
        backend.apply_excite_axpby(x, ok, 1.0, 0.5, mode='scale')
    with pytest.raises(ValueError, match='coefficient'):
        backend.apply_excite_axpby(x, ok, torch.ones(3), 0.5)
    with pytest.raises(ValueError, match='angle'):
        backend.apply_excite_rot(x, ok, torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match='shape'):
        backend.apply_excite_axpby(x, ok, 1.0, 0.5, out=torch.zeros(2, 8, dtype=x.dtype))
    flat = torch.zeros(40, dtype=torch.complex128)
    with pytest.raises(ValueError, match='overlap'):
        backend.apply_excite_axpby(flat[:32].reshape(2, 16), ok, 1.0, 0.5, out=flat[8:].reshape(2, 16))
    with pytest.raises(TypeError):
        backend.apply_excite_axpby(x.real.contiguous(), ok, 1.0, 0.5)
    with pytest.raises(ValueError, match='one shape'):
        backend.excite_cross(x[:1], x, ok)
    out = torch.empty_like(x)
    assert backend.apply_excite_axpby(x, ok, 1.0, 0.5, out=out) is out


def test_qubit_single_is_rbs_and_the_half_angle_convention(cpu_backend):
    n, theta = 4, 0.83
    x = tt(random_state(2, n, 6)).reshape(2, -1, 1)
    for p, q in ((1, 2), (3, 0), (0, 3)):
        a, b = dq.QubitCircuit(n), dq.QubitCircuit(n)
        a.single_excitation([p, q], inputs=torch.tensor(theta, dtype=torch.float64), fermionic=False)
        b.rbs([p, q], inputs=torch.tensor(theta, dtype=torch.float64))
        a.to(torch.double)
        b.to(torch.double)
        assert torch.allclose(a(state=x), b(state=x), atol=1e-14)
    # adjacent wires have no string: the fermionic single is rbs as well
    a, b = dq.QubitCircuit(n), dq.QubitCircuit(n)
    a.single_excitation([1, 2], inputs=torch.tensor(theta, dtype=torch.float64))
    b.rbs([1, 2], inputs=torch.tensor(theta, dtype=torch.float64))
    a.to(torch.double)
    b.to(torch.double)
    assert torch.allclose(a(state=x), b(state=x), atol=1e-14)
    # the half-angle convention: SingleExcitation(phi) on wires [0, 1] is [[1,0,0,0],[0,c,-s,0],[0,s,c,0],[0,0,0,1]],
    # c = cos(phi / 2), s = sin(phi / 2)
    phi = 1.1
    c, s = np.cos(phi / 2), np.sin(phi / 2)
    want = np.array([[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1]])
    g = dq.ExcitationGate([0], [1], nqubit=2, inputs=torch.tensor(phi / 2, dtype=torch.float64), fermionic=False)
    assert np.abs(g.get_unitary().numpy() - want).max() < 1e-15
    g = dq.ExcitationGate([1], [0], nqubit=2, inputs=torch.tensor(-phi / 2, dtype=torch.float64), fermionic=False)
    assert np.abs(g.get_unitary().numpy() - want).max() < 1e-15


def test_gate_circuit_and_ansatz_plumbing(cpu_backend):
    n = 5
    cir = dq.QubitCircuit(n)
    cir.hlayer()
    cir.excitation([3, 4], [0, 1])                               # trainable
    cir.single_excitation([4, 1], encode=True)                   # from data
    cir.double_excitation([0, 2, 3, 4], inputs=0.25, controls=[1])
    cir.rxlayer()
    assert (cir.npara, cir.ndata) == (2 + n, 1)                   # (a fixed angle counts as a parameter, as for every gate)
    assert sum(p.numel() for p in cir.parameters()) == 1 + n
    g_train, g_enc, g_fix = [op for op in cir.operators if isinstance(op, dq.ExcitationGate)]
    assert isinstance(g_train.theta, torch.nn.Parameter) and not isinstance(g_enc.theta, torch.nn.Parameter)
    assert (g_enc.create, g_enc.annihilate, g_enc.name) == ([1], [4], 'single_excitation')
    assert (g_fix.create, g_fix.annihilate, g_fix.controls, g_fix.name) == ([3, 4], [0, 2], [1], 'double_excitation')
    assert float(g_fix.theta) == 0.25 and g_fix.wires == [3, 4, 0, 2]
    assert g_fix.masks() == excitation_masks(n, [3, 4], [0, 2], True, [1]) and len(g_fix.masks()) == 4
    assert g_train._state_like() == (torch.complex64, torch.device('cpu'))
    cir.to(torch.double)
    assert g_train.theta.dtype == torch.float64 and g_train._state_like()[0] == torch.complex128
    inv = g_fix.inverse()
    assert inv.inv_mode and inv.name == 'double_excitation_dagger' and inv.theta is g_fix.theta
    x = tt(random_state(1, n, 2))
    assert torch.allclose(inv.apply_flat(g_fix.apply_flat(x)), x, atol=1e-14)
    u = g_fix.get_unitary().numpy()
    assert np.abs(u - dense_u(n, [3, 4], [0, 2], 0.25, True, [1])).max() < 1e-14
    assert np.abs(inv.get_unitary().numpy() - u.T).max() < 1e-14
    assert np.abs(u.T @ u - np.eye(1 << n)).max() < 1e-14
    # one theta per sample of a data batch
    data = torch.tensor([[0.1], [0.7], [-4.3]], dtype=torch.float64)
    batch = cir(data)
    assert batch.shape == (3, 1 << n, 1)
    for b in range(3):
        assert torch.allclose(cir(data[b]), batch[b], atol=1e-14)
    full = cir.get_unitary()
    assert torch.allclose(full.mH @ full, torch.eye(1 << n, dtype=torch.complex128), atol=1e-12)
    cir.observable(0)
    cir(data[0])
    cir.expectation().sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in cir.parameters())
    assert 'create=[3, 4]' in repr(g_fix) and 'fermionic=True' in repr(g_fix)

    # the ansatz
    for nq, ne in ((4, 2), (6, 2), (6, 3), (5, 1)):
        no, nv = ne, nq - ne
        count = no * nv + (no * (no - 1) // 2) * (nv * (nv - 1) // 2)
        uc = dq.UCCSD(nq, ne)
        assert uc.nparam == count and sum(p.numel() for p in uc.parameters()) == count
        assert [type(op).__name__ for op in uc.operators[ne:]] == ['ExcitationGate'] * count
    uc = dq.UCCSD(4, 2)
    assert uc.singles == [[0, 2], [0, 3], [1, 2], [1, 3]] and uc.doubles == [[0, 1, 2, 3]]
    angles = np.random.default_rng(7).uniform(-2, 2, 5)
    uc = dq.UCCSD(4, 2, inputs=torch.tensor(angles))
    uc.to(torch.double)
    assert sum(p.numel() for p in uc.parameters()) == 0
    psi = np.zeros(16)
    psi[0b1100] = 1.0
    for (i, a), th in zip(uc.singles, angles[:4]):
        psi = dense_u(4, [a], [i], th) @ psi
    psi = dense_u(4, [2, 3], [0, 1], angles[4]) @ psi
    got = uc().reshape(-1).numpy()
    assert np.abs(got - psi).max() < 1e-14
    weight = np.array([bin(i).count('1') for i in range(16)])
    assert np.all(got[weight != 2] == 0)                         # exact zeros stay exact
    with pytest.raises(ValueError, match='angles'):
        dq.UCCSD(4, 2, inputs=[0.1, 0.2])
    with pytest.raises(ValueError, match='nelectron'):
        dq.UCCSD(4, 4)


def test_refusals(cpu_backend):
    make = lambda **kw: dq.ExcitationGate(**{**dict(create=[1], annihilate=[0], nqubit=3), **kw})  # noqa: E731
    for kw in (dict(create=[0]), dict(create=[1, 1]), dict(create=[]), dict(annihilate=[]), dict(create=[3]), dict(annihilate=[-1]),
               dict(controls=[1]), dict(controls=[3]), dict(controls=[2, 2])):
        with pytest.raises(ValueError, match='excitation'):
            make(**kw)
    with pytest.raises(ValueError, match='wires'):
        dq.QubitCircuit(3).single_excitation([0, 1, 2])
    with pytest.raises(ValueError, match='wires'):
        dq.QubitCircuit(4).double_excitation([0, 1, 2])
    with pytest.raises(NotImplementedError, match='ExcitationGate'):
        make(den_mat=True)
    with pytest.raises(NotImplementedError, match='ExcitationGate'):
        make().op_dist_state(None)
    with pytest.raises(NotImplementedError, match='ExcitationGate'):
        make().prims()
    dm = dq.QubitCircuit(3, den_mat=True)
    with pytest.raises(NotImplementedError, match='ExcitationGate'):
        dm.single_excitation([0, 1])
    cir = dq.QubitCircuit(3)
    cir.single_excitation([0, 2])
    with pytest.raises(NotImplementedError, match='ExcitationGate'):
        cir.qasm()


def test_rotation_backward_is_one_rotation_and_one_cross(cpu_backend, monkeypatch):
    calls = []
    for name in ('apply_excite_axpby', 'excite_cross'):
        real = getattr(backend, name)
        monkeypatch.setattr(backend, name, lambda *a, _r=real, _n=name, **k: (calls.append(_n), _r(*a, **k))[1])
    spec = (0b011, 0b001, 0b100, 0)
    x = tt(random_state(2, 3, 1)).requires_grad_()
    th = torch.tensor([0.3, -0.8], dtype=torch.float64, requires_grad=True)
    y = ops.excite_rot(x, spec, th)
    assert calls == ['apply_excite_axpby']
    del calls[:]
    y.backward(tt(random_state(2, 3, 2)))
    assert calls == ['apply_excite_axpby', 'excite_cross']
