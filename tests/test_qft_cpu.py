"""The quantum Fourier transform without a GPU: the new exports by name, the stage count, the library's host-side
refusals, the CPU double route of ``backend.apply_qft`` / ``ops.qft`` against ``_qft_ref``, and the argument refusals."""

import os
import re

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import _lib, backend, ops
from _qft_ref import dft_matrix, qft_ref, random_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('dq_apply_qft_c64', 'dq_apply_qft_c128', 'dq_qft_tile_bits', 'dq_qft_passes')


def test_library_exports_the_new_symbols():
    lib = _lib.load()
    text = open(os.path.join(ROOT, 'include', 'dq_hip.h')).read()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.exported_symbols()
        assert re.search(r'\bint %s\(' % name, text)
    assert lib.dq_qft_tile_bits(0) == 12 and lib.dq_qft_tile_bits(1) == 11
    assert backend.qft_tile_bits(torch.complex64) == 12
    assert hasattr(dq, 'QFTGate') and hasattr(ops, 'qft')


def test_stage_counts_and_refusals():
    lib, ia = _lib.load(), _lib.int_array
    passes = lambda n, bits, c128=0: lib.dq_qft_passes(n, ia(bits), len(bits), c128)
    assert passes(28, range(27, -1, -1)) == 3 and passes(27, range(26, -1, -1), 1) == 3      # 8 + 8 + 12 / 8 + 8 + 11
    assert passes(5, [2]) == 1 and passes(12, range(12)) == 1 and passes(13, range(13)) == 2
    assert passes(20, range(19, 11, -1)) == 1 and passes(20, range(19, 10, -1)) == 2          # 8 wires above the line fill a tile
    assert passes(5, [1, 1]) == -1 and passes(5, [5]) == -1 and passes(5, [-1]) == -1 and passes(5, []) == -1
    assert backend.qft_passes(13, range(13), swaps=True) == 3 and backend.qft_passes(12, range(12), swaps=True) == 1
    with pytest.raises(ValueError, match='distinct'):
        backend.qft_passes(5, [1, 1])


def test_host_side_argument_checks_of_the_library():
    """DQ_ERR_ARG with a text, before any HIP call (no device is touched: the pointers are never dereferenced)."""
    lib, ia = _lib.load(), _lib.int_array
    p, q = 1 << 20, 1 << 30                             # aligned non-null "pointers", far apart

    def refused(rc, word):
        assert rc == -1 and word in lib.dq_last_error().decode(), lib.dq_last_error()

    for f in (lib.dq_apply_qft_c64, lib.dq_apply_qft_c128):
        refused(f(None, q, 3, ia([0]), 1, 0, 1, None), 'null')
        refused(f(p, None, 3, ia([0]), 1, 0, 1, None), 'null')
        refused(f(p + 8, q, 3, ia([0]), 1, 0, 1, None), 'aligned')
        refused(f(p, q + 8, 3, ia([0]), 1, 0, 1, None), 'aligned')
        refused(f(p, q, 41, ia([0]), 1, 0, 1, None), 'n=41')
        refused(f(p, q, 3, ia([0]), 1, 0, 0, None), 'batch')
        refused(f(p, q, 3, ia([0]), 0, 0, 1, None), 'm=0')
        refused(f(p, q, 3, ia([1, 1]), 2, 0, 1, None), 'twice')
        refused(f(p, q, 3, ia([3]), 1, 0, 1, None), 'out of range')
        refused(f(p, q, 3, ia([0]), 1, 4, 1, None), 'inverse=4')
        refused(f(p, q, 14, ia(range(14)), 14, 2, 1, None), 'one stage only')
    # the ranges [in, in + batch * 2^n) and [out, ..): 2 samples of 8 amplitudes are 128 (256) bytes
    refused(lib.dq_apply_qft_c64(p, p + 112, 3, ia([0]), 1, 0, 2, None), 'overlap without being equal')
    refused(lib.dq_apply_qft_c128(p + 240, p, 3, ia([0]), 1, 0, 2, None), 'overlap without being equal')


@pytest.mark.parametrize('n,bits', [(1, (0,)), (5, (2,)), (5, (3, 0)), (4, (0, 2, 3, 1)), (6, (4, 1, 2, 5))])
def test_cpu_double_route_against_the_reference(cpu_backend, n, bits):
    rng = np.random.default_rng(n + len(bits))
    for dtype, tol in ((np.complex64, 1e-6), (np.complex128, 1e-14)):   # (computed in double, rounded once to the dtype)
        x = random_state(rng, 2, n, dtype)
        for inverse in (False, True):
            for swaps in (False, True):
                got = backend.apply_qft(torch.from_numpy(x), bits, inverse, swaps).numpy()
                np.testing.assert_allclose(got, qft_ref(x, bits, inverse, swaps), rtol=0, atol=tol)
    xr = torch.from_numpy(random_state(rng, 2, n, np.complex128)).requires_grad_(True)
    g = torch.from_numpy(random_state(rng, 2, n, np.complex128))
    (gx,) = torch.autograd.grad(ops.qft(xr, bits), xr, g)
    np.testing.assert_allclose(gx.numpy(), qft_ref(g.numpy(), bits, inverse=True), rtol=0, atol=1e-14)


def test_gate_and_circuit_on_the_cpu_route(cpu_backend):
    gate = dq.QFTGate(nqubit=5, wires=[3, 0, 4, 1]).double()
    u = gate.get_unitary().numpy()
    x = random_state(np.random.default_rng(3), 2, 5, np.complex128)
    np.testing.assert_allclose(x @ u.T, qft_ref(x, [1, 4, 0, 3]), rtol=0, atol=1e-14)
    assert gate.inverse().name == 'QFTGate_dagger' and 'wires=[3, 0, 4, 1], swaps=True' in repr(gate)
    np.testing.assert_allclose(gate.inverse().get_unitary().numpy(), u.conj().T, rtol=0, atol=1e-14)
    np.testing.assert_allclose(dq.QFTGate(nqubit=4).double().get_unitary().numpy(), dft_matrix(4), rtol=0, atol=1e-14)
    for reverse in (False, True):
        native = dq.QuantumFourierTransform(6, minmax=[1, 4], reverse=reverse, native=True)
        assert len(native.operators) == 1 and native.operators[0].swaps == (not reverse)
    cir = dq.QubitCircuit(4)
    cir.qft(wires=[2, 0], swaps=False, inverse=True)
    assert cir.operators[0].inv_mode and not cir.operators[0].swaps


def test_refusals_by_name():
    with pytest.raises(ValueError, match='repeated wires'):
        dq.QFTGate(nqubit=4, wires=[1, 1])
    with pytest.raises(NotImplementedError, match='den_mat'):
        dq.QFTGate(nqubit=4, den_mat=True)
    with pytest.raises(NotImplementedError, match='den_mat'):
        dq.QubitCircuit(4, den_mat=True).qft()
    with pytest.raises(ValueError, match='show_barrier'):
        dq.QuantumFourierTransform(4, native=True, show_barrier=True)
