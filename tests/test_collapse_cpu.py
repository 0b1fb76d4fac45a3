"""Mid-circuit measurement without a GPU: the new symbols, the host refusals of ``dq_apply_collapse_*`` /
``dq_measure_draw`` before any HIP call, and the host logic of ``Measure`` / ``cir.mid_measure`` under the CPU test double
(whose collapse is ``_standin.collapse``)."""

import ctypes
import re

import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import _lib, backend, qmath


def test_symbols_and_record_layout():
    lib = _lib.load()
    names = ['dq_measure_draw', 'dq_apply_collapse_c64', 'dq_apply_collapse_c128', 'dq_collapse_rec_layout']
    assert set(names) <= set(_lib.exported_symbols()) and all(hasattr(lib, name) for name in names)
    assert lib.dq_abi_version() == 30 == _lib.ABI_VERSION
    got = (ctypes.c_int * 8)()
    r = _lib.DqCollapseRec
    assert lib.dq_collapse_rec_layout(got, 8) == 6
    assert list(got[:6]) == [ctypes.sizeof(r), r.outcome.offset, r.xmask.offset, r.zmask.offset, r.scale.offset, r.prob.offset]
    assert ctypes.sizeof(r) == 40                                       # a row of CollapseRec.data: five 8-byte words


A, O, R = 0x1000, 0x100000, 0x200000        # never dereferenced: every call below is refused on the host
REFUSALS = [
    pytest.param(dict(inp=0), 'null', id='null'),
    pytest.param(dict(out=O + 8), '16-byte aligned', id='unaligned'),
    pytest.param(dict(k=0), r'k=0 outside \[1, 20\]', id='k0'),
    pytest.param(dict(k=21, n=30), r'k=21 outside \[1, 20\].*dq_sample', id='k21'),
    pytest.param(dict(n=41), r'n=41 out of range', id='n41'),
    pytest.param(dict(batch=0), r'batch=0 outside', id='batch0'),
    pytest.param(dict(batch=65536), r'batch=65536 outside', id='batch65536'),
    pytest.param(dict(out=A + 64), 'overlap without being equal', id='overlap'),
    pytest.param(dict(out=A, layout=1), r'overlap \(out of place only\)', id='drop_in_place'),
    pytest.param(dict(out=A, flip=1), 'in place with an x table', id='in_place_with_x'),
    pytest.param(dict(bits=[1, 1], k=2), 'used twice', id='repeated_bit'),
    pytest.param(dict(layout=1, k=4, bits=[0, 1, 2, 3]), 'leaves no state', id='drop_all'),
]


@pytest.mark.parametrize('suffix', ['c64', 'c128'])
@pytest.mark.parametrize('change,message', REFUSALS)
def test_host_refusals_before_any_hip_call(suffix, change, message):
    lib = _lib.load()
    a = dict(inp=A, out=O, rec=R, n=4, bits=[2], k=1, layout=0, transpose=0, flip=0, batch=2)
    a.update(change)
    bits = a['bits'] + list(range(3, a['k'] + 2)) if len(a['bits']) < a['k'] else a['bits']
    rc = getattr(lib, f'dq_apply_collapse_{suffix}')(a['inp'], a['out'], a['rec'], a['n'], _lib.int_array(bits), a['k'], a['layout'],
                                                    a['transpose'], a['flip'], a['batch'], None)
    assert rc == -1
    assert re.search(message, lib.dq_last_error().decode()), lib.dq_last_error()


def test_correction_tables():
    fx, fz = qmath.collapse_tables(4, [1, 2], {'01': 'x3', 2: 'z0y3', '11': 'x0x3'})
    assert fx == [0, 1, 1, 9] and fz == [0, 0, 9, 0]
    fx2, fz2 = qmath.collapse_tables(4, [1, 2], lambda o: [None, 'x3', 'z0y3', 'X0 x3'][o])
    assert (fx2, fz2) == (fx, fz)
    fx, fz = qmath.collapse_tables(4, [1, 2], {'10': 'z0'}, reset=True)
    assert fx == [0, 2, 4, 6] and fz == [0, 0, 8, 0]
    assert qmath.collapse_tables(4, [1, 2]) == (None, None)
    for bad, message in [({'012': 'x0'}, 'string of 2 bits'), ({4: 'x0'}, r'not an int in \[0, 4\)'), ({0: 'x9'}, 'outside'),
                         ({0: 'q1'}, 'not a Pauli string'), ('x0', 'dict or a callable')]:
        with pytest.raises(ValueError, match=message):
            qmath.collapse_tables(4, [1, 2], bad)


def teleport(dtype=torch.complex128):
    cir = dq.QubitCircuit(3)
    cir.h(1)
    cir.cnot(1, 2)
    cir.cnot(0, 1)
    cir.h(0)
    cir.mid_measure([0, 1], correct={'00': '', '01': 'x2', '10': 'z2', '11': 'x2z2'})
    cir.rz(2)
    cir.mid_measure(2)
    return cir.to(torch.double) if dtype == torch.complex128 else cir


def test_teleportation_and_outcomes_under_the_double(cpu_backend):
    torch.manual_seed(0)
    a = torch.randn(8, 2, dtype=torch.complex128)
    a = a / a.norm(dim=1, keepdim=True)
    state = torch.zeros(8, 8, dtype=torch.complex128)
    state[:, 0], state[:, 4] = a[:, 0], a[:, 1]
    cir = teleport()
    assert cir.outcomes == [None, None]
    bell = dq.QubitCircuit(3)
    for op in list(cir.operators)[:5]:
        bell.add(op)
    with torch.no_grad():
        mid = bell(state=state.reshape(8, 8, 1)).reshape(8, 8)
        out = cir(state=state.reshape(8, 8, 1)).reshape(8, 8)
    first, second = cir.outcomes
    assert first.shape == second.shape == (8,) and first.dtype == torch.int64 and second.max() <= 1 < first.max()
    p1, p2 = cir.outcome_probs
    assert p1.dtype == torch.float64 and torch.allclose(p1, torch.full((8,), 0.25, dtype=torch.float64), atol=1e-14)
    rho = qmath.reduced_density_matrix(mid, 3, [2])
    assert torch.allclose(rho, a[:, :, None] * a[:, None, :].conj(), atol=1e-14)
    assert torch.allclose(p2, (a[torch.arange(8), second].abs() ** 2), atol=1e-14)
    assert torch.allclose(out.abs().sum(-1), torch.ones(8, dtype=torch.float64), atol=1e-14)    # one basis state is left


def test_refusals_by_name(cpu_backend):
    with pytest.raises(NotImplementedError, match='den_mat'):
        dq.QubitCircuit(3, den_mat=True).mid_measure(0)
    with pytest.raises(NotImplementedError, match='den_mat'):
        dq.Measure(3, [0], den_mat=True)
    gate = dq.Measure(3, [0])
    for call, name in [(gate.inverse, 'inverse'), (gate.get_unitary, 'get_unitary'), (gate.prims, 'DistributedQubitCircuit'),
                       (lambda: gate.op_dist_state(None), 'DistributedQubitCircuit'), (lambda: gate.op_mps(None), 'MPS')]:
        with pytest.raises(NotImplementedError, match=name):
            call()
    cir = teleport()
    with pytest.raises(NotImplementedError, match='inverse'):
        cir.inverse()
    with pytest.raises(NotImplementedError, match='get_unitary'):
        cir.get_unitary()
    with pytest.raises(ValueError, match='leaves no state'):
        qmath.collapse_state(torch.ones(4, dtype=torch.complex128), 2, [0, 1], drop=True)
    with pytest.raises(ValueError, match='at most 20'):
        qmath.collapse_tables(24, list(range(21)))
