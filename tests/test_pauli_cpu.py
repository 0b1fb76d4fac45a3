"""Host logic of the Pauli-string gates (PauliRot, PauliEvolution, ops.pauli_*) without a GPU: the kernels' stand-ins are
the plain-torch complex128 routes of ``backend.apply_pauli_axpby / apply_pauli_rot / pauli_cross`` under the CPU test
double, so what is checked here is the string parsing, the wire-to-mask mapping, the validation, the autograd rules
and the bookkeeping."""

import os
import re

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import _lib, backend, ops
from _pauli_ref import axpby_ref, cross_ref, dense_pauli, masks_of, pauli_apply, rot_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rand_state(batch, n, seed=0, dtype=torch.complex128):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, 1 << n, dtype=torch.complex128, generator=g).to(dtype)


def test_library_exports_the_new_symbols_and_still_reports_abi_30():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 30 and lib.dq_abi_version() == 30
    names = ['dq_pauli_cross_ws_bytes'] + [f'dq_{f}_{s}' for f in ('apply_pauli_axpby', 'pauli_cross') for s in ('c64', 'c128')]
    for name in names:
        assert hasattr(lib, name) and name in _lib.exported_symbols()
    text = open(os.path.join(ROOT, 'include', 'dq_hip.h')).read()
    assert re.search(r'#define DQ_ABI_VERSION 30\b', text)
    assert re.search(r'#define DQ_PAULI_GATE %d\b' % _lib.PAULI_GATE, text)
    assert re.search(r'#define DQ_PAULI_MAP %d\b' % _lib.PAULI_MAP, text)
    for name in ('PauliRot', 'PauliEvolution'):
        assert hasattr(dq, name)
    # one partial sum (re, im) per workgroup and sample, at most 2048 workgroups; a unit is 2^10 vectors of 16 bytes
    assert lib.dq_pauli_cross_ws_bytes(1, 1, 0, 0) == 16
    assert lib.dq_pauli_cross_ws_bytes(3, 1, 1, 0) == 16
    assert lib.dq_pauli_cross_ws_bytes(14, 3, 0, 1) == 3 * 8 * 16
    assert lib.dq_pauli_cross_ws_bytes(14, 3, 1, 1) == 3 * 16 * 16
    assert lib.dq_pauli_cross_ws_bytes(30, 2, 0, 0) == 2 * 2048 * 16
    assert lib.dq_pauli_cross_ws_bytes(0, 1, 0, 0) == -1 and lib.dq_pauli_cross_ws_bytes(41, 1, 0, 0) == -1
    assert lib.dq_pauli_cross_ws_bytes(5, 65536, 0, 0) == -1 and lib.dq_pauli_cross_ws_bytes(5, 0, 0, 0) == -1


def test_host_side_argument_checks_of_the_library():
    """DQ_ERR_ARG with a text, before any HIP call (no device is touched: the pointers are never dereferenced)."""
    lib = _lib.load()
    ia = _lib.int_array
    p = 4096                                                            # a 16-byte aligned non-null "pointer"
    ax, cr = lib.dq_apply_pauli_axpby_c64, lib.dq_pauli_cross_c128

    def refused(rc, word):
        assert rc == -1 and word in lib.dq_last_error().decode(), lib.dq_last_error()

    refused(ax(None, p, 1, 0, p, 0, 3, ia([]), 0, 1, None), 'null')
    refused(ax(p, p, 1, 0, None, 0, 3, ia([]), 0, 1, None), 'null')
    refused(ax(p, p, 1, 0, p, 2, 3, ia([]), 0, 1, None), 'mode')
    refused(ax(p, p, 1, 0, p, 0, 0, ia([]), 0, 1, None), 'n=0')
    refused(ax(p, p, 1, 0, p, 0, 41, ia([]), 0, 1, None), 'n=41')
    refused(ax(p, p, 8, 0, p, 0, 3, ia([]), 0, 1, None), 'at or above')
    refused(ax(p, p, 0, 8, p, 0, 3, ia([]), 0, 1, None), 'at or above')
    refused(ax(p, p, 1, 0, p, 0, 3, ia([3]), 1, 1, None), 'out of range')
    refused(ax(p, p, 1, 0, p, 0, 3, ia([1, 1]), 2, 1, None), 'twice')
    refused(ax(p, p, 1, 2, p, 0, 3, ia([1]), 1, 1, None), 'control')
    refused(ax(p, p, 1, 0, p, 0, 3, ia([]), 0, 0, None), 'batch')
    refused(ax(p + 8, p, 1, 0, p, 0, 3, ia([]), 0, 1, None), 'aligned')
    refused(cr(None, p, 1, 0, 3, ia([]), 0, 1, p, p, 16, None), 'null')
    refused(cr(p, p, 1, 0, 3, ia([]), 0, 1, p, None, 16, None), 'null')
    refused(cr(p, p, 8, 0, 3, ia([]), 0, 1, p, p, 16, None), 'at or above')
    refused(cr(p, p, 1, 0, 3, ia([0]), 1, 1, p, p, 16, None), 'control')
    refused(cr(p, p, 1, 0, 3, ia([]), 0, 1, p, p, 15, None), 'workspace')
    refused(cr(p, p, 1, 0, 12, ia([]), 0, 2, p, p, 2 * 4 * 16 - 1, None), 'workspace')


def test_string_parsing_and_the_wire_to_mask_mapping(cpu_backend):
    n = 5
    g = dq.PauliRot('xIyZ', nqubit=n, wires=[4, 2, 0, 1], inputs=0.3)
    assert g.pauli == 'xyz' and g.wires == [4, 0, 1]                   # identity letters drop out
    assert g.masks() == (0b10001, 0b11000)                              # wire 0 = the most significant bit; Y in both
    assert dq.PauliRot('zzzzz', nqubit=n).masks() == (0, 31)            # wires=None: all wires
    assert dq.PauliRot('Y', nqubit=n, wires=3).masks() == (2, 2)
    for pauli, wires in (('xyz', [0, 1, 2]), ('yixz', [3, 1, 4, 0]), ('y', [2]), ('yyy', [4, 0, 2])):
        xmask, zmask = masks_of(n, pauli, wires)
        gate = dq.PauliRot(pauli, nqubit=n, wires=wires, inputs=0.0)
        assert gate.masks() == (xmask, zmask)
        eye = np.eye(1 << n)
        assert np.array_equal(pauli_apply(eye, xmask, zmask).T, dense_pauli(n, pauli, wires))  # the formula is the Kronecker product
    with pytest.raises(ValueError):
        dq.PauliRot('iii', nqubit=3)
    with pytest.raises(ValueError):
        dq.PauliRot('xq', nqubit=2)
    with pytest.raises(ValueError):
        dq.PauliRot('xy', nqubit=3, wires=[0])
    with pytest.raises(AssertionError):
        dq.PauliRot('xy', nqubit=3, wires=[0, 0])
    with pytest.raises(AssertionError):
        dq.PauliRot('xy', nqubit=3, wires=[0, 1], controls=[1])        # a control inside the string
    dq.PauliRot('xi', nqubit=3, wires=[0, 1], controls=[1])            # an identity letter leaves its wire free


def test_backend_stand_ins_against_numpy(cpu_backend):
    n = 5
    x, y = rand_state(2, n, 1), rand_state(2, n, 2)
    a = torch.tensor([0.3 - 2j, 1.5j], dtype=torch.complex128)
    c = torch.tensor([-1.1 + 0.2j, 0.7], dtype=torch.complex128)
    for xmask, zmask, controls in ((0, 5, ()), (1, 0, (3,)), (0b10010, 0b10100, (0, 3)), (31, 31, ()), (0b01100, 0b00110, (4,))):
        for mode in ('gate', 'map'):
            got = backend.apply_pauli_axpby(x, xmask, zmask, a, c, controls, mode).numpy()
            assert np.allclose(got, axpby_ref(x.numpy(), xmask, zmask, a.numpy(), c.numpy(), controls, mode), atol=1e-14)
        assert np.allclose(backend.pauli_cross(x, y, xmask, zmask, controls).numpy(), cross_ref(x.numpy(), y.numpy(), xmask, zmask, controls),
                           atol=1e-13)
        th = torch.tensor([0.4, -2.2], dtype=torch.float64)
        assert np.allclose(backend.apply_pauli_rot(x, xmask, zmask, th, controls).numpy(), rot_ref(x.numpy(), xmask, zmask, th.numpy(), controls),
                           atol=1e-14)
    same = x.clone()
    assert backend.apply_pauli_axpby(same, 6, 3, a, c, out=same) is same
    assert np.allclose(same.numpy(), axpby_ref(x.numpy(), 6, 3, a.numpy(), c.numpy()), atol=1e-14)
    assert np.allclose(backend.apply_pauli_axpby(x, 6, 3, 2.0, -1j).numpy(), axpby_ref(x.numpy(), 6, 3, 2.0, -1j), atol=1e-14)
    for bad in (dict(xmask=32), dict(zmask=-1), dict(controls=[5]), dict(controls=[1, 1]), dict(xmask=2, controls=[1]),
                dict(zmask=4, controls=[2]), dict(mode='scale'), dict(a=torch.ones(3))):
        kw = dict(xmask=1, zmask=0, a=a, c=c, controls=(), mode='gate')
        kw.update(bad)
        with pytest.raises(ValueError):
            backend.apply_pauli_axpby(x, **kw)
    with pytest.raises(ValueError):
        backend.pauli_cross(x, y[:1], 1, 0)
    with pytest.raises(ValueError):
        backend.pauli_cross(x, y, 1, 0, [0])
    with pytest.raises(ValueError):
        backend.apply_pauli_rot(x, 1, 0, torch.zeros(3, dtype=torch.float64))


def test_one_parameter_gate_bookkeeping(cpu_backend):
    n = 3
    cir = dq.QubitCircuit(n)
    cir.hlayer()
    cir.pauli_rot('xyz')                                   # trainable
    cir.pauli_rot('zx', wires=[2, 0], encode=True)         # from data
    cir.pauli_rot('y', wires=[1], inputs=0.25, controls=[0])
    assert (cir.npara, cir.ndata) == (2, 1)
    g_train, g_enc, g_fix = cir.operators[-3:]
    assert isinstance(g_train.theta, torch.nn.Parameter) and not isinstance(g_enc.theta, torch.nn.Parameter)
    assert [p is g_train.theta for p in cir.parameters()] == [True]
    assert float(g_fix.theta) == 0.25
    assert g_train._state_like() == (torch.complex64, torch.device('cpu'))
    cir.to(torch.double)
    assert g_train.theta.dtype == torch.float64 and g_train._state_like()[0] == torch.complex128
    before = g_train.theta.item()
    cir.init_para()
    assert g_train.theta.item() != before
    inv = g_fix.inverse()
    assert inv.inv_mode and inv.name == 'pauli_rot_dagger' and inv.theta is g_fix.theta
    x = rand_state(1, n)
    assert torch.allclose(inv.apply_flat(g_fix.apply_flat(x)), x, atol=1e-14)
    data = torch.tensor([[0.1], [0.7], [-1.3]], dtype=torch.float64)
    batch = cir(data)
    assert batch.shape == (3, 1 << n, 1)
    for b in range(3):
        assert torch.allclose(cir(data[b]), batch[b], atol=1e-14)
    u = cir.get_unitary()
    assert torch.allclose(u[:, 0], cir(data[2]).reshape(-1), atol=1e-13)
    assert torch.allclose(u.mH @ u, torch.eye(1 << n, dtype=torch.complex128), atol=1e-6)
    # the gate against the dense exponential
    g = dq.PauliRot('yzx', nqubit=n, wires=[2, 0, 1], inputs=torch.tensor(0.9, dtype=torch.float64))
    dense = torch.linalg.matrix_exp(-0.45j * torch.from_numpy(dense_pauli(n, 'yzx', [2, 0, 1])))
    assert torch.allclose(g.get_unitary(), dense, atol=1e-14)
    assert torch.allclose(g.inverse().get_unitary(), dense.mH, atol=1e-14)


def test_pauli_evolution_bookkeeping(cpu_backend):
    n = 4
    ham = [[0.5, 'x0x1'], [-0.25, 'y0y1'], [0.75, 'z0z1'], [1.5, 'z3']]
    t = torch.tensor(0.37, dtype=torch.float64)
    g = dq.PauliEvolution(ham, t=t, nqubit=n, steps=3, order=2)
    assert (g.steps, g.order, g.npara, g.wires) == (3, 2, 1, [0, 1, 3])
    assert [term[1:] for term in g.terms] == [('xx', [0, 1]), ('yy', [0, 1]), ('zz', [0, 1]), ('z', [3])]
    assert g.slice_sequence() == [(0, 0.5), (1, 0.5), (2, 0.5), (3, 1.0), (2, 0.5), (1, 0.5), (0, 0.5)]
    assert dq.PauliEvolution(ham, t=t, nqubit=n).slice_sequence() == [(0, 1.0), (1, 1.0), (2, 1.0), (3, 1.0)]
    assert dq.PauliEvolution(ham, t=t, nqubit=n).inverse().slice_sequence() == [(3, 1.0), (2, 1.0), (1, 1.0), (0, 1.0)]
    # commuting terms: exact at any steps and order
    h = sum(c * dense_pauli(n, s[0::2], [int(w) for w in s[1::2]]) for c, s in ham)
    exact = torch.linalg.matrix_exp(-1j * float(t) * torch.from_numpy(h))
    for steps, order in ((1, 1), (3, 1), (2, 2)):
        u = dq.PauliEvolution(ham, t=t, nqubit=n, steps=steps, order=order).get_unitary()
        assert torch.allclose(u, exact, atol=1e-13)
    # non-commuting terms: the product formula itself, slice by slice
    ham2 = [[0.8, 'x0z2'], [-0.6, 'y2'], [0.3, 'z0y1x3']]
    x = rand_state(1, n, 5)
    for steps, order in ((1, 1), (3, 1), (1, 2), (3, 2)):
        gate = dq.PauliEvolution(ham2, t=t, nqubit=n, steps=steps, order=order)
        ref = x.numpy()
        for _ in range(steps):
            for j, share in gate.slice_sequence():
                coef, letters, ws = gate.terms[j]
                ref = rot_ref(ref, *masks_of(n, letters, ws), 2 * coef * float(t) * share / steps)
        assert np.allclose(gate.apply_flat(x).numpy(), ref, atol=1e-14)
        assert torch.allclose(gate.inverse().apply_flat(gate.apply_flat(x)), x, atol=1e-13)
    # one shared t: trainable, encoded, differentiable
    cir = dq.QubitCircuit(n)
    cir.hlayer()
    cir.pauli_evolution(ham2, steps=2, order=2)
    cir.pauli_evolution(ham, encode=True)
    assert (cir.npara, cir.ndata) == (1, 1) and isinstance(cir.operators[-2].t, torch.nn.Parameter)
    cir.to(torch.double)
    tt = torch.tensor(0.21, dtype=torch.float64, requires_grad=True)
    f = lambda v: dq.PauliEvolution(ham2, t=v, nqubit=n, steps=2, order=2).apply_flat(x)  # noqa: E731
    assert torch.autograd.gradcheck(f, (tt,))
    for bad in (dict(hamiltonian=[[1.0, 'x0y0']]), dict(hamiltonian=[[1.0, 'x4']]), dict(hamiltonian=[]), dict(hamiltonian=[[1.0, '']]),
                dict(order=3), dict(steps=0)):
        kw = dict(hamiltonian=ham, nqubit=n)
        kw.update(bad)
        with pytest.raises(ValueError):
            dq.PauliEvolution(**kw)


def test_refusals(cpu_backend):
    for make in (lambda **kw: dq.PauliRot('xy', nqubit=2, **kw), lambda **kw: dq.PauliEvolution([[1.0, 'x0y1']], nqubit=2, **kw)):
        name = type(make()).__name__
        with pytest.raises(NotImplementedError, match=name):
            make(den_mat=True)
        with pytest.raises(NotImplementedError, match=name):
            make().op_dist_state(None)
        with pytest.raises(NotImplementedError, match=name):
            make().prims()
        dm = dq.QubitCircuit(2, den_mat=True)
        with pytest.raises(NotImplementedError, match=name):
            dm.add(make())
            dm()
        cir = dq.QubitCircuit(2)
        cir.add(make())
        with pytest.raises(NotImplementedError, match=name):
            cir.qasm()


def test_rotation_backward_is_one_axpby_and_one_cross(cpu_backend, monkeypatch):
    """With gradients for the state and the angle, the backward of ``ops.pauli_rot`` passes over the state twice: the
    rotation of the cotangent and one cross reduction of it with the saved input -- the forward is not formed again."""
    calls = []
    for name in ('apply_pauli_rot', 'apply_pauli_axpby', 'pauli_cross'):
        real = getattr(backend, name)
        monkeypatch.setattr(backend, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    x = rand_state(2, 4, 3).requires_grad_()
    th = torch.tensor([0.3, -0.8], dtype=torch.float64, requires_grad=True)
    y = ops.pauli_rot(x, 0b1010, 0b0110, th, (0,))
    assert [c for c in calls if c != 'apply_pauli_axpby'] == ['apply_pauli_rot']      # (the stand-in of rot goes through axpby)
    calls.clear()
    y.abs().pow(2).mul(torch.arange(16.0)).sum().backward()
    assert [c for c in calls if c != 'apply_pauli_axpby'] == ['apply_pauli_rot', 'pauli_cross']
    assert calls.count('apply_pauli_axpby') == 1                                       # ... and nothing beside it
    assert th.grad.abs().min().item() > 1e-3


def test_out_is_the_state_or_disjoint_and_the_parameter_keeps_the_circuit_precision(cpu_backend):
    x = rand_state(1, 3)
    flat = torch.zeros(12, dtype=torch.complex128)
    for call in (lambda out: backend.apply_pauli_axpby(flat[:8].reshape(1, 8), 1, 0, 1.0, 1j, out=out),
                 lambda out: backend.apply_pauli_rot(flat[:8].reshape(1, 8), 1, 0, torch.zeros(1, dtype=torch.float64), out=out)):
        with pytest.raises(ValueError, match='overlaps'):
            call(flat[4:].reshape(1, 8))
        with pytest.raises(ValueError, match='shape'):
            call(torch.zeros(1, 4, dtype=torch.complex128))
        with pytest.raises(ValueError, match='shape'):
            call(torch.zeros(1, 8, dtype=torch.complex64))
        assert call(flat[:8].reshape(1, 8)).data_ptr() == flat.data_ptr()
    # float64 data on a complex64 circuit: the parameter, and with it get_unitary(), stays in the circuit's precision
    cir = dq.QubitCircuit(3)
    cir.pauli_rot('xy', wires=[0, 2], encode=True)
    cir.pauli_evolution([[0.5, 'z0x1']], encode=True)
    cir(torch.tensor([0.3, 0.7], dtype=torch.float64), state=x.to(torch.complex64).reshape(-1, 1))
    assert cir.operators[0].theta.dtype == torch.float32 and cir.operators[1].t.dtype == torch.float32
    assert cir.get_unitary().dtype == torch.complex64
