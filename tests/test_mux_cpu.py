"""Host logic of the multiplexed one-qubit gates (MultiplexedGate, MultiplexedRotation, ops.mux_apply, backend.apply_mux,
QubitCircuit.prepare_state) without a GPU: the kernel's stand-in is the plain-torch route of ``backend.apply_mux`` under
the CPU test double, so what is checked here is the library's argument checks, the wire-to-bit mapping, the validation of
tables, the autograd rules and the bookkeeping."""

import io
import os
import pickle
import re

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import _lib, backend, ops
from _mux_ref import block_diag, mux_ref, random_cs, random_state, random_unitaries, ry_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('dq_apply_mux_c64', 'dq_apply_mux_c128')


def tt(a):
    return torch.from_numpy(np.asarray(a))


def test_library_exports_the_new_symbols_and_still_reports_abi_30():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 30 and lib.dq_abi_version() == 30
    text = open(os.path.join(ROOT, 'include', 'dq_hip.h')).read()
    assert re.search(r'#define DQ_ABI_VERSION 30\b', text)
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.exported_symbols()
        assert re.search(r'\bint %s\(' % name, text)
    assert re.search(r'#define DQ_MUX_U %d\b' % _lib.MUX_U, text) and re.search(r'#define DQ_MUX_RY %d\b' % _lib.MUX_RY, text)
    assert (_lib.MUX_U, _lib.MUX_RY) == (0, 1)
    assert hasattr(dq, 'MultiplexedGate') and hasattr(dq, 'MultiplexedRotation')


def test_host_side_argument_checks_of_the_library():
    """DQ_ERR_ARG with a text, before any HIP call (no device is touched: the pointers are never dereferenced)."""
    lib = _lib.load()
    ia = _lib.int_array
    p, q, t = 1 << 20, 1 << 30, 4096                    # aligned non-null "pointers", far apart

    def refused(rc, word):
        assert rc == -1 and word in lib.dq_last_error().decode(), lib.dq_last_error()

    # f(in, out, table, kind, dagger, n, target, bits, k, controls, nc, batch, stream)
    for f in (lib.dq_apply_mux_c64, lib.dq_apply_mux_c128):
        refused(f(None, q, t, 0, 0, 3, 0, ia([1]), 1, ia([]), 0, 1, None), 'null')
        refused(f(p, None, t, 0, 0, 3, 0, ia([1]), 1, ia([]), 0, 1, None), 'null')
        refused(f(p, q, None, 0, 0, 3, 0, ia([1]), 1, ia([]), 0, 1, None), 'null')
        refused(f(p + 8, q, t, 0, 0, 3, 0, ia([1]), 1, ia([]), 0, 1, None), 'aligned')
        refused(f(p, q + 8, t, 0, 0, 3, 0, ia([1]), 1, ia([]), 0, 1, None), 'aligned')
        refused(f(p, q, t + 8, 1, 0, 3, 0, ia([1]), 1, ia([]), 0, 1, None), 'aligned')
        refused(f(p, q, t, 0, 0, 1, 0, ia([1]), 1, ia([]), 0, 1, None), 'n=1')
        refused(f(p, q, t, 0, 0, 0, 0, ia([1]), 1, ia([]), 0, 1, None), 'n=0')
        refused(f(p, q, t, 0, 0, 41, 0, ia([1]), 1, ia([]), 0, 1, None), 'n=41')
        refused(f(p, q, t, 0, 0, 3, 0, ia([1]), 0, ia([]), 0, 1, None), 'k=0')
        refused(f(p, q, t, 0, 0, 3, 0, ia([1]), -1, ia([]), 0, 1, None), 'k=-1')
        refused(f(p, q, t, 0, 0, 3, 0, ia([0, 1, 2]), 3, ia([]), 0, 1, None), 'k=3')              # k > n - 1
        refused(f(p, q, t, 0, 0, 3, 3, ia([1]), 1, ia([]), 0, 1, None), 'target 3')
        refused(f(p, q, t, 0, 0, 3, -1, ia([1]), 1, ia([]), 0, 1, None), 'target -1')
        refused(f(p, q, t, 0, 0, 3, 0, ia([3]), 1, ia([]), 0, 1, None), 'out of range')
        refused(f(p, q, t, 0, 0, 3, 0, ia([-1]), 1, ia([]), 0, 1, None), 'out of range')
        refused(f(p, q, t, 0, 0, 3, 0, ia([1]), 1, ia([3]), 1, 1, None), 'out of range')
        refused(f(p, q, t, 0, 0, 4, 0, ia([1, 1]), 2, ia([]), 0, 1, None), 'twice')
        refused(f(p, q, t, 0, 0, 4, 0, ia([1]), 1, ia([2, 2]), 2, 1, None), 'twice')
        refused(f(p, q, t, 0, 0, 4, 0, ia([1, 2]), 2, ia([2]), 1, 1, None), 'twice')              # a control among the selects
        refused(f(p, q, t, 0, 0, 3, 1, ia([1]), 1, ia([]), 0, 1, None), 'is the target')          # the target among the selects
        refused(f(p, q, t, 0, 0, 3, 2, ia([1]), 1, ia([2]), 1, 1, None), 'is the target')         # .. among the controls
        refused(f(p, q, t, 0, 0, 3, 0, ia([1]), 1, ia([]), 0, 0, None), 'batch')
        refused(f(p, q, t, 0, 0, 3, 0, ia([1]), 1, ia([]), 0, 65536, None), 'batch')
        refused(f(p, q, t, 2, 0, 3, 0, ia([1]), 1, ia([]), 0, 1, None), 'kind')
        refused(f(p, q, t, -1, 0, 3, 0, ia([1]), 1, ia([]), 0, 1, None), 'kind')
        refused(f(p, q, t, 0, 2, 3, 0, ia([1]), 1, ia([]), 0, 1, None), 'dagger')
        refused(f(p, q, t, 1, -1, 3, 0, ia([1]), 1, ia([]), 0, 1, None), 'dagger')
    # the ranges [in, in + batch * 2^n) and [out, ..): 2 samples of 8 amplitudes are 128 (256) bytes
    refused(lib.dq_apply_mux_c64(p, p + 112, t, 0, 0, 3, 0, ia([1]), 1, ia([]), 0, 2, None), 'overlap')
    refused(lib.dq_apply_mux_c64(p + 112, p, t, 0, 0, 3, 0, ia([1]), 1, ia([]), 0, 2, None), 'overlap')
    refused(lib.dq_apply_mux_c128(p, p + 240, t, 0, 0, 3, 0, ia([1]), 1, ia([]), 0, 2, None), 'overlap')


CASES = [
    # n, target, bits, controls
    (2, 0, (1,), ()),
    (2, 1, (0,), ()),
    (5, 2, (3, 0, 4), ()),              # unsorted, on both sides of the target
    (5, 0, (2,), ()),                   # k = 1
    (4, 1, (3, 2, 0), ()),              # k = n - 1
    (4, 3, (0, 2, 1), ()),              # k = n - 1, the target on top
    (5, 4, (1, 3), (0,)),               # one control
    (6, 3, (4, 1), (5, 0)),             # two controls, one on each side
]


@pytest.mark.parametrize('n,target,bits,controls', CASES)
def test_stand_in_against_the_definition(cpu_backend, n, target, bits, controls):
    k = len(bits)
    for dtype, tol in ((np.complex64, 1e-5), (np.complex128, 1e-13)):
        x = random_state(2, n, 3, dtype)
        u, cs = random_unitaries(k, 4), random_cs(k, 5)
        for dagger in (False, True):
            want = mux_ref(x, u, target, bits, controls, dagger)
            got = backend.apply_mux(tt(x), tt(u), 'u', target, bits, controls, dagger=dagger).numpy()
            assert got.dtype == dtype and np.abs(got - want).max() <= tol * np.abs(want).max()
            want = mux_ref(x, ry_blocks(cs), target, bits, controls, dagger)
            got = backend.apply_mux(tt(x), tt(cs), 'ry', target, bits, controls, dagger=dagger).numpy()
            assert got.dtype == dtype and np.abs(got - want).max() <= tol * np.abs(want).max()
            got = ops.mux_apply(tt(x), tt(cs), 'ry', target, bits, controls, dagger=dagger).numpy()
            assert np.abs(got - want).max() <= tol * np.abs(want).max()
        # in place
        y = tt(x.copy())
        assert backend.apply_mux(y, tt(u), 'u', target, bits, controls, out=y) is y
        assert np.abs(y.numpy() - mux_ref(x, u, target, bits, controls)).max() <= tol * np.abs(x).max() * 2


def test_backend_refusals(cpu_backend):
    x = tt(random_state(2, 4, 1, np.complex128))
    u, cs = tt(random_unitaries(2, 1)), tt(random_cs(2, 1))
    ok = dict(table=u, kind='u', target=0, bits=(1, 2), controls=())
    for bad, word in ((dict(bits=(1, 1)), 'distinct'), (dict(bits=(1, 4)), 'distinct'), (dict(controls=(2,)), 'distinct'),
                      (dict(target=1), 'distinct'), (dict(target=4), 'distinct'), (dict(controls=(0,)), 'distinct'),
                      (dict(bits=()), 'at least one'), (dict(kind='rz'), 'kind'), (dict(table=u[:2]), 'select bits'),
                      (dict(table=u.real), 'complex'), (dict(table=cs), 'select bits'), (dict(kind='ry'), 'real'),
                      (dict(kind='ry', table=cs[:3]), 'select bits'), (dict(table=u.clone().requires_grad_()), 'constant'),
                      (dict(table=[[1, 0], [0, 1]]), 'tensor'), (dict(out=torch.zeros(2, 8, dtype=x.dtype)), 'shape'),
                      (dict(out=torch.zeros(2, 16, dtype=torch.complex64)), 'shape')):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError, match=word):
            backend.apply_mux(x, **kw)
    flat = torch.zeros(40, dtype=torch.complex128)
    with pytest.raises(ValueError, match='overlap'):
        backend.apply_mux(flat[:32].reshape(2, 16), u, 'u', 0, (1, 2), out=flat[8:].reshape(2, 16))
    with pytest.raises(TypeError):
        backend.apply_mux(x.real.contiguous(), u, 'u', 0, (1, 2))
    out = torch.empty_like(x)
    assert backend.apply_mux(x, u, 'u', 0, (1, 2), out=out) is out
    # a float64 table goes to a complex64 state in the state's precision, and the other way round
    y = backend.apply_mux(x.to(torch.complex64), cs, 'ry', 0, (1, 2))
    assert y.dtype == torch.complex64 and torch.allclose(y.to(x.dtype), backend.apply_mux(x, cs.float(), 'ry', 0, (1, 2)), atol=1e-6)


def test_gate_validation():
    u = tt(random_unitaries(2, 3))
    make = lambda **kw: dq.MultiplexedGate(**{**dict(unitaries=u, nqubit=4, wires=[0, 2, 3]), **kw})  # noqa: E731
    bad = u.clone()
    bad[1] = bad[1] * 1.01
    for kw, word in ((dict(unitaries=bad), 'not unitary'), (dict(unitaries=u[:2]), 'shape'), (dict(unitaries=u.reshape(2, 2, 2, 2)), 'shape'),
                     (dict(wires=[3]), 'at least one select'), (dict(unitaries=u.clone().requires_grad_()), 'constant')):
        with pytest.raises(ValueError, match=word):
            make(**kw)
    for kw in (dict(wires=[0, 2, 2]), dict(controls=[2]), dict(wires=[0, 2, 4])):       # a repeated wire, as for every gate
        with pytest.raises(AssertionError):
            make(**kw)
    # 1e-4 is accepted, as UAnyGate accepts it
    make(unitaries=u * (1 + 2e-5))
    g = make(controls=[1])
    assert g.unitaries.dtype == torch.complex128 and g.controls == [1] and 'target=3' in repr(g)
    assert make(unitaries=u.numpy().tolist()).unitaries.dtype == torch.complex64

    rot = lambda **kw: dq.MultiplexedRotation(**{**dict(axis='y', angles=[0.1, 0.2, 0.3, 0.4], nqubit=4, wires=[0, 2, 3]), **kw})  # noqa: E731
    with pytest.raises(AssertionError):
        rot(wires=[0, 0, 3])
    for kw, word in ((dict(axis='w'), 'axis'), (dict(angles=[0.1, 0.2]), 'angles'), (dict(wires=[1]), 'at least one select'), (dict(angles=torch.zeros(4, requires_grad=True)), 'constants'),
                     (dict(angles=torch.nn.Parameter(torch.zeros(4))), 'constants')):
        with pytest.raises(ValueError, match=word):
            rot(**kw)
    # numbers and lists become float32, as every angle of the package; a float64 tensor stays
    assert rot().angles.dtype == torch.float32
    assert rot(angles=torch.zeros(4, dtype=torch.float64)).angles.dtype == torch.float64
    assert rot(angles=np.zeros(4)).angles.dtype == torch.float32
    assert rot().double().angles.dtype == torch.float64


def rotation_blocks(axis, angles):
    a = np.asarray(angles, dtype=np.float64) / 2
    c, s = np.cos(a), np.sin(a)
    m = np.zeros((len(a), 2, 2), dtype=np.complex128)
    if axis == 'x':
        m[:, 0, 0], m[:, 0, 1], m[:, 1, 0], m[:, 1, 1] = c, -1j * s, -1j * s, c
    elif axis == 'y':
        m[:, 0, 0], m[:, 0, 1], m[:, 1, 0], m[:, 1, 1] = c, -s, s, c
    else:
        m[:, 0, 0], m[:, 1, 1] = np.exp(-1j * a), np.exp(1j * a)
    return m


def test_unitary_is_the_block_diagonal_matrix_and_inverse_undoes_it(cpu_backend):
    n = 4
    u = random_unitaries(2, 7)
    # on (select.., target) = all wires of a 3-wire register in their order the unitary is the block-diagonal matrix itself
    full = dq.MultiplexedGate(tt(u), nqubit=3, wires=[0, 1, 2])
    assert torch.allclose(full.get_unitary(), tt(block_diag(u)), atol=1e-14)
    assert full.get_unitary().dtype == torch.complex128 and full.to(torch.float).get_unitary().dtype == torch.complex64
    # cir.multiplexer equals cir.any of the block-diagonal matrix, on scattered wires under a control
    wires, controls = [3, 0, 2], [1]
    a, b = dq.QubitCircuit(n), dq.QubitCircuit(n)
    a.multiplexer(tt(u), wires=wires, controls=controls)
    b.any(tt(block_diag(u)), wires=wires, controls=controls)
    a.to(torch.double)
    b.to(torch.double)
    assert torch.allclose(a.get_unitary(), b.get_unitary(), atol=1e-14)
    g = a.operators[0]
    inv = g.inverse()
    assert inv.name == 'multiplexer_dagger' and inv.unitaries is g.unitaries and inv.inv_mode
    eye = torch.eye(1 << n, dtype=torch.complex128)
    assert torch.allclose(inv.get_unitary() @ g.get_unitary(), eye, atol=1e-14)
    assert torch.allclose(inv.get_unitary(), g.get_unitary().mH, atol=1e-14)
    x = tt(random_state(3, n, 2, np.complex128))
    assert torch.equal(inv.inverse().apply_flat(x), g.apply_flat(x))
    back = a + a.inverse()
    assert len(back.operators) == 2 and torch.allclose(back(state=x.reshape(3, -1, 1)).reshape(3, -1), x, atol=1e-14)
    # the rotations, every axis
    angles = np.random.default_rng(3).uniform(-6, 6, 4)
    for axis in 'xyz':
        r = dq.MultiplexedRotation(axis, torch.tensor(angles), nqubit=n, wires=wires, controls=controls).double()
        d = dq.QubitCircuit(n)
        d.any(tt(block_diag(rotation_blocks(axis, angles))), wires=wires, controls=controls)
        d.to(torch.double)
        assert torch.allclose(r.get_unitary(), d.get_unitary(), atol=1e-14), axis
        ri = r.inverse()
        assert ri.angles is r.angles and ri.name == 'MultiplexedRotation_dagger'
        assert torch.allclose(ri.get_unitary() @ r.get_unitary(), eye, atol=1e-14), axis
        # the table is formed once per precision and kept
        t1 = r.table(torch.complex128)
        assert r.table(torch.complex128) is t1 and r.table(torch.complex64) is r.table(torch.complex64)
        assert r.table(torch.complex64).dtype in (torch.float32, torch.complex64)
        if axis != 'z':
            assert ri.table(torch.complex128) is t1          # the inverse applies the dagger of the same table
        r.angles.mul_(2.0)                                   # a write to the angles is seen
        assert r.table(torch.complex128) is not t1


def test_ucrz_is_the_diagonal_gate_of_the_same_phases(cpu_backend):
    n, wires, controls = 4, [2, 0, 3], [1]
    angles = torch.tensor(np.random.default_rng(5).uniform(-6, 6, 4))
    a, b = dq.QubitCircuit(n), dq.QubitCircuit(n)
    a.ucrz(angles, wires, controls=controls)
    phases = torch.stack([torch.exp(-0.5j * angles), torch.exp(0.5j * angles)], dim=-1).reshape(-1)
    b.diagonal(phases, wires=wires, controls=controls)
    a.to(torch.double)
    b.to(torch.double)
    x = tt(random_state(2, n, 6, np.complex128)).reshape(2, -1, 1)
    assert torch.equal(a(state=x), b(state=x))
    assert isinstance(a.operators[0], dq.MultiplexedRotation) and a.operators[0].name == 'ucrz'
    for name, axis in (('ucrx', 'x'), ('ucry', 'y')):
        c = dq.QubitCircuit(n)
        getattr(c, name)(angles, wires)
        assert c.operators[0].axis == axis and c.operators[0].name == name


def test_ucry_is_the_loop_of_controlled_rotations_with_x_flips(cpu_backend):
    n, k = 4, 2
    angles = np.random.default_rng(8).uniform(-6, 6, 1 << k)
    wires = [3, 1, 0]                                    # selects 3 (most significant), 1; target 0
    one, loop = dq.QubitCircuit(n), dq.QubitCircuit(n)
    one.ucry(torch.tensor(angles), wires)
    for s in range(1 << k):
        zeros = [w for j, w in enumerate(wires[:-1]) if not (s >> (k - 1 - j)) & 1]
        for w in zeros:
            loop.x(w)
        loop.ry(0, inputs=torch.tensor(angles[s]), controls=wires[:-1])
        for w in zeros:
            loop.x(w)
    one.to(torch.double)
    loop.to(torch.double)
    x = tt(random_state(2, n, 6, np.complex128)).reshape(2, -1, 1)
    assert torch.allclose(one(state=x), loop(state=x), atol=1e-10)


def test_tables_survive_moves_state_dict_pickle_and_addition(cpu_backend):
    n = 4
    u = random_unitaries(2, 5)
    angles = [0.3, -1.2, 2.5, 0.7]

    def build(u, angles):
        cir = dq.QubitCircuit(n)
        cir.hlayer()
        cir.multiplexer(tt(u).to(torch.complex64), wires=[3, 1, 0])
        cir.ucry(angles, wires=[0, 2, 1])
        cir.rxlayer()
        return cir

    cir = build(u, angles)
    x = tt(random_state(2, n, 9, np.complex128)).reshape(2, -1, 1)
    cir.to(torch.double)
    (ig,) = [i for i, op in enumerate(cir.operators) if isinstance(op, dq.MultiplexedGate)]
    (ir,) = [i for i, op in enumerate(cir.operators) if isinstance(op, dq.MultiplexedRotation)]
    g, r = cir.operators[ig], cir.operators[ir]
    assert g.unitaries.dtype == torch.complex128 and r.angles.dtype == torch.float64
    assert g._state_like()[0] == torch.complex128 and r._state_like()[0] == torch.complex128
    want = cir(state=x)
    other = build(random_unitaries(2, 6), [0.0, 0.0, 0.0, 0.0])
    other.to(torch.double)
    sd = cir.state_dict()
    assert {k for k in sd if k.startswith(f'operators.{ig}.')} == {f'operators.{ig}.unitaries'}
    assert {k for k in sd if k.startswith(f'operators.{ir}.')} == {f'operators.{ir}.angles'}
    assert not torch.equal(other(state=x), want)
    other.load_state_dict(sd)
    assert torch.equal(other(state=x), want)
    again = pickle.loads(pickle.dumps(cir))
    assert torch.equal(again.operators[ir].angles, r.angles) and torch.equal(again(state=x), want)
    buf = io.BytesIO()
    torch.save(cir, buf)
    buf.seek(0)
    assert torch.equal(torch.load(buf, weights_only=False)(state=x), want)
    both = cir + cir.inverse()
    assert torch.allclose(both(state=x), x, atol=1e-12)


def test_autograd_rules_through_the_stand_in(cpu_backend):
    """gradcheck / gradgradcheck, forward mode, vmap and the exact backward at n = 4 with a control."""
    n, target, bits, controls = 4, 1, (3, 0), (2,)
    u, cs = tt(random_unitaries(2, 8)), tt(random_cs(2, 9))
    gc, ggc = torch.autograd.gradcheck, torch.autograd.gradgradcheck
    for table, kind, blocks in ((u, 'u', u.numpy()), (cs, 'ry', ry_blocks(cs.numpy()))):
        for dagger in (False, True):
            x = tt(random_state(2, n, 1, np.complex128)).requires_grad_()
            f = lambda s: ops.mux_apply(s, table, kind, target, bits, controls, dagger=dagger)  # noqa: E731
            assert gc(f, (x,))
            assert ggc(f, (x,))
            assert gc(f, (x,), check_forward_ad=True, check_backward_ad=False)
            # the backward of the state is the dagger map, exactly
            gy = tt(random_state(2, n, 2, np.complex128))
            (gx,) = torch.autograd.grad(f(x), x, gy)
            assert torch.equal(gx, backend.apply_mux(gy, table, kind, target, bits, controls, dagger=not dagger))
            assert np.abs(gx.numpy() - mux_ref(gy.numpy(), blocks, target, bits, controls, not dagger)).max() < 1e-13
            # jvp: the same map of the tangent
            t = tt(random_state(2, n, 3, np.complex128))
            y, yt = torch.func.jvp(f, (x.detach(),), (t,))
            assert torch.equal(yt, backend.apply_mux(t, table, kind, target, bits, controls, dagger=dagger))
            assert torch.equal(y, backend.apply_mux(x.detach(), table, kind, target, bits, controls, dagger=dagger))
            # vmap folds the mapped dimension into the batch
            xs = tt(random_state(6, n, 4, np.complex128)).reshape(3, 2, -1)
            want = backend.apply_mux(xs.reshape(6, -1), table, kind, target, bits, controls, dagger=dagger)
            assert torch.equal(torch.vmap(f)(xs).reshape(6, -1), want)
            got = torch.vmap(f, in_dims=1)(xs.transpose(0, 1).contiguous())
            assert torch.equal(got.reshape(6, -1), want)
    with pytest.raises(ValueError, match='constant'):
        ops.mux_apply(x, u.clone().requires_grad_(), 'u', target, bits)
    with pytest.raises(ValueError, match='kind'):
        ops.mux_apply(x, u, 'rz', target, bits)
    # through a circuit: a trainable layer before and after the gates
    cir = dq.QubitCircuit(n)
    cir.rxlayer()
    cir.multiplexer(u, wires=[0, 3, 2], controls=[1])
    cir.ucrx([0.1, 0.2, 0.3, 0.4], wires=[1, 2, 0])
    cir.rylayer()
    cir.observable(0)
    cir.to(torch.double)
    cir()
    cir.expectation().sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in cir.parameters())


def prepared(k, seed, empty=False, real=False):
    rng = np.random.default_rng(seed)
    phi = rng.standard_normal(1 << k) + (0 if real else 1j) * rng.standard_normal(1 << k)
    if real:
        phi = np.abs(phi)
    if empty and k >= 2:
        phi = phi.reshape(4, -1)
        phi[1] = 0                                      # a branch of zero weight below the first two wires
        phi = phi.reshape(-1)
    return phi * 3.0                                    # (not normalised: prepare_state normalises)


@pytest.mark.parametrize('k', [1, 2, 3, 4, 5, 6])
def test_prepare_state_on_some_wires_of_a_register(cpu_backend, k):
    n = 8
    wires = [5, 2, 7, 0, 3, 6][:k]
    rest = [w for w in range(n) if w not in wires]
    for empty, real in ((False, False), (True, False), (False, True)):
        phi = prepared(k, 10 + k, empty, real)
        cir = dq.QubitCircuit(n)
        for w in rest:                                  # spectators in superposition, (|0> + |1>) / sqrt 2 in float64
            cir.ry(w, inputs=torch.tensor(np.pi / 2, dtype=torch.float64))
        cir.prepare_state(tt(phi), wires=wires)
        cir.to(torch.double)
        kinds = [type(op).__name__ for op in cir.operators[len(rest):]]
        assert kinds == ['Ry'] + ['MultiplexedRotation'] * (k - 1) + ([] if real else ['DiagonalGate'])
        out = cir().reshape(-1).numpy()
        # the amplitude of |rest = r>|wires = v> is phi[v] / |phi| / sqrt(2^(n-k)) for every r
        out = out.reshape([2] * n).transpose(rest + wires).reshape(1 << (n - k), 1 << k)
        want = phi / np.linalg.norm(phi) / np.sqrt(1 << (n - k))
        assert np.abs(out - want[None, :]).max() < 1e-10
    # under a control: nothing happens where the control is 0
    phi = prepared(3, 3)
    cir = dq.QubitCircuit(n)
    cir.ry(1, inputs=torch.tensor(np.pi / 2, dtype=torch.float64))
    cir.prepare_state(tt(phi), wires=[5, 2, 7], controls=[1])
    cir.to(torch.double)
    out = cir().reshape([2] * n).numpy().transpose([1, 5, 2, 7, 0, 3, 4, 6]).reshape(2, 8, -1)[:, :, 0]
    e0 = np.zeros(8)
    e0[0] = 1
    assert np.abs(out[0] - e0 / np.sqrt(2)).max() < 1e-10
    assert np.abs(out[1] - phi / np.linalg.norm(phi) / np.sqrt(2)).max() < 1e-10
    with pytest.raises(ValueError, match='entries'):
        dq.QubitCircuit(n).prepare_state(tt(phi), wires=[0, 1])
    with pytest.raises(ValueError, match='norm'):
        dq.QubitCircuit(n).prepare_state(torch.zeros(4), wires=[0, 1])


def hhl_with_one_ucry(ncount, mat):
    from deepquantum_amd.ansatz import QuantumPhaseEstimation

    ref = dq.HHL(ncount=ncount, mat=mat)
    n = ref.nqubit
    cir = dq.QubitCircuit(n)
    qpe = QuantumPhaseEstimation(nqubit=n, ncount=ncount, unitary=ref.unitary, minmax=[1, n - 1])
    cir.add(qpe)
    cir.ucry([2 * np.pi * v / 2**ncount for v in range(2**ncount)], wires=list(range(ncount, 0, -1)) + [0])
    cir.add(qpe.inverse())
    return ref, cir


def test_hhl_rotation_as_one_gate(cpu_backend):
    ref, cir = hhl_with_one_ucry(3, [[1.0, -1 / 3], [-1 / 3, 1.0]])
    assert sum(isinstance(op, dq.MultiplexedRotation) for op in cir.operators) == 1
    x = tt(random_state(2, ref.nqubit, 12, np.complex64)).reshape(2, -1, 1)
    want, got = ref(state=x), cir(state=x)
    assert torch.abs(got - want).max() <= 1e-4 * torch.abs(want).max()
    ref.to(torch.double)
    cir.to(torch.double)
    x = x.to(torch.complex128)
    want, got = ref(state=x), cir(state=x)
    # (the angles are float32 numbers in both circuits: the same values after .double())
    assert torch.abs(got - want).max() <= 1e-10 * torch.abs(want).max()


def test_refusals(cpu_backend):
    u = tt(random_unitaries(1, 1))
    makers = (('MultiplexedGate', lambda **kw: dq.MultiplexedGate(u, nqubit=2, wires=[0, 1], **kw)),
              ('MultiplexedRotation', lambda **kw: dq.MultiplexedRotation('y', [0.1, 0.2], nqubit=2, wires=[0, 1], **kw)))
    for name, make in makers:
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
