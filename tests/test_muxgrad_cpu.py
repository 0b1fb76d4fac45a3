"""Host logic of the trainable multiplexed rotations (backend.mux_cross, ops.mux_axpby / mux_cross / mux_rot,
MultiplexedRotation(requires_grad=True), cir.ucr*) without a GPU: the kernels' stand-ins are the plain-torch routes of
``backend`` under the CPU test double, so what is checked here is the library's argument checks, the autograd rules and
the bookkeeping."""

import io
import os
import pickle
import re

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import _lib, backend, ops
from _mux_ref import random_state
from _muxgrad_ref import mux_axpby_ref, mux_cross_ref, mux_rot_grads_ref, mux_rot_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('dq_mux_cross_c64', 'dq_mux_cross_c128')


def tt(a):
    return torch.from_numpy(np.asarray(a))


def test_library_exports_the_new_symbols_and_still_reports_abi_30():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 30 and lib.dq_abi_version() == 30
    text = open(os.path.join(ROOT, 'include', 'dq_hip.h')).read()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.exported_symbols()
        assert re.search(r'\bint %s\(' % name, text)
    assert hasattr(lib, 'dq_mux_cross_ws_bytes') and re.search(r'\bint64_t dq_mux_cross_ws_bytes\(', text)
    for letter, code in _lib.MUX_AXES.items():
        assert re.search(r'#define DQ_MUX_AXIS_%s %d\b' % (letter.upper(), code), text)
    assert _lib.MUX_AXES == {'i': 0, 'x': 1, 'y': 2, 'z': 3}
    for name in ('mux_axpby', 'mux_cross', 'mux_rot'):
        assert hasattr(ops, name)
    assert hasattr(backend, 'mux_cross')


def test_host_side_argument_checks_of_the_library():
    """DQ_ERR_ARG with a text, before any HIP call (no device is touched: the pointers are never dereferenced)."""
    lib = _lib.load()
    ia = _lib.int_array
    p, q, o, w = 1 << 20, 1 << 30, 1 << 24, 1 << 26     # aligned non-null "pointers", far apart
    big = 1 << 40

    def refused(rc, word):
        assert rc == -1 and word in lib.dq_last_error().decode(), lib.dq_last_error()

    # f(bra, ket, axis, n, target, bits, k, controls, nc, batch, out, ws, ws_bytes, stream)
    for f in (lib.dq_mux_cross_c64, lib.dq_mux_cross_c128):
        refused(f(None, q, 1, 3, 0, ia([1]), 1, ia([]), 0, 1, o, w, big, None), 'null')
        refused(f(p, None, 1, 3, 0, ia([1]), 1, ia([]), 0, 1, o, w, big, None), 'null')
        refused(f(p, q, 1, 3, 0, ia([1]), 1, ia([]), 0, 1, None, w, big, None), 'null')
        refused(f(p, q, 1, 3, 0, ia([1]), 1, ia([]), 0, 1, o, None, big, None), 'null')
        refused(f(p + 8, q, 1, 3, 0, ia([1]), 1, ia([]), 0, 1, o, w, big, None), 'aligned')
        refused(f(p, q + 8, 1, 3, 0, ia([1]), 1, ia([]), 0, 1, o, w, big, None), 'aligned')
        refused(f(p, q, 1, 3, 0, ia([1]), 1, ia([]), 0, 1, o + 4, w, big, None), 'aligned')
        refused(f(p, q, 1, 3, 0, ia([1]), 1, ia([]), 0, 1, o, w + 8, big, None), 'aligned')
        refused(f(p, q, 1, 1, 0, ia([1]), 1, ia([]), 0, 1, o, w, big, None), 'n=1')
        refused(f(p, q, 1, 41, 0, ia([1]), 1, ia([]), 0, 1, o, w, big, None), 'n=41')
        refused(f(p, q, 1, 3, 0, ia([1]), 0, ia([]), 0, 1, o, w, big, None), 'k=0')
        refused(f(p, q, 1, 3, 0, ia([0, 1, 2]), 3, ia([]), 0, 1, o, w, big, None), 'k=3')         # k > n - 1
        refused(f(p, q, 1, 3, 3, ia([1]), 1, ia([]), 0, 1, o, w, big, None), 'target 3')
        refused(f(p, q, 1, 3, -1, ia([1]), 1, ia([]), 0, 1, o, w, big, None), 'target -1')
        refused(f(p, q, 1, 3, 0, ia([3]), 1, ia([]), 0, 1, o, w, big, None), 'out of range')
        refused(f(p, q, 1, 3, 0, ia([1]), 1, ia([3]), 1, 1, o, w, big, None), 'out of range')
        refused(f(p, q, 1, 4, 0, ia([1, 1]), 2, ia([]), 0, 1, o, w, big, None), 'twice')          # duplicate bits
        refused(f(p, q, 1, 4, 0, ia([1]), 1, ia([2, 2]), 2, 1, o, w, big, None), 'twice')
        refused(f(p, q, 1, 4, 0, ia([1, 2]), 2, ia([2]), 1, 1, o, w, big, None), 'twice')         # a control among the selects
        refused(f(p, q, 1, 3, 1, ia([1]), 1, ia([]), 0, 1, o, w, big, None), 'is the target')     # the target among the selects
        refused(f(p, q, 1, 3, 2, ia([1]), 1, ia([2]), 1, 1, o, w, big, None), 'is the target')
        refused(f(p, q, 4, 3, 0, ia([1]), 1, ia([]), 0, 1, o, w, big, None), 'axis')
        refused(f(p, q, -1, 3, 0, ia([1]), 1, ia([]), 0, 1, o, w, big, None), 'axis')
        refused(f(p, q, 1, 3, 0, ia([1]), 1, ia([]), 0, 0, o, w, big, None), 'batch')
        refused(f(p, q, 1, 3, 0, ia([1]), 1, ia([]), 0, 65536, o, w, big, None), 'batch')
        # a workspace that is too small: one byte less than the sizing function asks for
        for n, k, batch in ((3, 1, 1), (16, 3, 2), (24, 10, 3)):
            need = lib.dq_mux_cross_ws_bytes(n, batch, 0, 1, k)
            assert need >= 16
            refused(f(p, q, 1, n, 0, ia(range(1, k + 1)), k, ia([]), 0, batch, o, w, need - 1, None), 'workspace')
    # the sizing function: -1 outside the ranges, the same for both precisions and for bra == ket
    size = lib.dq_mux_cross_ws_bytes
    for bad in ((1, 1, 0, 0, 1), (41, 1, 0, 0, 1), (3, 0, 0, 0, 1), (3, 65536, 0, 0, 1), (3, 1, 0, 0, 0), (3, 1, 0, 0, 3),
                (3, 1, 0, 0, -1)):
        assert size(*bad) == -1
    assert size(3, 1, 0, 0, 2) == 16                    # one workgroup owns every bin: nothing but a valid pointer
    assert size(24, 2, 0, 0, 4) == size(24, 2, 1, 1, 4) == 2 * 2048 * 16 * 16
    assert size(24, 2, 0, 0, 10) == 2 * 512 * 1024 * 16            # 2^19 partial sums per sample at most
    assert size(30, 1, 0, 0, 25) == 16


CASES = [
    # n, target, bits, controls
    (2, 0, (1,), ()),
    (2, 1, (0,), ()),
    (5, 2, (3, 0, 4), ()),              # unsorted, on both sides of the target
    (5, 0, (2,), ()),                   # k = 1
    (4, 1, (3, 2, 0), ()),              # k = n - 1
    (5, 4, (1, 3), (0,)),               # one control
    (6, 3, (4, 1), (5, 0)),             # two controls, one on each side
]


@pytest.mark.parametrize('n,target,bits,controls', CASES)
def test_stand_ins_against_the_definition(cpu_backend, n, target, bits, controls):
    k = len(bits)
    rng = np.random.default_rng(n + k)
    for dtype, tol in ((np.complex64, 1e-5), (np.complex128, 1e-13)):
        u, v = random_state(3, n, 3, dtype), random_state(3, n, 4, dtype)
        for axis in 'ixyz':
            want = mux_cross_ref(u, v, axis, target, bits, controls)
            got = backend.mux_cross(tt(u), tt(v), axis, target, bits, controls)
            assert got.dtype == torch.complex128 and got.shape == (3, 1 << k)
            assert np.abs(got.numpy() - want).max() <= 1e-13 * np.abs(want).max()
            x = tt(v)
            same = backend.mux_cross(x, x, axis, target, bits, controls).numpy()
            assert np.abs(same - mux_cross_ref(v, v, axis, target, bits, controls)).max() <= 1e-12
            for shape in ((1 << k,), (3, 1 << k)):
                a = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
                c = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
                for mode in ('gate', 'map'):
                    want = mux_axpby_ref(v, a, c, axis, target, bits, controls, mode)
                    got = backend.apply_mux_axpby(tt(v), tt(a), tt(c), axis, target, bits, controls, mode).numpy()
                    assert got.dtype == dtype and np.abs(got - want).max() <= 4 * tol * np.abs(want).max()
                if axis != 'i':
                    theta = rng.uniform(-6, 6, shape)
                    want = mux_rot_ref(v, theta, axis, target, bits, controls)
                    got = backend.apply_mux_rot(tt(v), tt(theta), axis, target, bits, controls).numpy()
                    assert got.dtype == dtype and np.abs(got - want).max() <= 4 * tol * np.abs(want).max()


def test_backend_refusals(cpu_backend):
    x = tt(random_state(2, 4, 1, np.complex128))
    ok = dict(axis='x', target=0, bits=(1, 2), controls=())
    for bad, word in ((dict(bits=(1, 1)), 'distinct'), (dict(bits=(1, 4)), 'distinct'), (dict(controls=(2,)), 'distinct'),
                      (dict(target=1), 'distinct'), (dict(target=4), 'distinct'), (dict(controls=(0,)), 'distinct'),
                      (dict(bits=()), 'at least one'), (dict(axis='w'), 'axis')):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError, match=word):
            backend.mux_cross(x, x, **kw)
    with pytest.raises(ValueError, match='one shape'):
        backend.mux_cross(x[:1], x, **ok)
    with pytest.raises(ValueError, match='select bits take'):
        backend.apply_mux_rot(x, torch.zeros(3), 'y', 0, (1, 2))
    with pytest.raises(ValueError, match='select bits take'):
        ops.mux_rot(x, torch.zeros(3, 4), 'y', 0, (1, 2))
    with pytest.raises(ValueError, match='axis'):
        ops.mux_rot(x, torch.zeros(4), 'i', 0, (1, 2))
    with pytest.raises(ValueError, match='real'):
        ops.mux_rot(x, torch.zeros(4, dtype=torch.complex128), 'y', 0, (1, 2))
    with pytest.raises(ValueError, match='mode'):
        ops.mux_axpby(x, torch.zeros(4), torch.zeros(4), 'x', 0, (1, 2), mode='both')
    # what stays refused: a table / an angle tensor that asks for a gradient on the constant routes
    with pytest.raises(ValueError, match='constant'):
        ops.mux_apply(x, torch.zeros(4, 2, dtype=torch.float64, requires_grad=True), 'ry', 0, (1, 2))
    with pytest.raises(ValueError, match='constants'):
        dq.MultiplexedRotation('y', torch.zeros(4, requires_grad=True), nqubit=4, wires=[0, 2, 3])
    with pytest.raises(ValueError, match='constants'):
        dq.MultiplexedRotation('y', torch.nn.Parameter(torch.zeros(4)), nqubit=4, wires=[0, 2, 3], requires_grad=False)


def test_gate_validation_and_bookkeeping(cpu_backend):
    n = 4
    g = dq.MultiplexedRotation('y', None, nqubit=n, wires=[0, 2, 3], controls=[1], requires_grad=True)
    assert isinstance(g.angles, torch.nn.Parameter) and g.angles.shape == (4,) and g.npara == 4 and g.requires_grad
    assert g.angles.dtype == torch.float32 and [name for name, _ in g.named_parameters()] == ['angles']
    with pytest.raises(ValueError, match='requires_grad=True'):
        dq.MultiplexedRotation('y', None, nqubit=n, wires=[0, 2, 3])
    with pytest.raises(ValueError, match='angles'):
        dq.MultiplexedRotation('y', [0.1, 0.2], nqubit=n, wires=[0, 2, 3], requires_grad=True)
    fixed = dq.MultiplexedRotation('y', [0.1, 0.2, 0.3, 0.4], nqubit=n, wires=[0, 2, 3])
    assert fixed.npara == 0 and not fixed.requires_grad and 'angles' in dict(fixed.named_buffers())
    assert not list(fixed.parameters())
    # given angles are kept (detached), a float64 tensor stays float64
    given = torch.tensor([0.1, 0.2, 0.3, 0.4], dtype=torch.float64, requires_grad=True)
    h = dq.MultiplexedRotation('x', given, nqubit=n, wires=[0, 2, 3], requires_grad=True)
    assert h.angles.dtype == torch.float64 and torch.equal(h.angles.detach(), given.detach()) and h.angles is not given
    # init_para: new random angles, or the given ones, in the parameter's precision; a constant gate is left alone
    old = h.angles.detach().clone()
    h.init_para()
    assert h.angles.dtype == torch.float64 and not torch.equal(h.angles.detach(), old) and isinstance(h.angles, torch.nn.Parameter)
    h.init_para([1.0, 2.0, 3.0, 4.0])
    assert torch.equal(h.angles.detach(), torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64))
    with pytest.raises(ValueError, match='angles expected'):
        h.init_para([1.0, 2.0])
    before = fixed.angles.clone()
    fixed.init_para()
    assert torch.equal(fixed.angles, before)

    cir = dq.QubitCircuit(n)
    cir.hlayer()
    cir.ucry(wires=[0, 2, 3], controls=[1], requires_grad=True)
    cir.ucrx([0.1, 0.2], wires=[1, 0], requires_grad=True)
    cir.ucrz([0.1, 0.2], wires=[1, 0])
    assert cir.npara == 6
    (p4, p2) = list(cir.parameters())
    assert p4.shape == (4,) and p2.shape == (2,) and torch.allclose(p2.detach(), torch.tensor([0.1, 0.2]))
    assert [op.name for op in cir.operators[-3:]] == ['ucry', 'ucrx', 'ucrz']
    with pytest.raises(ValueError, match='requires_grad=True'):
        dq.QubitCircuit(n).ucry(wires=[0, 1])
    with pytest.raises(ValueError, match='requires_grad=True'):
        dq.QubitCircuit(n).ucr('z', None, wires=[0, 1])
    # what stays refused by name
    make = lambda **kw: dq.MultiplexedRotation('y', None, nqubit=2, wires=[0, 1], requires_grad=True, **kw)  # noqa: E731
    with pytest.raises(NotImplementedError, match='MultiplexedRotation'):
        make(den_mat=True)
    with pytest.raises(NotImplementedError, match='MultiplexedRotation'):
        make().op_dist_state(None)
    with pytest.raises(NotImplementedError, match='MultiplexedRotation'):
        make().prims()
    c2 = dq.QubitCircuit(2)
    c2.add(make())
    with pytest.raises(NotImplementedError, match='MultiplexedRotation'):
        c2.qasm()
    with pytest.raises(AssertionError):
        dq.QubitCircuit(2).add(make(), encode=True)


def build(n, seed):
    torch.manual_seed(seed)
    cir = dq.QubitCircuit(n)
    cir.hlayer()
    cir.ucry(wires=[3, 1, 0], requires_grad=True)
    cir.ucrx(wires=[0, 2, 1], controls=[3], requires_grad=True)
    cir.ucrz(wires=[2, 3], requires_grad=True)
    cir.rxlayer()
    return cir


def test_parameters_survive_moves_state_dict_pickle_and_the_inverse(cpu_backend):
    n = 4
    cir = build(n, 1)
    x = tt(random_state(2, n, 9, np.complex128)).reshape(2, -1, 1)
    cir.to(torch.double)
    rots = [i for i, op in enumerate(cir.operators) if isinstance(op, dq.MultiplexedRotation)]
    assert len(rots) == 3
    for i in rots:
        op = cir.operators[i]
        assert op.angles.dtype == torch.float64 and isinstance(op.angles, torch.nn.Parameter)
        assert op._state_like()[0] == torch.complex128
    want = cir(state=x)
    other = build(n, 2)
    other.to(torch.double)
    sd = cir.state_dict()
    for i in rots:
        assert {k for k in sd if k.startswith(f'operators.{i}.')} == {f'operators.{i}.angles'}
    assert not torch.equal(other(state=x), want)
    other.load_state_dict(sd)
    assert torch.equal(other(state=x), want)
    again = pickle.loads(pickle.dumps(cir))
    assert torch.equal(again(state=x), want) and isinstance(again.operators[rots[0]].angles, torch.nn.Parameter)
    buf = io.BytesIO()
    torch.save(cir, buf)
    buf.seek(0)
    assert torch.equal(torch.load(buf, weights_only=False)(state=x), want)
    single = build(n, 1)
    assert single.operators[rots[0]].angles.dtype == torch.float32
    y = single(state=x.to(torch.complex64))
    assert y.dtype == torch.complex64 and torch.abs(y.to(want.dtype) - want).max() < 1e-5
    # G . G.inverse() = 1; the inverse shares the parameter
    eye = torch.eye(1 << n, dtype=torch.complex128)
    for i in rots:
        g = cir.operators[i]
        inv = g.inverse()
        assert inv.angles is g.angles and inv.inv_mode and inv.name == g.name + '_dagger'
        assert torch.allclose(inv.get_unitary() @ g.get_unitary(), eye, atol=1e-14)
        assert torch.allclose(inv.get_unitary(), g.get_unitary().mH, atol=1e-14)
        # the unitary is that of the constant gate with the same angles
        const = dq.MultiplexedRotation(g.axis, g.angles.detach(), nqubit=n, wires=g.wires, controls=g.controls).double()
        assert torch.allclose(g.get_unitary(), const.get_unitary(), atol=1e-14)
    both = cir + cir.inverse()
    assert torch.allclose(both(state=x), x, atol=1e-12)
    # gradients flow to the shared parameter from both directions
    cir.zero_grad()
    out = both(state=x)
    (out.abs() ** 2 * torch.arange(1 << n, dtype=torch.float64).reshape(1, -1, 1)).sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in cir.parameters())


GC = dict(n=4, target=1, bits=(3, 0), controls=(2,))


def _x(batch, seed):
    return tt(random_state(batch, GC['n'], seed, np.complex128)).requires_grad_()


def _coef(shape, seed):
    rng = np.random.default_rng(seed)
    return tt(rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).requires_grad_()


@pytest.mark.parametrize('axis', ['x', 'y', 'z'])
def test_mux_rot_gradcheck_in_state_and_angles(cpu_backend, axis):
    target, bits, controls = GC['target'], GC['bits'], GC['controls']
    gc, ggc = torch.autograd.gradcheck, torch.autograd.gradgradcheck
    f = lambda s, t: ops.mux_rot(s, t, axis, target, bits, controls)  # noqa: E731
    for shape in ((4,), (2, 4)):
        theta = tt(np.random.default_rng(5).uniform(-3, 3, shape)).requires_grad_()
        x = _x(2, 1)
        assert gc(f, (x, theta))
        assert ggc(f, (x, theta))
        assert gc(f, (x, theta), check_forward_ad=True, check_backward_ad=False)
        # the closed forms, exactly as the reference evaluates them
        gy = tt(random_state(2, GC['n'], 2, np.complex128))
        gx, gt = torch.autograd.grad(f(x, theta), (x, theta), gy)
        wx, wt = mux_rot_grads_ref(x.detach().numpy(), theta.detach().numpy(), gy.numpy(), axis, target, bits, controls)
        assert np.abs(gx.numpy() - wx).max() < 1e-13
        assert np.abs(gt.numpy() - (wt if len(shape) == 2 else wt.sum(0))).max() < 1e-13


@pytest.mark.parametrize('mode', ['gate', 'map'])
@pytest.mark.parametrize('axis', ['i', 'x', 'y', 'z'])
def test_mux_axpby_gradcheck_in_state_and_coefficients(cpu_backend, axis, mode):
    target, bits, controls = GC['target'], GC['bits'], GC['controls']
    f = lambda s, a, c: ops.mux_axpby(s, a, c, axis, target, bits, controls, mode)  # noqa: E731
    shapes = ((4,), (2, 4)) if axis == 'y' else ((4,),)
    for shape in shapes:
        x, a, c = _x(2, 3), _coef(shape, 6), _coef(shape, 7)
        assert torch.autograd.gradcheck(f, (x, a, c))
        assert torch.autograd.gradgradcheck(f, (x, a, c))
        assert torch.autograd.gradcheck(f, (x, a, c), check_forward_ad=True, check_backward_ad=False)
        want = mux_axpby_ref(x.detach().numpy(), a.detach().numpy(), c.detach().numpy(), axis, target, bits, controls, mode)
        assert np.abs(f(x, a, c).detach().numpy() - want).max() < 1e-13


@pytest.mark.parametrize('axis', ['i', 'x', 'y', 'z'])
def test_mux_cross_gradcheck_in_bra_and_ket(cpu_backend, axis):
    target, bits, controls = GC['target'], GC['bits'], GC['controls']
    f = lambda u, v: ops.mux_cross(u, v, axis, target, bits, controls)  # noqa: E731
    u, v = _x(2, 4), _x(2, 5)
    assert torch.autograd.gradcheck(f, (u, v))
    assert torch.autograd.gradgradcheck(f, (u, v))
    assert torch.autograd.gradcheck(f, (u, v), check_forward_ad=True, check_backward_ad=False)
    assert torch.autograd.gradcheck(lambda s: f(s, s), (v,))
    want = mux_cross_ref(u.detach().numpy(), v.detach().numpy(), axis, target, bits, controls)
    assert np.abs(f(u, v).detach().numpy() - want).max() < 1e-13


def test_vmap_folds_a_mapped_state_into_the_batch(cpu_backend):
    n, target, bits, controls = GC['n'], GC['target'], GC['bits'], GC['controls']
    xs = tt(random_state(6, n, 4, np.complex128)).reshape(3, 2, -1)
    us = tt(random_state(6, n, 5, np.complex128)).reshape(3, 2, -1)
    theta = tt(np.random.default_rng(1).uniform(-3, 3, 4))
    rot = lambda s: ops.mux_rot(s, theta, 'y', target, bits, controls)  # noqa: E731
    want = rot(xs.reshape(6, -1))
    assert torch.equal(torch.vmap(rot)(xs).reshape(6, -1), want)
    assert torch.equal(torch.vmap(rot, in_dims=1)(xs.transpose(0, 1).contiguous()).reshape(6, -1), want)
    # a mapped angle table becomes per sample
    thetas = tt(np.random.default_rng(2).uniform(-3, 3, (3, 4)))
    got = torch.vmap(lambda s, t: ops.mux_rot(s, t, 'x', target, bits, controls))(xs, thetas)
    for j in range(3):
        assert torch.allclose(got[j], ops.mux_rot(xs[j], thetas[j], 'x', target, bits, controls), atol=1e-15)
    cross = lambda u, v: ops.mux_cross(u, v, 'z', target, bits, controls)  # noqa: E731
    assert torch.equal(torch.vmap(cross)(us, xs).reshape(6, -1), cross(us.reshape(6, -1), xs.reshape(6, -1)))
    assert torch.equal(torch.vmap(lambda s: cross(s, s))(xs).reshape(6, -1), cross(xs.reshape(6, -1), xs.reshape(6, -1)))
    a, c = _coef((4,), 1).detach(), _coef((4,), 2).detach()
    axpby = lambda s: ops.mux_axpby(s, a, c, 'y', target, bits, controls, 'map')  # noqa: E731
    assert torch.equal(torch.vmap(axpby)(xs).reshape(6, -1), axpby(xs.reshape(6, -1)))
    # the Hessian in the angles through torch.func (forward over reverse)
    x = xs[0]
    w = torch.arange(1 << n, dtype=torch.float64)

    def loss(t):
        return ((ops.mux_rot(x, t, 'y', target, bits, controls).abs() ** 2) * w).sum()

    h1 = torch.func.hessian(loss)(theta)
    h2 = torch.autograd.functional.hessian(loss, theta)
    assert h1.shape == (4, 4) and torch.allclose(h1, h2, atol=1e-11) and torch.allclose(h1, h1.T, atol=1e-11)
