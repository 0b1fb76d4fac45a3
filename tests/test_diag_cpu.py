"""Host logic of the diagonal gates (DiagonalGate, CostPhase, expectation_cost, ising_cost) without a GPU: the kernels'
stand-ins are the plain-torch complex128 routes of ``backend.apply_diag / apply_cost / cost_cross`` under the CPU test
double, so what is checked here is the wire-to-bit mapping, the validation, the autograd rules and the bookkeeping."""

import os
import re

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import _lib, backend, ops, qmath

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sub_index(n, bits):
    i = np.arange(1 << n)
    k = len(bits)
    return sum(((i >> p) & 1) << (k - 1 - j) for j, p in enumerate(bits))


def rand_state(batch, n, seed=0, dtype=torch.complex128):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, 1 << n, dtype=torch.complex128, generator=g).to(dtype)


def rand_cost(k, seed=1):
    return torch.randn(1 << k, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def test_library_exports_the_new_symbols_and_reports_abi_30():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 30 and lib.dq_abi_version() == 30
    names = ['dq_cost_cross_ws_bytes'] + [f'dq_{f}_{s}' for f in ('apply_diag', 'apply_cost', 'cost_cross') for s in ('c64', 'c128')]
    for name in names:
        assert hasattr(lib, name) and name in _lib.exported_symbols()
    text = open(os.path.join(ROOT, 'include', 'dq_hip.h')).read()
    assert re.search(r'#define DQ_ABI_VERSION 30\b', text)
    assert re.search(r'#define DQ_COST_PHASE %d\b' % _lib.COST_PHASE, text)
    assert re.search(r'#define DQ_COST_SCALE %d\b' % _lib.COST_SCALE, text)
    for name in ('ising_cost', 'expectation_cost', 'CostPhase', 'DiagonalGate'):
        assert hasattr(dq, name)
    # one partial sum (re, im) per workgroup and sample, at most 2048 workgroups; a chunk is 2^11 (2^10) amplitudes
    assert lib.dq_cost_cross_ws_bytes(3, 1, 0, 0) == 16
    assert lib.dq_cost_cross_ws_bytes(14, 3, 0, 1) == 3 * 8 * 16
    assert lib.dq_cost_cross_ws_bytes(14, 3, 1, 1) == 3 * 16 * 16
    assert lib.dq_cost_cross_ws_bytes(30, 2, 0, 0) == 2 * 2048 * 16
    assert lib.dq_cost_cross_ws_bytes(0, 1, 0, 0) == -1 and lib.dq_cost_cross_ws_bytes(41, 1, 0, 0) == -1
    assert lib.dq_cost_cross_ws_bytes(5, 65536, 0, 0) == -1


def test_ising_cost_against_numpy(cpu_backend):
    n = 5
    terms = [(0.5, [0]), (-1.25, [4]), (2.0, [1, 3]), (1.0, [0, 4]), (-0.75, [0, 2, 3]), (3.0, [4, 1, 2])]
    i = np.arange(1 << n)
    ref = np.zeros(1 << n)
    for w, wires in terms:
        par = np.zeros_like(i)
        for q in wires:
            par ^= (i >> (n - 1 - q)) & 1
        ref += w * (1 - 2 * par)
    for dtype in (None, torch.float32, torch.float64):
        c = qmath.ising_cost(n, terms, dtype=dtype)
        assert c.dtype == (dtype or torch.float32) and c.shape == (1 << n,)
        assert np.array_equal(c.numpy().astype(np.float64), ref)         # (multiples of 1/4: exact in float32)
    assert torch.equal(qmath.ising_cost(n, [(2.0, 3)]), qmath.ising_cost(n, [(2.0, [3])]))      # a bare wire number
    with pytest.raises(ValueError):
        qmath.ising_cost(n, [(1.0, [0, 0])])
    with pytest.raises(ValueError):
        qmath.ising_cost(n, [(1.0, [5])])
    with pytest.raises(ValueError):
        qmath.ising_cost(n, [])
    with pytest.raises(ValueError):
        qmath.ising_cost(n, terms, dtype=torch.float16)


def test_backend_stand_ins_follow_the_bit_convention(cpu_backend):
    n, bits, controls = 5, [0, 4, 2], [3]
    x = rand_state(2, n)
    sub = sub_index(n, bits)
    on = ((np.arange(1 << n) >> 3) & 1) == 1
    d = torch.exp(1j * rand_cost(3, 5)).to(torch.complex128)
    ref = np.where(on, d.numpy()[sub] * x.numpy(), x.numpy())
    assert np.allclose(backend.apply_diag(x, d, bits, controls).numpy(), ref, atol=1e-15)
    c = rand_cost(3)
    t = torch.tensor([0.3, -1.1], dtype=torch.float64)
    ref = np.where(on, np.exp(-1j * t.numpy()[:, None] * c.numpy()[sub]) * x.numpy(), x.numpy())
    assert np.allclose(backend.apply_cost(x, c, t, bits, controls, 'phase').numpy(), ref, atol=1e-15)
    s = torch.tensor([0.3 - 2j, 1.5j], dtype=torch.complex128)
    ref = np.where(on, s.numpy()[:, None] * c.numpy()[sub] * x.numpy(), 0)
    assert np.allclose(backend.apply_cost(x, c, s, bits, controls, 'scale').numpy(), ref, atol=1e-15)
    y = rand_state(2, n, 9)
    ref = (np.where(on, c.numpy()[sub], 0) * x.numpy().conj() * y.numpy()).sum(-1)
    assert np.allclose(backend.cost_cross(x, y, c, bits, controls).numpy(), ref, atol=1e-14)
    for bad in (dict(bits=[0, 0]), dict(bits=[5]), dict(bits=[1], controls=[1]), dict(bits=[])):
        with pytest.raises(ValueError):
            backend.apply_diag(x, torch.ones(1 << len(bad['bits']), dtype=torch.complex128), bad['bits'], bad.get('controls', ()))
    with pytest.raises(ValueError):
        backend.apply_cost(x, rand_cost(2), t, bits)                       # table of the wrong size
    with pytest.raises(ValueError):
        backend.apply_cost(x, c, t[:1], bits)                              # one parameter per sample


def test_wire_to_bit_mapping_of_the_public_entry_points(cpu_backend):
    n = 4
    x = rand_state(1, n, 3)
    wires = [2, 0, 3]
    bits = [n - 1 - w for w in wires]
    sub = sub_index(n, bits)
    c = rand_cost(3, 7)
    # expectation_cost: every accepted form of the state, single and batched
    ref = float((c.numpy()[sub] * np.abs(x.numpy()[0]) ** 2).sum())
    for form in (x[0], x[0].reshape(-1, 1), x, x.reshape(1, -1, 1), x.reshape([1] + [2] * n)):
        v = qmath.expectation_cost(form, n, c, wires)
        assert v.shape == (() if form.ndim == 1 or form.shape[-1] == 1 and form.ndim == 2 else (1,))
        assert abs(float(v.reshape(-1)[0]) - ref) < 1e-13
    full = rand_cost(n, 8)
    assert abs(float(qmath.expectation_cost(x, n, full)) - float((full.numpy() * np.abs(x.numpy()[0]) ** 2).sum())) < 1e-13
    # the gates through a circuit
    cir = dq.QubitCircuit(n)
    cir.cost_phase(c, wires=wires, inputs=0.7, controls=[1])
    d = torch.exp(1j * rand_cost(2, 11)).to(torch.complex64)
    cir.diagonal(d, wires=[3, 1])
    cir.to(torch.double)
    out = cir(state=x.reshape(-1, 1)).reshape(-1).numpy()
    on = ((np.arange(1 << n) >> (n - 1 - 1)) & 1) == 1
    ref = np.where(on, np.exp(-0.7j * c.numpy()[sub]), 1) * x.numpy()[0]
    ref = d.to(torch.complex128).numpy()[sub_index(n, [0, 2])] * ref
    assert np.allclose(out, ref, atol=1e-6)                               # (0.7 is a float32 parameter)
    assert abs(float(cir.expectation_cost(c, wires)) - float((c.numpy()[sub] * np.abs(ref) ** 2).sum())) < 1e-12
    # validation
    for bad in ([0, 0], [4], []):
        with pytest.raises(ValueError):
            qmath.expectation_cost(x, n, c, bad)
    with pytest.raises(ValueError):
        qmath.expectation_cost(x, n, rand_cost(2), wires)
    with pytest.raises(ValueError):
        qmath.expectation_cost(x, n, c.to(torch.complex128), wires)
    with pytest.raises(ValueError):
        qmath.expectation_cost(x[:, :8], n, c, wires)
    with pytest.raises(AssertionError):
        dq.DiagonalGate(torch.ones(4), nqubit=n, wires=[0])
    with pytest.raises(AssertionError):
        dq.DiagonalGate([1, 1.01], nqubit=n, wires=[0])                   # not of unit modulus to 1e-4
    with pytest.raises(AssertionError):
        dq.CostPhase(rand_cost(3), nqubit=n, wires=[0, 1])
    with pytest.raises(AssertionError):
        dq.CostPhase(rand_cost(1), nqubit=n, wires=[0], controls=[0])


def test_tables_are_constants(cpu_backend):
    x = rand_state(1, 3)
    c = rand_cost(3).requires_grad_()
    t = torch.tensor(0.2, dtype=torch.float64)
    for call in (lambda: ops.cost_phase(x, c, t, [2, 1, 0]), lambda: ops.cost_cross(x, x, c, [2, 1, 0]),
                 lambda: ops.cost_scale(x, c, t + 0j, [2, 1, 0]), lambda: qmath.expectation_cost(x, 3, c),
                 lambda: dq.CostPhase(c, nqubit=3), lambda: ops.diag_mul(x, (c + 0j).detach().requires_grad_(), [2, 1, 0]),
                 lambda: dq.DiagonalGate(torch.exp(1j * c), nqubit=3)):
        with pytest.raises(ValueError, match='constant'):
            call()


def test_one_parameter_gate_bookkeeping(cpu_backend):
    n = 3
    c = rand_cost(n)
    cir = dq.QubitCircuit(n)
    cir.hlayer()
    cir.cost_phase(c)                          # trainable
    cir.cost_phase(c, encode=True)             # from data
    cir.cost_phase(c, inputs=0.25, wires=[0, 1, 2])
    assert (cir.npara, cir.ndata) == (2, 1)
    g_train, g_enc, g_fix = cir.operators[-3:]
    assert isinstance(g_train.t, torch.nn.Parameter) and not isinstance(g_enc.t, torch.nn.Parameter)
    assert [p is g_train.t for p in cir.parameters()] == [True]
    assert float(g_fix.t) == 0.25
    cir.to(torch.double)
    assert g_train.cost.dtype == torch.float64 and g_train.t.dtype == torch.float64
    before = g_train.t.item()
    cir.init_para()
    assert g_train.t.item() != before
    inv = g_fix.inverse()
    assert inv.inv_mode and inv.name == 'cost_phase_dagger' and inv.t is g_fix.t
    x = rand_state(1, n)
    assert torch.allclose(inv.apply_flat(g_fix.apply_flat(x)), x, atol=1e-14)
    # a batch of data: one t per sample, equal to the single runs
    data = torch.tensor([[0.1], [0.7], [-1.3]], dtype=torch.float64)
    batch = cir(data)
    assert batch.shape == (3, 1 << n, 1)
    for b in range(3):
        assert torch.allclose(cir(data[b]), batch[b], atol=1e-14)
    # after a gate that runs through apply_flat the |0..0> shortcut is off: the result equals the explicit product
    u = cir.get_unitary()
    assert torch.allclose(u[:, 0], cir(data[2]).reshape(-1), atol=1e-13)


def test_get_unitary_and_inverse(cpu_backend):
    n = 3
    c = rand_cost(2, 4)
    d = torch.exp(1j * rand_cost(n, 6)).to(torch.complex128)
    cir = dq.QubitCircuit(n)
    cir.h(0)
    cir.cost_phase(c, wires=[2, 0], inputs=0.4)
    cir.diagonal(d)
    cir.to(torch.double)
    h = torch.tensor([[1, 1], [1, -1]], dtype=torch.complex128) / 2**0.5
    eye = torch.eye(2, dtype=torch.complex128)
    u_h = torch.kron(torch.kron(h, eye), eye)
    sub = sub_index(n, [0, 2])
    u_c = torch.diag(torch.exp(-1j * float(cir.operators[1].t) * c[sub]))
    ref = torch.diag(d) @ u_c @ u_h
    got = cir.get_unitary()
    assert torch.allclose(got, ref, atol=1e-7)                            # (h is float32-rounded in the library)
    both = cir + cir.inverse()
    assert torch.allclose(both.get_unitary(), torch.eye(1 << n, dtype=torch.complex128), atol=1e-7)
    assert torch.allclose(cir.operators[2].get_unitary(), torch.diag(d), atol=1e-15)
    assert torch.allclose(cir.operators[2].inverse().get_unitary(), torch.diag(d.conj()), atol=1e-15)


def test_refusals(cpu_backend):
    c = rand_cost(2)
    for make in (lambda **kw: dq.CostPhase(c, nqubit=2, **kw), lambda **kw: dq.DiagonalGate(torch.ones(4) + 0j, nqubit=2, **kw)):
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


def test_autograd_closure_through_the_stand_ins(cpu_backend):
    """gradcheck / gradgradcheck at n = 3 of the three operations that differentiate into one another, with a control and
    a gathered table."""
    n, bits, controls = 3, (0, 2), (1,)
    c = rand_cost(2, 2)
    x = rand_state(2, n, 1).requires_grad_()
    y = rand_state(2, n, 2).requires_grad_()
    t = torch.tensor([0.3, -0.8], dtype=torch.float64, requires_grad=True)
    s = torch.tensor([0.3 - 0.2j, 1.1j], dtype=torch.complex128, requires_grad=True)
    d = torch.exp(1j * rand_cost(2, 3)).to(torch.complex128)
    gc, ggc = torch.autograd.gradcheck, torch.autograd.gradgradcheck
    assert gc(lambda a, b: ops.cost_phase(a, c, b, bits, controls), (x, t))
    assert ggc(lambda a, b: ops.cost_phase(a, c, b, bits, controls), (x, t))
    assert gc(lambda a, b: ops.cost_cross(a, b, c, bits, controls), (x, y))
    assert ggc(lambda a, b: ops.cost_cross(a, b, c, bits, controls), (x, y))
    assert gc(lambda a, b: ops.cost_scale(a, c, b, bits, controls), (x, s))
    assert ggc(lambda a, b: ops.cost_scale(a, c, b, bits, controls), (x, s))
    assert gc(lambda a: ops.diag_mul(a, d, bits, controls), (x,))
    assert gc(lambda a: qmath.expectation_cost(a, n, rand_cost(n, 5)), (x,))
    assert ggc(lambda a: qmath.expectation_cost(a, n, rand_cost(n, 5)), (x,))
    # a shared t gets the sum of the samples' gradients
    t1 = torch.tensor(0.3, dtype=torch.float64, requires_grad=True)
    assert gc(lambda b: ops.cost_phase(x.detach(), c, b, bits, controls), (t1,))
    # forward mode and vmap
    assert gc(lambda a, b: ops.cost_phase(a, c, b, bits, controls), (x, t), check_forward_ad=True, check_backward_ad=False)
    ts = torch.tensor([0.1, 0.5, -2.0], dtype=torch.float64)
    xs, cn = x.detach()[:1], rand_cost(n, 5)
    f = lambda th: qmath.expectation_cost(ops.cost_phase(xs, c, th, bits, controls) + xs, n, cn)[0]  # noqa: E731
    loop = torch.stack([f(th) for th in ts])
    assert torch.allclose(torch.vmap(f)(ts), loop, atol=1e-13)
    g = torch.vmap(torch.func.grad(f))(ts)
    eps = 1e-6
    fd = torch.stack([(f(th + eps) - f(th - eps)) / (2 * eps) for th in ts])
    assert torch.allclose(g, fd, atol=1e-7)


def test_the_circuit_itself_under_vmap_and_func_grad(cpu_backend):
    """The seam of ``_run_operators`` -- a fused stretch, ``apply_flat``, a new stretch with the zero-state shortcut off --
    with a wrapped ``t``: a loop over three values equals ``torch.vmap`` over the circuit, ``torch.func.grad`` matches
    finite differences, and so does ``vmap(grad)``.  ``t`` reaches the gate as data (``encode=True``)."""
    n = 3
    c = rand_cost(n, 12)
    cir = dq.QubitCircuit(n)
    cir.hlayer()
    cir.cost_phase(c, encode=True)
    cir.rxlayer(inputs=[0.4, -0.9, 1.3])
    cir.to(torch.double)

    def f(th):
        return qmath.expectation_cost(cir(th.reshape(1)), n, c)

    ts = torch.tensor([0.1, 0.5, -2.0], dtype=torch.float64)
    loop = torch.stack([f(th) for th in ts])
    assert loop.std() > 1e-2
    assert torch.allclose(torch.vmap(f)(ts), loop, atol=1e-13)
    eps = 1e-6
    fd = torch.stack([(f(th + eps) - f(th - eps)) / (2 * eps) for th in ts])
    g = torch.stack([torch.func.grad(f)(th) for th in ts])
    assert torch.allclose(g, fd, atol=1e-7) and g.abs().min() > 1e-3
    assert torch.allclose(torch.vmap(torch.func.grad(f))(ts), g, atol=1e-12)
    # the gate's parameter set by hand under the transform, as a trainable circuit's would be
    gate = cir.operators[n]

    def h(th):
        gate.init_para(th)
        return qmath.expectation_cost(cir(), n, c)

    assert torch.allclose(torch.vmap(h)(ts), loop, atol=1e-13)
    gate.init_para(0.0)


def test_to_double_and_back_keeps_the_complex_buffers_complex(cpu_backend):
    """``.to(torch.double)`` promotes the complex buffer of a DiagonalGate, a MultiplexedGate and a HamiltonianGate to
    complex128 with its imaginary part, so that the gate equals one built in double from the same numbers, and
    ``.to(torch.float)`` brings it back to complex64."""
    n = 3
    g = torch.Generator().manual_seed(5)
    phases = torch.exp(1j * torch.randn(1 << n, dtype=torch.float64, generator=g)).to(torch.complex64)
    blocks = torch.linalg.qr(torch.randn(4, 2, 2, dtype=torch.complex128, generator=g))[0].to(torch.complex64)
    ham = (0.5 * torch.from_numpy(np.kron([[0, 1], [1, 0]], [[0, -1j], [1j, 0]]))
           - 0.75 * torch.from_numpy(np.kron([[0, -1j], [1j, 0]], [[1, 0], [0, -1]])))       # complex128, exact in complex64
    cases = [
        ('diag', lambda dt: dq.DiagonalGate(phases.to(dt), nqubit=n), phases, lambda gate: gate.get_unitary()),
        ('unitaries', lambda dt: dq.MultiplexedGate(blocks.to(dt), nqubit=n, wires=[2, 0, 1]), blocks, lambda gate: gate.get_unitary()),
        ('ham_tsr', lambda dt: dq.HamiltonianGate(ham.to(dt), t=torch.tensor(0.375, dtype=dt.to_real()), nqubit=n, wires=[0, 1]), ham,
         lambda gate: gate.update_matrix()),
    ]
    for name, make, values, unitary in cases:
        gate, want = make(torch.complex64), make(torch.complex128)
        assert getattr(gate, name).dtype == torch.complex64 and getattr(want, name).dtype == torch.complex128
        assert gate.to(torch.double) is gate
        buf = getattr(gate, name)
        assert buf.dtype == torch.complex128 and torch.equal(buf, values.to(torch.complex128)) and buf.imag.abs().max() > 0.1
        assert unitary(gate).dtype == torch.complex128 and torch.equal(unitary(gate), unitary(want))
        gate.to(torch.float)
        assert getattr(gate, name).dtype == torch.complex64 and torch.equal(getattr(gate, name), values.to(torch.complex64))
        assert unitary(gate).dtype == torch.complex64
