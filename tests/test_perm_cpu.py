"""Host logic of the basis-state permutation gates (PermutationGate, ops.permute_basis, backend.apply_permutation)
without a GPU: the kernel's stand-in is the plain-torch route of ``backend.apply_permutation`` under the CPU test double,
so what is checked here is the library's argument checks, the wire-to-bit mapping, the validation of tables, the
autograd rules and the bookkeeping."""

import io
import os
import pickle
import re

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import _lib, backend, ops, qmath
from _perm_ref import (bit_reversal, identity, increment, inverse_of, perm_matrix, permute_ref, random_bijection, random_state,
                       same_bits)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tt(a):
    return torch.from_numpy(np.asarray(a))


def test_library_exports_the_new_symbols_and_still_reports_abi_30():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 30 and lib.dq_abi_version() == 30
    for name in ('dq_apply_permutation_c64', 'dq_apply_permutation_c128', 'dq_permutation_local_bits'):
        assert hasattr(lib, name) and name in _lib.exported_symbols()
    text = open(os.path.join(ROOT, 'include', 'dq_hip.h')).read()
    assert re.search(r'#define DQ_ABI_VERSION 30\b', text)
    for name in ('dq_apply_permutation_c64', 'dq_apply_permutation_c128', 'dq_permutation_local_bits'):
        assert re.search(r'\bint %s\(' % name, text)
    assert re.search(r'#define DQ_PERM_AUTO %d\b' % _lib.PERM_AUTO, text)
    assert re.search(r'#define DQ_PERM_GATHER %d\b' % _lib.PERM_GATHER, text)
    assert re.search(r'#define DQ_PERM_LOCAL %d\b' % _lib.PERM_LOCAL, text)
    assert (_lib.PERM_AUTO, _lib.PERM_GATHER, _lib.PERM_LOCAL) == (0, 1, 2)
    assert lib.dq_permutation_local_bits(0) == 11 and lib.dq_permutation_local_bits(1) == 10
    assert backend.permutation_local_bits(torch.complex64) == 11 and backend.permutation_local_bits(torch.complex128) == 10
    assert hasattr(dq, 'PermutationGate')


def test_host_side_argument_checks_of_the_library():
    """DQ_ERR_ARG with a text, before any HIP call (no device is touched: the pointers are never dereferenced)."""
    lib = _lib.load()
    ia = _lib.int_array
    p, q, t = 1 << 20, 1 << 30, 4096                    # aligned non-null "pointers", far apart
    f64, f128 = lib.dq_apply_permutation_c64, lib.dq_apply_permutation_c128

    def refused(rc, word):
        assert rc == -1 and word in lib.dq_last_error().decode(), lib.dq_last_error()

    for f in (f64, f128):
        refused(f(None, q, t, 3, ia([0]), 1, ia([]), 0, 1, 0, None), 'null')
        refused(f(p, None, t, 3, ia([0]), 1, ia([]), 0, 1, 0, None), 'null')
        refused(f(p, q, None, 3, ia([0]), 1, ia([]), 0, 1, 0, None), 'null')
        refused(f(p, q, t, 0, ia([0]), 1, ia([]), 0, 1, 0, None), 'n=0')
        refused(f(p, q, t, 41, ia([0]), 1, ia([]), 0, 1, 0, None), 'n=41')
        refused(f(p, q, t, 3, ia([0]), 0, ia([]), 0, 1, 0, None), 'k=0')
        refused(f(p, q, t, 3, ia([0, 1, 2, 3]), 4, ia([]), 0, 1, 0, None), 'k=4')                 # k > n
        refused(f(p, q, t, 40, ia(range(32)), 32, ia([]), 0, 1, 0, None), 'k=32')                 # k > 31
        refused(f(p, q, t, 3, ia([3]), 1, ia([]), 0, 1, 0, None), 'out of range')
        refused(f(p, q, t, 3, ia([-1]), 1, ia([]), 0, 1, 0, None), 'out of range')
        refused(f(p, q, t, 3, ia([0]), 1, ia([3]), 1, 1, 0, None), 'out of range')
        refused(f(p, q, t, 3, ia([1, 1]), 2, ia([]), 0, 1, 0, None), 'twice')
        refused(f(p, q, t, 3, ia([0]), 1, ia([2, 2]), 2, 1, 0, None), 'twice')
        refused(f(p, q, t, 3, ia([0, 1]), 2, ia([1]), 1, 1, 0, None), 'twice')                    # a control inside the table bits
        refused(f(p, q, t, 3, ia([0]), 1, ia([]), 0, 0, 0, None), 'batch')
        refused(f(p, q, t, 3, ia([0]), 1, ia([]), 0, 65536, 0, None), 'batch')
        refused(f(p + 8, q, t, 3, ia([0]), 1, ia([]), 0, 1, 0, None), 'aligned')
        refused(f(p, q + 8, t, 3, ia([0]), 1, ia([]), 0, 1, 0, None), 'aligned')
        refused(f(p, q, t + 2, 3, ia([0]), 1, ia([]), 0, 1, 0, None), 'aligned')
        refused(f(p, p, t, 3, ia([0]), 1, ia([]), 0, 1, 0, None), 'overlap')
        refused(f(p, q, t, 3, ia([0]), 1, ia([]), 0, 1, 3, None), 'path')
        refused(f(p, q, t, 3, ia([0]), 1, ia([]), 0, 1, -1, None), 'path')
    # the ranges [in, in + batch * 2^n) and [out, ..): 2 samples of 8 amplitudes are 128 (256) bytes
    refused(f64(p, p + 112, t, 3, ia([0]), 1, ia([]), 0, 2, 0, None), 'overlap')
    refused(f64(p + 112, p, t, 3, ia([0]), 1, ia([]), 0, 2, 0, None), 'overlap')
    refused(f128(p, p + 240, t, 3, ia([0]), 1, ia([]), 0, 2, 0, None), 'overlap')
    # LOCAL: every table bit below dq_permutation_local_bits
    refused(f64(p, q, t, 14, ia([11]), 1, ia([]), 0, 1, _lib.PERM_LOCAL, None), 'DQ_PERM_LOCAL')
    refused(f128(p, q, t, 14, ia([3, 10]), 2, ia([]), 0, 1, _lib.PERM_LOCAL, None), 'DQ_PERM_LOCAL')


CASES = [
    # n, bits, controls
    (5, (3, 0, 4), ()),                 # unsorted
    (5, (2,), ()),                      # k = 1
    (4, (3, 2, 1, 0), ()),              # k = n, the natural order
    (4, (0, 2, 3, 1), ()),              # k = n, shuffled
    (5, (1, 3), (0,)),                  # one control
    (6, (4, 1, 2), (5, 0)),             # two controls
]


@pytest.mark.parametrize('n,bits,controls', CASES)
def test_stand_in_against_the_definition(cpu_backend, n, bits, controls):
    k = len(bits)
    for dtype in (np.complex64, np.complex128):
        x = random_state(2, n, 3, dtype)
        for perm in (random_bijection(k, 11), identity(k), bit_reversal(k), increment(k)):
            want = permute_ref(x, perm, bits, controls)
            got = backend.apply_permutation(tt(x), tt(inverse_of(perm)), bits, controls).numpy()
            np.testing.assert_array_equal(got, want)
            assert same_bits(got, want)
            assert same_bits(ops.permute_basis(tt(x), tt(perm), bits, controls).numpy(), want)


def test_one_wire_swap_is_pauli_x(cpu_backend):
    n = 4
    x = tt(random_state(1, n, 5, np.complex128))
    for w in range(n):
        cir = dq.QubitCircuit(n)
        cir.x(w)
        want = cir(state=x.reshape(-1, 1)).reshape(1, -1)
        got = dq.PermutationGate([1, 0], nqubit=n, wires=[w]).apply_flat(x)
        assert torch.equal(got, want)


def test_backend_refusals(cpu_backend):
    x = tt(random_state(2, 4, 1, np.complex128))
    src = torch.arange(4)
    ok = dict(src=src, bits=(1, 2), controls=())
    for bad, word in ((dict(bits=(1, 1)), 'distinct'), (dict(bits=(1, 4)), 'distinct'), (dict(controls=(2,)), 'distinct'),
                      (dict(bits=()), 'at least one'), (dict(src=torch.arange(8)), 'entries'), (dict(src=torch.arange(4.0)), 'integer'),
                      (dict(path='lds'), 'path'), (dict(out=x), 'overlap'), (dict(out=torch.zeros(2, 8, dtype=x.dtype)), 'shape'),
                      (dict(out=torch.zeros(2, 16, dtype=torch.complex64)), 'shape')):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError, match=word):
            backend.apply_permutation(x, **kw)
    flat = torch.zeros(40, dtype=torch.complex128)
    with pytest.raises(ValueError, match='overlap'):
        backend.apply_permutation(flat[:32].reshape(2, 16), src, (1, 2), out=flat[8:].reshape(2, 16))
    big = torch.zeros(1, 1 << 12, dtype=torch.complex64)
    with pytest.raises(ValueError, match='local'):
        backend.apply_permutation(big, torch.arange(2), (11,), path='local')
    assert backend.apply_permutation(big, torch.arange(2), (10,), path='local').shape == big.shape
    out = torch.empty_like(x)
    assert backend.apply_permutation(x, src, (1, 2), out=out) is out and torch.equal(out, x)
    # an entry beyond the table is masked to k bits, as the kernels mask it: a wrong state, never an index out of range
    got = backend.apply_permutation(x, torch.tensor([0, 1, 2, 7]), (1, 2))
    assert torch.equal(got, backend.apply_permutation(x, torch.tensor([0, 1, 2, 3]), (1, 2)))


def test_tables_that_are_no_bijections_are_refused():
    for perm, word in (([0, 1, 2], 'entries'), ([0, 1, 2, 3, 4], 'entries'), ([0, 1, 2, 4], 'lie in'), ([0, -1, 2, 3], 'lie in'),
                       ([0, 1, 1, 3], 'bijection'), (torch.tensor([0.0, 1.0, 2.0, 3.0]), 'integers'), ([0, 1.5, 2, 3], 'integers')):
        with pytest.raises(ValueError, match=word):
            dq.PermutationGate(perm, nqubit=3, wires=[0, 2])
    with pytest.raises(AssertionError):
        dq.PermutationGate([0, 1, 2, 3], nqubit=3, wires=[0, 1], controls=[1])
    g = dq.PermutationGate(torch.tensor([2, 0, 3, 1], dtype=torch.int16), nqubit=3, wires=[0, 2], controls=[1])
    assert g.perm.dtype == torch.int32 and g.perm.tolist() == [2, 0, 3, 1] and g.inv.tolist() == [1, 3, 0, 2]


def test_gate_unitary_inverse_and_the_dense_route(cpu_backend):
    n, wires, controls = 4, [2, 0, 3], [1]
    perm = random_bijection(3, 21)
    g = dq.PermutationGate(perm, nqubit=n, wires=wires, controls=controls)
    m = perm_matrix(perm)
    # on all wires in their order the unitary is the 0/1 matrix itself
    full = dq.PermutationGate(random_bijection(n, 22), nqubit=n)
    assert torch.equal(full.get_unitary().real, tt(perm_matrix(random_bijection(n, 22))).float())
    assert full.get_unitary().dtype == torch.complex64 and full.double().get_unitary().dtype == torch.complex128
    # cir.permutation equals cir.any of the 0/1 matrix
    a, b = dq.QubitCircuit(n), dq.QubitCircuit(n)
    a.permutation(perm, wires=wires, controls=controls)
    b.any(tt(m).to(torch.complex64), wires=wires, controls=controls)
    assert torch.equal(a.get_unitary(), b.get_unitary())
    x = tt(random_state(3, n, 2, np.complex64))
    assert torch.allclose(a(state=x.reshape(3, -1, 1)), b(state=x.reshape(3, -1, 1)), atol=1e-6)
    # inverse() swaps the tables and undoes the gate, bit for bit; twice gives the gate back
    inv = g.inverse()
    assert inv.name == 'PermutationGate_dagger' and inv.tables()[0] is g.inv and inv.tables()[1] is g.perm
    assert torch.equal(inv.apply_flat(g.apply_flat(x)), x)
    assert torch.equal(inv.get_unitary(), g.get_unitary().T)
    assert torch.equal(inv.inverse().apply_flat(x), g.apply_flat(x))
    back = a + a.inverse()
    assert len(back.operators) == 2 and torch.equal(back(state=x.reshape(3, -1, 1)).reshape(3, -1), x)
    assert 'entries=8' in repr(g)


def test_tables_survive_moves_state_dict_pickle_and_addition(cpu_backend):
    n = 4
    perm = random_bijection(3, 5)
    cir = dq.QubitCircuit(n)
    cir.hlayer()
    cir.permutation(perm, wires=[3, 1, 0])
    cir.rxlayer()
    x = tt(random_state(2, n, 9, np.complex128)).reshape(2, -1, 1)
    cir.to(torch.double)
    at = [i for i, op in enumerate(cir.operators) if isinstance(op, dq.PermutationGate)]
    assert len(at) == 1
    g = cir.operators[at[0]]
    assert g.perm.dtype == torch.int32 and g.perm.tolist() == list(perm) and g._state_like()[0] == torch.complex128
    want = cir(state=x)
    # state_dict: into a circuit built with another table
    other = dq.QubitCircuit(n)
    other.hlayer()
    other.permutation(identity(3), wires=[3, 1, 0])
    other.rxlayer()
    other.to(torch.double)
    sd = cir.state_dict()
    assert {k for k in sd if k.startswith(f'operators.{at[0]}.')} == {f'operators.{at[0]}.perm', f'operators.{at[0]}.inv'}
    other.load_state_dict(sd)
    assert torch.equal(other(state=x), want)
    # pickle and torch.save
    again = pickle.loads(pickle.dumps(cir))
    assert again.operators[at[0]].inv.tolist() == list(inverse_of(perm)) and torch.equal(again(state=x), want)
    buf = io.BytesIO()
    torch.save(cir, buf)
    buf.seek(0)
    assert torch.equal(torch.load(buf, weights_only=False)(state=x), want)
    # cir1 + cir2
    both = cir + cir.inverse()
    assert torch.allclose(both(state=x), x, atol=1e-12)


def test_bit_oracle_and_modmul(cpu_backend):
    n = 5
    f = [3, 0, 2, 1, 1, 3, 0, 2]
    cir = dq.QubitCircuit(n)
    cir.bit_oracle(f, xwires=[4, 0, 2], ywires=[3, 1])
    g = cir.operators[0]
    assert g.wires == [4, 0, 2, 3, 1]
    assert g.perm.tolist() == [(x << 2) | (y ^ f[x]) for x in range(8) for y in range(4)]
    x = tt(random_state(2, n, 4, np.complex64))
    once = g.apply_flat(x)
    assert not torch.equal(once, x) and torch.equal(g.apply_flat(once), x)             # an involution
    # |x>|0> -> |x>|f(x)> on basis states (wire w is index bit n - 1 - w)
    for xv in range(8):
        idx = sum(((xv >> (2 - j)) & 1) << (n - 1 - w) for j, w in enumerate([4, 0, 2]))
        e = torch.zeros(1, 1 << n, dtype=torch.complex64)
        e[0, idx] = 1
        to = idx | sum(((f[xv] >> (1 - j)) & 1) << (n - 1 - w) for j, w in enumerate([3, 1]))
        assert int(g.apply_flat(e)[0].real.argmax()) == to
    for bad in (dict(f=[0] * 4), dict(f=[4] + [0] * 7), dict(f=[-1] + [0] * 7), dict(f=[0.5] * 8)):
        kw = dict(f=f, xwires=[4, 0, 2], ywires=[3, 1])
        kw.update(bad)
        with pytest.raises(ValueError):
            dq.QubitCircuit(n).bit_oracle(**kw)
    # modular multiplication
    for a, mod, k in ((7, 15, 4), (2, 15, 4), (5, 21, 5), (3, 16, 4), (1, 1, 2), (10, 21, 6)):
        t = qmath.modmul_table(a, mod, k)
        assert t.dtype == torch.int64 and sorted(t.tolist()) == list(range(1 << k))      # a bijection
        assert t[mod:].tolist() == list(range(mod, 1 << k))                             # x >= N stays
        assert t[:mod].tolist() == [(a * v) % mod for v in range(mod)]
    for a, mod, k in ((3, 15, 4), (6, 21, 5), (2, 16, 4), (0, 15, 4), (7, 17, 4), (7, 0, 4), (7, 15, 0), (7, 15, 32)):
        with pytest.raises(ValueError):
            qmath.modmul_table(a, mod, k)
    cir = dq.QubitCircuit(6)
    cir.modmul(7, 15, wires=[2, 3, 4, 5], controls=[0])
    g = cir.operators[0]
    assert g.controls == [0] and g.perm.tolist() == qmath.modmul_table(7, 15, 4).tolist()
    with pytest.raises(ValueError):
        cir.modmul(5, 15, wires=[2, 3, 4, 5])
    with pytest.raises(ValueError):
        cir.modmul(7, 17, wires=[2, 3, 4, 5])
    # 7^4 = 1 mod 15: four multiplications are the identity
    four = dq.QubitCircuit(4)
    for _ in range(4):
        four.modmul(7, 15)
    y = tt(random_state(1, 4, 6, np.complex64))
    assert torch.equal(four(state=y.reshape(-1, 1)).reshape(1, -1), y)


def test_autograd_rules_through_the_stand_in(cpu_backend):
    """gradcheck / gradgradcheck, forward mode, vmap and the exact backward at n = 3 with a control."""
    n, bits, controls = 3, (2, 0), (1,)
    perm = tt(random_bijection(2, 8))
    inv = tt(inverse_of(perm.numpy()))
    x = tt(random_state(2, n, 1, np.complex128)).requires_grad_()
    f = lambda s: ops.permute_basis(s, perm, bits, controls)  # noqa: E731
    gc, ggc = torch.autograd.gradcheck, torch.autograd.gradgradcheck
    assert gc(f, (x,))
    assert ggc(f, (x,))
    assert gc(f, (x,), check_forward_ad=True, check_backward_ad=False)
    # the backward of the state is the permutation by the inverse table, exactly
    gy = tt(random_state(2, n, 2, np.complex128))
    (gx,) = torch.autograd.grad(f(x), x, gy)
    assert same_bits(gx.numpy(), permute_ref(gy.numpy(), inv.numpy(), bits, controls))
    # jvp: the same permutation of the tangent
    t = tt(random_state(2, n, 3, np.complex128))
    y, yt = torch.func.jvp(f, (x.detach(),), (t,))
    assert same_bits(yt.numpy(), permute_ref(t.numpy(), perm.numpy(), bits, controls))
    assert same_bits(y.numpy(), permute_ref(x.detach().numpy(), perm.numpy(), bits, controls))
    # vmap folds the mapped dimension into the batch
    xs = tt(random_state(6, n, 4, np.complex128)).reshape(3, 2, -1)
    got = torch.vmap(f)(xs)
    assert same_bits(got.numpy().reshape(6, -1), permute_ref(xs.numpy().reshape(6, -1), perm.numpy(), bits, controls))
    got = torch.vmap(f, in_dims=1)(xs.transpose(0, 1).contiguous())
    assert same_bits(got.numpy().reshape(6, -1), permute_ref(xs.numpy().reshape(6, -1), perm.numpy(), bits, controls))
    with pytest.raises(ValueError, match='integer'):
        ops.permute_basis(x, perm.double(), bits)
    # through a circuit: a trainable layer before and after the permutation
    cir = dq.QubitCircuit(n)
    cir.rxlayer()
    cir.permutation(perm, wires=[0, 2], controls=[1])
    cir.rylayer()
    cir.observable(0)
    cir.to(torch.double)
    cir()
    cir.expectation().sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in cir.parameters())


def test_refusals(cpu_backend):
    make = lambda **kw: dq.PermutationGate([1, 0, 3, 2], nqubit=2, **kw)  # noqa: E731
    name = 'PermutationGate'
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
