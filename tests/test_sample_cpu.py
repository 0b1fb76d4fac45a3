"""The inverse-CDF shot sampler without a GPU: the C ABI's host-side checks (dq_sample_*), ``qmath.sample`` and
``measure(sampler='inverse_cdf')`` on the CPU test double, whose ``backend._sample_indices_double`` states the kernel's
contract in torch."""

import ctypes

import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import _lib, backend, qmath


def rand_state(n, batch=None, dtype=torch.complex64, seed=0):
    g = torch.Generator().manual_seed(seed)
    shape = (1 << n,) if batch is None else (batch, 1 << n)
    psi = torch.randn(*shape, dtype=dtype, generator=g)
    return psi / psi.norm(dim=-1, keepdim=True)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ghz(n, dtype=torch.complex64):
    psi = torch.zeros(1 << n, dtype=dtype)
    psi[0] = psi[-1] = 0.5**0.5
    return psi


# ---- C ABI -------------------------------------------------------------------------------------------------------
def test_ws_bytes_rejects_bad_arguments():
    lib = _lib.load()
    assert lib.dq_sample_ws_bytes(0, 1, 0) == -1
    assert lib.dq_sample_ws_bytes(41, 1, 0) == -1
    assert lib.dq_sample_ws_bytes(12, 0, 0) == -1
    assert lib.dq_sample_ws_bytes(12, 65536, 0) == -1


@pytest.mark.parametrize('is_c128', [0, 1])
@pytest.mark.parametrize('n', [1, 5, 6, 7, 12, 13, 28, 34])
def test_ws_bytes_within_budget(n, is_c128):
    lib = _lib.load()
    for batch in (1, 3, 65535):
        got = lib.dq_sample_ws_bytes(n, batch, is_c128)
        state_bytes = batch * (1 << n) * (16 if is_c128 else 8)
        assert 0 <= got <= 0.02 * state_bytes + 64 * 1024
        # the tree: levels of 2^(n - 6 l) doubles up to the first with at most 64 entries
        want = sum(batch * (1 << (n - 6 * l)) * 8 for l in range(1, (n + 5) // 6))
        assert got == want


def test_null_pointers_and_small_workspace_are_argument_errors_without_a_gpu():
    lib = _lib.load()
    rc = lib.dq_sample_c64(None, 10, 1, None, 16, None, None, 0, None)
    assert rc == -1 and b'null' in lib.dq_last_error()
    # (host memory: the checks return before anything touches it)
    raw = (ctypes.c_double * 4098)()
    psi = ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)
    u = (ctypes.c_double * 16)()
    out = (ctypes.c_int64 * 16)()
    ws = (ctypes.c_double * 16)()
    for fn in (lib.dq_sample_c64, lib.dq_sample_c128):
        assert fn(psi, 0, 1, u, 16, out, ws, 128, None) == -1 and b'n=0' in lib.dq_last_error()
        assert fn(psi, 41, 1, u, 16, out, ws, 128, None) == -1
        assert fn(psi, 10, 0, u, 16, out, ws, 128, None) == -1
        assert fn(psi, 10, 1, u, 0, out, ws, 128, None) == -1
        need = lib.dq_sample_ws_bytes(10, 1, 0)
        assert need == 16 * 8
        assert fn(psi, 10, 1, u, 16, out, ws, need - 8, None) == -1 and b'workspace' in lib.dq_last_error()
        assert fn(psi, 10, 1, u, 16, out, None, need, None) == -1


# ---- the contract in torch -------------------------------------------------------------------------------------------
def test_double_matches_a_longdouble_search():
    import numpy as np

    psi = rand_state(9, 2, torch.complex128, seed=3) * 1.7
    u = torch.rand(2, 500, dtype=torch.float64, generator=gen(1))
    u[0, 0], u[0, 1] = 0.0, float(np.nextafter(1.0, 0.0))
    got = backend._sample_indices_double(psi, u).numpy()
    for b in range(2):
        a = psi[b].numpy()
        p = a.real.astype(np.longdouble) ** 2 + a.imag.astype(np.longdouble) ** 2
        c = np.cumsum(p)
        ref = np.searchsorted(c, u[b].numpy().astype(np.longdouble) * c[-1], side='right')
        assert (got[b] != np.minimum(ref, len(p) - 1)).sum() <= 1


def test_double_never_returns_an_index_of_probability_zero():
    psi = torch.zeros(1, 64, dtype=torch.complex128)
    psi[0, 5], psi[0, 40] = 0.6, 0.8
    u = torch.tensor([[0.0, 0.3, 0.36, 0.999, 1.0 - 2.0**-53, 1.0]], dtype=torch.float64)     # (1.0: past the contract, clamped)
    got = backend._sample_indices_double(psi, u)
    assert got.tolist() == [[5, 5, 40, 40, 40, 40]]


def test_sample_indices_dispatches_to_the_double_and_checks_u(cpu_backend):
    psi = rand_state(6, 2)
    u = torch.rand(2, 9, dtype=torch.float64, generator=gen(0))
    got = backend.sample_indices(psi, u)
    assert got.dtype == torch.int64 and got.shape == (2, 9)
    assert torch.equal(got, backend._sample_indices_double(psi, u))
    with pytest.raises(ValueError):
        backend.sample_indices(psi, u.float())
    with pytest.raises(ValueError):
        backend.sample_indices(psi, u[:1])
    with pytest.raises(TypeError):
        backend.sample_indices(psi.real.contiguous(), u)


def test_sample_indices_without_a_backend_refuses_cpu_tensors():
    assert backend.get_test_backend() is None
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        backend.sample_indices(rand_state(4, 1), torch.rand(1, 3, dtype=torch.float64))


# ---- qmath.sample ----------------------------------------------------------------------------------------------------
def test_shapes_and_dtype_for_every_state_form(cpu_backend):
    n, dim = 5, 32
    single = rand_state(n)
    batch = rand_state(n, 3)
    forms = [(single, (7,)), (single.reshape(dim, 1), (7,)), (batch, (3, 7)), (batch.reshape(3, dim, 1), (3, 7)),
             (batch.reshape([3] + [2] * n), (3, 7)), (batch.to(torch.complex128), (3, 7)), (batch[:1], (1, 7)),
             (single.real.contiguous(), (7,))]
    for state, shape in forms:
        out = qmath.sample(state, n, shots=7, generator=gen(0))
        assert out.dtype == torch.int64 and tuple(out.shape) == shape and out.device == state.device
        assert int(out.min()) >= 0 and int(out.max()) < dim
    assert tuple(qmath.sample(single, n).shape) == (1024,)


def test_same_seed_same_tensor_and_all_forms_agree(cpu_backend):
    n = 6
    batch = rand_state(n, 2)
    a = qmath.sample(batch, n, shots=300, generator=gen(11))
    assert torch.equal(a, qmath.sample(batch, n, shots=300, generator=gen(11)))
    assert torch.equal(a, qmath.sample(batch.reshape([2] + [2] * n), n, shots=300, generator=gen(11)))
    assert not torch.equal(a, qmath.sample(batch, n, shots=300, generator=gen(12)))
    # the uniforms are the documented draw
    u = torch.rand(2, 300, dtype=torch.float64, generator=gen(11))
    assert torch.equal(a, backend._sample_indices_double(batch, u))


def test_wires_pick_bits_in_ascending_wire_order(cpu_backend):
    n = 6
    batch = rand_state(n, 2, seed=5)
    full = qmath.sample(batch, n, shots=400, generator=gen(3))
    for wires in ([1, 4], [4, 1], [5, 0, 3], 2, [0], [0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0]):
        got = qmath.sample(batch, n, shots=400, wires=wires, generator=gen(3))
        ws = sorted([wires] if isinstance(wires, int) else wires)
        want = torch.zeros_like(full)
        for w in ws:
            want = want * 2 + ((full >> (n - 1 - w)) & 1)
        assert torch.equal(got, want)


def test_outcome_is_the_key_of_measure(cpu_backend):
    # the basis state |1 0 1 1 0>: wire 0 is the most significant bit
    n = 5
    psi = torch.zeros(1 << n, dtype=torch.complex64)
    psi[0b10110] = 1.0
    assert qmath.sample(psi, n, shots=4).tolist() == [0b10110] * 4
    assert qmath.sample(psi, n, shots=4, wires=[0, 2, 4]).tolist() == [0b110] * 4
    key = next(iter(qmath.measure(psi, shots=4, wires=[0, 2, 4])))
    assert bin(0b110)[2:].zfill(3) == key


def test_ghz_and_basis_states_give_only_possible_outcomes(cpu_backend):
    n = 7
    out = qmath.sample(ghz(n), n, shots=500, generator=gen(2))
    assert set(out.tolist()) == {0, (1 << n) - 1}
    assert 150 < int((out == 0).sum()) < 350
    for k in (0, 77, (1 << n) - 1):
        psi = torch.zeros(3, 1 << n, dtype=torch.complex128)
        psi[:, k] = 2.5j                                           # (not normalised)
        assert (qmath.sample(psi, n, shots=50, generator=gen(k)) == k).all()


def test_density_matrix_route(cpu_backend):
    n = 3
    psi = rand_state(n, 2, torch.complex128, seed=8)
    rho = psi[:, :, None] * psi[:, None, :].conj()
    out = qmath.sample(rho, n, shots=200, generator=gen(4), den_mat=True)
    assert out.dtype == torch.int64 and tuple(out.shape) == (2, 200)
    assert torch.equal(out, qmath.sample(psi, n, shots=200, generator=gen(4)))       # the diagonal is |psi|^2
    one = qmath.sample(rho[0], n, shots=200, wires=[2, 0], generator=gen(4), den_mat=True)
    assert tuple(one.shape) == (200,)
    assert torch.equal(one, ((out[0] >> 2) & 1) * 2 + (out[0] & 1))
    mixed = torch.diag(torch.tensor([0, 0.25, 0, 0, 0.75, 0, 0, 0], dtype=torch.complex64))
    assert set(qmath.sample(mixed, n, shots=300, generator=gen(1), den_mat=True).tolist()) == {1, 4}
    with pytest.raises(ValueError):
        qmath.sample(psi, n, shots=5, den_mat=True)


def test_errors(cpu_backend):
    n = 4
    psi = rand_state(n)
    for shots in (0, -3):
        with pytest.raises(ValueError, match='shots'):
            qmath.sample(psi, n, shots=shots)
    for wires in ([0, 0], [4], [-1], [], [[0]]):
        with pytest.raises(ValueError, match='wires'):
            qmath.sample(psi, n, wires=wires)
    with pytest.raises(ValueError):
        qmath.sample(psi, 5)
    with pytest.raises(ValueError):
        qmath.sample([1.0, 0.0], 1)
    sharded = dq.state.DistributedQubitState.__new__(dq.state.DistributedQubitState)
    with pytest.raises(NotImplementedError):
        qmath.sample(sharded, n)


def test_runs_without_a_graph(cpu_backend):
    psi = rand_state(4).requires_grad_()
    out = qmath.sample(psi, 4, shots=8)
    assert not out.requires_grad


# ---- measure(sampler='inverse_cdf') ----------------------------------------------------------------------------------
def test_measure_inverse_cdf_has_the_dict_format_of_the_default_route(cpu_backend):
    n = 5
    psi = rand_state(n, seed=2).reshape(-1, 1)
    torch.manual_seed(0)
    old = qmath.measure(psi, shots=300)
    new = qmath.measure(psi, shots=300, sampler='inverse_cdf')
    for res in (old, new):
        assert isinstance(res, dict) and sum(res.values()) == 300
        assert all(isinstance(k, str) and len(k) == n and set(k) <= {'0', '1'} for k in res)
        assert all(isinstance(v, int) for v in res.values())
    sub = qmath.measure(psi, shots=100, wires=[3, 1], sampler='inverse_cdf')
    assert sum(sub.values()) == 100 and all(len(k) == 2 for k in sub)
    one = qmath.measure(psi, shots=100, wires=2, sampler='inverse_cdf')
    assert sum(one.values()) == 100 and set(one) <= {'0', '1'}


def test_measure_inverse_cdf_counts_the_samples_of_the_same_seed(cpu_backend):
    n = 5
    psi = rand_state(n, 2, seed=6)
    torch.manual_seed(5)
    res = qmath.measure(psi, shots=250, wires=[0, 3], sampler='inverse_cdf')
    torch.manual_seed(5)
    out = qmath.sample(psi, n, shots=250, wires=[0, 3])
    for b in range(2):
        want = {}
        for v in out[b].tolist():
            want[bin(v)[2:].zfill(2)] = want.get(bin(v)[2:].zfill(2), 0) + 1
        assert res[b] == want


def test_measure_inverse_cdf_with_prob(cpu_backend):
    n = 5
    psi = rand_state(n, seed=4)
    res = qmath.measure(psi, shots=200, with_prob=True, sampler='inverse_cdf')
    assert sum(c for c, _ in res.values()) == 200
    for key, (cnt, prob) in res.items():
        assert isinstance(cnt, int) and isinstance(prob, torch.Tensor) and prob.ndim == 0
        assert abs(prob.item() - abs(psi[int(key, 2)].item()) ** 2) < 1e-7
    wires = [1, 4]
    res = qmath.measure(psi, shots=200, with_prob=True, wires=wires, sampler='inverse_cdf')
    marg = (psi.abs() ** 2).reshape([2] * n).sum((0, 2, 3)).reshape(-1)
    assert sum(c for c, _ in res.values()) == 200
    for key, (_cnt, prob) in res.items():
        assert abs(prob.item() - marg[int(key, 2)].item()) < 1e-6
    old = qmath.measure(psi, shots=200, with_prob=True, wires=wires)
    for key in set(old) & set(res):
        assert abs(old[key][1].item() - res[key][1].item()) < 1e-6 and old[key][1].dtype == res[key][1].dtype


def test_measure_inverse_cdf_batch_and_density_matrix(cpu_backend):
    n = 3
    psi = rand_state(n, 3, seed=9)
    res = qmath.measure(psi.unsqueeze(-1), shots=64, sampler='inverse_cdf')
    assert isinstance(res, list) and len(res) == 3 and all(sum(r.values()) == 64 for r in res)
    rho = psi[0][:, None] * psi[0][None, :].conj()
    res = qmath.measure(rho, shots=64, with_prob=True, wires=[0, 2], den_mat=True, sampler='inverse_cdf')
    marg = (psi[0].abs() ** 2).reshape(2, 2, 2).sum(1).reshape(-1)
    assert sum(c for c, _ in res.values()) == 64
    for key, (_cnt, prob) in res.items():
        assert abs(prob.item() - marg[int(key, 2)].item()) < 1e-6


def test_measure_inverse_cdf_batch_of_one_returns_what_the_default_route_returns(cpu_backend):
    n = 3
    psi = rand_state(n, 1, seed=11)
    rho = psi[0][:, None] * psi[0][None, :].conj()
    forms = [(psi, False), (psi.unsqueeze(-1), False), (psi.reshape(1, 2, 2, 2), False), (psi[0], False),
             (psi[0].reshape(-1, 1), False), (rho, True), (rho.unsqueeze(0), True)]
    for state, den_mat in forms:
        for kw in ({}, {'wires': [0, 2]}, {'with_prob': True}):
            old = qmath.measure(state, shots=10, den_mat=den_mat, **kw)
            new = qmath.measure(state, shots=10, den_mat=den_mat, sampler='inverse_cdf', **kw)
            assert type(old) is dict and type(new) is dict, (tuple(state.shape), kw)
    two = rand_state(n, 2, seed=12)
    for state in (two, two.unsqueeze(-1)):
        old = qmath.measure(state, shots=10)
        new = qmath.measure(state, shots=10, sampler='inverse_cdf')
        assert type(old) is list and type(new) is list and len(old) == len(new) == 2


def test_circuit_with_batch_one_data_returns_the_same_type_from_both_samplers(cpu_backend):
    cir = dq.QubitCircuit(3)
    cir.hlayer()
    cir.rxlayer(encode=True)
    cir.cnot_ring()
    cir(data=torch.tensor([[0.3, 0.7, 1.1]]))
    assert tuple(cir.state.shape) == (1, 8, 1)
    old = cir.measure(shots=10)
    new = cir.measure(shots=10, sampler='inverse_cdf')
    assert type(old) is dict and type(new) is dict
    assert sum(new.values()) == 10 and all(len(k) == 3 for k in new)
    assert tuple(cir.sample(10).shape) == (1, 10)                 # (raw samples keep the batch axis of the state)


def test_measure_rejects_an_unknown_sampler(cpu_backend):
    with pytest.raises(ValueError, match='sampler'):
        qmath.measure(rand_state(3), shots=5, sampler='bogus')


def test_default_measure_never_reaches_sample_indices(cpu_backend, monkeypatch):
    calls = []
    real = backend.sample_indices
    monkeypatch.setattr(backend, 'sample_indices', lambda *a, **k: calls.append(1) or real(*a, **k))
    psi = rand_state(4, 2)
    qmath.measure(psi, shots=20)
    qmath.measure(psi, shots=20, wires=[1], with_prob=True)
    qmath.measure(psi, shots=20, sampler='multinomial')
    assert calls == []
    qmath.measure(psi, shots=20, sampler='inverse_cdf')
    assert calls == [1]


# ---- QubitCircuit ----------------------------------------------------------------------------------------------------
def test_circuit_sample_and_measure(cpu_backend):
    cir = dq.QubitCircuit(4)
    assert cir.sample() is None
    cir.h(0)
    for i in range(3):
        cir.cnot(i, i + 1)
    cir()
    out = cir.sample(120, generator=gen(1))
    assert cir.shots == 120 and tuple(out.shape) == (120,) and set(out.tolist()) == {0, 15}
    again = cir.sample(generator=gen(1))                 # (shots kept from the last call)
    assert torch.equal(out, again)
    sub = cir.sample(50, wires=[3, 1], generator=gen(1))
    assert set(sub.tolist()) == {0, 3} and cir.shots == 50
    res = cir.measure(shots=200, sampler='inverse_cdf')
    assert set(res) == {'0000', '1111'} and sum(res.values()) == 200
    with pytest.raises(ValueError):
        cir.measure(sampler='bogus')
