"""The inverse-CDF shot sampler on the MI355X (dq_sample_*), outcome by outcome against an 80-bit reference.

Reference: on the host, from the amplitudes as stored on the device, p = |psi|^2 and C = cumsum(p) in numpy.longdouble,
T = C[-1], ref = searchsorted(C, u * T, side='right').  Acceptance for EVERY shot, i = out[b, s]:

    p_i > 0   and   C(i-1) - tau T <= u T < C(i) + tau T,   tau = 1e-11 for both precisions

(the kernel's arithmetic is double; its accumulated rounding over the tree is of order 1e-12 T), and the number of shots
with out != ref is at most 4 of 4096 -- that cap keeps tau from hiding an off-by-one, which would miss on almost every
shot (a typical p_i >= 2^-24 >> tau).  n <= 22: there the reference itself has no threshold within tau T of a boundary
among 4096 uniform shots of the seeded states used here, other than the two forced edge values.

Sizes: n in {1, 3, 5} no tree, 6 exactly one group, 7 / 11 / 12 one level (root of 2 / 32 / 64), 13 / 18 two levels,
19 / 22 three (root of 2 / 16).  The descent strides over the shots once batch * shots > 4 * 65535 (the grid cap of
csrc/dq_sample.hip): `test_grid_limits[4-70000]`; the build strides over its chunks once batch * 2^(n-12) > 2048:
n = 22 with batch 3.  The upper-level kernel runs once at n = 19 .. 24 (level 3) and twice from n = 25 on (levels 3 and 4):
`test_second_upper_level` has n = 25 with a sparse state, whose reference needs the support only.  Its stride loop starts
at more than 4 * 65535 entries of one level >= 3, that is n >= 37 or 2^21 amplitudes at batch 32768: no test reaches it.
"""

import functools

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import _lib, backend, qmath

pytestmark = pytest.mark.gpu

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, 'the reference needs 80-bit long doubles'
TAU = 1e-11
DTYPES = {'c64': torch.complex64, 'c128': torch.complex128}
ONE_BELOW = float(np.nextafter(1.0, 0.0))


def reference(psi):
    """(p, C) in long double from the amplitudes as stored: (B, 2**n) each."""
    a = psi.cpu().numpy()
    p = a.real.astype(LD) ** 2 + a.imag.astype(LD) ** 2
    return p, np.cumsum(p, axis=1)


@functools.lru_cache(maxsize=4)
def gaussian(n, batch, dt, norm=1.7):
    """A seeded Gaussian state of the given norm on the device and its reference (shared, never modified)."""
    g = torch.Generator().manual_seed(1000 * n + batch)
    psi = torch.randn(batch, 1 << n, dtype=torch.complex128, generator=g)
    psi = (psi * (norm / psi.norm(dim=-1, keepdim=True))).to(DTYPES[dt]).cuda()
    return psi, reference(psi)


def uniforms(batch, shots, seed):
    u = torch.rand(batch, shots, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
    u[0, 0] = 0.0
    if shots > 1:         # (a single shot has room for one forced edge value only)
        u[0, 1] = ONE_BELOW
    return u


def accept(ref, u, out):
    """Every shot within the band and on an index of non-zero probability; at most 4 of 4096 away from the reference.

    The cap scales with the number of shots and is 0 below 1024 of them: none of the references used here has a
    threshold within tau T of a boundary, so a shot can only differ where u was forced to 1 - 2^-53, whose threshold
    lies 1.1e-16 T below the last boundary, inside the rounding of the kernel's own total -- one miss is allowed when
    that value is among the shots.  (u = 0 cannot miss: a sum of squares is zero only if every term is.)"""
    p, c = ref
    u = u.cpu().numpy().astype(LD)
    out = out.cpu().numpy()
    assert out.dtype == np.int64 and out.shape == u.shape
    assert out.min() >= 0 and out.max() < p.shape[1]
    t = c[:, -1:]
    thr = u * t
    assert (np.take_along_axis(p, out, 1) > 0).all(), 'an index of probability zero was returned'
    hi = np.take_along_axis(c, out, 1)
    lo = np.where(out > 0, np.take_along_axis(c, np.maximum(out - 1, 0), 1), LD(0))
    assert (lo - TAU * t <= thr).all() and (thr < hi + TAU * t).all()
    want = np.stack([np.searchsorted(c[b], thr[b], side='right') for b in range(len(c))])
    miss = int((out != want).sum())
    print(f'shots {out.size}: {miss} away from the reference')
    assert miss <= max(4 * out.size // 4096, int((u >= LD(ONE_BELOW)).any()))


def run(psi, u):
    return backend.sample_indices(psi, u.to(psi.device))


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('n', [1, 3, 5, 6, 7, 11, 12, 13, 18, 19, 22])
def test_gaussian_states(n, batch, dt):
    psi, ref = gaussian(n, batch, dt)
    for shots in (1, 7, 4096):
        u = uniforms(batch, shots, seed=n + shots)
        accept(ref, u, run(psi, u))


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('norm', [1.7, 1e-3])
def test_unnormalised_states(norm, dt):
    psi, ref = gaussian(13, 2, dt, norm)
    u = uniforms(2, 4096, seed=3)
    accept(ref, u, run(psi, u))


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_basis_and_ghz_states(dt):
    n = 13
    dim = 1 << n
    u = uniforms(1, 512, seed=4)
    for k in (0, dim - 1, 2741):
        psi = torch.zeros(1, dim, dtype=DTYPES[dt], device='cuda')
        psi[0, k] = 0.3 - 0.4j
        assert (run(psi, u) == k).all()
    psi = torch.zeros(1, dim, dtype=DTYPES[dt], device='cuda')
    psi[0, 0] = psi[0, -1] = 0.5**0.5
    out = run(psi, u).cpu()
    assert torch.equal(out, torch.where(u < 0.5, 0, dim - 1))
    accept(reference(psi), u, out)


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('kind', ['last_group', 'alternate_level1', 'alternate_level2'])
def test_sparse_states_never_return_an_index_of_probability_zero(kind, dt):
    n = 14                   # two levels, a root of 4 entries
    psi, _ = gaussian(n, 2, dt)
    psi = psi.clone()
    blocks = psi.view(2, -1, 64)
    if kind == 'last_group':
        blocks[:, :-1] = 0
    elif kind == 'alternate_level1':
        blocks[:, 0::2] = 0
    else:
        psi.view(2, -1, 4096)[:, 1::2] = 0
    ref = reference(psi)
    u = uniforms(2, 4096, seed=6)
    out = run(psi, u)
    accept(ref, u, out)
    if kind == 'last_group':
        assert int(out.min()) >= (1 << n) - 64


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_second_upper_level(dt):
    """n = 25: four levels, a root of 2 entries, levels 3 and 4 from two launches of the upper kernel over the
    contiguous rows of 2 samples.  4096 amplitudes per sample are non-zero, so the reference is their running sum."""
    n, batch, m = 25, 2, 4096
    g = torch.Generator().manual_seed(25)
    psi = torch.zeros(batch, 1 << n, dtype=DTYPES[dt], device='cuda')
    support = []
    for b in range(batch):
        at = torch.randperm(1 << n, generator=g)[:m].sort().values
        at[0], at[-1] = (0, (1 << n) - 1) if b == 0 else (at[0], at[-1])
        support.append(at.numpy())
        psi[b, at.cuda()] = torch.randn(m, dtype=torch.complex128, generator=g).to(DTYPES[dt]).cuda()
    support = np.stack(support)
    ref = reference(torch.stack([psi[b, torch.from_numpy(support[b]).cuda()] for b in range(batch)]))
    u = uniforms(batch, 4096, seed=25)
    out = run(psi, u).cpu().numpy()
    assert out.min() >= 0 and out.max() < 1 << n
    pos = np.stack([np.searchsorted(support[b], out[b]) for b in range(batch)])
    assert (np.take_along_axis(support, np.minimum(pos, m - 1), 1) == out).all(), 'an index of probability zero was returned'
    accept(ref, u, torch.from_numpy(pos))


def test_workspace_cache_keeps_one_tree_per_device_and_stream():
    u = uniforms(1, 8, seed=11).cuda()
    backend.clear_sample_workspace()
    for n in (13, 18, 13):
        psi, _ = gaussian(n, 1, 'c64')
        first = run(psi, u)
        assert len(backend._sample_ws_cache) == 1
        assert next(iter(backend._sample_ws_cache.values())).numel() * 8 == _lib.load().dq_sample_ws_bytes(n, 1, 0)
        assert torch.equal(run(psi, u), first) and len(backend._sample_ws_cache) == 1
    backend.clear_sample_workspace()
    assert not backend._sample_ws_cache
    assert torch.equal(run(psi, u), first)


def test_stratified_known_answer():
    n, shots = 10, 1 << 16
    for dt in DTYPES:
        psi, (p, c) = gaussian(n, 1, dt)
        u = ((torch.arange(shots, dtype=torch.float64) + 0.5) / shots).reshape(1, -1)
        out = run(psi, u).cpu().numpy()[0]
        counts = np.bincount(out, minlength=1 << n)
        expect = p[0] * shots / c[0, -1]
        assert (np.abs(counts - expect) <= 1).all()


@pytest.mark.parametrize('batch,shots', [(1, 70000), (300, 8), (4, 70000)])
def test_grid_limits(batch, shots):
    psi, ref = gaussian(8, batch, 'c64')
    u = uniforms(batch, shots, seed=7)
    accept(ref, u, run(psi, u))


def test_batches_beyond_65535_go_in_slices():
    batch = 65535 + 6
    g = torch.Generator().manual_seed(8)
    psi = torch.randn(batch, 4, dtype=torch.complex64, generator=g).cuda()
    u = uniforms(batch, 2, seed=8)
    accept(reference(psi), u, run(psi, u))


def test_reproducible_and_capturable():
    psi, ref = gaussian(13, 3, 'c64')
    u = uniforms(3, 4096, seed=9).cuda()
    first = run(psi, u)
    assert torch.equal(first, run(psi, u))
    graph = dq.CapturedGraph(lambda: backend.sample_indices(psi, u))
    assert torch.equal(graph.replay(), first)
    u2 = uniforms(3, 4096, seed=10)
    u.copy_(u2)
    out = graph.replay().clone()
    assert torch.equal(out, run(psi, u))
    accept(ref, u2, out)


def test_memory_above_the_state_is_the_tree_and_the_shots():
    n, shots = 22, 4096
    psi, _ = gaussian(n, 1, 'c64')
    gen = torch.Generator(device='cuda').manual_seed(1)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = qmath.sample(psi, n, shots=shots, generator=gen)
    torch.cuda.synchronize()
    above = torch.cuda.max_memory_allocated() - base
    ws = _lib.load().dq_sample_ws_bytes(n, 1, 0)
    print(f'above the state: {above} bytes; tree {ws}, u and out {2 * shots * 8}')
    assert tuple(out.shape) == (1, shots)
    assert above <= ws + 2 * shots * 8 + (1 << 20)
    assert ws <= 0.02 * psi.numel() * 8 + 65536


def test_qmath_sample_on_the_device():
    n = 12
    psi, ref = gaussian(n, 3, 'c128')
    gen = torch.Generator(device='cuda')
    out = qmath.sample(psi, n, shots=2000, generator=gen.manual_seed(3))
    u = torch.rand(3, 2000, dtype=torch.float64, device='cuda', generator=gen.manual_seed(3))
    assert out.is_cuda and out.dtype == torch.int64
    accept(ref, u, out)
    sub = qmath.sample(psi, n, shots=2000, wires=[11, 0, 5], generator=gen.manual_seed(3))
    assert torch.equal(sub, ((out >> 11) & 1) * 4 + ((out >> 6) & 1) * 2 + (out & 1))
    rho = psi[0, :64, None] * psi[0, None, :64].conj()               # (6 qubits, not normalised)
    got = qmath.sample(rho, 6, shots=2000, generator=gen.manual_seed(3), den_mat=True)
    u1 = torch.rand(1, 2000, dtype=torch.float64, device='cuda', generator=gen.manual_seed(3))
    accept(reference(psi[:1, :64]), u1, got.reshape(1, -1))


def test_circuit_end_to_end():
    n = 14
    cir = dq.QubitCircuit(n)
    cir.hlayer()
    cir.rxlayer()
    cir.cnot_ring()
    cir.rylayer()
    cir.to('cuda')
    cir()
    wires = [0, 7, 13]
    torch.manual_seed(5)
    out = cir.sample(500, wires=wires)
    torch.manual_seed(5)
    res = cir.measure(wires=wires, sampler='inverse_cdf')             # (shots kept: 500)
    assert out.is_cuda and tuple(out.shape) == (500,)
    want = {}
    for v in out.tolist():
        key = bin(v)[2:].zfill(3)
        want[key] = want.get(key, 0) + 1
    assert res == want and sum(res.values()) == 500
    ghz = dq.QubitCircuit(n)
    ghz.h(0)
    for i in range(n - 1):
        ghz.cnot(i, i + 1)
    ghz.to('cuda')
    ghz()
    res = ghz.measure(shots=200, sampler='inverse_cdf')
    assert set(res) == {'0' * n, '1' * n} and sum(res.values()) == 200
