"""The diagonal kernels on the MI355X (dq_apply_diag_*, dq_apply_cost_*, dq_cost_cross_*) against three lines of numpy in
complex128: the bit gather sub(i) = sum_j bit_{bits[j]}(i) << (k-1-j), exp, sum.

Geometry under test (csrc/dq_diag.hip): a lane moves 16 bytes, a workgroup iteration a chunk of 1024 such vectors --
2^11 complex64 or 2^10 complex128 amplitudes -- and at most 2048 workgroups per sample stride over the chunks.  So:
n = 1 and 3 are less than one vector per lane of a wave, n = 9 .. 12 lie on both sides of one chunk in both precisions,
and the grid-stride loop runs a second iteration from n = 23 (complex64) / n = 22 (complex128) on: `BIG`.  The gather is
split at the chunk size: runs of table bits below it are evaluated per lane, those above it per chunk; `CROSSING` has a
run of consecutive bits across that boundary in both precisions, (0, 5, n-1) has single bits on both sides.
bits = n-1 .. 0 without controls takes the instantiations that stream the table beside the state.

The table / in-flight switch of PHASE sits in ``backend.apply_cost``: complex128 with k <= 16, n >= k + 8 and n >= 24
builds the table of phases first (the PHASE kernel on a vector of ones over the k table bits) and runs the diagonal
kernel with one table per sample; everything else, and complex64 at every k, forms the phase in flight (DESIGN.md
section 4.8 has the measurements behind it).  The cases at n = 13 are therefore all in flight; `test_phase_switch`
runs both sides of each of the three conditions and observes the route taken by counting the calls of
``dq_apply_diag_c128``: at n = 24 / 23 with the thresholds as they are, and at n = 11 .. 14 with the thresholds scaled
down, so that no case is larger than it has to be.

Not reached: nothing.  The second grid-stride iteration needs n = 23 / 22: `test_full_width_gaussian[big-*]` and
`test_cost_cross_gaussian[big-*]` run it without a gather, `test_gathered_second_iteration` with one.  The batch is the
grid's y dimension and needs no loop (the Python wrapper slices batches above 32768).

Acceptance.  Exact rows: bit for bit.  Seeded Gaussian rows of apply_diag / PHASE / SCALE: the project's parity
criterion, max |out - ref| <= tol * max |ref| with tol = 1e-4 (complex64) / 1e-10 (complex128); the worst ratio
err / (tol * max |ref|) is printed (`-s`).  cost_cross: |out - ref| <= (2^-53 2^n + u_T) sum_i |c| |bra_i| |ket_i| with
u_T = 2^-24 / 2^-53, and the reference with its largest term dropped must fall outside that bound.
"""

import functools

import numpy as np
import pytest
import torch

from deepquantum_amd import backend
from _diag_ref import diag_ref, on_mask, phase_ref, sub_index

pytestmark = pytest.mark.gpu

DTYPES = {'c64': torch.complex64, 'c128': torch.complex128}
TOL = {'c64': 1e-4, 'c128': 1e-10}
U_T = {'c64': 2.0**-24, 'c128': 2.0**-53}
BIG = {'c64': 23, 'c128': 22}
FULL_N = (1, 3, 9, 10, 11, 12)
NG = 13                                        # gathered / controlled cases: 4 (8) chunks, table bits on both sides of the split
CROSSING = (12, 11, 10, 9)
GATHERED = {
    'k1_bit0': (0,), 'k1_top': (NG - 1,), 'k3_desc': (NG - 1, 5, 0), 'k3_asc': (0, 5, NG - 1), 'k3_mixed': (5, NG - 1, 0),
    'crossing': CROSSING, 'reversed': tuple(range(NG)), 'full_minus_one': tuple(range(NG - 1, 0, -1)),
}
CONTROLS = {'ctrl_bit0': ((6, 5), (0,)), 'ctrl_top': ((6, 5), (NG - 1,)), 'straddle': ((6, 5), (1, NG - 1)),
            'straddle_low': ((3, 2), (1, 4))}
WORST = {}


@functools.lru_cache(maxsize=None)
def gaussian(n, batch, dt, seed=0):
    """A seeded Gaussian state on the device and the same values in complex128 on the host (shared, never modified)."""
    g = torch.Generator().manual_seed(7919 * n + 31 * batch + seed)
    psi = torch.randn(batch, 1 << n, dtype=torch.complex128, generator=g).to(DTYPES[dt])
    return psi.cuda(), psi.numpy().astype(np.complex128)


@functools.lru_cache(maxsize=None)
def integer_state(n, batch, dt, seed=0):
    g = torch.Generator().manual_seed(104729 * n + batch + seed)
    re = torch.randint(-4, 5, (batch, 1 << n), generator=g)
    im = torch.randint(-4, 5, (batch, 1 << n), generator=g)
    psi = torch.complex(re.double(), im.double()).to(DTYPES[dt])
    return psi.cuda(), psi.numpy().astype(np.complex128)


def real_table(k, dt, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    c = (torch.randn(1 << k, dtype=torch.float64, generator=g) * scale).to(DTYPES[dt].to_real())
    return c.cuda(), c.numpy().astype(np.float64)


def phase_table(k, dt, seed, rows=None):
    g = torch.Generator().manual_seed(seed)
    shape = (1 << k,) if rows is None else (rows, 1 << k)
    d = torch.exp(1j * torch.rand(shape, dtype=torch.float64, generator=g) * 6.283).to(DTYPES[dt])
    return d.cuda(), d.numpy().astype(np.complex128)


EXACT_ENTRIES = np.array([1, -1, 1j, -1j, 1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j, 2, -3j], dtype=np.complex128)


def exact_table(k, dt, seed, rows=None):
    rng = np.random.default_rng(seed)
    shape = (1 << k,) if rows is None else (rows, 1 << k)
    d = EXACT_ENTRIES[rng.integers(0, len(EXACT_ENTRIES), shape)]
    return torch.from_numpy(d).to(DTYPES[dt]).cuda(), d


def parity(out, ref, dt, what):
    err = np.abs(out.cpu().numpy().astype(np.complex128) - ref).max()
    ratio = err / (TOL[dt] * np.abs(ref).max())
    WORST[(what, dt)] = max(WORST.get((what, dt), 0.0), ratio)
    print(f'{what} {dt}: worst err / (tol * max|ref|) = {ratio:.3e} (so far {WORST[(what, dt)]:.3e})')
    assert ratio <= 1.0, f'{what}: {err:.3e} against {TOL[dt]} * {np.abs(ref).max():.3e}'


def bitwise_equal(a, b):
    return torch.equal(torch.view_as_real(a).view(torch.int32 if a.dtype == torch.complex64 else torch.int64),
                       torch.view_as_real(b).view(torch.int32 if b.dtype == torch.complex64 else torch.int64))


def full(n):
    return tuple(range(n - 1, -1, -1))


# ---- exact rows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('n', FULL_N)
def test_apply_diag_exact_full_width(n, dt):
    x, xr = integer_state(n, 1, dt)
    d, dr = exact_table(n, dt, n)
    out = backend.apply_diag(x, d, full(n))
    assert np.array_equal(out.cpu().numpy().astype(np.complex128), diag_ref(xr, dr, n, full(n)))


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('name', sorted(GATHERED))
def test_apply_diag_exact_gathered(name, dt):
    bits = GATHERED[name]
    x, xr = integer_state(NG, 1, dt)
    d, dr = exact_table(len(bits), dt, 17)
    out = backend.apply_diag(x, d, bits)
    assert np.array_equal(out.cpu().numpy().astype(np.complex128), diag_ref(xr, dr, NG, bits))


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('stride', ['shared', 'per_sample'])
def test_apply_diag_batch_and_table_stride(stride, dt):
    bits = (NG - 1, 5, 0)
    for n, b in ((NG, bits), (12, full(12))):
        x, xr = integer_state(n, 3, dt)
        d, dr = exact_table(len(b), dt, 23, rows=None if stride == 'shared' else 3)
        out = backend.apply_diag(x, d, b)
        assert np.array_equal(out.cpu().numpy().astype(np.complex128), diag_ref(xr, dr, n, b))


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('same', [True, False], ids=['expect', 'cross'])
@pytest.mark.parametrize('case', ['n1', 'n3', 'n10', 'n11', 'n12', 'n14', 'gather', 'crossing', 'ctrl', 'batch3'])
def test_cost_cross_exact(case, same, dt):
    n = {'n1': 1, 'n3': 3, 'n10': 10, 'n11': 11, 'n12': 12, 'n14': 14}.get(case, NG)
    bits = {'gather': (5, NG - 1, 0), 'crossing': CROSSING, 'ctrl': (6, 5)}.get(case, full(n))
    controls = (1, NG - 1) if case == 'ctrl' else ()
    batch = 3 if case == 'batch3' else 1
    ket, kr = integer_state(n, batch, dt)
    bra, br = (ket, kr) if same else integer_state(n, batch, dt, seed=5)
    rng = np.random.default_rng(n)
    cr = rng.integers(-16, 17, 1 << len(bits)).astype(np.float64)
    c = torch.from_numpy(cr).to(DTYPES[dt].to_real()).cuda()
    out = backend.cost_cross(bra, ket, c, bits, controls)
    w = np.where(on_mask(n, controls), cr[sub_index(n, bits)], 0.0)
    ref = (w * br.conj() * kr).sum(-1)          # integers below 2^53: exact in any order
    assert out.dtype == torch.complex128 and out.shape == (batch,)
    assert np.array_equal(out.cpu().numpy(), ref)
    again = backend.cost_cross(bra, ket, c, bits, controls)
    assert torch.equal(torch.view_as_real(out), torch.view_as_real(again))


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('same', [True, False], ids=['expect', 'cross'])
def test_cost_cross_finish_second_stride_exact(same, dt):
    """512 partial sums per sample, batch 2: the finish kernel's lanes take a second stride of 256 partial sums and a
    second sample's row of the workspace (512 chunks: n = 20 complex64 / 19 complex128, full width).  Integer states in
    [-4, 4] and integer costs in [-16, 16]: every term is an integer of magnitude <= 512 and every sum of the 2^20 at most
    stays below 2^29 < 2^53, so the reference is exact in any order."""
    n = {'c64': 20, 'c128': 19}[dt]
    ket, kr = integer_state(n, 2, dt)
    bra, br = (ket, kr) if same else integer_state(n, 2, dt, seed=5)
    cr = np.random.default_rng(n).integers(-16, 17, 1 << n).astype(np.float64)
    c = torch.from_numpy(cr).to(DTYPES[dt].to_real()).cuda()
    out = backend.cost_cross(bra, ket, c, full(n))
    assert out.dtype == torch.complex128 and out.shape == (2,)
    assert np.array_equal(out.cpu().numpy(), (cr * br.conj() * kr).sum(-1))


# ---- seeded Gaussian rows -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('n', FULL_N + ('big',))
def test_full_width_gaussian(n, dt):
    n = BIG[dt] if n == 'big' else n
    x, xr = gaussian(n, 1, dt)
    d, dr = phase_table(n, dt, n)
    parity(backend.apply_diag(x, d, full(n)), diag_ref(xr, dr, n, full(n)), dt, 'apply_diag full')
    c, cr = real_table(n, dt, n + 1, scale=3.0)
    t = torch.tensor([0.83], dtype=torch.float64, device='cuda')
    parity(backend.apply_cost(x, c, t, full(n), (), 'phase'), phase_ref(xr, cr, [0.83], n, full(n)), dt, 'phase full')
    s = torch.tensor([0.4 - 1.3j], dtype=torch.complex128, device='cuda')
    parity(backend.apply_cost(x, c, s, full(n), (), 'scale'), (0.4 - 1.3j) * cr * xr, dt, 'scale full')


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('name', sorted(GATHERED))
def test_gathered_gaussian(name, dt):
    bits = GATHERED[name]
    k = len(bits)
    x, xr = gaussian(NG, 3, dt)
    d, dr = phase_table(k, dt, 3)
    parity(backend.apply_diag(x, d, bits), diag_ref(xr, dr, NG, bits), dt, 'apply_diag gathered')
    c, cr = real_table(k, dt, 4, scale=3.0)
    tv = [0.83, -2.1, 11.0]                     # batch 3, a different t per sample
    t = torch.tensor(tv, dtype=torch.float64, device='cuda')
    parity(backend.apply_cost(x, c, t, bits, (), 'phase'), phase_ref(xr, cr, tv, NG, bits), dt, 'phase gathered')
    x1, x1r = gaussian(NG, 1, dt)               # batch 1
    parity(backend.apply_cost(x1, c, t[:1], bits, (), 'phase'), phase_ref(x1r, cr, tv[:1], NG, bits), dt, 'phase gathered')


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('in_place', [False, True], ids=['out_of_place', 'in_place'])
@pytest.mark.parametrize('name', sorted(CONTROLS))
def test_controls_leave_the_other_amplitudes_bitwise_unchanged(name, in_place, dt):
    bits, controls = CONTROLS[name]
    x0, xr = gaussian(NG, 2, dt)
    off = torch.from_numpy(~on_mask(NG, controls)).cuda()
    d, dr = phase_table(2, dt, 5)
    c, cr = real_table(2, dt, 6, scale=3.0)
    tv = [0.7, -1.9]
    t = torch.tensor(tv, dtype=torch.float64, device='cuda')
    for what, run, ref in (
            ('apply_diag ctrl', lambda src, dst: backend.apply_diag(src, d, bits, controls, out=dst), diag_ref(xr, dr, NG, bits, controls)),
            ('phase ctrl', lambda src, dst: backend.apply_cost(src, c, t, bits, controls, 'phase', out=dst),
             phase_ref(xr, cr, tv, NG, bits, controls))):
        src = x0.clone()
        out = run(src, src if in_place else None)
        assert (out.data_ptr() == src.data_ptr()) == in_place
        parity(out, ref, dt, what)
        assert bitwise_equal(out[:, off], x0[:, off]), 'an amplitude outside the controls changed'
        if not in_place:
            assert bitwise_equal(src, x0)
    # SCALE is the cotangent of the sum that leaves them out: exactly zero there
    s = torch.tensor([0.4 - 1.3j, 2.0j], dtype=torch.complex128, device='cuda')
    src = x0.clone()
    out = backend.apply_cost(src, c, s, bits, controls, 'scale', out=src if in_place else None)
    ref = np.where(on_mask(NG, controls), np.array([0.4 - 1.3j, 2.0j])[:, None] * cr[sub_index(NG, bits)] * xr, 0)
    parity(out, ref, dt, 'scale ctrl')
    assert not out[:, off].any()


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('same', [True, False], ids=['expect', 'cross'])
@pytest.mark.parametrize('case', ['n1', 'n3', 'n10', 'n11', 'n12', 'big', 'gather', 'crossing', 'ctrl', 'ctrl_low', 'batch3'])
def test_cost_cross_gaussian(case, same, dt):
    n = {'n1': 1, 'n3': 3, 'n10': 10, 'n11': 11, 'n12': 12, 'big': BIG[dt]}.get(case, NG)
    bits = {'gather': (5, NG - 1, 0), 'crossing': CROSSING, 'ctrl': (6, 5), 'ctrl_low': (3, 2)}.get(case, full(n))
    controls = {'ctrl': (1, NG - 1), 'ctrl_low': (0, 4)}.get(case, ())
    batch = 3 if case == 'batch3' else 1
    ket, kr = gaussian(n, batch, dt)
    bra, br = (ket, kr) if same else gaussian(n, batch, dt, seed=5)
    c, cr = real_table(len(bits), dt, 8, scale=2.0)
    out = backend.cost_cross(bra, ket, c, bits, controls).cpu().numpy()
    w = np.where(on_mask(n, controls), cr[sub_index(n, bits)], 0.0)
    terms = w * br.conj() * kr
    ref = terms.sum(-1)
    bound = (2.0**-53 * 2.0**n + U_T[dt]) * np.abs(terms).sum(-1)
    err = np.abs(out - ref)
    print(f'cost_cross {case} {dt}: worst err / bound = {(err / bound).max():.3e}')
    assert (err <= bound).all(), f'{err} against {bound}'
    if same:
        assert (out.imag == 0).all()
    if n >= 3:            # the bound has teeth: the sum without its largest term lies outside it
        assert (np.abs(terms).max(-1) > bound).all()


def test_large_angles_are_reduced_in_double():
    """|t * cost| up to 1e4 rad at n = 10, complex64: still 1e-4 -- which an angle formed in float32 misses."""
    n, dt = 10, 'c64'
    x, xr = gaussian(n, 1, dt)
    rng = np.random.default_rng(3)
    cr = rng.uniform(-100.0, 100.0, 1 << n).astype(np.float32).astype(np.float64)
    cr[:2] = (100.0, -100.0)
    c = torch.from_numpy(cr).float().cuda()
    tv = 99.99999
    t = torch.tensor([tv], dtype=torch.float64, device='cuda')
    ref = phase_ref(xr, cr, [tv], n, full(n))
    assert np.abs(tv * cr).max() > 9.99e3
    parity(backend.apply_cost(x, c, t, full(n), (), 'phase'), ref, dt, 'phase large angle')
    parity(backend.apply_cost(x, c[:16].contiguous(), t, (3, 9, 0, 5), (), 'phase'), phase_ref(xr, cr[:16], [tv], n, (3, 9, 0, 5)), dt,
           'phase large angle')
    angle32 = (np.float32(tv) * cr.astype(np.float32)).astype(np.float64)      # what a float angle would be
    bad = np.exp(-1j * angle32) * xr
    assert np.abs(bad - ref).max() > TOL[dt] * np.abs(ref).max(), 'the row would not catch an angle formed in float'


def test_backend_argument_checks():
    x, _ = gaussian(4, 1, 'c64')
    d = torch.ones(2, dtype=torch.complex64, device='cuda')
    for bits, controls in (((1, 1), ()), ((4,), ()), ((2,), (2,)), ((), ())):
        with pytest.raises(ValueError):
            backend.apply_diag(x, torch.ones(1 << len(bits), dtype=torch.complex64, device='cuda'), bits, controls)
    # a misaligned state reaches the library, which refuses it before any launch (DQ_ERR_ARG)
    pad = torch.zeros(2, 17, dtype=torch.complex64, device='cuda')
    odd = pad.reshape(-1)[1:17].reshape(1, 16)
    assert odd.data_ptr() % 16 == 8 and odd.is_contiguous()
    with pytest.raises(RuntimeError, match='status -1'):
        backend.apply_diag(odd, d, (0,))
    with pytest.raises(RuntimeError, match='status -1'):
        backend.cost_cross(odd, odd, torch.ones(2, device='cuda'), (0,))
    # a misaligned table is copied, not refused
    tab = torch.ones(5, dtype=torch.complex64, device='cuda')[1:3]
    assert tab.data_ptr() % 16 == 8
    assert torch.equal(backend.apply_diag(x, tab, (0,)), x)


def test_library_error_returns():
    """DQ_ERR_ARG (-1) from the C entry points for real device buffers: nothing is launched."""
    from deepquantum_amd import _lib

    lib, ia = _lib.load(), _lib.int_array
    x = torch.zeros(1, 32, dtype=torch.complex64, device='cuda')
    d = torch.ones(4, dtype=torch.complex64, device='cuda')
    c = torch.ones(4, dtype=torch.float32, device='cuda')
    t = torch.zeros(2, dtype=torch.float64, device='cuda')
    ws = torch.zeros(64, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    xp, dp, cp, tp, wp = (v.data_ptr() for v in (x, d, c, t, ws))
    n = 4
    for bits, controls in (((1, 1), ()), ((4, 0), ()), ((2, 1), (2,)), ((), ())):
        k, nc = len(bits), len(controls)
        assert lib.dq_apply_diag_c64(xp, xp, dp, 0, n, ia(bits), k, ia(controls), nc, 1, None) == -1
        assert lib.dq_apply_cost_c64(xp, xp, cp, tp, _lib.COST_PHASE, n, ia(bits), k, ia(controls), nc, 1, None) == -1
        assert lib.dq_cost_cross_c64(xp, xp, cp, n, ia(bits), k, ia(controls), nc, 1, tp, wp, 512, None) == -1
        assert lib.dq_last_error()
    for bad in (8, 4):
        assert lib.dq_apply_diag_c64(xp + bad, xp, dp, 0, n, ia((1, 0)), 2, ia(()), 0, 1, None) == -1
        assert lib.dq_apply_diag_c64(xp, xp + bad, dp, 0, n, ia((1, 0)), 2, ia(()), 0, 1, None) == -1
        assert lib.dq_apply_cost_c64(xp, xp, cp + bad, tp, _lib.COST_SCALE, n, ia((1, 0)), 2, ia(()), 0, 1, None) == -1
        assert lib.dq_cost_cross_c64(xp, xp + bad, cp, n, ia((1, 0)), 2, ia(()), 0, 1, tp, wp, 512, None) == -1
    torch.cuda.synchronize()
    assert not x.any()


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_gathered_second_iteration(dt):
    """The gathered instantiations where a workgroup takes a second chunk (more than 2048 chunks per sample)."""
    n = BIG[dt]
    bits = (5, n - 1, 0, n - 2)
    x, xr = gaussian(n, 1, dt)
    c, cr = real_table(4, dt, 9, scale=3.0)
    t = torch.tensor([0.83], dtype=torch.float64, device='cuda')
    parity(backend.apply_cost(x, c, t, bits, (n - 3,), 'phase'), phase_ref(xr, cr, [0.83], n, bits, (n - 3,)), dt, 'phase big gathered')
    d, dr = phase_table(4, dt, 10)
    parity(backend.apply_diag(x, d, bits), diag_ref(xr, dr, n, bits), dt, 'apply_diag big gathered')
    out = backend.cost_cross(x, x, c, bits, (n - 3,)).cpu().numpy()
    terms = np.where(on_mask(n, (n - 3,)), cr[sub_index(n, bits)], 0.0) * np.abs(xr) ** 2
    bound = (2.0**-53 * 2.0**n + U_T[dt]) * np.abs(terms).sum(-1)
    assert (np.abs(out - terms.sum(-1)) <= bound).all() and (np.abs(terms).max(-1) > bound).all()


SWITCH_CASES = {
    # name: (dt, n, k, controls, table route?, thresholds patched to (max bits, min rest, min qubits) or None)
    'real_boundary_above': ('c128', 24, 3, (), True, None),
    'real_boundary_below': ('c128', 23, 3, (), False, None),
    'min_qubits_above': ('c128', 12, 3, (), True, (5, 8, 12)),
    'min_qubits_below': ('c128', 11, 3, (), False, (5, 8, 12)),
    'rest_above': ('c128', 12, 4, (), True, (5, 8, 12)),
    'rest_below': ('c128', 12, 5, (), False, (5, 8, 12)),
    'max_bits_below': ('c128', 14, 5, (), True, (5, 8, 12)),
    'max_bits_above': ('c128', 14, 6, (), False, (5, 8, 12)),
    'controls': ('c128', 14, 2, (1, 13), True, (5, 8, 12)),
    'complex64': ('c64', 14, 3, (), False, (5, 8, 12)),
}


@pytest.mark.parametrize('name', sorted(SWITCH_CASES))
def test_phase_switch(name, monkeypatch):
    """Both sides of each condition of the table / in-flight switch, with the route OBSERVED: the table route is the only
    caller of ``dq_apply_diag_*`` inside ``apply_cost``.  Both routes meet the same criterion.  The thresholds themselves
    are measured values: the two `real_boundary` cases run on them as they are, the others scale
    them down so that every condition has a case on each side at a small n."""
    from deepquantum_amd import _lib

    assert (backend.PHASE_TABLE_MAX_BITS, backend.PHASE_TABLE_MIN_REST, backend.PHASE_TABLE_MIN_QUBITS) == (16, 8, 24)
    dt, n, k, controls, via_table, patched = SWITCH_CASES[name]
    if patched:
        for attr, value in zip(('PHASE_TABLE_MAX_BITS', 'PHASE_TABLE_MIN_REST', 'PHASE_TABLE_MIN_QUBITS'), patched):
            monkeypatch.setattr(backend, attr, value)
    lib = _lib.load()
    calls = []
    for fn in ('dq_apply_diag_c128', 'dq_apply_diag_c64'):
        real = getattr(lib, fn)
        monkeypatch.setattr(lib, fn, lambda *a, _real=real, _fn=fn: (calls.append(_fn), _real(*a))[1])
    batch = 2 if n <= 14 else 1
    tv = [0.83, -2.1][:batch]
    t = torch.tensor(tv, dtype=torch.float64, device='cuda')
    free = [p for p in range(n) if p not in controls]
    bits = tuple(dict.fromkeys(free[::-1][i * (len(free) - 1) // (k - 1)] for i in range(k)))     # spread from the top bit to bit 0
    assert len(bits) == k
    x, xr = gaussian(n, batch, dt)
    c, cr = real_table(k, dt, 40 + k, scale=3.0)
    out = backend.apply_cost(x, c, t, bits, controls, 'phase')
    assert calls == (['dq_apply_diag_c128'] if via_table else []), calls
    parity(out, phase_ref(xr, cr, tv, n, bits, controls), dt, f'phase switch {name}')
