"""The Pauli-sum kernels on the MI355X (dq_apply_psum_axpby_*, dq_psum_cross_*) through ``backend``, against numpy complex128
from the sum of h_t * pauli_apply(x, x_t, z_t) (tests/_psum_ref.py).

Geometry of csrc/dq_psum.hip, which decides the cases: a lane owns OUTPUT vectors of 16 bytes (two complex64 amplitudes or
one complex128), four per iteration, 1024 per workgroup and iteration, at most 2048 workgroups per sample; for every group
it loads the partner vector v ^ (x >> VB).  So for complex64 amplitude bit 0 is inside the vector (a swap of elements),
bit 1 is the lowest vector bit, bits 6 / 7 sit across the wave, bit 10 is the top bit inside a unit and bit 11 the first
above it -- where the z masks are split into a per-lane and a per-unit part as well; complex128 is one lower, and XBITS
lists both sets.  A second grid-stride iteration starts at 2^21 vectors: n = 23 (complex64) / 22 (complex128).  The kernel
stages nothing in chunks of its own: the group and term loops read the table entry by entry, so 1, 2 and 17 terms per
group and 1, 2 and 40 groups are all the counts there are to tell apart.

Exact rows: Gaussian integers in [-4, 4], coefficients from {+-1, +-2, +-1/2, 3}, a and c from COEFS; with
8 * sum |h_t| < 2^22 every partial sum is a multiple of 1/4 below 2^24, exact in float32 in any order, so the result equals
the reference as numbers.  Gaussian rows: 1e-4 / 1e-10 of max |ref|; the cross reduction against
(2^-53 2^n + (Tmax + 2) u_T) sum_i |bra_i| (|H| |ket|)_i, with the check that the sum without its largest term lies outside
that bound."""

import functools

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import backend
from _psum_ref import abs_terms, hamiltonian_of, psum_apply_ref, psum_axpby_ref, psum_cross_ref
from test_pauli_gpu import COEFS, SIZES, TOL, U_T, XBITS, bitwise_equal, coefs, gaussian, host, integer_state, xmasks, zmasks

pytestmark = pytest.mark.gpu

HS = (1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 3.0)
COUNTS = (1, 2, 17)


def group_terms(n, xmask, count, rng, exact=True):
    """``count`` terms (as many as there are z masks, if fewer) with the flip ``xmask``: the z parts of
    ``test_pauli_gpu.zmasks`` -- and the constant term for xmask = 0 -- first, seeded ones after them."""
    zs = ([0] if xmask == 0 else []) + list(zmasks(n, xmask))
    for z in rng.permutation(1 << n):
        if len(zs) >= count:
            break
        if int(z) not in zs:
            zs.append(int(z))
    return [(float(rng.choice(HS)) if exact else float(rng.standard_normal()), xmask, z) for z in zs[:count]]


@functools.lru_cache(maxsize=None)
def hamiltonians(n, exact=True):
    """name -> terms: one Hamiltonian per class of flip and number of terms, one with every class, and 1, 2 and 40 groups
    (all 2^n flips where there are fewer)."""
    rng = np.random.default_rng(1000 + n)
    out = {}
    for xmask in xmasks(n):
        for count in COUNTS:
            out[f'x={xmask:#x} T={count}'] = group_terms(n, xmask, count, rng, exact)
    out['all classes'] = [t for xmask in xmasks(n) for t in group_terms(n, xmask, 17, rng, exact)]
    flips = list(xmasks(n))
    for x in rng.permutation(1 << n):
        if len(flips) >= 40:
            break
        if int(x) not in flips:
            flips.append(int(x))
    for groups in (2, 40):
        out[f'G={min(groups, len(flips))}'] = [t for i, xmask in enumerate(flips[:groups])
                                               for t in group_terms(n, xmask, 1 + i % 2, rng, exact)]
    return out


@functools.lru_cache(maxsize=None)
def built(n, name, exact=True):
    """The PauliSum of a Hamiltonian through the public list form, with what the host made of it checked once."""
    terms = hamiltonians(n, exact)[name]
    H = dq.PauliSum(hamiltonian_of(n, terms), n)
    assert sorted(H.terms) == sorted(terms) and H.ngroups == len({x for _, x, _ in terms})
    assert 8 * sum(abs(h) for h, _, _ in terms) < 2**22
    return H, terms


# ---- exact rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('n', SIZES)
def test_axpby_and_cross_exact(n, dt):
    x, xr = integer_state(n, 1, dt)
    y, yr = integer_state(n, 1, dt, seed=5)
    seen_ny, seen_groups, seen_counts = set(), set(), set()
    for k, name in enumerate(hamiltonians(n)):
        H, terms = built(n, name)
        seen_ny |= {bin(xm & zm).count('1') % 4 for _, xm, zm in terms}
        seen_groups.add(H.ngroups)
        seen_counts |= {sum(1 for t in terms if t[1] == xm) for xm in {t[1] for t in terms}}
        a, c, ar, cr = coefs(1, 1000 * n + k)
        out = backend.apply_psum_axpby(x, H.table, a, c)
        assert np.array_equal(host(out), psum_axpby_ref(xr, terms, ar, cr)), (n, dt, name)
        got = backend.psum_cross(x, x, H.table)
        assert got.dtype == torch.complex128 and got.shape == (1,)
        assert np.array_equal(got.cpu().numpy(), psum_cross_ref(xr, xr, terms)), (n, dt, name, 'expect')
        assert np.array_equal(backend.psum_cross(y, x, H.table).cpu().numpy(), psum_cross_ref(yr, xr, terms)), (n, dt, name, 'cross')
    if n >= 9:
        assert seen_ny == {0, 1, 2, 3}
        assert {1, 2, 40} <= seen_groups and {1, 2, 17} <= seen_counts
    assert np.array_equal(host(x), xr) and np.array_equal(host(y), yr)         # the shared inputs are untouched


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_batch_of_three_with_per_sample_coefficients(dt):
    n = 12
    x, xr = integer_state(n, 3, dt, seed=1)
    y, yr = integer_state(n, 3, dt, seed=6)
    for name in ('all classes', 'G=40', 'x=0x800 T=17'):
        H, terms = built(n, name)
        a, c, ar, cr = coefs(3, 17 + len(terms))
        assert len({(p, q) for p, q in zip(ar, cr)}) > 1                    # the samples' coefficients differ
        assert np.array_equal(host(backend.apply_psum_axpby(x, H.table, a, c)), psum_axpby_ref(xr, terms, ar, cr))
        assert np.array_equal(backend.psum_cross(y, x, H.table).cpu().numpy(), psum_cross_ref(yr, xr, terms))
        buf = torch.full_like(x, 7.0)
        assert backend.apply_psum_axpby(x, H.table, a, c, out=buf) is buf
        assert np.array_equal(host(buf), psum_axpby_ref(xr, terms, ar, cr))
    assert np.array_equal(host(x), xr)


# ---- Gaussian rows -------------------------------------------------------------------------------------------------------
def parity(out, ref, dt, what):
    err = np.abs(host(out) - ref).max()
    ratio = err / (TOL[dt] * np.abs(ref).max())
    print(f'{what} {dt}: err / (tol * max|ref|) = {ratio:.3e}')
    assert ratio <= 1.0, f'{what}: {err:.3e} against {TOL[dt]} * {np.abs(ref).max():.3e}'


def cross_within_bound(got, br, kr, terms, n, dt, what):
    """The reduction against (2^-53 2^n + (Tmax + 2) u_T) sum_i |bra_i| (|H| |ket|)_i -- and the bound has teeth: the sum
    without its largest term lies outside it."""
    parts = br.conj() * psum_apply_ref(kr, terms)
    tmax = max(sum(1 for t in terms if t[1] == xm) for xm in {t[1] for t in terms})
    bound = (2.0**-53 * 2.0**n + (tmax + 2) * U_T[dt]) * (np.abs(br) * psum_apply_ref(np.abs(kr), abs_terms(terms)).real).sum(-1)
    err = np.abs(got - parts.sum(-1))
    print(f'psum_cross {what} {dt}: worst err / bound = {(err / bound).max():.3e}')
    assert (err <= bound).all(), f'{what}: {err} against {bound}'
    assert (np.abs(parts).max(-1) > bound).all()


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('n', SIZES)
def test_axpby_and_cross_gaussian(n, dt):
    x, xr = gaussian(n, 2, dt)
    y, yr = gaussian(n, 2, dt, seed=5)
    a = torch.tensor([0.3 - 1.2j, -0.8 + 0.1j], dtype=torch.complex128, device='cuda')
    c = torch.tensor([1.1 + 0.4j, 0.25j], dtype=torch.complex128, device='cuda')
    names = ['all classes', f'G={min(40, 1 << n)}', f'x={(1 << n) - 1:#x} T=17', 'x=0x0 T=17']
    for name in names:
        H, terms = built(n, name, exact=False)
        parity(backend.apply_psum_axpby(x, H.table, a, c), psum_axpby_ref(xr, terms, host(a), host(c)), dt, f'axpby n={n} {name}')
        cross_within_bound(backend.psum_cross(x, x, H.table).cpu().numpy(), xr, xr, terms, n, dt, f'n={n} {name} expect')
        cross_within_bound(backend.psum_cross(y, x, H.table).cpu().numpy(), yr, xr, terms, n, dt, f'n={n} {name} cross')
    assert np.array_equal(host(x), xr)


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_second_grid_stride_iteration(dt):
    """More than 2048 units of 1024 vectors per sample, three groups -- no flip, the bit inside (complex64) or lowest over
    (complex128) the vectors, the top bit -- of at most four terms; the top z bit meets the unit's index."""
    n = {'c64': 23, 'c128': 22}[dt]
    top = 1 << (n - 1)
    terms = [(0.75, 0, 0), (-1.5, 0, top | 1 << 10 | 1), (0.6, 1, 1 << 12), (1.25, 1, 1 | top), (-0.8, top, top | 1 << 11),
             (0.4, top, 1 << 3)]
    H = dq.PauliSum(hamiltonian_of(n, terms), n)
    assert (H.ngroups, H.nterms) == (3, 6)
    x, xr = gaussian.__wrapped__(n, 1, dt)                         # (not kept: 2^23 amplitudes)
    a = torch.tensor([0.6 - 0.3j], dtype=torch.complex128, device='cuda')
    c = torch.tensor([-0.2 + 0.9j], dtype=torch.complex128, device='cuda')
    hx = psum_apply_ref(xr, terms)
    parity(backend.apply_psum_axpby(x, H.table, a, c), host(a) * xr + host(c) * hx, dt, f'axpby n={n}')
    got = backend.psum_cross(x, x, H.table).cpu().numpy()
    parts = xr.conj() * hx
    bound = (2.0**-53 * 2.0**n + 4 * U_T[dt]) * (np.abs(xr) * psum_apply_ref(np.abs(xr), abs_terms(terms)).real).sum(-1)
    assert (np.abs(got - parts.sum(-1)) <= bound).all() and (np.abs(parts).max(-1) > bound).all()


# ---- reproducibility, the bra slot, and the per-string routes -------------------------------------------------------------
@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('n', [3, 12, 14])
def test_cross_is_reproducible_and_the_bra_slot_changes_no_bit(n, dt):
    x, _ = gaussian(n, 2, dt)
    for name in ('all classes', f'G={min(40, 1 << n)}', 'x=0x1 T=2'):
        H, _ = built(n, name, exact=False)
        first = backend.psum_cross(x, x, H.table)
        for other in (backend.psum_cross(x, x, H.table), backend.psum_cross(x.clone(), x, H.table)):
            assert torch.equal(torch.view_as_real(other).view(torch.int64), torch.view_as_real(first).view(torch.int64)), (n, dt, name)


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_the_per_string_loops_agree_with_the_same_reference(dt):
    """<H> as sum_t h_t pauli_cross(...) and H|psi> as the loop of apply_pauli_axpby -- what the package offered before --
    against the reference that the one-launch results are held to, not against each other."""
    n = 13
    H, terms = built(n, 'all classes', exact=False)
    x, xr = gaussian(n, 2, dt)
    ref = psum_apply_ref(xr, terms)
    loop = torch.zeros_like(x)
    energy = torch.zeros(2, dtype=torch.complex128, device='cuda')
    one, zero = torch.ones(2, dtype=torch.complex128, device='cuda'), torch.zeros(2, dtype=torch.complex128, device='cuda')
    for h, xm, zm in terms:
        loop += backend.apply_pauli_axpby(x, xm, zm, zero, h * one, (), 'map')     # (a Python float would pass through float32)
        energy += h * backend.pauli_cross(x, x, xm, zm)
    # (the loop rounds once per string: |H| |x| is what its error scales with)
    scale = np.abs(psum_apply_ref(np.abs(xr), abs_terms(terms))).max()
    assert np.abs(host(loop) - ref).max() <= TOL[dt] * scale
    parity(backend.apply_psum_axpby(x, H.table, zero, one), ref, dt, 'H|psi> in one launch')
    want = (xr.conj() * ref).sum(-1)
    size = (np.abs(xr) * psum_apply_ref(np.abs(xr), abs_terms(terms)).real).sum(-1)
    assert (np.abs(energy.cpu().numpy() - want) <= TOL[dt] * size).all()
    assert (np.abs(backend.psum_cross(x, x, H.table).cpu().numpy() - want) <= TOL[dt] * size).all()
    assert (np.abs(want.imag) <= TOL[dt] * size).all()                      # H is Hermitian


# ---- argument checks ------------------------------------------------------------------------------------------------------
def test_library_error_returns():
    """DQ_ERR_ARG (-1) from the C entry points for real device buffers: nothing is launched."""
    from deepquantum_amd import _lib

    lib = _lib.load()
    H, _ = built(5, 'all classes')
    x = torch.zeros(1, 32, dtype=torch.complex64, device='cuda')
    z = torch.zeros(1, 32, dtype=torch.complex64, device='cuda')
    coef = torch.ones(4, dtype=torch.float64, device='cuda')
    out = torch.zeros(2, dtype=torch.float64, device='cuda')
    ws = torch.zeros(64, dtype=torch.float64, device='cuda')
    tb = [t.data_ptr() for t in H.device_table('cuda')]
    torch.cuda.synchronize()
    xp, zp, cp, op, wp = (v.data_ptr() for v in (x, z, coef, out, ws))
    g, t, n = H.ngroups, H.nterms, 5
    assert lib.dq_apply_psum_axpby_c64(xp, xp, cp, *tb, g, t, n, 1, None) == -1                      # out of place only
    assert b'overlap' in lib.dq_last_error()
    assert lib.dq_apply_psum_axpby_c64(xp, zp + 8, cp, *tb, g, t, n, 1, None) == -1
    assert lib.dq_apply_psum_axpby_c64(xp, zp, cp, *tb, 0, t, n, 1, None) == -1
    assert lib.dq_apply_psum_axpby_c64(xp, zp, cp, *tb, g, t, 41, 1, None) == -1
    assert lib.dq_apply_psum_axpby_c64(xp, zp, cp, tb[0], None, tb[2], tb[3], g, t, n, 1, None) == -1
    assert lib.dq_psum_cross_c64(xp, xp, *tb, g, t, n, 1, op, wp, 8, None) == -1                       # workspace too small
    assert lib.dq_psum_cross_c64(xp, xp, *tb, g, t, n, 1, None, wp, 512, None) == -1
    assert lib.dq_psum_cross_c64(xp, xp + 8, *tb, g, t, n, 1, op, wp, 512, None) == -1
    torch.cuda.synchronize()
    assert not x.any() and not z.any() and not out.any()
    with pytest.raises(ValueError, match='out of place'):
        backend.apply_psum_axpby(x, H.table, 1.0, 1.0, out=x)
