"""The Pauli-string kernels on the MI355X (dq_apply_pauli_axpby_*, dq_pauli_cross_*) through ``backend``, against numpy
complex128 from the formula (P psi)[i] = i^ny (-1)^popc((i ^ x) & z) psi[i ^ x] (tests/_pauli_ref.py).

Geometry of csrc/dq_pauli.hip, which decides the cases: a lane moves 16-byte vectors (two complex64 amplitudes or one
complex128); with vx = xmask >> VB != 0 a lane owns PAIRS of vectors, pair P -> (vA = P with a zero inserted at the top
bit of vx, vB = vA ^ vx), 4 pairs per lane, 1024 pairs per workgroup and iteration, at most 2048 workgroups per sample;
with vx == 0 (xmask = 0, or complex64 xmask = 1: a register swap) a lane owns 4 vectors.  So for complex64 amplitude
bit 0 is inside the vector, bit 1 is the lowest pair bit, bits 6 / 7 sit across the wave (vector bits 5 / 6), bit 10 is
the top bit inside a unit of 1024 vectors and bit 11 the first above it; complex128 is one lower, and XBITS lists both
sets.  A second grid-stride iteration starts at 2048 * 1024 pairs: n = 24 (complex64) / 23 (complex128) for any
vx != 0, one n lower for vx == 0.

Exact rows: small Gaussian integers and coefficients from {0, +-1, +-i, 1 +- i, 2, -3i} -- every product and sum is
exact in float32, so the result equals the reference as numbers.  Gaussian rows: 1e-4 / 1e-10 of max |ref|; the cross
reduction against (2^-53 2^n + u_T) sum_i |bra_i| |ket_i|, with the check that the sum without its largest term lies
outside that bound."""

import functools

import numpy as np
import pytest
import torch

from deepquantum_amd import backend, ops
from _pauli_ref import axpby_ref, cross_ref, inside, pauli_apply, rot_ref

pytestmark = pytest.mark.gpu

DTYPES = {'c64': torch.complex64, 'c128': torch.complex128}
TOL = {'c64': 1e-4, 'c128': 1e-10}
U_T = {'c64': 2.0**-24, 'c128': 2.0**-53}
SIZES = (1, 2, 3, 9, 10, 11, 12, 13, 14)
XBITS = (0, 1, 5, 6, 7, 9, 10, 11)              # single flipped bits (those below n are used), plus n - 1
COEFS = np.array([0, 1, -1, 1j, -1j, 1 + 1j, 1 - 1j, 2, -3j], dtype=np.complex128)


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


def host(t):
    return t.cpu().numpy().astype(np.complex128)


def bitwise_equal(a, b):
    return torch.equal(torch.view_as_real(a).view(torch.int32 if a.dtype == torch.complex64 else torch.int64),
                       torch.view_as_real(b).view(torch.int32 if b.dtype == torch.complex64 else torch.int64))


def xmasks(n):
    """Every class of flip the kernels tell apart, at this n."""
    out = [0] + [1 << b for b in XBITS if b < n]
    if n > 1:
        out += [1 << (n - 1), (1 << n) - 1]
    if n > 6:
        out.append(1 | 1 << 5 | 1 << (n - 1))
    return sorted(set(out))


def zmasks(n, xmask):
    """z parts for a flip: none; disjoint from x; a lone Y; two and three Ys (all four powers of i) with a Z beside them."""
    full = (1 << n) - 1
    if xmask == 0:
        return sorted({1, 1 << min(5, n - 1), 1 << (n - 1), (1 | 1 << min(5, n - 1) | 1 << (n - 1))})
    xbits = [b for b in range(n) if (xmask >> b) & 1]
    free = [b for b in range(n) if not (xmask >> b) & 1]
    disjoint = sum(1 << b for b in set(free[:1] + free[-1:]))
    out = [0, 1 << xbits[0], 1 << xbits[-1] | disjoint]
    if disjoint:
        out.append(disjoint)
    if len(xbits) >= 2:
        out.append(1 << xbits[0] | 1 << xbits[-1] | disjoint)
    if len(xbits) >= 3:
        out += [1 << xbits[0] | 1 << xbits[1] | 1 << xbits[-1] | disjoint, full]
    return sorted(set(out))


def coefs(batch, seed):
    rng = np.random.default_rng(seed)
    a, c = COEFS[rng.integers(0, len(COEFS), batch)], COEFS[rng.integers(1, len(COEFS), batch)]
    return torch.from_numpy(a).cuda(), torch.from_numpy(c).cuda(), a, c


# ---- exact rows, out of place and in place ----------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('n', SIZES)
def test_axpby_exact_and_aliased(n, dt):
    x, xr = integer_state(n, 1, dt)
    seen_ny = set()
    for xmask in xmasks(n):
        for zmask in zmasks(n, xmask):
            seen_ny.add(bin(xmask & zmask).count('1') % 4)
            a, c, ar, cr = coefs(1, 1000 * n + 7 * xmask + zmask)
            for mode in ('gate', 'map'):
                out = backend.apply_pauli_axpby(x, xmask, zmask, a, c, (), mode)
                assert np.array_equal(host(out), axpby_ref(xr, xmask, zmask, ar, cr, (), mode)), (n, dt, hex(xmask), hex(zmask), mode)
                buf = x.clone()
                assert backend.apply_pauli_axpby(buf, xmask, zmask, a, c, (), mode, out=buf) is buf
                assert bitwise_equal(buf, out), (n, dt, hex(xmask), hex(zmask), mode, 'in place')
    if n >= 9:
        assert seen_ny == {0, 1, 2, 3}
    assert np.array_equal(host(x), xr)                                     # the shared input is untouched


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('n', [3, 12, 13])
def test_axpby_controls(n, dt):
    """A low control (inside the vector for complex64), a high one, both: outside amplitudes bitwise unchanged (GATE) or
    exactly 0 (MAP), in place and out of place."""
    x, xr = integer_state(n, 1, dt, seed=3)
    mid = [1 << 1] + ([1 << 6 | 1 << 2, 1 << (n - 2) | 1 << 1] if n > 8 else [])
    for controls in ((0,), (n - 1,), (0, n - 1)):
        on = inside(n, controls)
        for xmask in [0] + mid:
            for zmask in ({0, xmask, 1 << 1} - ({0} if xmask == 0 else set())):
                a, c, ar, cr = coefs(1, 50 * n + xmask + zmask + len(controls))
                for mode in ('gate', 'map'):
                    ref = axpby_ref(xr, xmask, zmask, ar, cr, controls, mode)
                    out = backend.apply_pauli_axpby(x, xmask, zmask, a, c, controls, mode)
                    assert np.array_equal(host(out), ref), (n, dt, controls, hex(xmask), hex(zmask), mode)
                    if mode == 'gate':
                        assert bitwise_equal(out[:, ~torch.from_numpy(on).cuda()], x[:, ~torch.from_numpy(on).cuda()])
                    else:
                        assert not out[:, ~torch.from_numpy(on).cuda()].any()
                    buf = x.clone()
                    backend.apply_pauli_axpby(buf, xmask, zmask, a, c, controls, mode, out=buf)
                    assert bitwise_equal(buf, out)


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_axpby_batch_of_three(dt):
    n = 12
    x, xr = integer_state(n, 3, dt, seed=1)
    for xmask, zmask, controls in ((0, 0b100001, ()), (1, 1, ()), (1 << 11 | 1 << 3, 1 << 3 | 1 << 7, (5,)), ((1 << n) - 1, 0b111, ())):
        a, c, ar, cr = coefs(3, 17 + xmask)
        assert len({(p, q) for p, q in zip(ar, cr)}) > 1                    # the samples' coefficients differ
        for mode in ('gate', 'map'):
            out = backend.apply_pauli_axpby(x, xmask, zmask, a, c, controls, mode)
            assert np.array_equal(host(out), axpby_ref(xr, xmask, zmask, ar, cr, controls, mode))


# ---- Gaussian rows ----------------------------------------------------------------------------------------------------
def parity(out, ref, dt, what):
    err = np.abs(host(out) - ref).max()
    ratio = err / (TOL[dt] * np.abs(ref).max())
    print(f'{what} {dt}: err / (tol * max|ref|) = {ratio:.3e}')
    assert ratio <= 1.0, f'{what}: {err:.3e} against {TOL[dt]} * {np.abs(ref).max():.3e}'


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('n', SIZES)
def test_axpby_and_rotation_gaussian(n, dt):
    x, xr = gaussian(n, 2, dt)
    a = torch.tensor([0.3 - 1.2j, -0.8 + 0.1j], dtype=torch.complex128, device='cuda')
    c = torch.tensor([1.1 + 0.4j, 0.25j], dtype=torch.complex128, device='cuda')
    theta = torch.tensor([0.83, -2.4], dtype=torch.float64, device='cuda')
    norm = np.linalg.norm(xr, axis=-1)
    for xmask in xmasks(n):
        zmask = zmasks(n, xmask)[-1]
        controls = () if n < 3 or (xmask | zmask) & 0b10 else (1,)
        parity(backend.apply_pauli_axpby(x, xmask, zmask, a, c, controls), axpby_ref(xr, xmask, zmask, host(a), host(c), controls), dt,
               f'axpby n={n} x={xmask:#x}')
        with torch.no_grad():
            y = ops.pauli_rot(x, xmask, zmask, theta, controls)
        parity(y, rot_ref(xr, xmask, zmask, theta.cpu().numpy(), controls), dt, f'rot n={n} x={xmask:#x}')
        got = np.linalg.norm(host(y), axis=-1)
        assert (np.abs(got - norm) <= TOL[dt] * norm).all(), 'the rotation is unitary'


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_second_grid_stride_iteration(dt):
    """More than 2048 units of 1024 pairs per sample: once with a high flipped bit, once with a low one -- and one n lower
    for the kernel without a partner vector (xmask = 0)."""
    n = {'c64': 24, 'c128': 23}[dt]
    a = torch.tensor([0.6 - 0.3j], dtype=torch.complex128, device='cuda')
    c = torch.tensor([-0.2 + 0.9j], dtype=torch.complex128, device='cuda')
    for m, xmask, zmask, controls in ((n, 1 << (n - 1) | 1 << 4, 1 << (n - 1) | 1 << 9, (n - 3,)), (n, 1 << 3, 1 << (n - 2), ()),
                                      (n - 1, 0, 1 << (n - 2) | 1, ())):
        x, xr = gaussian.__wrapped__(m, 1, dt)                     # (not kept: 2^24 amplitudes)
        on, px = inside(m, controls), pauli_apply(xr, xmask, zmask)
        parity(backend.apply_pauli_axpby(x, xmask, zmask, a, c, controls), np.where(on, host(a) * xr + host(c) * px, xr), dt,
               f'axpby n={m} x={xmask:#x}')
        out = backend.pauli_cross(x, x, xmask, zmask, controls).cpu().numpy()
        terms = on * xr.conj() * px
        bound = (2.0**-53 * 2.0**m + U_T[dt]) * np.abs(terms).sum(-1)
        assert (np.abs(out - terms.sum(-1)) <= bound).all() and (np.abs(terms).max(-1) > bound).all()


# ---- pauli_cross ------------------------------------------------------------------------------------------------------
CROSS_CASES = {
    # name: (n, xmask, zmask, controls, batch)
    'n1_z': (1, 0, 1, (), 1), 'n1_y': (1, 1, 1, (), 1), 'n3_plain': (3, 0, 0, (), 1), 'n3_xy': (3, 0b101, 0b100, (), 1),
    'n10_bit0': (10, 1, 0, (), 1), 'n10_top': (10, 1 << 9, 1 << 9 | 1, (), 1), 'n11_z': (11, 0, 1 << 10 | 1 << 5, (), 1),
    'n11_bit10': (11, 1 << 10, 1 << 2, (), 1), 'n12_bit11': (12, 1 << 11, 1 << 11, (), 1), 'n12_all': (12, (1 << 12) - 1, 0b111, (), 1),
    'n14_mixed': (14, 1 | 1 << 5 | 1 << 13, 1 << 5 | 1 << 13 | 1 << 8, (), 1), 'ctrl_low': (12, 1 << 6 | 1 << 1, 1 << 6, (0,), 1),
    'ctrl_high': (12, 1 << 3, 1 << 5, (11,), 1), 'ctrl_both_z': (12, 0, 1 << 4, (0, 11), 1), 'batch3': (12, 1 << 11 | 1 << 2, 1 << 2 | 1, (4,), 3),
}


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('same', [True, False], ids=['expect', 'cross'])
@pytest.mark.parametrize('case', list(CROSS_CASES))
def test_pauli_cross_exact(case, same, dt):
    n, xmask, zmask, controls, batch = CROSS_CASES[case]
    ket, kr = integer_state(n, batch, dt)
    bra, br = (ket, kr) if same else integer_state(n, batch, dt, seed=5)
    out = backend.pauli_cross(bra, ket, xmask, zmask, controls)
    assert out.dtype == torch.complex128 and out.shape == (batch,)
    assert np.array_equal(out.cpu().numpy(), cross_ref(br, kr, xmask, zmask, controls))      # (integers: exact in double)
    assert torch.equal(torch.view_as_real(backend.pauli_cross(bra, ket, xmask, zmask, controls)).view(torch.int64),
                       torch.view_as_real(out).view(torch.int64))                              # reproducible bit for bit


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('same', [True, False], ids=['expect', 'cross'])
def test_pauli_cross_finish_second_stride_exact(same, dt):
    """512 partial sums per sample, batch 2: the finish kernel's lanes take a second stride of 256 partial sums and a
    second sample's row of the workspace (2^19 pairs of vectors: n = 21 complex64 / 20 complex128 with the top bit
    flipped).  Integer states in [-4, 4]: every term is an integer of magnitude <= 32 and every sum of the 2^21 at most
    stays below 2^26 < 2^53, so the reference is exact in any order."""
    n = {'c64': 21, 'c128': 20}[dt]
    xmask, zmask, controls = 1 << (n - 1) | 1 << 3, 1 << (n - 1) | 1 << 6, (2,)
    ket, kr = integer_state(n, 2, dt)
    bra, br = (ket, kr) if same else integer_state(n, 2, dt, seed=5)
    out = backend.pauli_cross(bra, ket, xmask, zmask, controls)
    assert out.dtype == torch.complex128 and out.shape == (2,)
    assert np.array_equal(out.cpu().numpy(), cross_ref(br, kr, xmask, zmask, controls))


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('same', [True, False], ids=['expect', 'cross'])
@pytest.mark.parametrize('case', list(CROSS_CASES))
def test_pauli_cross_gaussian(case, same, dt):
    n, xmask, zmask, controls, batch = CROSS_CASES[case]
    ket, kr = gaussian(n, batch, dt)
    bra, br = (ket, kr) if same else gaussian(n, batch, dt, seed=5)
    out = backend.pauli_cross(bra, ket, xmask, zmask, controls).cpu().numpy()
    terms = inside(n, controls) * br.conj() * pauli_apply(kr, xmask, zmask)
    ref = terms.sum(-1)
    bound = (2.0**-53 * 2.0**n + U_T[dt]) * np.abs(terms).sum(-1)
    err = np.abs(out - ref)
    print(f'pauli_cross {case} {dt}: worst err / bound = {(err / bound).max():.3e}')
    assert (err <= bound).all(), f'{err} against {bound}'
    assert (np.abs(terms).max(-1) > bound).all()       # the bound has teeth: the sum without its largest term lies outside it


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_plain_inner_product_and_expectation(dt):
    """xmask = zmask = 0 is ``backend.inner``; bra is ket gives ``backend.expect_pauli`` in its real part."""
    n = 12
    ket, kr = gaussian(n, 2, dt)
    bra, br = gaussian(n, 2, dt, seed=5)
    scale = np.abs(br.conj() * kr).sum(-1)
    got = backend.pauli_cross(bra, ket, 0, 0).cpu().numpy()
    assert (np.abs(got - backend.inner(bra, ket).cpu().numpy()) <= TOL[dt] * scale).all()
    for xmask, zmask in ((0, 0b1001), (1 << 11 | 1, 1), (0b110, 0b011)):
        got = backend.pauli_cross(ket, ket, xmask, zmask).cpu().numpy()
        ex = backend.expect_pauli(ket, xmask, zmask).cpu().numpy()
        assert (np.abs(got.real - ex) <= TOL[dt] * (np.abs(kr) ** 2).sum(-1)).all()
        assert (np.abs(got.imag) <= TOL[dt] * (np.abs(kr) ** 2).sum(-1)).all()


# ---- argument checks --------------------------------------------------------------------------------------------------
def test_backend_argument_checks():
    x, _ = gaussian(4, 1, 'c64')
    for kw in (dict(xmask=16), dict(zmask=16), dict(controls=(4,)), dict(controls=(1, 1)), dict(xmask=2, controls=(1,)), dict(mode='scale')):
        args = dict(xmask=1, zmask=0, a=1.0, c=1j, controls=(), mode='gate')
        args.update(kw)
        with pytest.raises(ValueError):
            backend.apply_pauli_axpby(x, **args)
    with pytest.raises(ValueError):
        backend.pauli_cross(x, x, 1, 0, (0,))
    with pytest.raises(ValueError):
        backend.pauli_cross(x, x.to(torch.complex128), 1, 0)
    with pytest.raises(ValueError):
        backend.apply_pauli_axpby(x, 1, 0, torch.ones(2), 1j)              # one coefficient, or one per sample
    # a misaligned state reaches the library, which refuses it before any launch (DQ_ERR_ARG)
    pad = torch.zeros(2, 17, dtype=torch.complex64, device='cuda')
    odd = pad.reshape(-1)[1:17].reshape(1, 16)
    assert odd.data_ptr() % 16 == 8 and odd.is_contiguous()
    with pytest.raises(RuntimeError, match='status -1'):
        backend.apply_pauli_axpby(odd, 1, 0, 1.0, 1j)
    with pytest.raises(RuntimeError, match='status -1'):
        backend.pauli_cross(odd, odd, 1, 0)


def test_library_error_returns():
    """DQ_ERR_ARG (-1) from the C entry points for real device buffers: nothing is launched."""
    from deepquantum_amd import _lib

    lib, ia = _lib.load(), _lib.int_array
    x = torch.zeros(1, 32, dtype=torch.complex64, device='cuda')
    coef = torch.ones(4, dtype=torch.float64, device='cuda')
    out = torch.zeros(2, dtype=torch.float64, device='cuda')
    ws = torch.zeros(64, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    xp, cp, op, wp = (v.data_ptr() for v in (x, coef, out, ws))
    n = 5
    for xmask, zmask, controls in ((32, 0, ()), (0, 32, ()), (1, 0, (5,)), (1, 0, (2, 2)), (2, 0, (1,)), (0, 4, (2,))):
        nc = len(controls)
        assert lib.dq_apply_pauli_axpby_c64(xp, xp, xmask, zmask, cp, _lib.PAULI_GATE, n, ia(controls), nc, 1, None) == -1
        assert lib.dq_pauli_cross_c64(xp, xp, xmask, zmask, n, ia(controls), nc, 1, op, wp, 512, None) == -1
        assert lib.dq_last_error()
    assert lib.dq_apply_pauli_axpby_c64(xp, xp, 1, 0, cp, 2, n, ia(()), 0, 1, None) == -1             # mode
    assert lib.dq_apply_pauli_axpby_c64(xp, xp, 1, 0, cp, 0, 41, ia(()), 0, 1, None) == -1            # n
    assert lib.dq_apply_pauli_axpby_c64(xp, None, 1, 0, cp, 0, n, ia(()), 0, 1, None) == -1
    assert lib.dq_pauli_cross_c64(xp, xp, 1, 0, n, ia(()), 0, 1, op, wp, 8, None) == -1               # workspace too small
    assert lib.dq_pauli_cross_c64(xp, xp, 1, 0, n, ia(()), 0, 1, None, wp, 512, None) == -1
    for bad in (8, 4):
        assert lib.dq_apply_pauli_axpby_c64(xp + bad, xp, 1, 0, cp, 0, n, ia(()), 0, 1, None) == -1
        assert lib.dq_apply_pauli_axpby_c64(xp, xp + bad, 1, 0, cp, 0, n, ia(()), 0, 1, None) == -1
        assert lib.dq_pauli_cross_c64(xp, xp + bad, 1, 0, n, ia(()), 0, 1, op, wp, 512, None) == -1
    torch.cuda.synchronize()
    assert not x.any() and not out.any()
