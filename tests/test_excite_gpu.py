"""The excitation kernels on the MI355X (dq_apply_excite_axpby_*, dq_excite_cross_*) through ``backend``, against numpy
complex128 from the pair formula (tests/_excite_ref.py).

Geometry of csrc/dq_excite.hip, which decides the cases: a lane moves 16-byte vectors (two complex64 amplitudes or one
complex128); the fixed bits are xmask | controls, and the item index runs over the FREE vector-index bits only -- a
deposit cut into runs at the unit size of 2^10 items, the low runs per lane, the high runs per unit, the parity of
i0 & zmask split the same way.  An item is a pair of vectors, or (complex64, xmask == 1) one vector; in complex64 an
amplitude next to a pair's end in a vector whose bit 0 is fixed is a bystander.  At most 2048 workgroups per sample: a
workgroup takes a second unit from 2^22 items on -- a single at n = 24 in complex128, and in complex64 when bit 0 is one
of its two bits.  Item counts are powers of two, so the first count above one unit is 2^11.

Every case runs in both precisions, in place and out of place, in 'gate' and 'map' mode, as a rotation, and through the
cross with bra the ket and another tensor.  Criteria: error <= TOL max|ref| (1e-4 / 1e-10); every amplitude outside the
pairs bit-identical to the input ('gate') or exactly 0 ('map'); in place and out of place bit-identical; two runs of the
cross bit-identical; Re cross(x, x) <= TOL |x|^2."""

import functools

import numpy as np
import pytest
import torch

from deepquantum_amd import backend
from deepquantum_amd.gate import excitation_masks
from _excite_ref import index_axpby, index_cross, index_rot, outside

pytestmark = pytest.mark.gpu

DTYPES = {'c64': torch.complex64, 'c128': torch.complex128}
TOL = {'c64': 1e-4, 'c128': 1e-10}


def bits(*positions):
    return sum(1 << p for p in positions)


def wires_spec(n, create, annihilate, controls=()):
    return (*excitation_masks(n, create, annihilate, True, controls), tuple(n - 1 - c for c in controls))


CASES = {
    # name: (n, (xmask, amask, zmask, negate[, controls]), batch)
    'n2-single-up': (2, (0b11, 0b10, 0, 0), 1),                                  # 1. one pair, a bystander on each side
    'n2-single-down': (2, (0b11, 0b01, 0, 1), 2),
    'n4-double-all': (4, (0b1111, 0b1100, 0, 1), 1),
    'n12-low-four': (12, (0b1111, 0b0101, bits(4, 7, 11), 0), 2),                # 2. every line is touched
    'n12-bit0-free': (12, (bits(1, 5), bits(5), bits(0, 2, 3, 4), 0), 2),        # 3. both elements of a vector rotate
    'n12-bit0-free-no-z0': (12, (bits(1, 5), bits(1), bits(2, 3, 4, 11), 1), 1),
    'n12-bit0-control': (12, (bits(3, 9), bits(3), bits(4, 5, 6, 7, 8), 0, (0,)), 2),    # 4.
    'n15-across-the-unit': (15, (bits(9, 10, 11, 12), bits(9, 12), bits(0, 8, 13, 14), 0), 1),   # 5.
    'n12-one-unit': (12, (bits(4, 7), bits(4), bits(5, 6), 0), 1),               # items: 2^10 (c128), 2^9 (c64)
    'n13-one-unit': (13, (bits(4, 7), bits(7), bits(5, 6, 12), 1), 1),           # items: 2^11 (c128), 2^10 (c64)
    'n14-two-units': (14, (bits(4, 7), bits(4), bits(0, 13), 0), 1),             # items: 2^12 (c128), 2^11 (c64)
    'n16-top-four': (16, (0xF000, 0x3000, bits(0, 5, 11), 0), 1),                # 6.
    'n13-triple': (13, (bits(0, 3, 5, 8, 10, 12), bits(0, 5, 10), bits(1, 4, 11), 1), 2),        # 7.
    'n11-weight1-bit0-a0': (11, (1, 0, bits(1, 10), 0), 2),                      # complex64: both ends in one vector
    'n11-weight1-bit0-a1': (11, (1, 1, bits(5), 1), 2),
    'n11-weight1-bit0-ctrl': (11, (1, 1, 0, 0, (1, 10)), 1),
    'n11-weight1-bit6-a0': (11, (bits(6), 0, bits(0, 7), 0), 1),
    'n11-weight1-bit6-a1': (11, (bits(6), bits(6), 0, 0), 1),
    'n14-fermionic-double': (14, wires_spec(14, [9, 13], [0, 5]), 1),            # 8. the string on both sides of the split
    'n14-fermionic-double-2c': (14, wires_spec(14, [9, 13], [0, 5], (2, 7)), 2),
    'n12-batch3': (12, (bits(1, 5), bits(5), bits(2, 3, 4), 0), 3),              # 9. per-sample angles
}
BIG = ('n24-single', (24, (bits(0, 20), bits(20), bits(1, 7, 12, 19), 0), 1))    # 10. a workgroup strides over two units
THETAS = np.array([0.4, -1.3, 3.9])                     # (one negative, one above pi)
A = np.array([0.3 - 0.2j, 1.1j, -0.7 + 0.0j])
C = np.array([-0.6 + 0.1j, 0.4, 0.9j])


@functools.lru_cache(maxsize=None)
def gaussian(n, batch, dt, seed=0):
    """A seeded Gaussian state on the device and the same values in complex128 on the host (shared, never modified)."""
    g = torch.Generator().manual_seed(7919 * n + 31 * batch + seed)
    psi = torch.randn(batch, 1 << n, dtype=torch.complex128, generator=g).to(DTYPES[dt])
    return psi.cuda(), psi.numpy().astype(np.complex128)


def host(t):
    return t.cpu().numpy().astype(np.complex128)


def bitwise_equal(a, b):
    kind = torch.int32 if a.dtype == torch.complex64 else torch.int64
    return torch.equal(torch.view_as_real(a).view(kind), torch.view_as_real(b).view(kind))


def close(got, ref, tol, what):
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    print(f'{what}: err / (tol * max|ref|) = {err / (tol * scale):.3e}')
    assert err <= tol * scale, f'{what}: {err:.3e} against {tol} * {scale:.3e}'


def check_case(name, n, spec, batch, dt):
    tol = TOL[dt]
    x, xh = gaussian(n, batch, dt)
    y, yh = gaussian(n, batch, dt, seed=1)
    rest = torch.from_numpy(outside(n, spec)).cuda()
    a, c, th = torch.from_numpy(A[:batch]), torch.from_numpy(C[:batch]), torch.from_numpy(THETAS[:batch])
    for mode in ('gate', 'map'):
        ref = index_axpby(xh, spec, A[:batch], C[:batch], mode)
        got = backend.apply_excite_axpby(x, spec, a, c, mode)
        close(host(got), ref, tol, f'{name} {dt} axpby {mode}')
        if mode == 'gate':
            assert bitwise_equal(got[:, rest], x[:, rest]), f'{name} {dt}: an amplitude outside the pairs changed'
        else:
            assert not torch.view_as_real(got[:, rest]).any(), f'{name} {dt}: a non-zero outside the pairs'
        z = x.clone()
        assert backend.apply_excite_axpby(z, spec, a, c, mode, out=z) is z
        assert bitwise_equal(z, got), f'{name} {dt} {mode}: in place differs from out of place'
        buf = torch.full_like(x, 7.0)                   # a given `out` is filled, whatever it held
        assert backend.apply_excite_axpby(x, spec, a, c, mode, out=buf) is buf and bitwise_equal(buf, got)
    ref = index_rot(xh, spec, THETAS[:batch].reshape(-1, 1))
    got = backend.apply_excite_rot(x, spec, th)
    close(host(got), ref, tol, f'{name} {dt} rot')
    assert bitwise_equal(got[:, rest], x[:, rest])
    z = x.clone()
    backend.apply_excite_rot(z, spec, th, out=z)
    assert bitwise_equal(z, got)
    # the cross
    for bra, brah, what in ((y, yh, 'bra != ket'), (x, xh, 'bra is ket')):
        ref = index_cross(brah, xh, spec)
        got = backend.excite_cross(bra, x, spec)
        again = backend.excite_cross(bra, x, spec)
        assert got.dtype == torch.complex128 and torch.equal(torch.view_as_real(got), torch.view_as_real(again))
        scale = np.linalg.norm(brah, axis=1) * np.linalg.norm(xh, axis=1)
        err = np.abs(host(got) - ref)
        print(f'{name} {dt} cross {what}: err / (tol * |bra| |ket|) = {(err / (tol * scale)).max():.3e}')
        assert np.all(err <= tol * scale)
        if bra is x:
            assert np.all(np.abs(host(got).real) <= tol * scale)
    del z, buf


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('name', list(CASES))
def test_every_path_against_the_pair_formula(name, dt):
    n, spec, batch = CASES[name]
    check_case(name, n, spec, batch, dt)


@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_a_workgroup_strides_over_several_units(dt):
    name, (n, spec, batch) = BIG
    check_case(name, n, spec, batch, dt)
    torch.cuda.empty_cache()
    gaussian.cache_clear()


def test_a_cpu_tensor_is_refused():
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        backend.apply_excite_axpby(torch.zeros(1, 4, dtype=torch.complex64), (3, 1, 0, 0), 1.0, 0.0)
