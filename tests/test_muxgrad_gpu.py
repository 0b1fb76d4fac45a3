"""The binned cross reduction of the multiplexer on the MI355X (dq_mux_cross_*) through ``backend.mux_cross``, against
numpy complex128 from the definition (tests/_muxgrad_ref.py: ``np.add.at`` over the full amplitude index).

Geometry of csrc/dq_muxgrad.hip, which decides the cases.  The item is the pair (i0, i0 | 1 << target) and all bin
arithmetic is done on the (n - 1)-bit pair index (the amplitude index without the target bit).  A unit is 2^P pairs,
P = 10 + (1 for complex64 with target != 0): in amplitude positions it spans bits 0 .. P with the target among them, or
0 .. P - 1 with the target above.  A lane slot keeps the select bits below the unit for the whole loop (its own
accumulator); the kh select bits at or above the unit name a bin group hv, and the units of a group are enumerated over
the rb unit-index bits that are neither select bits nor controls.  G = min(2^rb, 2^(11 - kh), 2^(19 - k)) workgroups share
a group; a workgroup takes the tasks (hv, g) blockIdx.x, blockIdx.x + 2048, ..  Per task: a butterfly over the lane bits
that are no select bits (pair bits PB .. PB + 5), the slot sums through LDS, one lane per low bin; G > 1: a finishing
kernel, one wave per bin, lane l adding the partial sums l, l + 64, ..  So the cases are

  * n = 2, 3, 5 (less than a wave), 11 / 12 = P + 1 (one unit), 13 / 14 = P + 3 (8 units): every target position the
    kernels tell apart (0: INNER for complex64; 1; 5 - 7 across the wave; P, P + 1; n - 1) with every placement of
    PLACEMENTS, all four axes, bra is ket and two buffers, batch 1 and 3;
  * `finish_two_strides`: n = P + 8 with k = 2 low selects: G = 128 partial sums per bin, two strides of the 64 lanes;
  * `two_units_per_group`: n = P + 11 with k = 10 low selects: 2^10 units in the one bin group, G = 2^(19 - 10) = 512, so
    every workgroup visits two units of its group (and the finishing lanes take eight strides);
  * `task_loop`: n = 23 with the 12 top bits as selects (complex64: target 0, P = 10; complex128: P = 10): 4096 bin groups
    of one unit for 2048 workgroups, so every workgroup flushes twice.

Exact rows: Gaussian integers in [-3, 3], every sum exact in double, ``np.array_equal`` and a second call bit for bit.
Gaussian rows (n <= P + 3): per bin |err| <= (2^-53 m + u_T) sum_bin |terms|, m the bin's number of terms, and the bound's
teeth: the largest term of every bin exceeds it."""

import functools

import numpy as np
import pytest
import torch

from deepquantum_amd import backend
from _muxgrad_ref import binned, cross_terms, gaussian_integer_state3, inside, mux_cross_ref

pytestmark = pytest.mark.gpu

DTYPES = {'c64': torch.complex64, 'c128': torch.complex128}
NP = {'c64': np.complex64, 'c128': np.complex128}
U_T = {'c64': 2.0**-24, 'c128': 2.0**-53}
SIZES = (2, 3, 5, 11, 12, 13, 14)
AXES = 'ixyz'


def unit_bits(dt, target):
    return 10 + (1 if dt == 'c64' and target != 0 else 0)


def targets(n):
    return sorted({t for t in (0, 1, 5, 6, 7, 10, 11, 12, n - 1) if t < n})


def amp(q, target):
    """The amplitude position of pair bit q."""
    return q if q < target else q + 1


def placements(n, target, dt):
    """(bits, controls) in amplitude positions, from lists over pair bits with P the first bit above the unit; positions
    the register does not have are dropped, and what is then empty or seen already is left out."""
    P, npair = unit_bits(dt, target), n - 1
    top = npair - 1
    raw = [
        ([2, 4, 7], []),                                # selects all below the unit boundary
        ([P + 1, P], []),                               # all above it
        ([1, top, P - 1], []),                          # on both sides
        ([P + 1, P, P - 1, P - 2], []),                 # a run that crosses the boundary
        ([0, 3], []),                                   # bit 0 as a select (the element bit of a complex64 vector)
        ([5, 0, P, 3, top], []),                        # unsorted
        ([3], []), ([top], []), ([0], []),              # k = 1
        (list(np.random.default_rng(n).permutation(npair)), []),        # k = n - 1: every bin is one pair
        ([1, 3], [0, 6]),                               # controls below the boundary
        ([1, P - 1], [P]),                              # above it
        ([P + 1, 2], [4, top]),                         # on both sides
        ([8, 9], [5, 7]),                               # selects in the wave bits' place, controls across the wave
    ]
    out, seen = [], set()
    for sel, ctl in raw:
        sel = list(dict.fromkeys(int(q) for q in sel if 0 <= q < npair))
        ctl = [int(q) for q in dict.fromkeys(ctl) if 0 <= q < npair and q not in sel]
        key = (tuple(sel), tuple(ctl))
        if sel and key not in seen:
            seen.add(key)
            out.append(([amp(q, target) for q in sel], [amp(q, target) for q in ctl]))
    return out


@functools.lru_cache(maxsize=None)
def integer_state(n, batch, dt, seed=0):
    """A seeded Gaussian-integer state on the device and the same values in complex128 on the host (shared, never
    modified)."""
    x = gaussian_integer_state3(batch, n, 7919 * n + 31 * batch + seed, NP[dt])
    return torch.from_numpy(x).cuda(), x.astype(np.complex128)


@functools.lru_cache(maxsize=None)
def gaussian(n, batch, dt, seed=0):
    g = torch.Generator().manual_seed(104729 * n + batch + seed)
    psi = torch.randn(batch, 1 << n, dtype=torch.complex128, generator=g).to(DTYPES[dt])
    return psi.cuda(), psi.numpy().astype(np.complex128)


def as_bits(z):
    return torch.view_as_real(z).view(torch.int64)


def check_exact(bra, br, ket, kr, axis, target, bits, controls, what):
    out = backend.mux_cross(bra, ket, axis, target, bits, controls)
    assert out.dtype == torch.complex128 and out.shape == (kr.shape[0], 1 << len(bits)), what
    assert np.array_equal(out.cpu().numpy(), mux_cross_ref(br, kr, axis, target, bits, controls)), what
    again = backend.mux_cross(bra, ket, axis, target, bits, controls)
    assert torch.equal(as_bits(again), as_bits(out)), what             # reproducible bit for bit


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('n', SIZES)
def test_mux_cross_exact(n, dt):
    count = 0
    for target in targets(n):
        for j, (bits, controls) in enumerate(placements(n, target, dt)):
            batch = 3 if j % 2 else 1
            ket, kr = integer_state(n, batch, dt)
            other, orr = integer_state(n, batch, dt, seed=5)
            for axis in AXES:
                for same in (True, False):
                    bra, br = (ket, kr) if same else (other, orr)
                    check_exact(bra, br, ket, kr, axis, target, bits, controls, (n, dt, target, bits, controls, axis, same))
                    count += 1
            assert np.array_equal(ket.cpu().numpy().astype(np.complex128), kr)         # the shared input is untouched
    assert count >= 8


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('n', SIZES)
def test_mux_cross_gaussian(n, dt):
    worst = 0.0
    for target in targets(n):
        for j, (bits, controls) in enumerate(placements(n, target, dt)):
            batch = 1 if j % 2 else 3
            axis = AXES[(j + target) % 4]
            same = bool((j // 2) % 2)
            ket, kr = gaussian(n, batch, dt)
            bra, br = (ket, kr) if same else gaussian(n, batch, dt, seed=5)
            out = backend.mux_cross(bra, ket, axis, target, bits, controls).cpu().numpy()
            terms = cross_terms(br, kr, axis, target, controls)
            ref = binned(terms, n, bits)
            mag = binned(np.abs(terms), n, bits)
            m = binned(np.broadcast_to(inside(n, controls), terms.shape).astype(np.float64), n, bits)
            bound = (2.0**-53 * m + U_T[dt]) * mag
            err = np.abs(out - ref)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (n, dt, target, bits, controls, axis, same, float((err / bound).max()))
            # the bound has teeth: the sum of a bin without its largest term lies outside it
            largest = np.zeros_like(mag)
            s = np.zeros(1 << n, dtype=np.int64)
            for p, b in enumerate(bits):
                s |= ((np.arange(1 << n) >> b) & 1) << (len(bits) - 1 - p)
            for b in range(batch):
                np.maximum.at(largest[b], s, np.abs(terms[b]))
            assert (largest > bound).all(), (n, dt, target, bits, controls)
    print(f'mux_cross gaussian n={n} {dt}: worst err / bound = {worst:.3e}')


BIG = {
    # name: {dt: (n, target, bits, controls)}, batch
    'finish_two_strides': ({'c64': (19, 3, (0, 5), ()), 'c128': (18, 3, (0, 5), ())}, 2),
    'finish_two_strides_high_control': ({'c64': (20, 3, (1, 8), (19,)), 'c128': (19, 3, (1, 8), (18,))}, 1),
    'two_units_per_group': ({'c64': (22, 3, (0, 1, 2, 4, 5, 6, 7, 8, 9, 10), ()),
                             'c128': (21, 3, (10, 9, 8, 7, 6, 5, 4, 2, 1, 0), ())}, 1),
    # three selects above the unit, nine below, a control below: 2^8 units per group for G = 2^(19 - 12) = 128 workgroups
    'two_units_per_group_selects_high': ({'c64': (23, 6, (22, 0, 1, 2, 21, 3, 4, 5, 7, 20, 8, 9), (11,)),
                                          'c128': (22, 6, (21, 0, 1, 2, 20, 3, 4, 5, 7, 19, 8, 9), (10,))}, 1),
    'task_loop': ({'c64': (23, 0, tuple(range(22, 10, -1)), ()), 'c128': (23, 2, tuple(range(22, 10, -1)), ())}, 1),
}


@pytest.mark.parametrize('dt', ['c64', 'c128'])
@pytest.mark.parametrize('same', [True, False], ids=['same', 'cross'])
@pytest.mark.parametrize('case', list(BIG))
def test_mux_cross_exact_beyond_one_stride(case, same, dt):
    """Entries in [-3, 3]: a term is an integer of magnitude <= 36 and a bin adds at most 2^23 of them, below 2^53."""
    shapes, batch = BIG[case]
    n, target, bits, controls = shapes[dt]
    ket, kr = integer_state.__wrapped__(n, batch, dt)              # (not kept: up to 2^23 amplitudes)
    bra, br = (ket, kr) if same else integer_state.__wrapped__(n, batch, dt, seed=5)
    axis = AXES[(len(case) + same) % 4]
    check_exact(bra, br, ket, kr, axis, target, bits, controls, (case, dt, same))


def test_backend_argument_checks():
    x, _ = integer_state(5, 1, 'c64')
    for kw in (dict(bits=(1, 1)), dict(bits=(5,)), dict(controls=(1,)), dict(target=1), dict(target=5), dict(axis='w'), dict(bits=())):
        args = dict(axis='x', target=0, bits=(1, 2), controls=())
        args.update(kw)
        with pytest.raises(ValueError):
            backend.mux_cross(x, x, **args)
    with pytest.raises(ValueError):
        backend.mux_cross(x, x.to(torch.complex128), 'x', 0, (1,))
    # a misaligned state reaches the library, which refuses it before any launch (DQ_ERR_ARG)
    flat = torch.zeros(2 * 32 + 1, dtype=torch.complex64, device='cuda')
    with pytest.raises(RuntimeError, match='aligned'):
        backend.mux_cross(flat[1:33].reshape(1, 32), flat[1:33].reshape(1, 32), 'x', 0, (1,))
