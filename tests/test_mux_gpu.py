"""dq_apply_mux_* on the GPU against the numpy complex128 reference of the definition (``_mux_ref``).

The cases follow the geometry of csrc/dq_mux.hip.  A lane moves 16-byte vectors (two complex64 or one complex128
amplitude); an item is a pair of vectors (va, va | 1 << tv) or, for complex64 with the target at bit 0, one vector that
holds the pair (INNER); a workgroup of 256 lanes takes a unit of 1024 items per iteration and at most 2048 workgroups
stride over the units of a sample.  The table arithmetic runs on the pair index -- the amplitude index with the target
bit removed, so that positions above the target move down by one -- whose bits below ``P`` = 10 + log2(pairs of an
item) depend on the lane alone and whose bits from ``P`` upward on the unit alone.  In amplitude positions a unit
therefore spans the bits 0 .. P with the target among them, or 0 .. P - 1 and the target above.  Hence:

  * samples smaller than a workgroup (n = 2, 3, 5), exactly one unit (n = P + 1), a few units (n = P + 3), and one case
    whose workgroups stride twice (complex64 n = 24, complex128 n = 23: 4096 units, 128 MiB);
  * the target at bit 0 (complex64: INNER), at bit 1 (the lowest vector bit of complex64), across the wave (the lane bits
    of a wave are the item bits 0 .. 5: amplitude bits 5, 6, 7), at P (the top bit inside a unit), at P + 1 (the first
    above it) and at n - 1;
  * for every target select bits below it, above it and on both sides -- the shift into pair space --, among them runs
    that end below, at and across the unit boundary, bit 0 as a select (two table entries per complex64 vector) and as a
    control, unsorted lists, k = 1 and k = n - 1;
  * controls below the unit boundary (a lane's test) and above it (a unit that is copied, or skipped in place).

Exact rows: Gaussian-integer states and tables whose entries are small integers (they need not be unitary), so that
every product and sum is exact in float32 and the comparison is one of numbers with zero tolerance, for both ``dagger``
values, out of place and in place; the amplitudes outside the controls are compared with the input bit for bit.
Gaussian rows: random states and unitaries to 1e-4 (complex64) / 1e-10 (complex128) of max |reference|."""

import numpy as np
import pytest
import torch

from deepquantum_amd import _lib, backend
from _mux_ref import (exact_cs, exact_unitaries, gaussian_integer_state, mux_ref, outside, random_cs, random_state,
                      random_unitaries, ry_blocks, same_bits)

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(np.complex64, id='c64'), pytest.param(np.complex128, id='c128')]
TOL = {np.complex64: 1e-4, np.complex128: 1e-10}


def pair_unit_bits(dtype, target=1):
    """log2 of the pairs of a unit."""
    return 10 + (1 if dtype == np.complex64 and target != 0 else 0)


def real_of(dtype):
    return np.float32 if dtype == np.complex64 else np.float64


def exact_rows(x, target, bits, controls, seed=0, kinds=('u', 'ry'), daggers=(False, True)):
    """Zero tolerance, both kinds and directions, out of place and in place; the input stays as it was."""
    n = x.shape[-1].bit_length() - 1
    k = len(bits)
    out_idx = outside(n, controls)
    dev = torch.from_numpy(x).cuda()
    for kind in kinds:
        table = exact_unitaries(k, seed + 1) if kind == 'u' else exact_cs(k, seed + 2)
        blocks = table if kind == 'u' else ry_blocks(table)
        tdev = torch.from_numpy(table.astype(x.dtype if kind == 'u' else real_of(x.dtype))).cuda()
        for dagger in daggers:
            what = f'kind={kind} dagger={dagger} n={n} target={target} bits={bits} controls={controls}'
            want = mux_ref(x, blocks, target, bits, controls, dagger)
            got = backend.apply_mux(dev, tdev, kind, target, bits, controls, dagger=dagger).cpu().numpy()
            assert got.dtype == x.dtype
            np.testing.assert_array_equal(got.astype(np.complex128), want, err_msg=what)
            assert same_bits(got[:, out_idx], x[:, out_idx]), what + ': an amplitude outside the controls changed'
            inplace = dev.clone()
            assert backend.apply_mux(inplace, tdev, kind, target, bits, controls, dagger=dagger, out=inplace) is inplace
            got = inplace.cpu().numpy()
            np.testing.assert_array_equal(got.astype(np.complex128), want, err_msg=what + ' (in place)')
            assert same_bits(got[:, out_idx], x[:, out_idx]), what + ' (in place): an amplitude outside the controls changed'
    assert same_bits(dev.cpu().numpy(), x)


def gaussian_rows(x, target, bits, controls, seed=0):
    """Random unitaries / rotations to the tolerance of the precision: out of place forward, in place daggered."""
    k = len(bits)
    dev = torch.from_numpy(x).cuda()
    for kind in ('u', 'ry'):
        table = random_unitaries(k, seed + 3) if kind == 'u' else random_cs(k, seed + 4)
        blocks = table if kind == 'u' else ry_blocks(table)
        tdev = torch.from_numpy(table).cuda()                       # (float64 / complex128: converted to the state's precision)
        for dagger, inplace in ((False, False), (True, True)):
            want = mux_ref(x, blocks, target, bits, controls, dagger)
            src = dev.clone() if inplace else dev
            got = backend.apply_mux(src, tdev, kind, target, bits, controls, dagger=dagger, out=src if inplace else None)
            err = np.abs(got.cpu().numpy() - want).max()
            assert err <= TOL[x.dtype.type] * np.abs(want).max(), (kind, dagger, target, bits, controls, err)


@pytest.mark.parametrize('dtype', DTYPES)
def test_samples_smaller_than_a_workgroup(dtype):
    cases = (
        (2, 0, (1,), ()), (2, 1, (0,), ()),
        (3, 0, (2, 1), ()), (3, 1, (0, 2), ()), (3, 2, (1, 0), ()), (3, 1, (2,), (0,)), (3, 0, (1,), (2,)), (3, 2, (0,), ()),
        (5, 0, (3, 1, 4), ()), (5, 2, (3, 0, 4), (1,)), (5, 4, (2, 1), (0,)), (5, 1, (4, 3, 2, 0), ()), (5, 3, (0, 4, 1, 2), ()),
        (5, 0, (1, 2, 3, 4), ()), (5, 4, (3, 2, 1, 0), ()), (5, 2, (4,), (0, 3)),
    )
    for n, target, bits, controls in cases:
        x = gaussian_integer_state(3, n, 10 + n, dtype)
        exact_rows(x, target, bits, controls, seed=n)
        gaussian_rows(random_state(3, n, 20 + n, dtype), target, bits, controls, seed=n)


def select_sets(n, t, p):
    """Select lists for target t in a sample of n bits: below t, above t, on both sides, runs that end below / at /
    across the unit boundary p (amplitude positions), unsorted ones, k = 1."""
    free = [q for q in range(n) if q != t]
    below, above = [q for q in free if q < t], [q for q in free if q > t]
    sets = []
    if below:
        sets += [tuple(below[-2:][::-1]), (below[0],)]
    if above:
        sets += [tuple(above[:2][::-1]), (above[-1],)]
    if below and above:
        sets += [(above[0], below[-1]), (below[0], above[-1], below[-1], above[0])]          # both sides, unsorted
    # runs around the unit boundary, as far as the target leaves them free
    for run in ((p - 1, p - 2, p - 3), (p, p - 1, p - 2), (p + 1, p, p - 1), (p + 2, p + 1)):
        run = tuple(q for q in run if q in free)
        if run:
            sets.append(run)
    if 0 in free:
        sets.append((n - 1 if t != n - 1 else n - 2, 0))                                     # bit 0 as a select
    return list(dict.fromkeys(tuple(dict.fromkeys(b)) for b in sets))           # (no position twice, no list twice)


def control_sets(n, t, bits, p):
    free = [q for q in range(n) if q != t and q not in bits]
    low, high = [q for q in free if q < p], [q for q in free if q > p + 1]
    sets = [()]
    if low:
        sets.append((low[len(low) // 2],))
    if high:
        sets.append((high[-1],))
    if low and high:
        sets.append((high[0], low[0]))                                                      # (low[0] is bit 0 where it is free)
    return sets


@pytest.mark.parametrize('dtype', DTYPES)
def test_exactly_one_unit(dtype):
    p = pair_unit_bits(dtype)
    n = p + 1
    x = gaussian_integer_state(2, n, 1, dtype)
    g = random_state(2, n, 2, dtype)
    for t in (1, 6, p, n - 1):
        for bits in select_sets(n, t, p)[:4]:
            exact_rows(x, t, bits, (), seed=t)
        full = tuple(q for q in range(n - 1, -1, -1) if q != t)                              # k = n - 1
        exact_rows(x, t, full, (), seed=t, kinds=('ry',))
        gaussian_rows(g, t, full[::-1], (), seed=t)
    # complex64, target 0: a unit is 1024 vectors, n = 11
    m = pair_unit_bits(dtype, 0) + 1
    x = gaussian_integer_state(2, m, 3, dtype)
    exact_rows(x, 0, tuple(range(m - 1, 0, -1)), ())
    exact_rows(x, 0, (1, m - 1, 5), (3,))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('where', ['bit0', 'bit1', 'wave5', 'wave6', 'wave7', 'unit_top', 'above_unit', 'top'])
def test_a_few_units_every_target_class(dtype, where):
    p = pair_unit_bits(dtype)
    n = p + 3
    t = {'bit0': 0, 'bit1': 1, 'wave5': 5, 'wave6': 6, 'wave7': 7, 'unit_top': p, 'above_unit': p + 1, 'top': n - 1}[where]
    pu = pair_unit_bits(dtype, t)                       # (complex64 with target 0: one pair per item)
    x = gaussian_integer_state(2, n, 30 + t, dtype)
    g = random_state(2, n, 40 + t, dtype)
    for j, bits in enumerate(select_sets(n, t, pu)):
        for controls in control_sets(n, t, bits, pu):
            exact_rows(x, t, bits, controls, seed=j, daggers=(bool(j & 1),) if controls else (False, True))
        gaussian_rows(g, t, bits, control_sets(n, t, bits, pu)[-1], seed=j)
    # k = n - 1: the table has as many entries as there are pairs
    full = tuple(q for q in range(n - 1, -1, -1) if q != t)
    exact_rows(x, t, full, (), seed=7)
    gaussian_rows(g, t, tuple(int(q) for q in np.random.default_rng(t).permutation(full)), (), seed=8)
    # k = 1
    exact_rows(x, t, (full[len(full) // 2],), (), seed=9)
    # bit 0 as a control (per amplitude of a complex64 vector)
    if t != 0:
        bits = tuple(q for q in (pu + 1, 3) if q != t)
        exact_rows(x, t, bits, (0,), seed=10)
        high = max(q for q in range(n) if q != t and q not in bits)
        exact_rows(x, t, bits, (0, high), seed=11, kinds=('ry',))


@pytest.mark.parametrize('dtype', DTYPES)
def test_every_workgroup_strides_over_more_than_one_unit(dtype):
    """4096 units of pairs for at most 2048 workgroups: complex64 n = 24, complex128 n = 23, batch 1 (128 MiB); complex64
    with the target at bit 0 runs 8192 units of vectors.  One reference per row, shared by the out-of-place and the
    in-place run."""
    p = pair_unit_bits(dtype)
    n = p + 13
    x = gaussian_integer_state(1, n, 5, dtype)
    dev = torch.from_numpy(x).cuda()
    rows = (('u', False, 4, (n - 1, p + 2, 0, 7), (n - 2,)),            # a high control: half of the units are copied / skipped
            ('ry', True, 0, (n - 1, 1, p + 1), (3,)))
    for kind, dagger, t, bits, controls in rows:
        k = len(bits)
        table = exact_unitaries(k, 61) if kind == 'u' else exact_cs(k, 62)
        want = mux_ref(x, table if kind == 'u' else ry_blocks(table), t, bits, controls, dagger)
        tdev = torch.from_numpy(table.astype(x.dtype if kind == 'u' else real_of(x.dtype))).cuda()
        got = backend.apply_mux(dev, tdev, kind, t, bits, controls, dagger=dagger)
        assert np.array_equal(got.cpu().numpy().astype(np.complex128), want), (kind, 'out of place')
        del got
        work = dev.clone()
        backend.apply_mux(work, tdev, kind, t, bits, controls, dagger=dagger, out=work)
        assert np.array_equal(work.cpu().numpy().astype(np.complex128), want), (kind, 'in place')
        del work, want


@pytest.mark.parametrize('dtype', DTYPES)
def test_batch_of_three_from_a_slice_at_a_sample_offset(dtype):
    p = pair_unit_bits(dtype)
    n = p + 2
    big = gaussian_integer_state(5, n, 6, dtype)
    dev = torch.from_numpy(big).cuda()
    view = dev[1:4]
    assert view.data_ptr() != dev.data_ptr() and view.is_contiguous()
    for kind, t, bits, controls in (('u', 3, (p + 1, 2, 0), (5,)), ('ry', p + 1, (7, 1), (p,)), ('u', 0, (p - 1, 3), ())):
        k = len(bits)
        table = exact_unitaries(k, 70) if kind == 'u' else exact_cs(k, 71)
        want = mux_ref(big[1:4], table if kind == 'u' else ry_blocks(table), t, bits, controls)
        tdev = torch.from_numpy(table.astype(big.dtype if kind == 'u' else real_of(big.dtype))).cuda()
        out = torch.zeros(5, 1 << n, dtype=dev.dtype, device='cuda')
        got = backend.apply_mux(view, tdev, kind, t, bits, controls, out=out[2:5])
        assert got.data_ptr() == out[2:5].data_ptr()
        np.testing.assert_array_equal(out[2:5].cpu().numpy().astype(np.complex128), want)
        assert not out[:2].any()                                            # nothing written before the slice
        # in place on the slice: the neighbouring samples stay
        work = dev.clone()
        backend.apply_mux(work[1:4], tdev, kind, t, bits, controls, out=work[1:4])
        np.testing.assert_array_equal(work[1:4].cpu().numpy().astype(np.complex128), want)
        assert same_bits(work[:1].cpu().numpy(), big[:1]) and same_bits(work[4:].cpu().numpy(), big[4:])
    assert same_bits(dev.cpu().numpy(), big)


@pytest.mark.parametrize('dtype', DTYPES)
def test_refusals_launch_nothing(dtype):
    n = 6
    lib = _lib.load()
    fn = getattr(lib, 'dq_apply_mux_' + ('c128' if dtype == np.complex128 else 'c64'))
    ia = _lib.int_array
    x = torch.from_numpy(random_state(2, n, 7, dtype)).cuda()
    before = x.clone()
    out = torch.zeros_like(x)
    table = torch.from_numpy(random_unitaries(1, 1).astype(dtype)).cuda()

    def refused(rc, word):
        assert rc == -1 and word in lib.dq_last_error().decode(), lib.dq_last_error()

    args = lambda **kw: tuple({**dict(i=x.data_ptr(), o=out.data_ptr(), t=table.data_ptr(), kind=0, dagger=0, n=n, target=2,  # noqa: E731
                                     bits=ia([1]), k=1, controls=ia([]), nc=0, batch=2, stream=None), **kw}.values())
    refused(fn(*args(kind=2)), 'kind')
    refused(fn(*args(dagger=2)), 'dagger')
    refused(fn(*args(target=1)), 'is the target')
    refused(fn(*args(target=n)), 'target')
    refused(fn(*args(bits=ia([n]))), 'out of range')
    refused(fn(*args(k=0)), 'k=0')
    refused(fn(*args(bits=ia([0, 1, 3, 4, 5, 2]), k=6)), 'k=6')
    refused(fn(*args(controls=ia([1]), nc=1)), 'twice')
    refused(fn(*args(batch=0)), 'batch')
    refused(fn(*args(t=table.data_ptr() + 8)), 'aligned')
    refused(fn(*args(i=x[0:1].data_ptr(), o=x[1:2].data_ptr())), 'overlap')                 # shifted by one sample
    with pytest.raises(ValueError, match='distinct'):
        backend.apply_mux(x, table, 'u', 1, (1,), out=out)
    with pytest.raises(ValueError, match='overlap'):
        flat = torch.zeros(3 << n, dtype=x.dtype, device='cuda')
        backend.apply_mux(flat[:2 << n].reshape(2, -1), table, 'u', 2, (1,), out=flat[1 << n:].reshape(2, -1))
    torch.cuda.synchronize()
    assert not out.any() and torch.equal(x, before)
    # the neighbouring sample is no overlap, and the same buffer is allowed
    got = backend.apply_mux(x[0:1], table, 'u', 2, (1,), out=x[1:2])
    want = mux_ref(before[0:1].cpu().numpy(), random_unitaries(1, 1), 2, (1,))
    assert np.abs(got.cpu().numpy() - want).max() <= TOL[dtype] * np.abs(want).max()
