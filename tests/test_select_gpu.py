"""dq_apply_select_pauli_* on the GPU, path by path, against the numpy reference of the definition (``_select_ref``): the
result is a gather of input amplitudes with re / im swapped and signs flipped, so every comparison is exact
(``assert_array_equal``).  The unit boundary ``u`` is read from ``dq_select_pauli_unit_bits``: select bits at or above it
take the uniform instantiation, one below it the per-lane one, and index bit 0 of a complex64 state as a select bit or a
control the split one.  Every string set holds an identity entry, a diagonal string, a pure flip, an all-Y string and a
number of strings that is no power of two; the adjoint table applied after the table gives the input back, bit for bit."""

import numpy as np
import pytest
import torch

from deepquantum_amd import _lib, backend
from _select_ref import random_entries, random_state, random_words, select_ref, words

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(np.complex64, id='c64'), pytest.param(np.complex128, id='c128')]


def unit_bits(dtype):
    return _lib.load().dq_select_pauli_unit_bits(int(dtype == np.complex128))


def on_gpu(table):
    return torch.from_numpy(table.view(np.int64)).cuda()


def check(x, n, bits, controls=(), seed=0, nstrings=None, flips=None, adjoint_reference=True):
    """The table and its adjoint against the definition, the round trip, and the input as it was.  The strings are drawn
    over the free positions (``flips``: over these of them), 2^k - 1 of them by default (k = 1: 2): the rest of the table
    is the identity.  (``adjoint_reference=False``: the adjoint is checked by the round trip alone.)"""
    rng = np.random.default_rng(seed)
    k = len(bits)
    free = [p for p in range(n) if p not in bits and p not in controls]
    if nstrings is None:
        nstrings = max((1 << k) - 1, 2)
    entries = random_entries(rng, nstrings, free if flips is None else flips)
    dev = torch.from_numpy(x).cuda()
    forward, dagger = words(entries, k=k), words(entries, dagger=True, k=k)
    tag = f'n={n} bits={bits} controls={controls}'
    got = backend.apply_select_pauli(dev, on_gpu(forward), bits, controls)
    np.testing.assert_array_equal(got.cpu().numpy(), select_ref(x, forward, bits, controls), err_msg=tag)
    back = backend.apply_select_pauli(got, on_gpu(dagger), bits, controls)
    if adjoint_reference:
        np.testing.assert_array_equal(back.cpu().numpy(), select_ref(got.cpu().numpy(), dagger, bits, controls), err_msg=tag)
    np.testing.assert_array_equal(back.cpu().numpy(), x, err_msg=tag + ': the adjoint table does not undo the table')
    np.testing.assert_array_equal(dev.cpu().numpy(), x, err_msg=tag + ': the input was written to')


@pytest.mark.parametrize('dtype', DTYPES)
def test_samples_smaller_than_a_workgroup(dtype):
    for n, bits, controls in ((1, (0,), ()), (2, (0, 1), ()), (2, (1,), ()), (2, (1,), (0,)), (2, (0,), (1,)), (3, (1,), ()),
                              (4, (3, 0), ()), (4, (2,), (0, 3)), (5, (3, 0, 4), ()), (5, (3, 0), (1,)), (5, (2, 1), (0, 4)),
                              (5, (4, 3, 2, 1, 0), ()), (5, (1, 3, 0, 4, 2), ())):        # (k = n: every entry a bare phase)
        check(random_state(np.random.default_rng(10 + n), 3, n, dtype), n, bits, controls, seed=20 + n)


@pytest.mark.parametrize('dtype', DTYPES)
def test_exactly_one_unit(dtype):
    u = unit_bits(dtype)
    x = random_state(np.random.default_rng(1), 2, u, dtype)
    for bits, controls in (((u - 1, 4), ()), ((3, 1), (u - 1,)), ((0, 2), ()), ((5,), (0,)), ((u - 1, u - 2, u - 3), (1,))):
        check(x, u, bits, controls, seed=31)


def control_sets(u, bits):
    """none, below u, at or above u, both, and bit 0 -- out of the positions the select bits leave free."""
    free = [p for p in range(u + 2) if p not in bits]
    low, high = [p for p in free if 0 < p < u], [p for p in free if p >= u]
    sets = [()]
    if low:
        sets.append((low[len(low) // 2],))
    if high:
        sets.append((high[-1],))
    if low and high:
        sets.append((high[0], low[0]))
    if 0 in free:
        sets.append((0,))
    return sets


@pytest.mark.parametrize('dtype', DTYPES)
def test_uniform_case_select_bits_at_or_above_the_unit(dtype):
    u = unit_bits(dtype)
    n = u + 2
    x = random_state(np.random.default_rng(2), 2, n, dtype)
    # one select bit at or above u: the other such position is free, so a string can send its partner into another unit
    for bits in ((u,), (u + 1,)):
        other = 2 * u + 1 - bits[0]
        check(x, n, bits, seed=41, flips=(0,))                                  # partner in the same vector (complex64)
        check(x, n, bits, seed=42, flips=(u // 2,))                             # a middle bit
        check(x, n, bits, seed=43, flips=(other,))                              # another unit
        check(x, n, bits, seed=44, flips=(0, u // 2, other))
        for controls in control_sets(u, bits):
            check(x, n, bits, controls, seed=45)
    for controls in control_sets(u, (u + 1, u)):
        check(x, n, (u + 1, u), controls, seed=46, nstrings=3)
        check(x, n, (u, u + 1), controls, seed=47, nstrings=3)


@pytest.mark.parametrize('dtype', DTYPES)
def test_lane_case_select_bits_below_the_unit(dtype):
    u = unit_bits(dtype)
    n = u + 2
    x = random_state(np.random.default_rng(3), 2, n, dtype)
    cases = [
        (3, 1), (u - 1,),                # below u only
        (u, u - 1, u - 2),               # one run that straddles u
        (u + 1, u, u - 1, u - 2),
        (u + 1, 3, u - 1),               # runs on both sides
        (1, 4, 7, u, 3),                 # unsorted: runs of length 1
        (u + 1, u - 1, 6, 2),            # descending runs of length 1
    ]
    for bits in cases:
        for controls in control_sets(u, bits):
            check(x, n, bits, controls, seed=50 + len(bits), nstrings=(1 << len(bits)) - 3 if len(bits) > 2 else None)


@pytest.mark.parametrize('dtype', DTYPES)
def test_bit_0_as_a_select_bit(dtype):
    """complex64: the two amplitudes of a vector read different entries (8-byte loads)."""
    u = unit_bits(dtype)
    n = u + 2
    x = random_state(np.random.default_rng(4), 3, n, dtype)
    for bits in ((0, 2), (u + 1, 1, 0), (0,), (0, u), (1, 0, u, u - 1)):
        for controls in control_sets(u, bits):
            check(x, n, bits, controls, seed=60 + len(bits))


@pytest.mark.parametrize('dtype', DTYPES)
def test_a_table_over_every_index_bit_is_confined_to_the_free_bits(dtype):
    """Flip masks with select and control bits set: the kernel masks them, as the definition says."""
    u = unit_bits(dtype)
    n = u + 1
    x = random_state(np.random.default_rng(5), 2, n, dtype)
    dev = torch.from_numpy(x).cuda()
    for bits, controls in (((u, 3), (1,)), ((0, 2), (u,)), ((u,), ())):
        table = random_words(np.random.default_rng(6), len(bits), range(n))
        got = backend.apply_select_pauli(dev, on_gpu(table), bits, controls).cpu().numpy()
        np.testing.assert_array_equal(got, select_ref(x, table, bits, controls))


@pytest.mark.parametrize('dtype', DTYPES)
def test_every_workgroup_strides_over_more_than_one_unit(dtype):
    """4096 units for at most 2048 workgroups: complex64 n = 23, complex128 n = 22, batch 1."""
    u = unit_bits(dtype)
    n = u + 12
    x = random_state(np.random.default_rng(7), 1, n, dtype)
    check(x, n, (n - 1, 4), seed=71, adjoint_reference=False)


@pytest.mark.parametrize('dtype', DTYPES)
def test_batch_of_three_from_a_slice_at_a_sample_offset(dtype):
    u = unit_bits(dtype)
    n = u + 1
    big = random_state(np.random.default_rng(8), 5, n, dtype)
    dev = torch.from_numpy(big).cuda()
    view = dev[1:4]
    for bits, controls in (((u, 2, 0), (5,)), ((7, 1), (u,)), ((u,), (3,))):
        free = [p for p in range(n) if p not in bits and p not in controls]
        table = words(random_entries(np.random.default_rng(9), max((1 << len(bits)) - 1, 2), free), k=len(bits))
        out = torch.zeros(5, 1 << n, dtype=dev.dtype, device='cuda')
        got = backend.apply_select_pauli(view, on_gpu(table), bits, controls, out=out[2:5])
        assert got.data_ptr() == out[2:5].data_ptr()
        np.testing.assert_array_equal(out[2:5].cpu().numpy(), select_ref(big[1:4], table, bits, controls))
        assert not out[:2].any()                                                # nothing written before the slice
    np.testing.assert_array_equal(dev.cpu().numpy(), big)


@pytest.mark.parametrize('dtype', DTYPES)
def test_refusals_launch_nothing(dtype):
    u = unit_bits(dtype)
    n = u + 1
    lib = _lib.load()
    fn = getattr(lib, 'dq_apply_select_pauli_' + ('c128' if dtype == np.complex128 else 'c64'))
    ia = _lib.int_array
    x = torch.from_numpy(random_state(np.random.default_rng(11), 2, n, dtype)).cuda()
    out = torch.zeros_like(x)
    table = on_gpu(words([(1, 0, 0), (0, 1, 1)]))

    def refused(rc, word):
        assert rc == -1 and word in lib.dq_last_error().decode(), lib.dq_last_error()

    refused(fn(x.data_ptr(), x.data_ptr(), table.data_ptr(), n, ia([u]), 1, ia([]), 0, 2, None), 'overlap')
    refused(fn(x[0:1].data_ptr(), x[1:2].data_ptr(), table.data_ptr(), n, ia([u]), 1, ia([]), 0, 2, None), 'overlap')
    refused(fn(x.data_ptr(), out.data_ptr(), table.data_ptr() + 8, n, ia([u]), 1, ia([]), 0, 2, None), 'aligned')
    with pytest.raises(ValueError, match='overlap'):
        backend.apply_select_pauli(x, table, (u,), out=x)
    torch.cuda.synchronize()
    assert not out.any()
