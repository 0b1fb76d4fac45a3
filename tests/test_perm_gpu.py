"""dq_apply_permutation_* on the GPU, path by path, against the numpy reference of the definition (``_perm_ref``): the
result is a copy of input amplitudes, so every comparison is exact -- ``assert_array_equal`` and, for the sign of zeros,
equality of the bit patterns.  The unit boundary ``u`` (the amplitudes of a 16-KiB chunk, log2) is read from
``dq_permutation_local_bits``; every shape runs with each path that applies set explicitly and once with 'auto'."""

import numpy as np
import pytest
import torch

from deepquantum_amd import _lib, backend
from _perm_ref import bit_reversal, identity, increment, inverse_of, permute_ref, random_bijection, random_state, same_bits

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(np.complex64, id='c64'), pytest.param(np.complex128, id='c128')]


def unit_bits(dtype):
    return _lib.load().dq_permutation_local_bits(int(dtype == np.complex128))


def tables(k, seed):
    return [random_bijection(k, seed), identity(k), bit_reversal(k), increment(k)]


def paths_for(bits, u):
    return ('gather', 'local', 'auto') if max(bits) < u else ('gather', 'auto')


def check(x, perm, bits, controls=(), paths=None, u=None):
    """Every path that applies, bit for bit against the definition; the input stays as it was."""
    want = permute_ref(x, perm, bits, controls)
    dev = torch.from_numpy(x).cuda()
    src = torch.from_numpy(inverse_of(perm)).cuda()
    for path in paths or paths_for(bits, u):
        got = backend.apply_permutation(dev, src, bits, controls, path=path).cpu().numpy()
        np.testing.assert_array_equal(got, want, err_msg=f'path={path} bits={bits} controls={controls}')
        assert same_bits(got, want), f'path={path} bits={bits} controls={controls}: a zero changed its sign'
    assert same_bits(dev.cpu().numpy(), x)


@pytest.mark.parametrize('dtype', DTYPES)
def test_samples_smaller_than_a_workgroup(dtype):
    u = unit_bits(dtype)
    for n, bits, controls in ((1, (0,), ()), (2, (0, 1), ()), (2, (1, 0), ()), (2, (1,), (0,)), (2, (0,), (1,)),
                              (5, (3, 0, 4), ()), (5, (3, 0, 4), (1,)), (5, (2, 1), (0, 4)), (5, (4, 3, 2, 1, 0), ()),
                              (5, (1, 3, 0, 4, 2), ())):
        x = random_state(3, n, 10 + n, dtype)
        for perm in tables(len(bits), 20 + n):
            check(x, perm, bits, controls, u=u)


@pytest.mark.parametrize('dtype', DTYPES)
def test_exactly_one_unit_and_k_equal_n(dtype):
    u = unit_bits(dtype)
    x = random_state(2, u, 1, dtype)
    natural, shuffled = tuple(range(u - 1, -1, -1)), tuple(int(b) for b in np.random.default_rng(3).permutation(u))
    for bits in (natural, shuffled):
        for perm in tables(u, 31):
            check(x, perm, bits, u=u)
    check(x, random_bijection(3, 4), (u - 1, 0, 4), (2,), u=u)
    # k = n over a few units: the table spans every index bit (GATHER only)
    n = u + 2
    x = random_state(2, n, 2, dtype)
    natural, shuffled = tuple(range(n - 1, -1, -1)), tuple(int(b) for b in np.random.default_rng(5).permutation(n))
    for bits in (natural, shuffled):
        for perm in tables(n, 32):
            check(x, perm, bits, u=u)


def control_sets(u, bits):
    """none, below u, at or above u, both -- out of the positions the table leaves free."""
    free = [p for p in range(u + 2) if p not in bits]
    low, high = [p for p in free if p < u], [p for p in free if p >= u]
    sets = [()]
    if low:
        sets.append((low[len(low) // 2],))
    if high:
        sets.append((high[-1],))
    if low and high:
        sets.append((high[0], low[0]))
    return sets


@pytest.mark.parametrize('dtype', DTYPES)
def test_local_path_with_bit_0_in_and_out_of_the_table(dtype):
    u = unit_bits(dtype)
    n = u + 2
    x = random_state(2, n, 3, dtype)
    for bits in ((0, 3, u - 1, 5), (1, 4, u - 1), (u - 1, u - 2, u - 3), (2, 1, 0), (6,), (0,), (u - 1,)):
        for controls in control_sets(u, bits) + [(0,)] * (0 not in bits):       # (bit 0 as a control: per amplitude)
            for perm in tables(len(bits), 40 + len(bits)):
                check(x, perm, bits, controls, paths=('local', 'auto', 'gather'))


@pytest.mark.parametrize('dtype', DTYPES)
def test_gather_path_wide_and_narrow_loads(dtype):
    u = unit_bits(dtype)
    n = u + 2
    x = random_state(2, n, 4, dtype)
    cases = [
        (u + 1, u),                      # all table bits at or above u (16-byte loads)
        (u, u + 1),
        (u, u - 1, u - 2),               # one run that straddles u
        (u + 1, u, u - 1, u - 2),
        (u + 1, 3, u - 1),               # runs on both sides
        (0, 2),                          # bit 0 a table bit (complex64: 8-byte loads), nothing at or above u
        (0, u),                          # ... with a bit at u
        (u + 1, 1, 0),
        (1, 0, u, u - 1),
        (1, 4, 7, u, 3),                 # unsorted: runs of length 1
        (u + 1, u - 1, 6, 2),            # descending runs of length 1
        (u,), (u + 1,),                  # k = 1
    ]
    for bits in cases:
        for controls in control_sets(u, bits):
            for perm in tables(len(bits), 50 + len(bits)):
                check(x, perm, bits, controls, paths=('gather', 'auto'))
    check(x, random_bijection(2, 1), (u, 3), (0,), paths=('gather', 'auto'))    # bit 0 as a control: per amplitude
    check(x, random_bijection(2, 2), (u, 3), (0, u + 1), paths=('gather', 'auto'))


@pytest.mark.parametrize('dtype', DTYPES)
def test_every_workgroup_strides_over_more_than_one_unit(dtype):
    """4096 units for at most 2048 workgroups: complex64 n = 23, complex128 n = 22, batch 1."""
    u = unit_bits(dtype)
    n = u + 12
    x = random_state(1, n, 5, dtype)
    check(x, random_bijection(3, 61), (n - 1, u + 1, 3), (n - 2,), paths=('gather',))
    check(x, random_bijection(3, 62), (6, 0, 9), (n - 1, 2), paths=('local', 'auto'))
    check(x, random_bijection(4, 63), (u, u - 1, 0, n - 1), paths=('auto',))


@pytest.mark.parametrize('dtype', DTYPES)
def test_batch_of_three_from_a_slice_at_a_sample_offset(dtype):
    u = unit_bits(dtype)
    n = u + 1
    big = random_state(5, n, 6, dtype)
    dev = torch.from_numpy(big).cuda()
    view = dev[1:4]
    assert view.data_ptr() != dev.data_ptr() and view.is_contiguous()
    for bits, controls, paths in (((u, 2, 0), (5,), ('gather', 'auto')), ((7, 1), (u,), ('local', 'gather', 'auto')),
                                  ((u - 1, 3), (), ('local',))):
        perm = random_bijection(len(bits), 70)
        want = permute_ref(big[1:4], perm, bits, controls)
        src = torch.from_numpy(inverse_of(perm)).cuda()
        for path in paths:
            out = torch.zeros(5, 1 << n, dtype=dev.dtype, device='cuda')
            got = backend.apply_permutation(view, src, bits, controls, out=out[2:5], path=path)
            assert got.data_ptr() == out[2:5].data_ptr()
            assert same_bits(out[2:5].cpu().numpy(), want), (bits, path)
            assert not out[:2].any()                                            # nothing written before the slice
    assert same_bits(dev.cpu().numpy(), big)


@pytest.mark.parametrize('dtype', DTYPES)
def test_refusals_launch_nothing(dtype):
    u = unit_bits(dtype)
    n = u + 1
    lib = _lib.load()
    fn = getattr(lib, 'dq_apply_permutation_' + ('c128' if dtype == np.complex128 else 'c64'))
    ia = _lib.int_array
    x = torch.from_numpy(random_state(2, n, 7, dtype)).cuda()
    out = torch.zeros_like(x)
    src = torch.tensor([1, 0], dtype=torch.int32, device='cuda')

    def refused(rc, word):
        assert rc == -1 and word in lib.dq_last_error().decode(), lib.dq_last_error()

    # LOCAL with a table bit at u
    refused(fn(x.data_ptr(), out.data_ptr(), src.data_ptr(), n, ia([u]), 1, ia([]), 0, 2, _lib.PERM_LOCAL, None), 'DQ_PERM_LOCAL')
    with pytest.raises(ValueError, match='local'):
        backend.apply_permutation(x, src, (u,), out=out, path='local')
    # in and out overlap: the same buffer, and shifted by one sample
    refused(fn(x.data_ptr(), x.data_ptr(), src.data_ptr(), n, ia([0]), 1, ia([]), 0, 2, _lib.PERM_AUTO, None), 'overlap')
    refused(fn(x[0:1].data_ptr(), x[1:2].data_ptr(), src.data_ptr(), n, ia([0]), 1, ia([]), 0, 2, _lib.PERM_GATHER, None), 'overlap')
    with pytest.raises(ValueError, match='overlap'):
        backend.apply_permutation(x, src, (0,), out=x)
    torch.cuda.synchronize()
    assert not out.any()
    # the neighbouring sample is no overlap
    got = backend.apply_permutation(x[0:1], src, (0,), out=x[1:2])
    assert same_bits(got.cpu().numpy(), permute_ref(x[0:1].cpu().numpy(), [1, 0], (0,)))
