"""The per-string kernel on the MI355X (dq_pauli_terms_cross_*) through ``backend.pauli_terms_cross`` against the numpy
complex128 reference of tests/_terms_ref.py.  A unit is 2^s amplitudes, s = 11 (complex64) / 10 (complex128): amplitude bit 0
is the element of a complex64 vector, then six lane bits, two wave bits and two unroll bits (one lower in complex128).

Integer rows: states of Gaussian integers in [-4, 4] make every product and partial sum an integer below 2^53, so the
result must EQUAL the reference.  Gaussian rows: |out - ref| <= (2^n + 4) 2^-53 sum_i |bra_i| |ket_{i ^ x}| -- any-order
summation of 2^n terms in double plus the rounding of a complex128 product; the reference with its largest summand's sign
flipped lies 2 max_i |bra_i| |ket_{i ^ x}| away, and the test checks that this is outside the bound."""

import numpy as np
import pytest
import torch

import deepquantum_amd as dq
from deepquantum_amd import backend, qmath
from _psum_ref import hamiltonian_of
from _terms_ref import term_overlaps_ref

pytestmark = pytest.mark.gpu
DTYPES = [pytest.param(torch.complex64, id='c64'), pytest.param(torch.complex128, id='c128')]


def sbits(dtype):
    return 11 if dtype == torch.complex64 else 10


def states(batch, n, dtype, seed, integers):
    rng = np.random.default_rng(seed)
    if integers:
        x = rng.integers(-4, 5, (batch, 1 << n)) + 1j * rng.integers(-4, 5, (batch, 1 << n))
    else:
        x = rng.standard_normal((batch, 1 << n)) + 1j * rng.standard_normal((batch, 1 << n))
    return torch.from_numpy(x).to(dtype).cuda()


def pauli_sum(n, pairs):
    """The PauliSum of the distinct (xmask, zmask) pairs with coefficients of alternating sign."""
    pairs = list(dict.fromkeys(pairs))
    return dq.PauliSum(hamiltonian_of(n, [((-1.0) ** k * (1 + k % 3), x, z) for k, (x, z) in enumerate(pairs)]), n)


def check(H, bra, ket, integers):
    got = backend.pauli_terms_cross(bra, ket, H.table).cpu().numpy()
    want, mag = term_overlaps_ref(bra.cpu().numpy(), ket.cpu().numpy(), H.terms)
    assert got.shape == want.shape
    if integers:
        bad = np.argwhere(got != want)
        assert bad.size == 0, (bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
        return
    bound = ((1 << H.nqubit) + 4) * 2.0 ** -53 * mag[..., 0]
    print('largest error / bound:', (np.abs(got - want) / bound).max(), 'flip / bound:', (2 * mag[..., 1] / bound).min())
    assert (2 * mag[..., 1] > bound).all()            # the bound is sharp enough to see one wrong sign
    assert (np.abs(got - want) <= bound).all()


def special_masks(n):
    bits = [1 << b for b in (0, 1, 6, 7, 9, 10, 11, n - 1) if b < n]
    return list(dict.fromkeys([0, *bits, (1 << n) - 1]))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('size', ['1', '3', 's', 's+1', '13'])
def test_every_special_bit_as_flip_and_as_sign(dtype, size):
    """Flip masks and sign masks from {0, the in-vector bit, the lowest and the top lane bit, the first wave bit, the unroll
    bits, the first bit above the unit, n - 1, all ones}, every pair of them; masks of 2, 3 and 4 low bits under the
    all-ones flip give ny = 2, 3, 0 next to the single bits' ny = 1.  Batch 3 with two buffers, batch 1 with one."""
    s = sbits(dtype)
    n = {'s': s, 's+1': s + 1}.get(size) or int(size)
    masks = special_masks(n)
    ys = [((1 << n) - 1, (1 << k) - 1) for k in (2, 3, 4) if k <= n]
    H = pauli_sum(n, [(x, z) for x in masks for z in masks] + ys)
    assert {bin(x & z).count('1') % 4 for _, x, z in H.terms} == ({0, 1, 2, 3} if n >= 3 else {0, 1})
    check(H, states(3, n, dtype, 1, True), states(3, n, dtype, 2, True), True)
    psi = states(1, n, dtype, 3, True)
    check(H, psi, psi, True)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('integers', [True, False], ids=['integers', 'gaussian'])
def test_group_and_term_counts(dtype, integers):
    """40 groups of 1 and 2 terms and one of 257 (a thread owns two terms of it) at n = 13: more than one workgroup a sample."""
    n = 13
    pairs = [(5, z) for z in range(257)] + [(64 * g + 3, (g * 37) % (1 << n)) for g in range(1, 40)]
    pairs += [(64 * g + 3, 1 << (g % n)) for g in range(1, 40, 2)]
    H = pauli_sum(n, pairs)
    assert H.ngroups == 40 and H.nterms == 257 + 39 + 20
    check(H, states(3, n, dtype, 4, integers), states(3, n, dtype, 5, integers), integers)
    psi = states(1, n, dtype, 6, integers)
    check(H, psi, psi, integers)


@pytest.mark.parametrize('dtype', DTYPES)
def test_one_term_more_than_a_launch_takes(dtype):
    """A group of dq_pauli_terms_max() + 1 terms at n = 12: cut inside the group into two launches."""
    n, cap = 12, backend.pauli_terms_max()
    H = pauli_sum(n, [(0b101, z) for z in range(cap + 1)])
    assert H.ngroups == 1 and len(backend._terms_pieces(H.table, cap)) == 2
    psi = states(1, n, dtype, 7, True)
    check(H, psi, psi, True)


@pytest.mark.parametrize('dtype', DTYPES)
def test_a_workgroup_takes_a_second_unit(dtype):
    """n = s + 11: 2048 units for the 1024 workgroups of a sample.  Six terms: flips and signs at the unit's index bits."""
    s = sbits(dtype)
    n = s + 11
    top, above = 1 << (n - 1), 1 << s
    H = pauli_sum(n, [(0, top), (0, above | 1), (top | 1, 0), (top | 1, top | above), (top | 1, top | 1), (above, (1 << n) - 1)])
    psi = states(1, n, dtype, 8, True)
    check(H, psi, psi, True)


@pytest.mark.parametrize('dtype', DTYPES)
def test_bitwise_reproducible_and_independent_of_the_batch(dtype):
    n = 13
    H = pauli_sum(n, [(x, z) for x in (0, 1, 1 << 12) for z in (0, 3, 1 << 11, 1 << 7)])
    bra, ket = states(3, n, dtype, 9, False), states(3, n, dtype, 10, False)
    a, b = backend.pauli_terms_cross(bra, ket, H.table), backend.pauli_terms_cross(bra, ket, H.table)
    alone = backend.pauli_terms_cross(bra[1:2].clone(), ket[1:2].clone(), H.table)
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(b)) and torch.equal(torch.view_as_real(a[1:2]), torch.view_as_real(alone))
    # through qmath: the same bits, the real part where bra is ket, (T,) for a single state
    assert torch.equal(qmath.pauli_term_overlaps(bra, ket, n, H), a)
    e = qmath.pauli_term_expectations(ket[0], n, H)
    assert e.shape == (H.nterms,) and torch.equal(e, backend.pauli_terms_cross(ket[:1], ket[:1], H.table).real[0])
