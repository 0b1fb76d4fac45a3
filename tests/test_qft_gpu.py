"""dq_apply_qft_* on the GPU, path by path, against the numpy definition (``_qft_ref``) at the project's parity bars:
1e-4 (complex64) / 1e-10 (complex128) of the largest reference amplitude.  T = ``dq_qft_tile_bits`` and the line bits L
(a 128-byte line: 4 / 3) shape the cases; the stage count of each is checked against ``dq_qft_passes``."""

import numpy as np
import pytest
import torch

from deepquantum_amd import _lib, backend
from _qft_ref import qft_ref, random_state

pytestmark = pytest.mark.gpu

BAR = {np.complex64: 1e-4, np.complex128: 1e-10}


def shuffled(seq, seed):
    return [int(v) for v in np.random.default_rng(seed).permutation(list(seq))]


# name -> (T, L) -> (n, bits, stages); a group holds T wires less the line bits it misses
CASES = {
    'hadamard': lambda T, L: (5, [2], 1),
    'hadamard-bit0-n1': lambda T, L: (1, [0], 1),
    'two-wires-spectators-between': lambda T, L: (5, [3, 0], 1),
    'all-n2': lambda T, L: (2, [0, 1], 1),
    'all-n3-shuffled': lambda T, L: (3, [1, 2, 0], 1),
    'all-n4': lambda T, L: (4, [3, 2, 1, 0], 1),
    'all-n5-shuffled': lambda T, L: (5, [2, 4, 0, 3, 1], 1),
    'bottom-at-capacity': lambda T, L: (T + 2, list(range(T - 1, -1, -1)), 1),
    'bottom-one-below-capacity': lambda T, L: (T + 2, list(range(T - 2, -1, -1)), 1),
    'above-the-line-with-riders': lambda T, L: (T + 3, list(range(T + 2, L + 2, -1)), 1),
    'straddling-the-line': lambda T, L: (T + 2, list(range(L + 5, L - 3, -1)), 1),
    'scattered-shuffled': lambda T, L: (T + 4, [T + 3, 2, 9, 5, T + 1, 0, 7], 1),
    'capacity-plus-one': lambda T, L: (T + 2, list(range(T + 1)), 2),
    # Two full groups of T - L shuffled wires above the line, one more such wire (a line bit there would still fit the second
    # group), then the line bits: riders that are later wires of the list.  A full group has T - L wires above the line
    # whatever it covers of the line, so three stages need 2 (T - L) + 1 + L index bits: n = 21 (complex64) / 20.
    'three-stages': lambda T, L: (2 * T - L + 1, shuffled(range(L, 2 * T - L + 1), 5) + shuffled(range(L), 6), 3),
}
SWAPS = ('all-n5-shuffled', 'scattered-shuffled', 'capacity-plus-one', 'three-stages')


def geometry(dtype, name):
    c128 = int(dtype == np.complex128)
    lib = _lib.load()
    n, bits, stages = CASES[name](lib.dq_qft_tile_bits(c128), 3 if c128 else 4)
    assert n <= 21 and lib.dq_qft_passes(n, _lib.int_array(bits), len(bits), c128) == stages
    return n, bits


def close(got, want, dtype):
    err = np.abs(got.cpu().numpy() - want).max() / np.abs(want).max()
    assert err < BAR[dtype], err


@pytest.mark.parametrize('name', CASES)
@pytest.mark.parametrize('dtype', [np.complex64, np.complex128], ids=['c64', 'c128'])
def test_swap_free_transform(dtype, name):
    n, bits = geometry(dtype, name)
    x = random_state(np.random.default_rng(len(name) + n), 3, n, dtype)
    dev = torch.from_numpy(x).cuda()
    fwd = backend.apply_qft(dev, bits)
    inv = backend.apply_qft(dev, bits, inverse=True)
    assert np.array_equal(dev.cpu().numpy(), x)                           # out of place: the input is left alone
    close(fwd, qft_ref(x, bits, swaps=False), dtype)
    close(inv, qft_ref(x, bits, inverse=True, swaps=False), dtype)
    close(backend.apply_qft(fwd, bits, inverse=True), x.astype(np.complex128), dtype)
    for inverse, want in ((False, fwd), (True, inv)):
        buf = dev.clone()
        assert backend.apply_qft(buf, bits, inverse=inverse, out=buf) is buf and torch.equal(buf, want)


@pytest.mark.parametrize('name', SWAPS)
@pytest.mark.parametrize('dtype', [np.complex64, np.complex128], ids=['c64', 'c128'])
def test_swap_form(dtype, name):
    """One stage: the reversal is the store addressing of the kernel; more: one ``permute_bits`` pass."""
    n, bits = geometry(dtype, name)
    x = random_state(np.random.default_rng(len(name)), 3, n, dtype)
    dev = torch.from_numpy(x).cuda()
    fwd = backend.apply_qft(dev, bits, swaps=True)
    close(fwd, qft_ref(x, bits), dtype)
    close(backend.apply_qft(dev, bits, inverse=True, swaps=True), qft_ref(x, bits, inverse=True), dtype)
    close(backend.apply_qft(fwd, bits, inverse=True, swaps=True, out=fwd), x.astype(np.complex128), dtype)
