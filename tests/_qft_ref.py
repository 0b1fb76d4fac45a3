"""The quantum Fourier transform on a list of index bits in numpy complex128, from its definition: the wires' bits moved to
one axis in significance order, ``ifft(norm='ortho')`` along it (``fft`` for the inverse), the bits of the result
reversed over the list for the swap-free form."""

import numpy as np


def random_state(rng, batch, n, dtype):
    x = rng.standard_normal((batch, 1 << n)) + 1j * rng.standard_normal((batch, 1 << n))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(dtype)


def qft_ref(x, bits, inverse=False, swaps=True):
    """``bits[0]`` is the most significant bit of the transformed number; x is (batch, 2**n)."""
    batch, n, m = x.shape[0], x.shape[1].bit_length() - 1, len(bits)
    axes = [1 + (n - 1 - p) for p in bits]                  # index bit p as an axis of the (batch, 2, .., 2) view
    last = list(range(n + 1 - m, n + 1))
    y = np.moveaxis(x.astype(np.complex128).reshape([batch] + [2] * n), axes, last)
    if inverse and not swaps:
        y = np.moveaxis(y, last, last[::-1])
    shape = y.shape
    y = y.reshape(-1, 1 << m)
    y = (np.fft.fft if inverse else np.fft.ifft)(y, axis=1, norm='ortho').reshape(shape)
    if not inverse and not swaps:
        y = np.moveaxis(y, last, last[::-1])
    return np.ascontiguousarray(np.moveaxis(y, last, axes)).reshape(batch, -1)


def dft_matrix(m):
    k = np.arange(1 << m)
    return np.exp(2j * np.pi * np.outer(k, k) / (1 << m)) / np.sqrt(1 << m)
