"""numpy complex128 reference of the multiplexed one-qubit gates, written from the definition

    sub(i) = sum_j bit_{bits[j]}(i) << (k - 1 - j)
    for every pair i0 (target bit 0), i1 = i0 | 1 << target whose control bits are all 1:
        (out[i0], out[i1]) = M[sub(i0)] (in[i0], in[i1])
    every other amplitude: out[i] = in[i]

with ``np.arange`` index arithmetic over the full n-bit amplitude index: it never forms the (n - 1)-bit pair index of the
kernel and of nothing else in the package."""

import numpy as np


def sub_of(n, bits):
    i = np.arange(1 << n, dtype=np.int64)
    k = len(bits)
    s = np.zeros_like(i)
    for j, p in enumerate(bits):
        s |= ((i >> p) & 1) << (k - 1 - j)
    return s


def ry_blocks(cs):
    """(2^k, 2) rows (c, s) -> (2^k, 2, 2) blocks [[c, -s], [s, c]], complex128."""
    cs = np.asarray(cs, dtype=np.float64)
    m = np.zeros((cs.shape[0], 2, 2), dtype=np.complex128)
    m[:, 0, 0] = cs[:, 0]
    m[:, 0, 1] = -cs[:, 1]
    m[:, 1, 0] = cs[:, 1]
    m[:, 1, 1] = cs[:, 0]
    return m


def mux_ref(x, blocks, target, bits, controls=(), dagger=False):
    """M x for x of shape (B, 2^n) and ``blocks`` of shape (2^k, 2, 2); complex128 whatever x is."""
    x = np.asarray(x).astype(np.complex128)
    m = np.asarray(blocks).astype(np.complex128)
    if dagger:
        m = np.conj(np.swapaxes(m, -1, -2))
    n = x.shape[-1].bit_length() - 1
    i = np.arange(1 << n, dtype=np.int64)
    cmask = sum(1 << c for c in controls)
    i0 = i[((i & cmask) == cmask) & (((i >> target) & 1) == 0)]
    i1 = i0 | (1 << target)
    s = sub_of(n, bits)[i0]
    out = x.copy()
    out[:, i0] = m[s, 0, 0] * x[:, i0] + m[s, 0, 1] * x[:, i1]
    out[:, i1] = m[s, 1, 0] * x[:, i0] + m[s, 1, 1] * x[:, i1]
    return out


def outside(n, controls):
    """The amplitude indices with a control bit at 0."""
    i = np.arange(1 << n, dtype=np.int64)
    cmask = sum(1 << c for c in controls)
    return i[(i & cmask) != cmask]


def block_diag(blocks):
    """The dense 2^(k+1) x 2^(k+1) matrix of the multiplexer on (select wires, target)."""
    blocks = np.asarray(blocks)
    d = blocks.shape[0]
    m = np.zeros((2 * d, 2 * d), dtype=blocks.dtype)
    for s in range(d):
        m[2 * s:2 * s + 2, 2 * s:2 * s + 2] = blocks[s]
    return m


def random_unitaries(k, seed):
    """2^k Haar-ish 2x2 unitaries (QR of a Gaussian matrix), complex128."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((1 << k, 2, 2)) + 1j * rng.standard_normal((1 << k, 2, 2))
    q, _ = np.linalg.qr(a)
    return q.astype(np.complex128)


def random_cs(k, seed):
    """2^k rows (cos, sin) of random half angles, float64."""
    t = np.random.default_rng(seed).uniform(-np.pi, np.pi, 1 << k)
    return np.stack([np.cos(t), np.sin(t)], axis=-1)


U_ENTRIES = np.array([0, 1, -1, 1j, -1j, 1 + 1j, 1 - 1j, 2], dtype=np.complex128)
CS_ROWS = np.array([(1, 0), (0, 1), (0, -1), (-1, 0), (2, -3)], dtype=np.float64)


def exact_unitaries(k, seed):
    """2^k blocks (not unitary, on purpose) with entries from {0, +-1, +-i, 1 +- i, 2}: exact in float32."""
    rng = np.random.default_rng(seed)
    return U_ENTRIES[rng.integers(0, len(U_ENTRIES), size=(1 << k, 2, 2))]


def exact_cs(k, seed):
    """2^k rows (c, s) from {(1, 0), (0, 1), (0, -1), (-1, 0), (2, -3)}: exact in float32."""
    rng = np.random.default_rng(seed)
    return CS_ROWS[rng.integers(0, len(CS_ROWS), size=1 << k)]


def gaussian_integer_state(batch, n, seed, dtype):
    """Amplitudes a + bi with small integers a, b (|a|, |b| <= 8), zeros of both signs among them: sums of a few products
    with the exact tables stay far inside the 24 bits of a float32 significand."""
    rng = np.random.default_rng(seed)
    re = rng.integers(-8, 9, size=(batch, 1 << n))
    im = rng.integers(-8, 9, size=(batch, 1 << n))
    x = (re + 1j * im).astype(dtype)
    parts = x.view(x.real.dtype)
    parts[:, 5::13][parts[:, 5::13] == 0] = -0.0        # negative zeros among the zeros
    return x


def random_state(batch, n, seed, dtype):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((batch, 1 << n)) + 1j * rng.standard_normal((batch, 1 << n))).astype(dtype)


def same_bits(a, b):
    """Equality as bit patterns (distinguishes -0.0 from 0.0, which == does not)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
