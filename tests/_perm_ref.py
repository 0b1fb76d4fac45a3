"""numpy reference of the basis-state permutation gates, written from the definition

    sub(i)    = sum_j bit_{bits[j]}(i) << (k - 1 - j)
    put(i, v) = i with the k bits at ``bits`` replaced by the bits of v        (sub(put(i, v)) = v)
    (U psi)[put(i, perm[sub(i)])] = psi[i]   where all control bits of i are 1,   (U psi)[i] = psi[i] elsewhere

in scatter form and with ``np.arange`` index arithmetic: independent of the package's gather form and of its
``_sub_index``."""

import numpy as np


def sub_of(n, bits):
    i = np.arange(1 << n, dtype=np.int64)
    k = len(bits)
    s = np.zeros_like(i)
    for j, p in enumerate(bits):
        s |= ((i >> p) & 1) << (k - 1 - j)
    return s


def put_of(n, bits, v):
    """put(i, v[i]) for every i."""
    i = np.arange(1 << n, dtype=np.int64)
    k = len(bits)
    v = np.asarray(v, dtype=np.int64)
    out = i.copy()
    for j, p in enumerate(bits):
        out = (out & ~(np.int64(1) << p)) | (((v >> (k - 1 - j)) & 1) << p)
    return out


def permute_ref(x, perm, bits, controls=()):
    """U x for x of shape (B, 2^n); bit for bit (no arithmetic)."""
    x = np.asarray(x)
    n = x.shape[-1].bit_length() - 1
    perm = np.asarray(perm, dtype=np.int64)
    i = np.arange(1 << n, dtype=np.int64)
    cmask = sum(1 << c for c in controls)
    ok = (i & cmask) == cmask
    to = put_of(n, bits, perm[sub_of(n, bits)])
    out = x.copy()
    out[:, to[ok]] = x[:, i[ok]]
    return out


def perm_matrix(perm):
    """M[perm[x], x] = 1."""
    perm = np.asarray(perm, dtype=np.int64)
    m = np.zeros((len(perm), len(perm)))
    m[perm, np.arange(len(perm))] = 1.0
    return m


def inverse_of(perm):
    perm = np.asarray(perm, dtype=np.int64)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm), dtype=np.int64)
    return inv


def random_bijection(k, seed):
    return np.random.default_rng(seed).permutation(1 << k).astype(np.int64)


def identity(k):
    return np.arange(1 << k, dtype=np.int64)


def bit_reversal(k):
    x = np.arange(1 << k, dtype=np.int64)
    r = np.zeros_like(x)
    for j in range(k):
        r |= ((x >> j) & 1) << (k - 1 - j)
    return r


def increment(k):
    return (np.arange(1 << k, dtype=np.int64) + 1) % (1 << k)


def random_state(batch, n, seed, dtype):
    """Amplitudes that are all different bit patterns, with negative zeros among them."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((batch, 1 << n)) + 1j * rng.standard_normal((batch, 1 << n))).astype(dtype)
    x[:, ::7] = x[:, ::7].real + 0j
    x[:, 3::11] = -0.0 * x[:, 3::11]
    return x


def same_bits(a, b):
    """Equality as bit patterns (distinguishes -0.0 from 0.0, which == does not)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
