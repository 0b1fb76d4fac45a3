"""numpy complex128 reference of the per-string values ``<bra|P_t|ket>``, straight from the masks: with ny = popc(x & z),
``(P psi)[i] = i^ny (-1)^popc((i ^ x) & z) psi[i ^ x]``.  Shared by the test_terms_* files."""

import numpy as np


def term_overlaps_ref(bra, ket, terms):
    """``(val, mag)`` for (B, 2**n) states and terms ``(h, xmask, zmask)`` (h is not used): val[b, t] = <bra_b|P_t|ket_b> and
    mag[b, t, :] = (sum_i, max_i) of |bra_i| |ket_{i ^ x_t}|, what an error bound and its sharpness are made of."""
    bra, ket = np.asarray(bra, dtype=np.complex128), np.asarray(ket, dtype=np.complex128)
    i = np.arange(bra.shape[-1])
    parity = np.zeros_like(i)
    for sh in range(int(bra.shape[-1]).bit_length()):
        parity ^= i >> sh & 1
    val = np.empty((bra.shape[0], len(terms)), dtype=np.complex128)
    mag = np.empty((bra.shape[0], len(terms), 2))
    last = None
    for t, (_, x, z) in enumerate(terms):
        if x != last:
            p, last = np.conj(bra) * ket[:, i ^ x], x
            m = np.abs(bra) * np.abs(ket[:, i ^ x])
            msum, mmax = m.sum(-1), m.max(-1)
        val[:, t] = 1j ** (bin(x & z).count('1') % 4) * (p * (1 - 2 * parity[(i ^ x) & z])).sum(-1)
        mag[:, t, 0], mag[:, t, 1] = msum, mmax
    return val, mag
