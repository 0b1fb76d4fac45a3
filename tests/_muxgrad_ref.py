"""numpy complex128 reference of the binned multiplexer operations, written from the definition over the full n-bit
amplitude index

    G = the one-qubit Pauli sigma on bit ``target`` inside the controls, 0 elsewhere;  bin s = {i inside the controls: sub(i) = s}
    mux_axpby(x; a, c, mode)[i] = a[sub i] x[i] + c[sub i] (G x)[i] inside the controls, x[i] ('gate') / 0 ('map') elsewhere
    mux_cross(u, v)[b, s]       = sum over bin s of conj(u[b, i]) (G v[b])[i]
    mux_rot(x; theta)           = mux_axpby(x; cos(theta/2), -i sin(theta/2), 'gate')

It bins with ``np.add.at`` and never forms the (n - 1)-bit pair index of the kernels."""

import numpy as np

from _mux_ref import sub_of


def inside(n, controls):
    i = np.arange(1 << n, dtype=np.int64)
    cmask = sum(1 << c for c in controls)
    return (i & cmask) == cmask


def pauli_on(v, axis, target):
    """(sigma on bit ``target``) v for v of shape (B, 2^n), everywhere (no controls); complex128."""
    v = np.asarray(v).astype(np.complex128)
    n = v.shape[-1].bit_length() - 1
    i = np.arange(1 << n, dtype=np.int64)
    t = (i >> target) & 1
    if axis == 'i':
        return v
    if axis == 'z':
        return v * (1 - 2 * t)
    w = v[:, i ^ (1 << target)]
    return w if axis == 'x' else w * (1j * (2 * t - 1))                 # (Y v)_0 = -i v_1, (Y v)_1 = i v_0


def cross_terms(bra, ket, axis, target, controls=()):
    """conj(bra_i) (G ket)_i for every i (0 outside the controls): (B, 2^n) complex128."""
    bra = np.asarray(bra).astype(np.complex128)
    n = bra.shape[-1].bit_length() - 1
    return np.where(inside(n, controls), np.conj(bra) * pauli_on(ket, axis, target), 0)


def binned(terms, n, bits):
    """sum of ``terms`` (B, 2^n) over the amplitudes of each bin: (B, 2^k)."""
    out = np.zeros((terms.shape[0], 1 << len(bits)), dtype=terms.dtype)
    s = sub_of(n, bits)
    for b in range(terms.shape[0]):
        np.add.at(out[b], s, terms[b])
    return out


def mux_cross_ref(bra, ket, axis, target, bits, controls=()):
    n = np.asarray(ket).shape[-1].bit_length() - 1
    return binned(cross_terms(bra, ket, axis, target, controls), n, bits)


def mux_axpby_ref(x, a, c, axis, target, bits, controls=(), mode='gate'):
    x = np.asarray(x).astype(np.complex128)
    n = x.shape[-1].bit_length() - 1
    s = sub_of(n, bits)
    a = np.asarray(a, dtype=np.complex128).reshape(-1, 1 << len(bits))[:, s]
    c = np.asarray(c, dtype=np.complex128).reshape(-1, 1 << len(bits))[:, s]
    y = a * x + c * pauli_on(x, axis, target)
    return np.where(inside(n, controls), y, x if mode == 'gate' else 0)


def mux_rot_ref(x, theta, axis, target, bits, controls=()):
    half = np.asarray(theta, dtype=np.float64) / 2
    return mux_axpby_ref(x, np.cos(half), -1j * np.sin(half), axis, target, bits, controls, 'gate')


def mux_rot_grads_ref(x, theta, gy, axis, target, bits, controls=()):
    """The closed forms: gx = rot(gy; -theta), gtheta[b, s] = Im cross(gx, x)[b, s] / 2 (per sample)."""
    gx = mux_rot_ref(gy, -np.asarray(theta, dtype=np.float64), axis, target, bits, controls)
    return gx, 0.5 * mux_cross_ref(gx, x, axis, target, bits, controls).imag


def dense_mux_rot(theta, axis, n, target, bits, controls=()):
    """The dense oracle: the 2^n x 2^n matrix that is block_diag(R_axis(theta[s])) on (select bits, target) inside the
    controls and the identity elsewhere, built differentiably in torch complex128 on the CPU from a real ``theta`` (2^k,)."""
    import torch

    i = torch.arange(1 << n)
    s = torch.from_numpy(sub_of(n, bits))
    ok = torch.from_numpy(inside(n, controls))
    t = ((i >> target) & 1).to(torch.float64)
    half = theta.to(torch.float64)[s] / 2
    c, sn = torch.cos(half).to(torch.complex128), torch.sin(half).to(torch.complex128)
    one, zero = torch.ones_like(c), torch.zeros_like(c)
    if axis == 'x':
        diag, off = c, -1j * sn
    elif axis == 'y':
        diag, off = c, sn * (2 * t - 1)                 # row 0: -s, row 1: +s
    else:
        diag, off = c + 1j * sn * (2 * t - 1), zero     # exp(-i theta/2) on |0>, exp(i theta/2) on |1>
    u = torch.zeros(1 << n, 1 << n, dtype=torch.complex128)
    u = u.index_put((i, i), torch.where(ok, diag, one))
    return u.index_put((i, i ^ (1 << target)), torch.where(ok, off, zero))


def gaussian_integer_state3(batch, n, seed, dtype):
    """Amplitudes a + bi with integers a, b in [-3, 3]: every product and every sum of 2^24 of them is exact in double."""
    rng = np.random.default_rng(seed)
    re = rng.integers(-3, 4, size=(batch, 1 << n))
    im = rng.integers(-3, 4, size=(batch, 1 << n))
    return (re + 1j * im).astype(dtype)
