"""numpy complex128 references of the Pauli-sum evolution (backend.apply_psum_evolve and the kernel dq_pauli_sum_cheb_step_*),
over terms ``(h, xmask, zmask)`` in the mask convention of tests/_pauli_ref.py, shared by the test_evolve_* files."""

import numpy as np

from _psum_ref import psum_apply_ref


def bessel_integral(z, kmax, npoints=4096):
    """J_0(z) .. J_kmax(z) as (1/N) sum_m cos(k tau_m - z sin tau_m) over N equispaced points of [0, 2 pi): the trapezoid
    rule of Bessel's integral, spectrally exact while N exceeds k plus the bandwidth of exp(-i z sin tau), about z."""
    tau = 2.0 * np.pi * np.arange(npoints) / npoints
    k = np.arange(kmax + 1)[:, None]
    return np.cos(k * tau - z * np.sin(tau)).mean(axis=1)


def smallest_order(values, tol):
    """The smallest K with 2 sum_{k > K} |values[k]| < tol, by suffix sums."""
    tails = 2.0 * np.concatenate([np.cumsum(np.abs(values)[::-1])[::-1][1:], [0.0]])
    return int(np.argmax(tails < tol))


def cheb_step_ref(cur, prev, acc, terms, alpha, beta, gamma, delta):
    """(next, acc + delta next) with next = alpha H cur + beta cur + gamma prev; coefficients one per sample."""
    col = lambda p: np.asarray(p).reshape(-1, 1)  # noqa: E731
    cur, prev, acc = (np.asarray(v, dtype=np.complex128) for v in (cur, prev, acc))
    nxt = col(alpha) * psum_apply_ref(cur, terms) + col(beta) * cur + col(gamma) * prev
    return nxt, acc + col(delta) * nxt


def split_constant(terms):
    """(b, a, the other terms): the coefficient of the empty string and the sum of |h| over the rest."""
    b = sum(h for h, x, z in terms if x == 0 and z == 0)
    rest = [(h, x, z) for h, x, z in terms if x or z]
    return b, sum(abs(h) for h, _, _ in rest), rest


def evolve_ref(x, terms, t, order):
    """exp(-i t H) x by the Chebyshev expansion cut after ``order``, with the Bessel values of the integral."""
    x = np.asarray(x, dtype=np.complex128)
    b, a, rest = split_constant(terms)
    z = a * abs(t)
    j = bessel_integral(z, max(order, 1))
    step = -1j if t >= 0 else 1j
    prev, cur = x, psum_apply_ref(x, rest) / a
    acc = j[0] * prev + (2 * step * j[1] * cur if order >= 1 else 0)
    for k in range(2, order + 1):
        prev, cur = cur, 2 * psum_apply_ref(cur, rest) / a - prev
        acc = acc + 2 * step ** k * j[k] * cur
    return np.exp(-1j * t * b) * acc


def product_evolution(n, u, v, c, t):
    """exp(-i t H) for H = sum_w (u_w X_w + v_w Z_w) + c as its n 2x2 factors, wire 0 first:
    exp(-i t (u X + v Z)) = cos(r t) - i sin(r t) (u X + v Z) / r, r = sqrt(u^2 + v^2)."""
    mats = []
    for w in range(n):
        r = np.hypot(u[w], v[w])
        cs, sn = np.cos(r * t), np.sin(r * t) / r
        mats.append(np.array([[cs - 1j * sn * v[w], -1j * sn * u[w]], [-1j * sn * u[w], cs + 1j * sn * v[w]]]))
    return mats, np.exp(-1j * t * c)


def apply_product(x, mats, phase):
    """The tensor product of the 2x2 ``mats`` (wire 0 = the most significant index bit) on x of shape (B, 2**n)."""
    n = len(mats)
    y = np.asarray(x, dtype=np.complex128).reshape((-1,) + (2,) * n)
    for w, m in enumerate(mats):
        y = np.moveaxis(np.tensordot(m, y, axes=([1], [w + 1])), 0, w + 1)
    return phase * y.reshape(len(x), -1)


def flip_class_terms(n, bits, nterms, rng, dyadic=False):
    """One group whose flip mask has exactly ``bits`` set, with ``nterms`` distinct sign masks (Y where they meet the flip)."""
    xmask = sum(1 << b for b in bits)
    zs = set()
    while len(zs) < min(nterms, 1 << n):
        zs.add(int(rng.integers(0, 1 << n)))
    out = []
    for z in sorted(zs):
        h = float(rng.integers(-4, 5) or 1) / 4 if dyadic else float(rng.normal())
        out.append((h, xmask, z))
    return out
