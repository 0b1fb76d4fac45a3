"""References for the excitation gates, in numpy complex128.

* ``dense_k`` / ``dense_u``: the definition itself -- Jordan-Wigner matrices a_j = (prod_{l<j} Z_l) (x) |0><1|_j over wire
  numbers (wire 0 is the most significant index bit, |1> is occupied), E the product in the order given, K = E - E^dagger,
  U = I + sin(theta) K + (1 - cos(theta)) K^2.  For n <= 8.
* ``index_axpby`` / ``index_cross``: the pair formula over index arithmetic from a spec (xmask, amask, zmask, negate,
  controls over index BITS), for larger n.
* ``pauli_terms``: the Pauli strings a dense operator projects onto.
"""

import itertools

import numpy as np

I2 = np.eye(2)
Z = np.diag([1.0, -1.0])
LOWER = np.array([[0.0, 1.0], [0.0, 0.0]])             # |0><1|
PAULIS = {'i': I2.astype(complex), 'x': np.array([[0, 1], [1, 0]], dtype=complex),
          'y': np.array([[0, -1j], [1j, 0]]), 'z': Z.astype(complex)}


def kron_all(mats):
    out = np.ones((1, 1))
    for m in mats:
        out = np.kron(out, m)
    return out


def lower(n, j, fermionic=True):
    """a_j on n wires."""
    return kron_all([Z if (fermionic and l < j) else LOWER if l == j else I2 for l in range(n)])


def dense_k(n, create, annihilate, fermionic=True, controls=()):
    e = np.eye(1 << n)
    for j in create:
        e = e @ lower(n, j, fermionic).T
    for j in annihilate:
        e = e @ lower(n, j, fermionic)
    if controls:
        proj = kron_all([np.diag([0.0, 1.0]) if l in controls else I2 for l in range(n)])
        e = proj @ e @ proj
    return e - e.T


def dense_u(n, create, annihilate, theta, fermionic=True, controls=()):
    k = dense_k(n, create, annihilate, fermionic, controls)
    return np.eye(1 << n) + np.sin(theta) * k + (1.0 - np.cos(theta)) * (k @ k)


def pairs(n, spec):
    """i0, i1, sigma of every pair of ``spec = (xmask, amask, zmask, negate[, controls])`` (controls: index bits)."""
    xmask, amask, zmask, negate = spec[:4]
    cmask = sum(1 << c for c in (spec[4] if len(spec) == 5 else ()))
    i = np.arange(1 << n, dtype=np.int64)
    i0 = i[(i & (xmask | cmask)) == (amask | cmask)]
    par = i0 & zmask
    for sh in (32, 16, 8, 4, 2, 1):
        par = par ^ (par >> sh)
    return i0, i0 ^ xmask, 1.0 - 2.0 * ((par & 1) ^ negate)


def index_k(n, spec):
    """K as a dense matrix, from the pair formula."""
    i0, i1, sigma = pairs(n, spec)
    k = np.zeros((1 << n, 1 << n))
    k[i1, i0] = sigma
    k[i0, i1] = -sigma
    return k


def index_axpby(x, spec, a, c, mode='gate'):
    """a x + c K x on the pairs; elsewhere x ('gate') or 0 ('map').  x: (B, 2^n), a and c: scalars or (B,)."""
    x = np.asarray(x, dtype=np.complex128)
    n = x.shape[1].bit_length() - 1
    i0, i1, sigma = pairs(n, spec)
    a = np.broadcast_to(np.asarray(a, dtype=np.complex128).reshape(-1, 1), (x.shape[0], 1))
    c = np.broadcast_to(np.asarray(c, dtype=np.complex128).reshape(-1, 1), (x.shape[0], 1))
    y = x.copy() if mode == 'gate' else np.zeros_like(x)
    y[:, i0] = a * x[:, i0] - c * sigma * x[:, i1]
    y[:, i1] = a * x[:, i1] + c * sigma * x[:, i0]
    return y


def index_rot(x, spec, theta):
    theta = np.asarray(theta, dtype=np.float64)
    return index_axpby(x, spec, np.cos(theta), np.sin(theta), 'gate')


def index_cross(bra, ket, spec):
    bra, ket = np.asarray(bra, dtype=np.complex128), np.asarray(ket, dtype=np.complex128)
    n = ket.shape[1].bit_length() - 1
    i0, i1, sigma = pairs(n, spec)
    return (sigma * (bra[:, i1].conj() * ket[:, i0] - bra[:, i0].conj() * ket[:, i1])).sum(axis=1)


def outside(n, spec):
    """The indices that belong to no pair."""
    i0, i1, _ = pairs(n, spec)
    keep = np.ones(1 << n, dtype=bool)
    keep[i0] = keep[i1] = False
    return np.nonzero(keep)[0]


def pauli_terms(op, n, wires=None, tol=1e-12):
    """[(coefficient, letters)] of the Pauli strings on ``wires`` (all by default; the operator must be the identity
    elsewhere) with a non-zero coefficient tr(P op) / 2^n."""
    wires = list(range(n)) if wires is None else list(wires)
    terms = []
    for letters in itertools.product('ixyz', repeat=len(wires)):
        where = dict(zip(wires, letters))
        p = kron_all([PAULIS[where.get(l, 'i')] for l in range(n)])
        coef = np.vdot(p, op) / (1 << n)                # tr(P^dagger op) / 2^n
        if abs(coef) > tol:
            terms.append((coef, ''.join(letters)))
    return terms


def random_state(batch, n, seed, dtype=np.complex128):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((batch, 1 << n)) + 1j * rng.standard_normal((batch, 1 << n))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(dtype)
