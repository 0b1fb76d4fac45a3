"""The numpy reference of SELECT over Pauli strings (csrc/dq_select.hip), written from the definition:

    s = sub(i),  (x, z, q) = table[s],  x &= free,  j = i ^ x,  out[b, i] = i^q (-1)^popc(j & z) in[b, j]

on the amplitudes whose control bits are all 1, a copy elsewhere.  An index gather and then a swap of re / im and sign
flips in the state's own dtype: every comparison against it is exact.  Also the helpers that build tables from strings,
independently of ``backend.SelectTable``, and the dense matrix ``sum_s |s><s| (x) c_s P_s`` from ``np.kron``.
"""

import re

import numpy as np

PAULI = {
    'i': np.eye(2, dtype=np.complex128),
    'x': np.array([[0, 1], [1, 0]], dtype=np.complex128),
    'y': np.array([[0, -1j], [1j, 0]], dtype=np.complex128),
    'z': np.array([[1, 0], [0, -1]], dtype=np.complex128),
}


def factors(string):
    """'x0y2' -> [('x', 0), ('y', 2)]"""
    return [(p.lower(), int(w)) for p, w in re.findall(r'([xyzXYZ])(\d+)', string)]


def masks(string, n, system_wires):
    """(xmask, zmask) over index bits of a string whose wire w is system_wires[w]; wire v is index bit n - 1 - v."""
    x = z = 0
    for p, w in factors(string):
        bit = 1 << (n - 1 - system_wires[w])
        x |= bit if p in 'xy' else 0
        z |= bit if p in 'yz' else 0
    return x, z


def parity(a):
    """popc(a) & 1 of uint64 values, by folding"""
    a = np.array(a, dtype=np.uint64)
    for shift in (32, 16, 8, 4, 2, 1):
        a ^= a >> np.uint64(shift)
    return (a & np.uint64(1)).astype(np.int64)


def words(entries, dagger=False, k=None):
    """The kernel's table (2^k, 2) uint64 from one (xmask, zmask, q_user) per select value (missing ones: the identity;
    ``k``: the smallest that holds them by default): the power of i in front of X^x Z^z is q_user + ny for the operator and
    ny - q_user for its adjoint (ny = popc(x & z): Y = i X Z)."""
    size = 1 << k if k is not None else 2
    while size < len(entries):
        size *= 2
    out = np.zeros((size, 2), dtype=np.uint64)
    for s, (x, z, q) in enumerate(entries):
        ny = bin(x & z).count('1')
        kq = (ny - q) % 4 if dagger else (q + ny) % 4
        out[s, 0], out[s, 1] = np.uint64(x | kq << 62), np.uint64(z)
    return out


def random_words(rng, k, positions, specials=True):
    """2^k entries whose flip and sign masks are drawn over ``positions`` (index bits), raw powers q in 0..3; with
    ``specials`` the first entries are an identity, a diagonal one (x = 0), a pure flip (z = 0) and an all-Y one."""
    size = 1 << k
    out = np.zeros((size, 2), dtype=np.uint64)
    for s in range(size):
        x = sum(1 << p for p in positions if rng.integers(2))
        z = sum(1 << p for p in positions if rng.integers(2))
        out[s, 0], out[s, 1] = np.uint64(x | int(rng.integers(4)) << 62), np.uint64(z)
    if specials:
        allbits = sum(1 << p for p in positions)
        special = [(0, 0), (int(rng.integers(4)) << 62, allbits), (allbits | 1 << 62, 0), (allbits | 3 << 62, allbits)]
        for s, (w0, w1) in enumerate(special[:size]):
            out[s, 0], out[s, 1] = np.uint64(w0), np.uint64(w1)
    return out


def random_entries(rng, nstrings, positions):
    """``nstrings`` entries (xmask, zmask, q_user) drawn over ``positions`` (index bits); the first ones are an all-Y
    string, a pure flip (z = 0), a diagonal string (x = 0) and an identity, each with its own power of i."""
    positions = list(positions)
    allbits = sum(1 << p for p in positions)
    out = [(allbits, allbits, 3), (allbits, 0, 2), (0, allbits, 1), (0, 0, 0)][:nstrings]
    while len(out) < nstrings:
        x = sum(1 << p for p in positions if rng.integers(2))
        z = sum(1 << p for p in positions if rng.integers(2))
        out.append((x, z, int(rng.integers(4))))
    return out


def sub_index(n, bits):
    i = np.arange(1 << n, dtype=np.uint64)
    k = len(bits)
    s = np.zeros_like(i)
    for j, p in enumerate(bits):
        s |= ((i >> np.uint64(p)) & np.uint64(1)) << np.uint64(k - 1 - j)
    return s


def select_ref(state, table, bits, controls=()):
    """``state``: (B, 2^n) complex64 / complex128 numpy array; ``table``: (2^k, 2) uint64.  Exact."""
    n = state.shape[-1].bit_length() - 1
    i = np.arange(1 << n, dtype=np.uint64)
    s = sub_index(n, bits).astype(np.int64)
    cmask = np.uint64(sum(1 << c for c in controls))
    smask = sum(1 << p for p in bits)
    free = np.uint64(((1 << n) - 1) & ~(smask | int(cmask)))
    ok = (i & cmask) == cmask
    w0, z = table[s, 0], table[s, 1]
    j = i ^ (w0 & free)
    q = (w0 >> np.uint64(62)).astype(np.int64)
    power = np.where(ok, (q + 2 * parity(j & z)) & 3, 0)
    g = state[:, np.where(ok, j, i).astype(np.int64)]
    swap = (power & 1).astype(bool)
    re = np.where(swap, g.imag, g.real)
    im = np.where(swap, g.real, g.imag)
    re = np.where((((power + 1) >> 1) & 1).astype(bool), -re, re)
    im = np.where((power >> 1).astype(bool), -im, im)
    out = np.empty_like(state)
    out.real = re
    out.imag = im
    return out


def dense_select(n, select_wires, system_wires, strings, phases=None, controls=()):
    """sum_s |s><s| (x) i^phases[s] P_s as a 2^n x 2^n matrix from np.kron, wire 0 the most significant bit: the strings'
    wire w is system_wires[w], select_wires[0] is the most significant bit of s, missing strings are the identity; on the
    subspace where a control wire is 0 the matrix is the identity."""
    k = len(select_wires)
    phases = [0] * len(strings) if phases is None else phases
    proj = [np.diag([1.0 + 0j, 0]), np.diag([0, 1.0 + 0j])]
    total = np.zeros((1 << n, 1 << n), dtype=np.complex128)
    for s in range(1 << k):
        ops = [PAULI['i']] * n
        for j, w in enumerate(select_wires):
            ops[w] = proj[(s >> (k - 1 - j)) & 1]
        if s < len(strings):
            for p, w in factors(strings[s]):
                ops[system_wires[w]] = PAULI[p]
        term = np.array([[1.0 + 0j]])
        for op in ops:
            term = np.kron(term, op)
        total += (1j ** (phases[s] if s < len(strings) else 0)) * term
    if controls:
        inside = np.array([[1.0 + 0j]])
        for w in range(n):
            inside = np.kron(inside, proj[1] if w in controls else PAULI['i'])
        total = inside @ total + (np.eye(1 << n) - inside)
    return total


def pauli_sum_matrix(terms, m):
    """sum_t h_t P_t on m wires from [[h, 'x0y1'], ..], wire 0 the most significant bit."""
    total = np.zeros((1 << m, 1 << m), dtype=np.complex128)
    for h, string in terms:
        ops = [PAULI['i']] * m
        for p, w in factors(string):
            ops[w] = PAULI[p]
        term = np.array([[1.0 + 0j]])
        for op in ops:
            term = np.kron(term, op)
        total += h * term
    return total


def random_state(rng, batch, n, dtype):
    real = np.float32 if dtype == np.complex64 else np.float64
    a = rng.standard_normal((batch, 1 << n)).astype(real) + 1j * rng.standard_normal((batch, 1 << n)).astype(real)
    return np.ascontiguousarray(a.astype(dtype))
