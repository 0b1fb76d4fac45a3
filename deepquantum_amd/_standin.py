"""The complex128 contracts of the streaming primitives of ``backend``, in plain torch: one function per entry point, under
its name, on arguments that the entry point has already checked and normalised (``PsumTable`` and ``CollapseRec`` arrive as
objects and are used through their public attributes).  They are reached only for CPU tensors while a test double is
installed -- the package has no CPU fallback -- by name, looked up on this module at call time, under :func:`no_graph`.
The one exception is :func:`sample_indices`, which the product also uses for the diagonal of a small density matrix
(``qmath.sample``); :func:`parity` is plain integer arithmetic that the product shares.
"""

from __future__ import annotations

import math

import torch


class no_graph(torch.no_grad):
    """What a test double must not do more of than the product: the HIP entry points return tensors without an autograd
    graph and without a forward-mode tangent, so ``no_grad`` with forward-mode gradients switched off (and restored)."""

    def __enter__(self):
        self._fwd = torch._C._is_fwd_grad_enabled()
        torch._C._set_fwd_grad_enabled(False)
        super().__enter__()

    def __exit__(self, *exc):
        super().__exit__(*exc)
        torch._C._set_fwd_grad_enabled(self._fwd)


def parity(v: torch.Tensor) -> torch.Tensor:
    """popcount(v) mod 2 of every entry of an int64 tensor: 0 or 1."""
    for sh in (32, 16, 8, 4, 2, 1):
        v = v ^ (v >> sh)
    return v & 1


def sub_index(n: int, bits: list[int], controls: list[int]) -> tuple[torch.Tensor, torch.Tensor]:
    """sub(i) and the control test for every i."""
    i = torch.arange(1 << n)
    k = len(bits)
    sub = torch.zeros_like(i)
    for j, p in enumerate(bits):
        sub |= ((i >> p) & 1) << (k - 1 - j)
    cmask = sum(1 << c for c in controls)
    return sub, (i & cmask) == cmask


def pauli_gather(n: int, xmask: int, zmask: int, controls: list[int]) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Source index i ^ x, factor i^ny (-1)^popc((i ^ x) & z) and the control test for every i."""
    i = torch.arange(1 << n)
    j = i ^ xmask
    factor = (1j ** (bin(xmask & zmask).count('1') % 4)) * (1 - 2 * parity(j & zmask)).to(torch.complex128)
    cmask = sum(1 << c for c in controls)
    return j, factor, (i & cmask) == cmask


def excite_pairs(n: int, xmask: int, amask: int, zmask: int, negate: int, controls: list[int]):
    """i0, i1 and sigma of every pair."""
    i = torch.arange(1 << n)
    cmask = sum(1 << c for c in controls)
    i0 = i[(i & (xmask | cmask)) == (amask | cmask)]
    sigma = (1 - 2 * (parity(i0 & zmask) ^ negate)).to(torch.complex128)
    return i0, i0 ^ xmask, sigma


def scale_z_signs(state, zmasks, coef, n):
    i = torch.arange(1 << n)
    w = torch.zeros(state.shape[0], 1 << n, dtype=torch.float64)
    for k, z in enumerate(zmasks):
        w += coef[:, k : k + 1].to(torch.float64) * (1 - 2 * parity(i & int(z))).to(torch.float64)
    return (state * w.to(state.real.dtype)).contiguous()


def sample_indices(probs_or_state: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """The contract of ``backend.sample_indices``, and the sampler of the (small) diagonal of a density matrix: float64
    ``cumsum`` + ``searchsorted(right=True)``, then the clamp onto the last entry of non-zero probability.  A real input is
    taken as the probabilities, a complex one as amplitudes."""
    if probs_or_state.is_complex():
        p = probs_or_state.real.to(torch.float64) ** 2 + probs_or_state.imag.to(torch.float64) ** 2
    else:
        p = probs_or_state.to(torch.float64)
    c = torch.cumsum(p, dim=-1)
    idx = torch.searchsorted(c, (u * c[:, -1:]).contiguous(), right=True)
    # the last index of non-zero probability == the number of entries below the total: nothing beyond it is returned
    last = (c < c[:, -1:]).sum(-1, keepdim=True)
    return torch.minimum(idx, last)


def apply_diag(state, diag, n, bits, controls, out):
    k = len(bits)
    sub, ok = sub_index(n, bits, controls)
    f = diag.reshape(-1, 1 << k).to(torch.complex128)[:, sub]
    out.copy_(torch.where(ok, f * state.to(torch.complex128), state.to(torch.complex128)).to(state.dtype))
    return out


def apply_cost(state, cost, par, n, bits, controls, op, out):
    sub, ok = sub_index(n, bits, controls)
    c = cost.to(torch.float64)[sub]
    x = state.to(torch.complex128)
    if op == 'phase':
        y = torch.where(ok, torch.exp(-1j * par.to(torch.float64).reshape(-1, 1) * c) * x, x)
    else:
        y = torch.where(ok, par.to(torch.complex128).reshape(-1, 1) * c * x, torch.zeros_like(x))
    out.copy_(y.to(state.dtype))
    return out


def cost_cross(bra, ket, cost, n, bits, controls):
    sub, ok = sub_index(n, bits, controls)
    w = cost.to(torch.float64)[sub] * ok
    return (w * bra.to(torch.complex128).conj() * ket.to(torch.complex128)).sum(dim=-1)


def cost_hist(bra, ket, bins, nbins, n, bits, controls):
    sub, ok = sub_index(n, bits, controls)
    terms = ok * bra.to(torch.complex128).conj() * ket.to(torch.complex128)
    out = torch.zeros(ket.shape[0], nbins, dtype=torch.complex128)
    return out.index_add_(1, bins.to(torch.int64)[sub], terms)


def apply_binned(state, g, bins, n, bits, controls, out):
    sub, ok = sub_index(n, bits, controls)
    x = state.to(torch.complex128)
    f = g.to(torch.complex128)[:, bins.to(torch.int64)[sub]]
    out.copy_(torch.where(ok, f * x, torch.zeros_like(x)).to(state.dtype))
    return out


def apply_pauli_axpby(state, xmask, zmask, a, c, n, controls, mode, out):
    j, factor, ok = pauli_gather(n, xmask, zmask, controls)
    x = state.to(torch.complex128)
    y = a.reshape(-1, 1) * x + c.reshape(-1, 1) * factor * x[:, j]
    out.copy_(torch.where(ok, y, x if mode == 'gate' else torch.zeros_like(x)).to(state.dtype))
    return out


def pauli_cross(bra, ket, xmask, zmask, n, controls):
    j, factor, ok = pauli_gather(n, xmask, zmask, controls)
    return (ok * bra.to(torch.complex128).conj() * factor * ket.to(torch.complex128)[:, j]).sum(dim=-1)


def apply_permutation(state, src, n, bits, controls, out):
    k = len(bits)
    sub, ok = sub_index(n, bits, controls)
    v = src.to(torch.int64)[sub] & ((1 << k) - 1)
    i = torch.arange(1 << n)
    index = i & ~sum(1 << p for p in bits)
    for j, p in enumerate(bits):
        index = index | (((v >> (k - 1 - j)) & 1) << p)
    out.copy_(state[:, torch.where(ok, index, i)])
    return out


def apply_select_pauli(state, words, n, bits, controls, out):
    sub, ok = sub_index(n, bits, controls)
    i = torch.arange(1 << n)
    free = ((1 << n) - 1) & ~sum(1 << p for p in [*bits, *controls])
    w0, z = words[sub, 0], words[sub, 1]
    j = i ^ (w0 & free)
    q = torch.where(ok, ((w0 >> 62) + 2 * parity(j & z)) & 3, 0)
    factor = torch.tensor([1, 1j, -1, -1j], dtype=state.dtype)[q]
    out.copy_(state[:, torch.where(ok, j, i)] * factor)
    return out


def apply_qft(state, n, bits, inverse, swaps, out):
    m = len(bits)
    rest = [p for p in range(n - 1, -1, -1) if p not in bits]
    axis = lambda p: 1 + (n - 1 - p)                    # index bit p as an axis of the (B, 2, .., 2) view
    x = state.to(torch.complex128).reshape(-1, *([2] * n))
    order = [0] + [axis(p) for p in rest] + [axis(p) for p in bits]
    x = x.permute(order).reshape(state.shape[0], 1 << (n - m), *([2] * m))
    flip = lambda t: t.permute([0, 1] + list(range(m + 1, 1, -1)))
    if not swaps and inverse:
        x = flip(x)
    x = x.reshape(state.shape[0], 1 << (n - m), 1 << m)
    x = torch.fft.fft(x, dim=-1, norm='ortho') if inverse else torch.fft.ifft(x, dim=-1, norm='ortho')
    x = x.reshape(state.shape[0], 1 << (n - m), *([2] * m))
    if not swaps and not inverse:
        x = flip(x)
    x = x.reshape(state.shape[0], *([2] * n))
    back = [0] * (n + 1)
    for at, ax in enumerate(order):
        back[ax] = at
    out.copy_(x.permute(back).reshape(state.shape).to(state.dtype))
    return out


def apply_mux(state, table, kind, n, target, bits, controls, dagger, out):
    sub, ok = sub_index(n, bits, controls)
    if kind == 'ry':
        c, s = table[:, 0].to(torch.complex128), table[:, 1].to(torch.complex128)
        m = torch.stack([torch.stack([c, -s], -1), torch.stack([s, c], -1)], -2)
    else:
        m = table.to(torch.complex128)
    if dagger:
        m = m.mH.resolve_conj()
    m = m[sub]                                          # (2^n, 2, 2)
    i = torch.arange(1 << n)
    x = state.to(torch.complex128)
    x0, x1 = x[:, i & ~(1 << target)], x[:, i | (1 << target)]
    t = (i >> target) & 1
    row = m[i, t]                                       # (2^n, 2): the row of M that makes amplitude i
    out.copy_(torch.where(ok, row[:, 0] * x0 + row[:, 1] * x1, x).to(state.dtype))
    return out


def mux_cross(bra, ket, axis, n, target, bits, controls):
    sub, ok = sub_index(n, bits, controls)
    i = torch.arange(1 << n)
    v = ket.to(torch.complex128)
    t = (i >> target) & 1
    if axis in 'xy':
        v = v[:, i ^ (1 << target)]
    if axis == 'y':
        v = v * (1j * (2 * t - 1)).to(torch.complex128)             # (Y v)_0 = -i v_1, (Y v)_1 = i v_0
    elif axis == 'z':
        v = v * (1 - 2 * t).to(torch.complex128)
    terms = torch.where(ok, bra.to(torch.complex128).conj() * v, torch.zeros((), dtype=torch.complex128))
    out = torch.zeros(ket.shape[0], 1 << len(bits), dtype=torch.complex128)
    return out.index_add_(1, sub, terms)


def apply_excite_axpby(state, out, a, c, n, xmask, amask, zmask, negate, controls):
    """The pairs only: ``out`` arrives filled with what lies outside them."""
    i0, i1, sigma = excite_pairs(n, xmask, amask, zmask, negate, controls)
    x0, x1 = state[:, i0].to(torch.complex128), state[:, i1].to(torch.complex128)
    out[:, i0] = (a.reshape(-1, 1) * x0 - c.reshape(-1, 1) * sigma * x1).to(state.dtype)
    out[:, i1] = (a.reshape(-1, 1) * x1 + c.reshape(-1, 1) * sigma * x0).to(state.dtype)
    return out


def excite_cross(bra, ket, n, xmask, amask, zmask, negate, controls):
    i0, i1, sigma = excite_pairs(n, xmask, amask, zmask, negate, controls)
    u, v = bra.to(torch.complex128).conj(), ket.to(torch.complex128)
    return (sigma * (u[:, i1] * v[:, i0] - u[:, i0] * v[:, i1])).sum(dim=-1)


def psum_apply(x: torch.Tensor, table) -> torch.Tensor:
    """H x in complex128, group by group."""
    xmasks, bounds, zmasks, weights = (t.tolist() for t in table.on('cpu'))
    j = torch.arange(x.shape[-1])
    y = torch.zeros_like(x)
    for g, xmask in enumerate(xmasks):
        w = torch.zeros(x.shape[-1], dtype=torch.complex128)
        for t in range(bounds[2 * g], bounds[2 * g + 2]):
            w += (weights[t] if t < bounds[2 * g + 1] else 1j * weights[t]) * (1 - 2 * parity(j & zmasks[t])).to(torch.complex128)
        y += (w * x)[:, j ^ xmask]
    return y


def apply_psum_axpby(state, table, a, c, out):
    x = state.to(torch.complex128)
    return out.copy_((a.reshape(-1, 1) * x + c.reshape(-1, 1) * psum_apply(x, table)).to(state.dtype))


def psum_cross(bra, ket, table):
    return (bra.to(torch.complex128).conj() * psum_apply(ket.to(torch.complex128), table)).sum(dim=-1)


def pauli_terms_cross(bra: torch.Tensor, ket: torch.Tensor, table) -> torch.Tensor:
    """What ``dq_pauli_terms_cross_*`` leaves for ``table`` (one piece of at most ``pauli_terms_max()`` terms)."""
    xmasks, bounds, zmasks, weights = (t.tolist() for t in table.on('cpu'))
    u, v = bra.to(torch.complex128).conj(), ket.to(torch.complex128)
    i = torch.arange(v.shape[-1])
    out = torch.empty(v.shape[0], table.nterms, dtype=torch.complex128)
    for g, x in enumerate(xmasks):
        p = u * v[:, i ^ x]
        for t in range(bounds[2 * g], bounds[2 * g + 2]):
            c = math.copysign(1.0, weights[t]) * (1j if t >= bounds[2 * g + 1] else 1.0)
            out[:, t] = c * (p * (1 - 2 * parity((i ^ x) & zmasks[t])).to(torch.complex128)).sum(dim=-1)
    return out


def psum_evolve(state, table, coefs, order, a, b, out):
    """The Chebyshev recurrence of ``apply_psum_evolve`` for ``order >= 1``: ``coefs`` (B, order + 1) from its plan, the
    spectrum of H inside [b - a, b + a]."""
    x = state.to(torch.complex128)
    c = torch.tensor(coefs, dtype=torch.complex128)             # (B, K + 1)
    prev, cur = x, (psum_apply(x, table) - b * x) / a
    acc = c[:, 0:1] * prev + c[:, 1:2] * cur
    for k in range(2, order + 1):
        prev, cur = cur, (2.0 / a) * psum_apply(cur, table) - (2.0 * b / a) * cur - prev
        acc = acc + c[:, k:k + 1] * cur
    return out.copy_(acc.to(state.dtype))


class Lanczos:
    """The recurrence of ``psum_lanczos`` in complex128 on the host, sample by sample, with the methods of its device
    engine: every sum is taken over one sample's own 1-D tensors, so that a sample's record does not depend on its batch."""

    def __init__(self, table, start: torch.Tensor, n: int, acc):
        self.table, self.acc, self.batch = table, acc, start.shape[0]
        self.cur = [start[b].to(torch.complex128) for b in range(self.batch)]
        self.prev = [torch.zeros_like(x) for x in self.cur]
        self.norm2 = [float((x.real * x.real + x.imag * x.imag).sum()) for x in self.cur]

    @staticmethod
    def sums(x, y):
        return float((x.real * y.real + x.imag * y.imag).sum()), float((y.real * y.real + y.imag * y.imag).sum())

    def step(self, rows, read=True):
        if isinstance(rows, torch.Tensor):
            rows = rows.tolist()
        self.w, out = [], []
        for b, (alpha, beta, gamma) in enumerate(rows):
            hx = psum_apply(self.cur[b].reshape(1, -1), self.table)[0] if alpha != 0.0 else torch.zeros_like(self.cur[b])
            u = alpha * hx + beta * self.cur[b] + gamma * self.prev[b]
            self.w.append(u)
            out.append(list(self.sums(self.cur[b], u)))
        return out

    def finish(self, rows, read=True):
        if isinstance(rows, torch.Tensor):
            rows = rows.tolist()
        out = []
        for b, (e, d) in enumerate(rows):
            self.w[b] = self.w[b] + e * self.cur[b]
            if self.acc is not None:
                self.acc[b] += d * self.cur[b]
            out.append(list(self.sums(self.cur[b], self.w[b]))[::-1])
        self.cur, self.prev = self.w, self.cur
        return out

    def last(self, rows):
        if isinstance(rows, torch.Tensor):
            rows = rows.tolist()
        for b, (_e, d) in enumerate(rows):
            self.acc[b] += d * self.cur[b]


def gram(bra, ket):
    g = bra.to(torch.complex128).conj() @ ket.to(torch.complex128).T
    if bra.data_ptr() == ket.data_ptr() and bra.shape == ket.shape:      # the self-Gram, as the kernel leaves it
        up = torch.triu(g, 1)
        g = up + up.mH + torch.diag(g.diagonal().real).to(torch.complex128)
    return g.resolve_conj()


def combine(states, coef, out):
    return out.copy_((coef @ states.to(torch.complex128)).to(states.dtype))


def measure_draw(probs, u, forced, fx, fz, rec):
    draw = sample_indices(probs, (torch.zeros_like(probs[:, 0]) if u is None else u)[:, None])[:, 0]
    want = torch.full_like(draw, -1) if forced is None else forced
    o = torch.where(want >= 0, want & (probs.shape[1] - 1), draw)
    po = torch.gather(probs, 1, o[:, None])[:, 0]
    total = probs.sum(-1)
    live = (po > 0) & (total > 0) & (want < probs.shape[1])
    one = torch.ones_like(po)
    rec.data[:, 0] = o
    if fx is not None:
        rec.data[:, 1] = fx[o]
    if fz is not None:
        rec.data[:, 2] = fz[o]
    rec.scale.copy_(torch.where(live, torch.where(live, po, one) ** -0.5, 0 * one))
    rec.prob.copy_(torch.where(live, po / torch.where(total > 0, total, one), 0 * one))
    return rec


def collapse(state, n, bits, rec, layout, transpose, out):
    """The four maps of ``backend.collapse`` as they are defined."""
    k = len(bits)
    kept = [p for p in range(n - 1, -1, -1) if p not in bits]           # ext(): the kept positions, high to low
    full = (1 << n) - 1
    meas = sum(1 << p for p in bits)
    o, s = rec.outcome[:, None], rec.scale[:, None]
    x = (rec.xmask[:, None] & full) if rec.has_x else torch.zeros_like(o)
    z = rec.zmask[:, None] & full
    idx = torch.arange(1 << n, device=state.device)[None]

    def sub(i, positions):
        r = torch.zeros_like(i)
        for j, p in enumerate(positions):
            r |= ((i >> p) & 1) << (len(positions) - 1 - j)
        return r

    wide = state.to(torch.complex128)
    if layout == 'full':
        src = idx ^ x
        at = idx if transpose else src                                  # the index of the input basis that P and Z see
        val = torch.where(sub(at, bits) == o, (1 - 2 * parity(at & z)) * s * torch.gather(wide, 1, src), 0)
    elif transpose:
        val = torch.where(sub(idx, bits) == o, (1 - 2 * parity(idx & z)) * s * torch.gather(wide, 1, sub(idx ^ x, kept)), 0)
    else:
        keep = sub(idx, bits) == o                                      # (B, 2^n): 2^(n-k) kept indices per sample, ascending
        i = idx.expand(state.shape[0], -1)[keep].reshape(state.shape[0], -1)
        t = sub(i ^ (x & ~meas), kept)
        val = torch.zeros(state.shape[0], 1 << (n - k), dtype=torch.complex128, device=state.device)
        val.scatter_(1, t, (1 - 2 * parity(i & z)) * s * torch.gather(wide, 1, i))
    out.copy_(val.to(state.dtype))
    return out


def jump_product(table, n):
    """prod_p table[b, p, bit_p(i)] for every i: float64 (B, 2^n)."""
    i = torch.arange(1 << n, device=table.device)
    w = torch.ones(table.shape[0], 1 << n, dtype=torch.float64, device=table.device)
    for p in range(n):
        w = w * table[:, p, :].to(torch.float64)[:, (i >> p) & 1]
    return w


def jump_apply(state, n, factors, xmask, phase, scale, transpose, out):
    """The two maps of ``backend.jump_apply`` as they are defined: seen from the output index q, the source is q ^ x and the
    factors belong to the source (or, transposed, to q itself)."""
    q = torch.arange(1 << n, device=state.device)[None]
    src = q ^ (xmask[:, None] & ((1 << n) - 1))
    f = jump_product(factors, n)
    f = f if transpose else torch.gather(f, 1, src)
    turn = torch.tensor([1, 1j, -1, -1j], dtype=torch.complex128, device=state.device)[(-phase if transpose else phase) & 3]
    val = (turn * scale)[:, None] * f * torch.gather(state.to(torch.complex128), 1, src)
    out.copy_(val.to(state.dtype))
    return out


def jump_cross(bra, ket, n, weights):
    return (jump_product(weights, n) * bra.to(torch.complex128).conj() * ket.to(torch.complex128)).sum(-1)
