"""Plain complex128 / float64 references of the kernels, built from torch tensor operations only (index arithmetic,
gathers, reshape / permute + matmul) on whatever device the inputs live on: the large-grid tests run them on the GPU,
test_grid_paths_cpu.py checks them against the CPU oracle at small n.  None of them calls a project kernel.  (f32_chain,
the emulation of a k-ordered float32 accumulation, adds on the host with numpy: torch has no sequential float32 scan.)

The reductions return the value and S, the same sum taken over the absolute values of its terms: the scale a rounding
error of the summation is measured against."""

from __future__ import annotations

import numpy as np
import torch

C128 = torch.complex128


def parity(v: torch.Tensor) -> torch.Tensor:
    """popcount(v) & 1 of a non-negative int64 tensor."""
    for s in (32, 16, 8, 4, 2, 1):
        v = v ^ (v >> s)
    return v & 1


def z_sign(i: torch.Tensor, zmask: int) -> torch.Tensor:
    """(-1)^popcount(i & zmask) as float64."""
    return (1 - 2 * parity(i & zmask)).to(torch.float64)


def _nbits(t: torch.Tensor) -> int:
    return t.shape[-1].bit_length() - 1


def bit_view(t: torch.Tensor, special) -> tuple[torch.Tensor, dict]:
    """View (B, 2^n) as (B, d_1, .., d_m), most significant index bits first, where every bit of ``special`` has an axis of
    its own (size 2) and the runs of other bits between them share one axis.  Returns the view and {bit: axis}."""
    n = _nbits(t)
    sizes, axis_of, run = [], {}, 0
    for p in range(n - 1, -1, -1):
        if p in special:
            if run:
                sizes.append(1 << run)
                run = 0
            axis_of[p] = len(sizes) + 1
            sizes.append(2)
        else:
            run += 1
    if run:
        sizes.append(1 << run)
    return t.reshape(t.shape[0], *sizes), axis_of


def gate_matrix_view(t: torch.Tensor, targets, controls=()) -> torch.Tensor:
    """The controlled slice of ``t`` (controls = 1) as a (B, 2^k, rest) VIEW-permuted tensor: axis 1 the targets
    (targets[0] = matrix-index MSB), then the other bits, most significant first -- so the flattened column index is the
    uncontrolled non-target bits in ascending order, the kernels' column numbering (insert_zeros)."""
    v, axis_of = bit_view(t, set(targets) | set(controls))
    idx = [slice(None)] * v.ndim
    for c in controls:
        idx[axis_of[c]] = 1
    sl = v[tuple(idx)]
    gone = sorted(axis_of[c] for c in controls)
    pos = {a: a - sum(g < a for g in gone) for a in range(v.ndim) if a not in gone}
    tax = [pos[axis_of[q]] for q in targets]
    rest = [a for a in range(1, sl.ndim) if a not in tax]
    return sl.permute([0] + tax + rest)


def apply_gate(x: torch.Tensor, mats: torch.Tensor, targets, controls=()):
    """(U on ``targets`` where all ``controls`` are 1) x in complex128: gather the controlled slice to (B, 2^k, rest), one
    matmul, scatter back.  ``mats``: (D, D), (1, D, D) or (B, D, D).  Returns (out, xm, ym): xm / ym the (B, D, rest)
    matrices before and after (for the negative controls)."""
    k = len(targets)
    out = x.to(C128, copy=True)
    view = gate_matrix_view(out, targets, controls)
    xm = view.clone(memory_format=torch.contiguous_format).reshape(x.shape[0], 1 << k, -1)     # (a copy, never a view of out)
    u = mats.to(device=x.device, dtype=C128)
    ym = (u if u.ndim == 3 else u.unsqueeze(0)) @ xm
    view.copy_(ym.reshape(view.shape))
    return out, xm, ym


def expect_pauli(psi: torch.Tensor, xmask: int, zmask: int):
    """Re <psi|P|psi> for P = i^ny X^x Z^z (Y = i X Z on its bit): (B,) float64 and S = sum_i |psi_i| |psi_{i^x}|."""
    i = torch.arange(psi.shape[-1], device=psi.device)
    j = i ^ xmask
    y = psi.to(C128)
    terms = y.conj() * y[:, j] * z_sign(j, zmask)
    ny = bin(xmask & zmask).count('1')
    val = (terms.sum(-1) * (1j ** ny)).real
    return val, (y.abs() * y.abs()[:, j]).sum(-1)


def inner(bra: torch.Tensor, ket: torch.Tensor):
    a, b = bra.to(C128), ket.to(C128)
    return (a.conj() * b).sum(-1), (a.abs() * b.abs()).sum(-1)


def probabilities(psi: torch.Tensor) -> torch.Tensor:
    y = torch.view_as_real(psi).to(torch.float64)
    return y[..., 0] ** 2 + y[..., 1] ** 2


def expect_z_multi(psi: torch.Tensor, zmasks):
    """<psi| Z-string_k |psi>: (B, K) float64, and S = sum_i |psi_i|^2 (B, 1)."""
    p = probabilities(psi)
    i = torch.arange(psi.shape[-1], device=psi.device)
    return torch.stack([(p * z_sign(i, z)).sum(-1) for z in zmasks], dim=1), p.sum(-1, keepdim=True)


def scale_z_signs(x: torch.Tensor, zmasks, coef: torch.Tensor) -> torch.Tensor:
    """(sum_k coef[b, k] Z-string_k) x_b in complex128."""
    i = torch.arange(x.shape[-1], device=x.device)
    w = torch.zeros(x.shape, dtype=torch.float64, device=x.device)
    for k, z in enumerate(zmasks):
        w += coef[:, k : k + 1].to(device=x.device, dtype=torch.float64) * z_sign(i, z)
    return x.to(C128) * w


def outcome_index(n: int, bits, device) -> torch.Tensor:
    """Outcome of every index for a marginal over ``bits`` (bits[0] = the outcome's MSB)."""
    i = torch.arange(1 << n, device=device)
    o = torch.zeros_like(i)
    for q, b in enumerate(bits):
        o |= ((i >> b) & 1) << (len(bits) - 1 - q)
    return o


def marginal(psi: torch.Tensor, bits) -> torch.Tensor:
    """(B, 2^len(bits)) float64.  Its terms are non-negative: S is the value itself."""
    o = outcome_index(_nbits(psi), bits, psi.device)
    out = torch.zeros(psi.shape[0], 1 << len(bits), dtype=torch.float64, device=psi.device)
    return out.index_add_(1, o, probabilities(psi))


def rdm1_cross(bra: torch.Tensor, ket: torch.Tensor):
    """T[b, k, a, c] = sum over the other wires of conj(bra[.. a on wire k ..]) ket[.. c on wire k ..] (wire k = index bit
    n - 1 - k): (B, n, 2, 2) complex128, and S, the same sums over |bra| |ket|.  Elementwise products and torch's own
    (cascaded) sums rather than an einsum: a GEMM whose inner dimension is the whole state adds in an order of its own,
    and its rounding at 2^22 terms is of the order this reference is used to judge."""
    b, n = ket.shape[0], _nbits(ket)
    x, y = bra.to(C128), ket.to(C128)
    t = torch.empty(b, n, 2, 2, dtype=C128, device=ket.device)
    s = torch.empty(b, n, 2, 2, dtype=torch.float64, device=ket.device)
    for k in range(n):
        xv, yv = x.reshape(b, 1 << k, 2, -1), y.reshape(b, 1 << k, 2, -1)
        for a in (0, 1):
            for c in (0, 1):
                t[:, k, a, c] = (xv[:, :, a].conj() * yv[:, :, c]).sum((1, 2))
                s[:, k, a, c] = (xv[:, :, a].abs() * yv[:, :, c].abs()).sum((1, 2))
    return t, s


def src_index(nl: int, src_of_dst, device) -> torch.Tensor:
    """sigma(i) = sum_p bit_p(i) << src_of_dst[p]: permute_bits reads out[i] = in[sigma(i)]."""
    i = torch.arange(1 << nl, device=device)
    s = torch.zeros_like(i)
    for p, sp in enumerate(src_of_dst):
        s |= ((i >> p) & 1) << sp
    return s


def expand_index(nl: int, mask: int, value: int, device) -> torch.Tensor:
    """Packed position c -> amplitude index with ``value`` re-inserted at the ``mask`` bits."""
    c = torch.arange(1 << (nl - bin(mask).count('1')), device=device)
    out = torch.zeros_like(c)
    src = 0
    for p in range(nl):
        if not (mask >> p) & 1:
            out |= ((c >> src) & 1) << p
            src += 1
    return out | value


def tile_cross(x: torch.Tensor, gy: torch.Tensor, tile_bits, tile: int, target: int, controls=()) -> torch.Tensor:
    """The share of gate_grad(x, gy, [target], controls) that one tile of gate_grad_multi holds: the pairs whose index bits
    outside ``tile_bits`` spell ``tile`` (ascending).  (B, 2, 2) complex128; zero when a control outside the tile is 0."""
    n = _nbits(x)
    outside = [p for p in range(n) if p not in tile_bits]
    base = 0
    for q, p in enumerate(outside):
        base |= ((tile >> q) & 1) << p
    e = torch.full((1 << len(tile_bits),), base, dtype=torch.long, device=x.device)
    a = torch.arange(1 << len(tile_bits), device=x.device)
    for q, p in enumerate(tile_bits):
        e |= ((a >> q) & 1) << p
    cm = sum(1 << c for c in controls)
    e0 = e[(((e >> target) & 1) == 0) & ((e & cm) == cm)]
    e1 = e0 | (1 << target)
    xs = torch.stack([x[:, e0], x[:, e1]], dim=1).to(C128)
    ys = torch.stack([gy[:, e0], gy[:, e1]], dim=1).to(C128)
    return ys @ xs.mH


# ---- the k-wire cross reduction (dq_rdm.hip) -------------------------------------------------------------------------------
def cross_index(n: int, targets, controls, device):
    """The amplitude index of matrix row a (MSB = targets[0]; the controls at 1 folded in) and of contraction column r:
    bit q of r is the q-th lowest rest bit, the kernel's own order (a chunk is a run of columns, a split a run of chunks)."""
    k = len(targets)
    rest = [p for p in range(n) if p not in targets and p not in controls]
    va = torch.arange(1 << k, device=device)
    a = torch.full_like(va, sum(1 << c for c in controls))
    for i, p in enumerate(targets):
        a |= ((va >> (k - 1 - i)) & 1) << p
    vr = torch.arange(1 << len(rest), device=device)
    r = torch.zeros_like(vr)
    for q, p in enumerate(rest):
        r |= ((vr >> q) & 1) << p
    return a, r


def _cross_sample(xs, ys, idx):
    """One sample: ``idx`` (W, D, kw) amplitude indices.  W small matmuls and one sum over W in float64, so that no GEMM adds
    more than 2^14 terms in an order of its own."""
    ym = ys.to(C128)[idx]
    xm = ym if xs is ys else xs.to(C128)[idx]
    return (ym @ xm.mH).sum(0), (ym.abs() @ xm.abs().mT).sum(0)


def cross(x: torch.Tensor, gy: torch.Tensor, targets, controls=()):
    """out[b, a, c] = sum over the contraction columns of gy[b, a, r] conj(x[b, c, r]) (the controls at 1) in complex128,
    and S, the same sum over |gy| |x|: (B, D, D) each.  One sample at a time: the gather of one sample's 2^(n - nc)
    amplitudes is the largest temporary."""
    n = _nbits(x)
    a, r = cross_index(n, targets, controls, x.device)
    kw = min(r.numel(), 1 << 14)
    idx = r.reshape(-1, 1, kw) | a.reshape(1, -1, 1)
    same = x.data_ptr() == gy.data_ptr()
    vals, ss = zip(*(_cross_sample(gy[b] if same else x[b], gy[b], idx) for b in range(x.shape[0])))
    return torch.stack(vals), torch.stack(ss)


def chunk_columns(geo: dict, split: int, chunk: int) -> tuple[int, int]:
    """(first column, count) of chunk ``chunk`` of contraction split ``split`` under the plan ``geo``
    (_launch_geometry.rdmk): chunks are runs of kc columns (the lowest rest bits), the split is the top of the chunk number."""
    assert 0 <= split < geo['nsplit'] and 0 <= chunk < geo['nch']
    return (split * geo['nch'] + chunk) * geo['kc'], min(geo['kc'], geo['terms'])


def cross_columns(x, gy, targets, controls, sample: int, first: int, count: int):
    """What the contraction columns [first, first + count) of one sample add to cross(): (D, D) complex128 and its S.
    The reference less this is the negative control of a dropped chunk."""
    a, r = cross_index(_nbits(x), targets, controls, x.device)
    idx = (r[first : first + count].reshape(1, 1, -1) | a.reshape(1, -1, 1))
    return _cross_sample(x[sample], gy[sample], idx)


def internal_order(targets) -> list[int]:
    """p[i] = the caller's matrix index of the kernel's internal row i, whose bit q is the q-th lowest target position
    (tiles are runs of dt internal rows)."""
    k = len(targets)
    rank = {t: q for q, t in enumerate(sorted(targets))}
    p = [0] * (1 << k)
    for a in range(1 << k):
        p[sum(((a >> (k - 1 - i)) & 1) << rank[t] for i, t in enumerate(targets))] = a
    return p


def to_internal(m: torch.Tensor, targets) -> torch.Tensor:
    p = torch.tensor(internal_order(targets), device=m.device)
    return m[..., p, :][..., :, p]


def swap_tiles(m: torch.Tensor, dt: int, t1, t2) -> torch.Tensor:
    """(internal order) the dt x dt blocks at tile coordinates t1 and t2 exchanged."""
    out = m.clone()
    (i1, j1), (i2, j2) = t1, t2
    out[..., i1 * dt : (i1 + 1) * dt, j1 * dt : (j1 + 1) * dt] = m[..., i2 * dt : (i2 + 1) * dt, j2 * dt : (j2 + 1) * dt]
    out[..., i2 * dt : (i2 + 1) * dt, j2 * dt : (j2 + 1) * dt] = m[..., i1 * dt : (i1 + 1) * dt, j1 * dt : (j1 + 1) * dt]
    return out


def conj_tile(m: torch.Tensor, dt: int, t) -> torch.Tensor:
    """(internal order) the block at tile coordinates t conjugated: a mirrored tile that lost its sign."""
    out = m.clone()
    i, j = t
    out[..., i * dt : (i + 1) * dt, j * dt : (j + 1) * dt] = m[..., i * dt : (i + 1) * dt, j * dt : (j + 1) * dt].conj()
    return out


def f32_chain(ye: torch.Tensor, xe: torch.Tensor, window: int | None) -> torch.Tensor:
    """sum_r ye[e, r] conj(xe[e, r]) for complex64 rows (E, K) as a k-ordered float32 chain, the accumulation DESIGN 4.6
    documents for the complex64 kernel: float32 products (re: yr xr, yi xi; im: yi xr, -yr xi, index by index), added one
    after the other in float32 over ``window`` contraction indices, the windows added in float64.  ``window`` None: one
    float32 chain over all K (a flush that never happens).  (E,) complex128."""
    assert ye.dtype == xe.dtype == torch.complex64 and ye.shape == xe.shape
    yr, yi, xr, xi = ye.real, ye.imag, xe.real, xe.imag
    terms = torch.stack([torch.stack([yr * xr, yi * xi], -1), torch.stack([yi * xr, -(yr * xi)], -1)])    # (2, E, K, 2) f32
    e, k = ye.shape
    w = 2 * (window or k)
    t = terms.reshape(2, e, (2 * k) // w, w).cpu().numpy()
    acc = np.add.accumulate(t, axis=-1, dtype=np.float32)[..., -1]          # (sequential; np.sum would add in pairs)
    tot = torch.from_numpy(acc.astype(np.float64).sum(-1))
    return torch.complex(tot[0], tot[1]).to(ye.device)


# ---- the reductions of a wave-tile pass (include/dq_hip.h, DQ_FG_GRAD / DQ_FG_EXPZ) ----------------------------------------
def grad_sums(x: torch.Tensor, t: int, s: int, controls=()):
    """G[b, a, c] = sum lambda[t = a] conj(psi[t = c]) over the amplitudes whose ``controls`` are all 1 (index bit s: 0 = psi,
    1 = lambda): (B, 2, 2) complex128, and S, the same sums over |lambda| |psi| (float64)."""
    v = gate_matrix_view(x.to(C128), [t, s], controls)                     # (B, 2 [t], 2 [s], rest ..)
    lam, psi = v[:, :, 1].flatten(2), v[:, :, 0].flatten(2)
    g = torch.empty(x.shape[0], 2, 2, dtype=C128, device=x.device)
    sa = torch.empty(x.shape[0], 2, 2, dtype=torch.float64, device=x.device)
    for a in (0, 1):
        for c in (0, 1):
            g[:, a, c] = (lam[:, a] * psi[:, c].conj()).sum(-1)
            sa[:, a, c] = (lam[:, a].abs() * psi[:, c].abs()).sum(-1)
    return g, sa


def grad_components(g: torch.Tensor, sa: torch.Tensor, variant: int):
    """The eight components a DQ_FG_GRAD record of this ``loc`` variant adds (include/dq_hip.h:110-121) and the sums over
    absolute values each was formed from: (B, 8) float64 each, NaN where the variant leaves the component untouched."""
    full = torch.view_as_real(g.reshape(-1, 4)).reshape(-1, 8)
    fabs = sa.reshape(-1, 4).repeat_interleave(2, dim=1)
    out, oabs = torch.full_like(full, float('nan')), torch.full_like(fabs, float('nan'))
    if variant == 0:
        out, oabs = full.clone(), fabs.clone()
    elif variant == 1:
        out[:, 0::2], oabs[:, 0::2] = full[:, 0::2], fabs[:, 0::2]
    elif variant == 2:
        out[:, 0], oabs[:, 0] = full[:, 0] + full[:, 6], fabs[:, 0] + fabs[:, 6]
        out[:, 3], oabs[:, 3] = full[:, 3] + full[:, 5], fabs[:, 3] + fabs[:, 5]
    elif variant == 3:
        out[:, [0, 1, 6, 7]], oabs[:, [0, 1, 6, 7]] = full[:, [0, 1, 6, 7]], fabs[:, [0, 1, 6, 7]]
    else:
        out[:, 3], oabs[:, 3] = full[:, 3] + full[:, 5], fabs[:, 3] + fabs[:, 5]
    return out, oabs


def tile_indices(n: int, blk_pos, tile: int, device, held_zero=()) -> tuple[torch.Tensor, list[int]]:
    """The amplitude indices of tile number ``tile`` of a wave-tile pass -- bit j of the number at index bit blk_pos[j], the
    bits ``held_zero`` at 0, every other index bit free -- in ascending order, and the free bits (ascending: local bit q of
    the gathered tile is free[q])."""
    fixed = set(blk_pos) | set(held_zero)
    free = [p for p in range(n) if p not in fixed]
    a = torch.arange(1 << len(free), device=device)
    idx = torch.full_like(a, sum(((tile >> j) & 1) << p for j, p in enumerate(blk_pos)))
    for q, p in enumerate(free):
        idx |= ((a >> q) & 1) << p
    return idx, free


def tile_grad_sums(x, idx, free, t, s, controls=()):
    """What the amplitudes ``idx`` (tile_indices) add to grad_sums(x, t, s, controls): t and s are free bits of the tile; a
    control outside the tile is the same for all of them."""
    inside = [c for c in controls if c in free]
    for c in controls:
        if c not in free and not (int(idx[0]) >> c) & 1:
            z = torch.zeros(x.shape[0], 2, 2, dtype=C128, device=x.device)
            return z, z.real.clone()
    return grad_sums(x[:, idx], free.index(t), free.index(s), [free.index(c) for c in inside])


# ---- the one-wire entanglement kernels path by path (dq_entangle.hip; rows in _entangle_cases.py) ----------------------------
_M32 = 0xFFFFFFFF


def _mix32(x: torch.Tensor) -> torch.Tensor:
    """An integer hash of the low 32 bits of an int64 tensor; every intermediate stays below 2^63, so CPU and GPU agree."""
    x = x & _M32
    for _ in range(2):
        x = x ^ (x >> 16)
        x = (x * 0x45D9F3B) & _M32
    return x ^ (x >> 16)


def int_parts(seed: int, stream: int, samples: torch.Tensor, attempt: int, count: int) -> torch.Tensor:
    """(len(samples), count) int64 in -2 .. 2: a counter-based generator, a function of (seed, stream, sample number,
    attempt, position) alone -- not of the device, the dtype or the batch the sample sits in."""
    h = _mix32(_mix32(_mix32(torch.full_like(samples, seed * 4 + stream)) ^ samples) ^ attempt)
    pos = (torch.arange(count, device=samples.device) * 0x9E3779B1) & _M32
    return _mix32(h[:, None] ^ pos[None, :]) % 5 - 2


def int_state(n: int, samples: torch.Tensor, seed: int, stream: int = 0, attempt: int = 0) -> torch.Tensor:
    """Amplitudes with integer real and imaginary parts in -2 .. 2 for the sample numbers ``samples``: complex128
    (len(samples), 2^n), made in chunks of at most 2^22 amplitudes."""
    out = torch.empty(len(samples), 1 << n, dtype=C128, device=samples.device)
    real = torch.view_as_real(out)
    step = max(1, (1 << 22) >> n)
    for lo in range(0, len(samples), step):
        part = int_parts(seed, stream, samples[lo : lo + step], attempt, 2 << n)
        real[lo : lo + step] = part.reshape(-1, 1 << n, 2).to(torch.float64)
    return out


def rdm1_exact(bra: torch.Tensor, ket: torch.Tensor) -> torch.Tensor:
    """rdm1_cross without S, for integer amplitudes: wire by wire, elementwise products and sums in complex128, every
    partial sum an integer below 2^53 whatever the order.  A few samples at a time (the host's caches)."""
    b, n = ket.shape[0], _nbits(ket)
    t = torch.empty(b, n, 2, 2, dtype=C128, device=ket.device)
    step = max(1, (1 << 18) >> n) if ket.device.type == 'cpu' else b
    for lo in range(0, b, step):
        x, y = bra[lo : lo + step].to(C128), ket[lo : lo + step].to(C128)
        for k in range(n):
            xv, yv = x.reshape(x.shape[0], 1 << k, 2, -1), y.reshape(x.shape[0], 1 << k, 2, -1)
            for a in (0, 1):
                for c in (0, 1):
                    t[lo : lo + step, k, a, c] = (xv[:, :, a].conj() * yv[:, :, c]).sum((1, 2))
    return t


def rdm1_inputs_ok(t: torch.Tensor, cross: bool) -> torch.Tensor:
    """Per sample: the n matrices T_k differ pairwise, T00 != T11 and T01 != 0 in each, and for a cross reduction
    T01 != conj(T10) -- so that no exchange of wires, of components or of bra and ket leaves T as it is."""
    b, n = t.shape[:2]
    ok = (t[:, :, 0, 0] != t[:, :, 1, 1]).all(1) & (t[:, :, 0, 1] != 0).all(1)
    if cross:
        ok &= (t[:, :, 0, 1] != t[:, :, 1, 0].conj()).all(1)
    flat = t.reshape(b, n, 4)
    differ = (flat[:, :, None] != flat[:, None, :]).any(-1) | torch.eye(n, dtype=torch.bool, device=t.device)
    return ok & differ.all((1, 2))


def exact_states(n: int, batch: int, seed: int, cross: bool, device) -> tuple[torch.Tensor, torch.Tensor]:
    """(bra, ket) with integer parts for the exact criterion, complex128; ``bra is ket`` unless ``cross``.  The seed of a
    sample is chosen: sample b takes the first attempt = 0, 1, .. whose amplitudes pass rdm1_inputs_ok (a same-state
    sample of 2^13 amplitudes has T00 == T11 on some wire about once in 50 draws; at n = 2 half the draws fail)."""
    todo = torch.arange(batch, device=device)
    ket = torch.empty(batch, 1 << n, dtype=C128, device=device)
    bra = torch.empty_like(ket) if cross else ket
    for attempt in range(64):
        k = int_state(n, todo, seed, 0, attempt)
        x = int_state(n, todo, seed, 1, attempt) if cross else k
        ok = rdm1_inputs_ok(rdm1_exact(x, k), cross)
        ket[todo[ok]] = k[ok]
        if cross:
            bra[todo[ok]] = x[ok]
        todo = todo[~ok]
        if not len(todo):
            return bra, ket
    raise AssertionError(f'no seed found for {len(todo)} samples at n = {n}')


def int_mats(n: int, batch: int, seed: int, device) -> torch.Tensor:
    """One-wire operators with integer parts in -2 .. 2: complex128 (batch, n, 2, 2), mended so that in every matrix
    M01 != 0, M10 != 0, M10 != M01 and M11 != M00 (a dropped or exchanged entry changes the operator)."""
    parts = int_parts(seed, 2, torch.arange(batch, device=device), 0, n * 8).reshape(batch, n, 2, 2, 2)
    m = torch.view_as_complex(parts.to(torch.float64).contiguous())
    m[:, :, 0, 1] = torch.where(m[:, :, 0, 1] == 0, torch.ones_like(m[:, :, 0, 1]), m[:, :, 0, 1])
    m[:, :, 1, 0] = torch.where((m[:, :, 1, 0] == 0) | (m[:, :, 1, 0] == m[:, :, 0, 1]), -m[:, :, 0, 1], m[:, :, 1, 0])
    shift = torch.where(m[:, :, 0, 0].real < 2, 1.0, -1.0).to(C128)
    m[:, :, 1, 1] = torch.where(m[:, :, 1, 1] == m[:, :, 0, 0], m[:, :, 0, 0] + shift, m[:, :, 1, 1])
    return m


def wire_sum(state: torch.Tensor, mats: torch.Tensor) -> torch.Tensor:
    """sum_k (mats[b, k] on wire k) state[b] in complex128, wire by wire with elementwise products: exact for integer
    parts in -2 .. 2 (|out| parts <= 16 n)."""
    b, n = state.shape[0], _nbits(state)
    y, m = state.to(C128), mats.to(device=state.device, dtype=C128)
    out = torch.zeros_like(y)
    for k in range(n):
        yv, ov = y.reshape(b, 1 << k, 2, -1), out.view(b, 1 << k, 2, -1)
        for a in (0, 1):
            for c in (0, 1):
                ov[:, :, a] += m[:, k, a, c].reshape(b, 1, 1) * yv[:, :, c]
    return out


def wire_offdiag(state_row: torch.Tensor, mats_row: torch.Tensor, p: int) -> torch.Tensor:
    """What the off-diagonal entries of the operator on wire bit p (wire n - 1 - p) add to wire_sum for one sample: (2^n,)."""
    n = state_row.shape[-1].bit_length() - 1
    y, m = state_row.to(C128).reshape(-1, 2, 1 << p), mats_row[n - 1 - p].to(C128)
    out = torch.empty_like(y)
    out[:, 0], out[:, 1] = m[0, 1] * y[:, 1], m[1, 0] * y[:, 0]
    return out.reshape(-1)


def ent_tile_indices(p: dict, base: int, device) -> torch.Tensor:
    """The amplitude indices of one tile of pass ``p`` (_launch_geometry.entangle_passes) in tile-local order, ``base``
    from _launch_geometry.ent_tile_base: the low s local bits contiguous, the others at lo, lo + 1, .."""
    l = torch.arange(1 << p['m'], device=device)                            # noqa: E741
    return base | (l & ((1 << p['s']) - 1)) | ((l >> p['s']) << p['lo'])


def rdm1_tile_share(bra_row: torch.Tensor, ket_row: torch.Tensor, plan: dict, which: int, base: int, tile: int):
    """What tile number ``tile`` (index bits ``base``) of pass ``which`` of ``plan`` adds to rdm1_cross of ONE sample:
    the pairs along the tile bits the pass settles and, in pass 0, the diagonals -- of a wire inside the tile by its
    local bit, of a wire outside it the tile's whole sum, at the entry its bit of the tile number names.  (n, 2, 2)."""
    p, n, m0 = plan['passes'][which], len(plan['diag']), plan['m0']
    idx = ent_tile_indices(p, base, ket_row.device)
    xs, ys = bra_row[idx].to(C128), ket_row[idx].to(C128)
    d = torch.zeros(n, 2, 2, dtype=C128, device=ket_row.device)
    for wp, j, _ in p['settles']:
        xv, yv = xs.reshape(-1, 2, 1 << j), ys.reshape(-1, 2, 1 << j)
        for a in (0, 1):
            for c in (0, 1):
                if a != c or p['first']:
                    d[n - 1 - wp, a, c] = (xv[:, a].conj() * yv[:, c]).sum()
    if p['first']:
        total = (xs.conj() * ys).sum()
        for wp in range(m0, n):
            a = (tile >> (wp - m0)) & 1
            d[n - 1 - wp, a, a] = total
    return d
