"""The case tables and the checks that test_stream_autograd_cpu.py (through the plain-torch stand-ins) and
test_stream_autograd_gpu.py (through the HIP kernels) run alike: every streaming node of ``ops`` -- ``_CostPhase``,
``_CostCross``, ``_CostScale``, ``_DiagMul``, ``_GenAxpby`` / ``_GenCross`` / ``_GenRot`` for both generator families,
``_PermuteBasis``, ``_MuxApply``, ``_MuxAxpby`` / ``_MuxCross`` / ``_MuxRot`` (the trainable multiplexers, whose parameters
are a row of 2^k values per sample or one shared row) -- differentiated in reverse and in forward mode against the closed
forms of tests/_stream_grad_ref.py.

The shapes come from the families' kernel tests (named behind each case): at n = 11 .. 15 a sample is more than one unit
of work, so the backward, jvp and vmap rules run on the gathered, unit-crossing and batch-strided kernel paths.  The batch
of a case is chosen here: 3 with one parameter per sample, 2 with one 0-d parameter for all samples (its gradient is the
sum over the samples), 1.

Criteria (those of test_excite_gpu.py), TOL = 1e-4 (complex64) / 1e-10 (complex128): a state-shaped result within
TOL max|ref|; a reduction-shaped one (a parameter's gradient, a cross value's tangent) within TOL |u| |v|, the norms of
the two tensors it reduces, per sample (summed where the parameter is shared); outside the support a 'gate'-mode gradient
bit-identical to the cotangent and a 'map' / scale-mode one exactly 0.  References are formed from the amplitudes as
stored -- rounded to the precision under test, then taken to complex128.

The trainable multiplexers reduce per bin (the amplitudes with one select value inside the controls), so their
reduction-shaped results -- ga, gc, gtheta, the cross and its tangent, all (B, 2^k) -- are judged per bin: entry [b, s]
within TOL |u restricted to bin s| |v restricted to bin s| (summed over b for a shared row).  A per-sample scale would be
2^(k/2) times looser and would hide an error confined to one bin; `negative_controls` shows on reference tensors alone
that the per-bin rule rejects reversed select bits, a shared gradient without its sum over the batch, a conjugation on
the wrong factor and a gtheta formed with +theta."""

import numpy as np
import torch
from torch.autograd import forward_ad as fwad

from deepquantum_amd import backend, ops
from deepquantum_amd.gate import excitation_masks

import _diag_ref
import _mux_ref
import _perm_ref
import _stream_grad_ref as ref

DTYPES = {'c64': torch.complex64, 'c128': torch.complex128}
TOL = {'c64': 1e-4, 'c128': 1e-10}
THETAS = np.array([0.4, -1.3, 3.9])                     # (test_excite_gpu.py: one negative, one above pi)
A = np.array([0.3 - 0.2j, 1.1j, -0.7 + 0.0j])
C = np.array([-0.6 + 0.1j, 0.4, 0.9j])


def bits(*positions):
    return sum(1 << p for p in positions)


def wires_spec(n, create, annihilate, controls=()):
    return (*excitation_masks(n, create, annihilate, True, controls), tuple(n - 1 - c for c in controls))


# name: (..., batch, shared parameter?)
EXCITE = {
    # test_excite_gpu.CASES: (n, (xmask, amask, zmask, negate[, controls]))
    'n15-across-the-unit': (15, (bits(9, 10, 11, 12), bits(9, 12), bits(0, 8, 13, 14), 0), 1, False),   # bit 0 outside the pairs' bits
    'n14-fermionic-double-2c': (14, wires_spec(14, [9, 13], [0, 5], (2, 7)), 2, True),    # the string on both sides of the split, controls
    'n12-batch3': (12, (bits(1, 5), bits(5), bits(2, 3, 4), 0), 3, False),
    'n11-weight1-bit0-a1': (11, (1, 1, bits(5), 1), 2, False),                             # bit 0 the pair bit, negate = 1
    'n13-triple': (13, (bits(0, 3, 5, 8, 10, 12), bits(0, 5, 10), bits(1, 4, 11), 1), 2, True),
}
PAULI = {
    # test_pauli_gpu.CROSS_CASES: (n, xmask, zmask, controls)
    'n14_mixed': (14, 1 | 1 << 5 | 1 << 13, 1 << 5 | 1 << 13 | 1 << 8, (), 1, False),    # bit 0 flipped, partners across the unit
    'batch3': (12, 1 << 11 | 1 << 2, 1 << 2 | 1, (4,), 3, False),
    'ctrl_low': (12, 1 << 6 | 1 << 1, 1 << 6, (0,), 2, True),                            # bit 0 a control
    'n12_bit11': (12, 1 << 11, 1 << 11, (), 2, False),                                   # a lone Y on the first bit above a unit (c64)
    'ctrl_both_z': (12, 0, 1 << 4, (0, 11), 2, True),                                    # a Z string: no partner
}
NG = 13
DIAG = {
    # test_diag_gpu.GATHERED / CONTROLS at n = NG: (bits, controls)
    'crossing': ((12, 11, 10, 9), (), 2, True),                                          # a run of table bits across the chunk size
    'k3_mixed': ((5, NG - 1, 0), (), 3, False),                                          # bit 0 a table bit
    'straddle': ((6, 5), (1, NG - 1), 2, False),                                         # bit 0 neither
    'ctrl_bit0': ((6, 5), (0,), 1, False),
}
UNIT = {'c64': 11, 'c128': 10}                          # log2 of the amplitudes of a 16-KiB chunk (dq_permutation_local_bits)
PERM = {
    # test_perm_gpu.py at n = u + 2, u = UNIT[dt]: (bits, controls) as functions of u
    'gather-straddle': (lambda u: (u, u - 1, u - 2), lambda u: (), 2),
    'gather-bit0-control': (lambda u: (u, 3), lambda u: (0, u + 1), 3),
    'gather-bit0-table': (lambda u: (0, u), lambda u: (), 1),
    'local-bit0-table': (lambda u: (0, 3, u - 1, 5), lambda u: (u + 1, 1), 2),
    'local-bit0-free': (lambda u: (1, 4, u - 1), lambda u: (), 1),
}
MUX = {
    # test_mux_gpu.test_a_few_units_every_target_class at n = p + 3, p = UNIT[dt] (the pairs of a unit, log2, for a target
    # above bit 0): (kind, dagger, target, bits, controls) as functions of p
    'bit0-run-across': ('u', False, lambda p: 0, lambda p: (p, p - 1, p - 2), lambda p: (), 2),        # c64: the pair inside a vector
    'unit_top-bit0-select': ('ry', True, lambda p: p, lambda p: (p + 2, 0), lambda p: (p + 1,), 3),
    'wave6-bit0-control': ('ry', False, lambda p: 6, lambda p: (p + 1, 3), lambda p: (0, p + 2), 2),
    'top-bit0-free': ('u', True, lambda p: p + 2, lambda p: (p - 1, p - 2, p - 3), lambda p: (1,), 1),
}


def every_other_position(p, target=5):
    """All n - 1 positions of n = p + 3 but the target, in a seeded order: every bin is one pair."""
    rest = [q for q in range(p + 3) if q != target]
    return tuple(int(rest[j]) for j in np.random.default_rng(p).permutation(len(rest)))


MUXGRAD = {
    # test_muxgrad_gpu.PLACEMENTS at n = p + 3 (a sample is eight units): (axis, target, bits, controls) as functions of p,
    # batch, shared row?
    'bit0-target-run-across': ('x', lambda p: 0, lambda p: (p, p - 1, p - 2), lambda p: (), 2, True),   # c64: the pair inside a vector
    # the ry table route, bit 0 a select, 'map' with k + nc = 7 table bits, one launch per sample
    'selects-both-sides-2c': ('y', lambda p: 4, lambda p: (p + 2, 0, p + 1, p, 6), lambda p: (2, p - 1), 3, False),
    'top-target-bit0-control': ('z', lambda p: p + 2, lambda p: (p + 1, 3, 1), lambda p: (0,), 2, True),
    'wave-selects-identity': ('i', lambda p: 7, lambda p: (8, 9), lambda p: (5, p + 1), 1, True),
    'every-pair-a-bin': ('y', lambda p: 5, every_other_position, lambda p: (), 2, True),              # k = n - 1
}
FAMILIES = {'diag': DIAG, 'pauli': PAULI, 'excite': EXCITE, 'perm': PERM, 'mux': MUX, 'muxgrad': MUXGRAD}
#: the case of each family that also runs with other cotangent and state layouts, and under vmap
LAYOUT_CASE = {'diag': 'straddle', 'pauli': 'ctrl_low', 'excite': 'n11-weight1-bit0-a1', 'perm': 'gather-bit0-control',
               'mux': 'wave6-bit0-control', 'muxgrad': 'selects-both-sides-2c'}


# ---- data ------------------------------------------------------------------------------------------------------------------
def gauss(rng, shape, dtype):
    """Seeded Gaussian values as stored in ``dtype`` (a CPU tensor) and the same values in complex128 numpy."""
    a = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if dtype.is_complex else 0.0)
    t = torch.from_numpy(np.asarray(a)).to(dtype)
    return t, t.numpy().astype(np.complex128 if dtype.is_complex else np.float64)


def norms(a):
    return np.linalg.norm(a.reshape(a.shape[0], -1), axis=-1)


def bitwise_equal(a, b):
    kind = torch.int32 if a.dtype == torch.complex64 else torch.int64
    return torch.equal(torch.view_as_real(a.contiguous()).view(kind), torch.view_as_real(b.contiguous()).view(kind))


class Node:
    """One differentiable call: ``call(states, params)`` on torch tensors, its forward, VJP and JVP references on numpy
    complex128 (``vjp`` returns the states' gradients and the parameters' per-sample rows), and what the criteria need:
    ``out`` ('state' or 'reduction'), ``pair(states)`` -- the two tensors a reduction-shaped output reduces --, ``ppairs(states,
    g)`` -- those of each parameter's gradient --, ``off`` (the indices outside the support) and ``off_kind`` ('same': the
    gradient there is the cotangent bit for bit, 'zero': exactly 0).  A parameter is one value per sample, (B,), or -- with
    ``bins``, a ``ref.MuxBins`` -- a row per sample, (B, 2^k); its reductions are then (B, 2^k) and judged bin by bin."""

    def __init__(self, name, call, states, params, fwd, vjp, jvp, out='state', pair=None, ppairs=None, off=None,
                 off_kind='same', bins=None):
        self.name, self.call, self.states, self.params, self.fwd, self.vjp, self.jvp = name, call, states, params, fwd, vjp, jvp
        self.out, self.pair, self.ppairs, self.off, self.off_kind, self.bins = out, pair, ppairs, off, off_kind, bins

    def scale(self, u, v):
        """|u| |v| of the two tensors a reduction reduces: per sample (B,), or per sample and bin (B, 2^k)."""
        return norms(u) * norms(v) if self.bins is None else self.bins.norms(u) * self.bins.norms(v)


def param_rows(values, batch, shared):
    v = np.asarray(values[:batch]).copy()
    if shared:
        v[:] = v[0]
    return v, shared


# ---- the nodes of a case -----------------------------------------------------------------------------------------------------
def generator_nodes(tag, fam, f_axpby, f_cross, f_rot, batch, shared, dt, rng):
    size = (batch, 1 << fam.n)
    x, u = gauss(rng, size, DTYPES[dt]), gauss(rng, size, DTYPES[dt])
    a, c, th = param_rows(A, batch, shared), param_rows(C, batch, shared), param_rows(THETAS, batch, shared)
    off = ~fam.support()
    nodes = []
    for mode in ('gate', 'map'):
        nodes.append(Node(
            f'{tag} axpby {mode}', lambda s, p, mode=mode: f_axpby(s[0], p[0], p[1], mode), [x], [a, c],
            fwd=lambda s, p, mode=mode: fam.axpby(s[0], p[0], p[1], mode),
            vjp=lambda s, p, g, mode=mode: (lambda r: ([r[0]], [r[1], r[2]]))(ref.axpby_vjp(fam, s[0], p[0], p[1], mode, g)),
            jvp=lambda s, p, ds, dp, mode=mode: ref.axpby_jvp(fam, s[0], p[0], p[1], mode, ds[0], dp[0], dp[1]),
            ppairs=lambda s, g: [(s[0], g), (s[0], g)], off=off, off_kind='same' if mode == 'gate' else 'zero'))
    nodes.append(Node(
        f'{tag} cross, two tensors', lambda s, p: f_cross(s[0], s[1]), [u, x], [],
        fwd=lambda s, p: fam.cross(s[0], s[1]),
        vjp=lambda s, p, g: (list(ref.cross_vjp(fam, s[0], s[1], g)), []),
        jvp=lambda s, p, ds, dp: ref.cross_jvp(fam, s[0], s[1], ds[0], ds[1]),
        out='reduction', pair=lambda s: (s[0], s[1]), off=off, off_kind='zero'))
    nodes.append(Node(
        f'{tag} cross, bra is ket', lambda s, p: f_cross(s[0], s[0]), [x], [],
        fwd=lambda s, p: fam.cross(s[0], s[0]),
        vjp=lambda s, p, g: ([sum(ref.cross_vjp(fam, s[0], s[0], g))], []),
        jvp=lambda s, p, ds, dp: ref.cross_jvp(fam, s[0], s[0], ds[0], ds[0]),
        out='reduction', pair=lambda s: (s[0], s[0]), off=off, off_kind='zero'))
    nodes.append(Node(
        f'{tag} rot', lambda s, p: f_rot(s[0], p[0]), [x], [th],
        fwd=lambda s, p: fam.rot(s[0], p[0]),
        vjp=lambda s, p, g: (lambda r: ([r[0]], [r[1]]))(ref.rot_vjp(fam, s[0], p[0], g)),
        jvp=lambda s, p, ds, dp: ref.rot_jvp(fam, s[0], p[0], ds[0], dp[0]),
        ppairs=lambda s, g: [(g, s[0])], off=off, off_kind='same'))
    return nodes


def excite_nodes(name, dt, rng):
    n, spec, batch, shared = EXCITE[name]
    return generator_nodes(
        f'excite {name} {dt}', ref.Excitations(n, spec),
        lambda s, a, c, mode: ops.excite_axpby(s, spec, a, c, mode), lambda u, v: ops.excite_cross(u, v, spec),
        lambda s, th: ops.excite_rot(s, spec, th), batch, shared, dt, rng)


def pauli_nodes(name, dt, rng):
    n, xmask, zmask, controls, batch, shared = PAULI[name]
    return generator_nodes(
        f'pauli {name} {dt}', ref.PauliStrings(n, xmask, zmask, controls),
        lambda s, a, c, mode: ops.pauli_axpby(s, xmask, zmask, a, c, controls, mode),
        lambda u, v: ops.pauli_cross(u, v, xmask, zmask, controls),
        lambda s, th: ops.pauli_rot(s, xmask, zmask, th, controls), batch, shared, dt, rng)


def diag_nodes(name, dt, rng):
    tbits, controls, batch, shared = DIAG[name]
    where = (NG, tbits, controls)
    tag = f'diag {name} {dt}'
    size = (batch, 1 << NG)
    x, u = gauss(rng, size, DTYPES[dt]), gauss(rng, size, DTYPES[dt])
    cost = gauss(rng, 1 << len(tbits), DTYPES[dt].to_real())[0] * 3.0
    cr = cost.numpy().astype(np.float64)
    d =torch.exp(1j * torch.from_numpy(rng.uniform(0, 6.283, (batch, 1 << len(tbits))))).to(DTYPES[dt])    # one table per sample
    dr = d.numpy().astype(np.complex128)
    t, s = param_rows(THETAS, batch, shared), param_rows(A, batch, shared)
    off = ~_diag_ref.on_mask(NG, controls)
    on_dev = lambda table, like: table.to(like.device)  # noqa: E731
    return [
        Node(f'{tag} cost_phase', lambda xs, p: ops.cost_phase(xs[0], on_dev(cost, xs[0]), p[0], tbits, controls), [x], [t],
             fwd=lambda xs, p: _diag_ref.phase_ref(xs[0], cr, p[0], *where),
             vjp=lambda xs, p, g: (lambda r: ([r[0]], [r[1]]))(ref.phase_vjp(xs[0], cr, p[0], where, g)),
             jvp=lambda xs, p, ds, dp: ref.phase_jvp(xs[0], cr, p[0], where, ds[0], dp[0]),
             ppairs=lambda xs, g: [(g, xs[0])], off=off, off_kind='same'),
        Node(f'{tag} cost_scale', lambda xs, p: ops.cost_scale(xs[0], on_dev(cost, xs[0]), p[0], tbits, controls), [x], [s],
             fwd=lambda xs, p: _diag_ref.scale_ref(xs[0], cr, p[0], *where),
             vjp=lambda xs, p, g: (lambda r: ([r[0]], [r[1]]))(ref.scale_vjp(xs[0], cr, p[0], where, g)),
             jvp=lambda xs, p, ds, dp: ref.scale_jvp(xs[0], cr, p[0], where, ds[0], dp[0]),
             ppairs=lambda xs, g: [(xs[0], g)], off=off, off_kind='zero'),
        Node(f'{tag} cost_cross, two tensors', lambda xs, p: ops.cost_cross(xs[0], xs[1], on_dev(cost, xs[0]), tbits, controls),
             [u, x], [],
             fwd=lambda xs, p: _diag_ref.cross_ref(xs[0], xs[1], cr, *where),
             vjp=lambda xs, p, g: (list(ref.cost_cross_vjp(xs[0], xs[1], cr, where, g)), []),
             jvp=lambda xs, p, ds, dp: ref.cost_cross_jvp(xs[0], xs[1], cr, where, ds[0], ds[1]),
             out='reduction', pair=lambda xs: (xs[0], xs[1]), off=off, off_kind='zero'),
        Node(f'{tag} cost_cross, bra is ket', lambda xs, p: ops.cost_cross(xs[0], xs[0], on_dev(cost, xs[0]), tbits, controls),
             [x], [],
             fwd=lambda xs, p: _diag_ref.cross_ref(xs[0], xs[0], cr, *where),
             vjp=lambda xs, p, g: ([sum(ref.cost_cross_vjp(xs[0], xs[0], cr, where, g))], []),
             jvp=lambda xs, p, ds, dp: ref.cost_cross_jvp(xs[0], xs[0], cr, where, ds[0], ds[0]),
             out='reduction', pair=lambda xs: (xs[0], xs[0]), off=off, off_kind='zero'),
        Node(f'{tag} diag_mul', lambda xs, p: ops.diag_mul(xs[0], on_dev(d, xs[0]), tbits, controls), [x], [],
             fwd=lambda xs, p: _diag_ref.diag_ref(xs[0], dr, *where),
             vjp=lambda xs, p, g: ([ref.diag_mul_vjp(dr, where, g)], []),
             jvp=lambda xs, p, ds, dp: ref.diag_mul_jvp(dr, where, ds[0]), off=off, off_kind='same'),
    ]


def perm_nodes(name, dt, rng):
    u = UNIT[dt]
    n = u + 2
    fbits, fcontrols, batch = PERM[name]
    tbits, controls = fbits(u), fcontrols(u)
    x = gauss(rng, (batch, 1 << n), DTYPES[dt])
    perm = rng.permutation(1 << len(tbits)).astype(np.int64)
    table = torch.from_numpy(perm)
    return [Node(f'perm {name} {dt}', lambda xs, p: ops.permute_basis(xs[0], table.to(xs[0].device), tbits, controls), [x], [],
                 fwd=lambda xs, p: _perm_ref.permute_ref(xs[0], perm, tbits, controls),
                 vjp=lambda xs, p, g: ([ref.permute_vjp(perm, tbits, controls, g)], []),
                 jvp=lambda xs, p, ds, dp: ref.permute_jvp(perm, tbits, controls, ds[0]),
                 off=~_diag_ref.on_mask(n, controls), off_kind='same')]


def mux_nodes(name, dt, rng):
    p = UNIT[dt]
    n = p + 3
    kind, dagger, ftarget, fbits, fcontrols, batch = MUX[name]
    target, tbits, controls = ftarget(p), fbits(p), fcontrols(p)
    x = gauss(rng, (batch, 1 << n), DTYPES[dt])
    seed = int(rng.integers(1 << 30))
    if kind == 'u':
        table = torch.from_numpy(_mux_ref.random_unitaries(len(tbits), seed)).to(DTYPES[dt])
        blocks = table.numpy().astype(np.complex128)
    else:
        table = torch.from_numpy(_mux_ref.random_cs(len(tbits), seed)).to(DTYPES[dt].to_real())
        blocks = _mux_ref.ry_blocks(table.numpy().astype(np.float64))
    return [Node(f'mux {name} {dt}',
                 lambda xs, q: ops.mux_apply(xs[0], table.to(xs[0].device), kind, target, tbits, controls, dagger), [x], [],
                 fwd=lambda xs, q: _mux_ref.mux_ref(xs[0], blocks, target, tbits, controls, dagger),
                 vjp=lambda xs, q, g: ([ref.mux_vjp(blocks, target, tbits, controls, dagger, g)], []),
                 jvp=lambda xs, q, ds, dq: ref.mux_jvp(blocks, target, tbits, controls, dagger, ds[0]),
                 off=~_diag_ref.on_mask(n, controls), off_kind='same')]


def muxgrad_spec(name, dt):
    p = UNIT[dt]
    axis, ftarget, fbits, fcontrols, batch, shared = MUXGRAD[name]
    return p + 3, (axis, ftarget(p), fbits(p), fcontrols(p)), batch, shared


def bin_rows(rng, batch, count, shared, real=False):
    """A parameter of the binned nodes: seeded rows (batch, 2^k) -- equal rows for a shared one -- and ``shared``."""
    v = rng.uniform(-6, 6, (batch, count)) if real else rng.standard_normal((batch, count)) + 1j * rng.standard_normal((batch, count))
    return param_rows(v, batch, shared)


def muxgrad_nodes(name, dt, rng):
    n, mux, batch, shared = muxgrad_spec(name, dt)
    axis = mux[0]
    fam = ref.MuxBins(n, *mux)
    tag = f'muxgrad {name} {dt}'
    size = (batch, 1 << n)
    x, u = gauss(rng, size, DTYPES[dt]), gauss(rng, size, DTYPES[dt])
    a, c, th = (bin_rows(rng, batch, fam.count, shared, real) for real in (False, False, True))
    off = ~fam.support()
    nodes = []
    for mode in ('gate', 'map'):
        nodes.append(Node(
            f'{tag} axpby {mode}', lambda s, p, mode=mode: ops.mux_axpby(s[0], p[0], p[1], *mux, mode), [x], [a, c],
            fwd=lambda s, p, mode=mode: fam.axpby(s[0], p[0], p[1], mode),
            vjp=lambda s, p, g, mode=mode: (lambda r: ([r[0]], [r[1], r[2]]))(ref.binned_axpby_vjp(fam, s[0], p[0], p[1], mode, g)),
            jvp=lambda s, p, ds, dp, mode=mode: ref.binned_axpby_jvp(fam, s[0], p[0], p[1], mode, ds[0], dp[0], dp[1]),
            ppairs=lambda s, g: [(s[0], g), (s[0], g)], off=off, off_kind='same' if mode == 'gate' else 'zero', bins=fam))
    nodes.append(Node(
        f'{tag} cross, two tensors', lambda s, p: ops.mux_cross(s[0], s[1], *mux), [u, x], [],
        fwd=lambda s, p: fam.cross(s[0], s[1]),
        vjp=lambda s, p, g: (list(ref.binned_cross_vjp(fam, s[0], s[1], g)), []),
        jvp=lambda s, p, ds, dp: ref.binned_cross_jvp(fam, s[0], s[1], ds[0], ds[1]),
        out='reduction', pair=lambda s: (s[0], s[1]), off=off, off_kind='zero', bins=fam))
    nodes.append(Node(
        f'{tag} cross, bra is ket', lambda s, p: ops.mux_cross(s[0], s[0], *mux), [x], [],
        fwd=lambda s, p: fam.cross(s[0], s[0]),
        vjp=lambda s, p, g: ([sum(ref.binned_cross_vjp(fam, s[0], s[0], g))], []),
        jvp=lambda s, p, ds, dp: ref.binned_cross_jvp(fam, s[0], s[0], ds[0], ds[0]),
        out='reduction', pair=lambda s: (s[0], s[0]), off=off, off_kind='zero', bins=fam))
    if axis != 'i':
        nodes.append(Node(
            f'{tag} rot', lambda s, p: ops.mux_rot(s[0], p[0], *mux), [x], [th],
            fwd=lambda s, p: fam.rot(s[0], p[0]),
            vjp=lambda s, p, g: (lambda r: ([r[0]], [r[1]]))(ref.binned_rot_vjp(fam, s[0], p[0], g)),
            jvp=lambda s, p, ds, dp: ref.binned_rot_jvp(fam, s[0], p[0], ds[0], dp[0]),
            ppairs=lambda s, g: [(g, s[0])], off=off, off_kind='same', bins=fam))
    return nodes


BUILDERS = {'diag': diag_nodes, 'pauli': pauli_nodes, 'excite': excite_nodes, 'perm': perm_nodes, 'mux': mux_nodes,
            'muxgrad': muxgrad_nodes}
CASE_IDS = [(family, name) for family, cases in FAMILIES.items() for name in cases]


def nodes_of(family, name, dt):
    seed = sum(ord(ch) for ch in family + name) + (0 if dt == 'c64' else 1000)
    return BUILDERS[family](name, dt, np.random.default_rng(seed))


# ---- the checks --------------------------------------------------------------------------------------------------------------
def host(t):
    return t.detach().cpu().numpy().astype(np.complex128 if t.is_complex() else np.float64)


def close_state(got, want, dt, what):
    err, scale = np.abs(host(got) - want).max(), np.abs(want).max()
    print(f'{what}: err / (tol * max|ref|) = {err / (TOL[dt] * scale):.3e}')
    assert got.shape == want.shape and err <= TOL[dt] * scale, f'{what}: {err:.3e} against {TOL[dt]} * {scale:.3e}'


def close_reduction(got, want, scale, dt, what):
    """``scale``: |u| |v| per sample (per sample and bin for the binned nodes), or their sum over the samples for a shared
    parameter."""
    err = np.abs(host(got) - want)
    print(f'{what}: err / (tol * |u| |v|) = {(err / (TOL[dt] * scale)).max():.3e}')
    assert got.shape == want.shape and np.all(err <= TOL[dt] * scale), f'{what}: {err} against {TOL[dt]} * {scale}'


def laid_out(t, layout, device):
    """The values of the CPU tensor ``t`` on ``device`` in one of the layouts autograd hands a node: 'plain'; 'expanded'
    (stride 0 along the amplitudes -- the values of column 0 in every column); 'strided' (every second column of a tensor
    twice as wide); 'offset' (contiguous at element offset 1 of a flat buffer: a complex64 pointer at 8 mod 16).  Returns
    the tensor and its values."""
    if layout == 'plain':
        out = t.to(device)
    elif layout == 'expanded':
        out = t[:, :1].to(device).expand(*t.shape)
        assert out.stride(-1) == 0
    elif layout == 'strided':
        big = torch.zeros(t.shape[0], 2 * t.shape[1], dtype=t.dtype, device=device)
        big[:, ::2] = t.to(device)
        out = big[:, ::2]
        assert out.stride(-1) == 2
    else:
        assert layout == 'offset'
        flat = torch.zeros(t.numel() + 1, dtype=t.dtype, device=device)
        flat[1:] = t.to(device).reshape(-1)
        out = flat[1:].reshape(t.shape)
        assert out.is_contiguous() and out.storage_offset() == 1
        if t.dtype == torch.complex64:
            assert out.data_ptr() % 16 == 8
    return out, host(out)


def device_inputs(node, device, state_layout='plain'):
    xs, xr = zip(*(laid_out(t, state_layout, device) for t, _ in node.states))
    ps = [torch.tensor(v[0] if shared else v, device=device) for v, shared in node.params]
    return [x.detach() for x in xs], list(xr), ps, [v for v, _ in node.params]


def cotangent(node, dt, device, rng, batch, size, layout='plain'):
    if node.out == 'reduction':
        shape = batch if node.bins is None else (batch, node.bins.count)
        g = torch.from_numpy(rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).to(device)
        return g, host(g)
    return laid_out(gauss(rng, (batch, size), DTYPES[dt])[0], layout, device)


def check_forward(node, dt, device, state_layout='plain'):
    xs, xr, ps, pr = device_inputs(node, device, state_layout)
    with torch.no_grad():
        got = node.call(xs, ps)
    want = node.fwd(xr, pr)
    if node.out == 'state':
        close_state(got, want, dt, f'{node.name} forward, state {state_layout}')
    else:
        u, v = node.pair(xr)
        close_reduction(got, want, node.scale(u, v), dt, f'{node.name} forward, state {state_layout}')


def check_vjp(node, dt, device, state_layout='plain', cot_layout='plain'):
    xs, xr, ps, pr = device_inputs(node, device, state_layout)
    for t in xs + ps:
        t.requires_grad_()
    rng = np.random.default_rng(7)
    g, gr = cotangent(node, dt, device, rng, *xr[0].shape, cot_layout)
    what = f'{node.name} vjp' + ('' if (state_layout, cot_layout) == ('plain', 'plain') else f', state {state_layout}, cotangent {cot_layout}')
    grads = torch.autograd.grad(node.call(xs, ps), xs + ps, g)
    want_states, want_params = node.vjp(xr, pr, gr)
    for k, (got, want) in enumerate(zip(grads, want_states)):
        assert got.dtype == xs[k].dtype
        close_state(got, want, dt, f'{what}: gradient of state {k}')
        if node.off is not None and node.off.any():
            rest = torch.from_numpy(np.nonzero(node.off)[0]).to(device)
            if node.off_kind == 'zero':
                assert not torch.view_as_real(got[:, rest]).any(), f'{what}: a non-zero gradient outside the support'
            else:
                assert bitwise_equal(got[:, rest], g[:, rest]), f'{what}: outside the support the gradient is not the cotangent'
    if node.params:
        for k, (got, want, (u, v)) in enumerate(zip(grads[len(xs):], want_params, node.ppairs(xr, gr))):
            scale = node.scale(u, v)
            if node.params[k][1]:
                want, scale = want.sum(0), scale.sum(0)         # (one value, or one row, for all samples)
            assert got.dtype == ps[k].dtype
            close_reduction(got, want if np.iscomplexobj(pr[k]) else np.real(want), scale, dt, f'{what}: gradient of parameter {k}')


def check_jvp(node, dt, device):
    xs, xr, ps, pr = device_inputs(node, device)
    rng = np.random.default_rng(11)
    dxs, dxr = zip(*(laid_out(gauss(rng, x.shape, DTYPES[dt])[0], 'plain', device) for x in xs))
    dps, dpr = [], []
    for p, (v, shared) in zip(ps, node.params):
        d = rng.standard_normal(v.shape) + (1j * rng.standard_normal(v.shape) if np.iscomplexobj(v) else 0.0)
        if shared:
            d[:] = d[0]
        dps.append(torch.tensor(d[0] if shared else d, device=device))
        dpr.append(d)
    with fwad.dual_level():
        out = node.call([fwad.make_dual(x, d) for x, d in zip(xs, dxs)], [fwad.make_dual(p, d) for p, d in zip(ps, dps)])
        got = fwad.unpack_dual(out).tangent
    assert got is not None, f'{node.name}: no tangent came out'
    want = node.jvp(xr, pr, list(dxr), dpr)
    if node.out == 'state':
        close_state(got, want, dt, f'{node.name} jvp')
    else:
        u, v = node.pair(xr)
        du, dv = node.pair(list(dxr))
        close_reduction(got, want, node.scale(du, v) + node.scale(u, dv), dt, f'{node.name} jvp')


def check_layouts(node, dt, device):
    """The node with its state at element offset 1 (forward and VJP) and, for a state-shaped output, with a cotangent that
    is expanded, strided, and contiguous at element offset 1."""
    check_forward(node, dt, device, 'offset')
    check_vjp(node, dt, device, state_layout='offset')
    if node.out == 'state':
        for layout in ('expanded', 'strided', 'offset'):
            check_vjp(node, dt, device, cot_layout=layout)


def check_cat_loss(dt, device):
    """loss = sum (w) |cat([h, y.reshape(-1)])|^2 with y = excite_rot(x), y = cost_phase(x) and y = mux_rot(x) (a row of
    angles per sample, its gradient judged per bin): the backward of ``cat`` hands the node a contiguous cotangent at
    element offset 1, 2 w y -- plain (w = 1, the gradients are 2 x and 0: the maps are unitary) and with a weight per
    element."""
    rng = np.random.default_rng(5)
    n, spec, batch, _ = EXCITE['n11-weight1-bit0-a1']
    fam = ref.Excitations(n, spec)
    tbits, controls = DIAG['straddle'][:2]
    where = (NG, tbits, controls)
    cost, cr = gauss(rng, 1 << len(tbits), DTYPES[dt].to_real())
    per_sample = lambda u, v: norms(u) * norms(v)  # noqa: E731
    nm, mux, mbatch, shared = muxgrad_spec(LAYOUT_CASE['muxgrad'], dt)
    bins = ref.MuxBins(nm, *mux)
    assert not shared                                   # (a row of angles per sample: the rows of gtheta are not summed)
    routes = (
        ('excite_rot', n, batch, THETAS[:batch], lambda x, p: ops.excite_rot(x, spec, p), lambda x, p: fam.rot(x, p),
         lambda x, p, g: ref.rot_vjp(fam, x, p, g), per_sample),
        ('cost_phase', NG, batch, THETAS[:batch], lambda x, p: ops.cost_phase(x, cost.to(x.device), p, tbits, controls),
         lambda x, p: _diag_ref.phase_ref(x, cr, p, *where), lambda x, p, g: ref.phase_vjp(x, cr, p, where, g), per_sample),
        ('mux_rot', nm, mbatch, bin_rows(np.random.default_rng(6), mbatch, bins.count, False, real=True)[0],
         lambda x, p: ops.mux_rot(x, p, *mux),
         bins.rot, lambda x, p, g: ref.binned_rot_vjp(bins, x, p, g), lambda u, v: bins.norms(u) * bins.norms(v)))
    for name, nq, batch, thetas, call, fwd, vjp, scale in routes:
        x, xr = laid_out(gauss(rng, (batch, 1 << nq), DTYPES[dt])[0], 'plain', device)
        th = torch.tensor(thetas, device=device, requires_grad=True)
        h = torch.tensor([0.5 + 0.25j], dtype=DTYPES[dt], device=device)
        w, wr = gauss(rng, batch * (1 << nq) + 1, DTYPES[dt].to_real())
        for weighted in (False, True):
            x = x.detach().requires_grad_()
            sq = torch.cat([h, call(x, th).reshape(-1)]).abs().pow(2)
            gx, gth = torch.autograd.grad((sq * w.to(device)).sum() if weighted else sq.sum(), (x, th))
            gy = 2.0 * (wr[1:].reshape(batch, -1) if weighted else 1.0) * fwd(xr, thetas)
            want_x, want_th = vjp(xr, thetas, gy)
            what = f'{name} {dt} under cat' + (', weighted' if weighted else '')
            close_state(gx, want_x, dt, what + ': gradient of the state')
            close_reduction(gth, want_th, scale(gy, xr), dt, what + ': gradient of the parameter')


def vmap_checks(family, dt, device):
    """``torch.vmap`` over 3 x batch 2 equals the folded ``backend`` call bit for bit (for the trainable multiplexers with a
    mapped and with an unmapped row of parameters)."""
    rng = np.random.default_rng(3)
    name = LAYOUT_CASE[family]
    same = lambda got, want: torch.equal(torch.view_as_real(got.reshape(want.shape)), torch.view_as_real(want))  # noqa: E731
    ths = torch.linspace(-1, 1, 6, dtype=torch.float64, device=device).reshape(3, 2)

    def states(n):
        return gauss(rng, (6, 1 << n), DTYPES[dt])[0].to(device).reshape(3, 2, -1)

    if family == 'diag':
        tbits, controls = DIAG[name][:2]
        xs = states(NG)
        cost = gauss(rng, 1 << len(tbits), DTYPES[dt].to_real())[0].to(device)
        ss = torch.complex(ths, ths.flip(0))
        got = torch.vmap(lambda s, t: ops.cost_phase(s, cost, t, tbits, controls))(xs, ths)
        assert same(got, backend.apply_cost(xs.reshape(6, -1), cost, ths.reshape(-1), tbits, controls, 'phase'))
        got = torch.vmap(lambda s, t: ops.cost_scale(s, cost, t, tbits, controls))(xs, ss)
        assert same(got, backend.apply_cost(xs.reshape(6, -1), cost, ss.reshape(-1), tbits, controls, 'scale'))
        other = xs.flip(0)
        got = torch.vmap(lambda u, v: ops.cost_cross(u, v, cost, tbits, controls))(xs, other)
        assert same(got, backend.cost_cross(xs.reshape(6, -1), other.reshape(6, -1).contiguous(), cost, tbits, controls))
    elif family in ('pauli', 'excite'):
        if family == 'pauli':
            n, xmask, zmask, controls = PAULI[name][:4]
            rot, cross = (lambda s, t: ops.pauli_rot(s, xmask, zmask, t, controls)), (lambda u, v: ops.pauli_cross(u, v, xmask, zmask, controls))
            b_rot = lambda s, t: backend.apply_pauli_rot(s, xmask, zmask, t, controls)  # noqa: E731
            b_cross = lambda u, v: backend.pauli_cross(u, v, xmask, zmask, controls)  # noqa: E731
        else:
            n, spec = EXCITE[name][:2]
            rot, cross = (lambda s, t: ops.excite_rot(s, spec, t)), (lambda u, v: ops.excite_cross(u, v, spec))
            b_rot, b_cross = (lambda s, t: backend.apply_excite_rot(s, spec, t)), (lambda u, v: backend.excite_cross(u, v, spec))
        xs = states(n)
        other = xs.flip(0)
        assert same(torch.vmap(rot)(xs, ths), b_rot(xs.reshape(6, -1), ths.reshape(-1)))
        assert same(torch.vmap(cross)(xs, other), b_cross(xs.reshape(6, -1), other.reshape(6, -1).contiguous()))
    elif family == 'perm':
        u = UNIT[dt]
        tbits, controls = PERM[name][0](u), PERM[name][1](u)
        xs = states(u + 2)
        perm = torch.from_numpy(rng.permutation(1 << len(tbits)).astype(np.int64)).to(device)
        got = torch.vmap(lambda s: ops.permute_basis(s, perm, tbits, controls))(xs)
        assert same(got, backend.apply_permutation(xs.reshape(6, -1), ops.invert_table(perm), tbits, controls))
    elif family == 'muxgrad':
        n, mux, _, _ = muxgrad_spec(name, dt)
        count = 1 << len(mux[2])
        xs, flat = states(n), lambda t: t.reshape(6, -1)  # noqa: E731
        other = xs.flip(0)
        rows = torch.from_numpy(rng.uniform(-6, 6, (3, count))).to(device)
        per_sample = rows.unsqueeze(1).expand(3, 2, count).reshape(6, count)   # row v of the map for its two samples
        # a mapped row of angles becomes one row per sample (one launch each); an unmapped shared row stays one launch
        got = torch.vmap(lambda s, t: ops.mux_rot(s, t, *mux))(xs, rows)
        assert same(got, backend.apply_mux_rot(flat(xs), per_sample, *mux))
        assert not same(got[1], backend.apply_mux_rot(xs[1], rows[0], *mux))          # (the rows differ: the order matters)
        got = torch.vmap(lambda s: ops.mux_rot(s, rows[2], *mux))(xs)
        assert same(got, backend.apply_mux_rot(flat(xs), rows[2], *mux))
        cross = lambda u, v: ops.mux_cross(u, v, *mux)  # noqa: E731
        assert same(torch.vmap(cross)(xs, other), backend.mux_cross(flat(xs), flat(other).contiguous(), *mux))
        assert same(torch.vmap(lambda s: cross(s, s))(xs), backend.mux_cross(flat(xs), flat(xs), *mux))
        # only `a` mapped: it becomes per sample, the unmapped `c` stays one shared row
        a = torch.complex(rows, rows.flip(1))
        c = torch.complex(rows[0].flip(0), rows[1]) / 6
        for mode in ('gate', 'map'):
            got = torch.vmap(lambda s, t, mode=mode: ops.mux_axpby(s, t, c, *mux, mode))(xs, a)
            want = backend.apply_mux_axpby(flat(xs), a.unsqueeze(1).expand(3, 2, count).reshape(6, count), c, *mux, mode)
            assert same(got, want)
    else:
        p = UNIT[dt]
        kind, dagger = MUX[name][:2]
        target, tbits, controls = (f(p) for f in MUX[name][2:5])
        xs = states(p + 3)
        table = torch.from_numpy(_mux_ref.random_cs(len(tbits), 9)).to(DTYPES[dt].to_real()).to(device)
        assert kind == 'ry'
        got = torch.vmap(lambda s: ops.mux_apply(s, table, kind, target, tbits, controls, dagger))(xs)
        assert same(got, backend.apply_mux(xs.reshape(6, -1), table, kind, target, tbits, controls, dagger))


def negative_controls(dt):
    """The per-bin criterion of the binned nodes on reference tensors alone (no node, no kernel): each bin-shaped result --
    ga, gc, gtheta, the cross, its tangent -- passes as the closed forms give it and is rejected with (a) the bins indexed
    with ``bits`` reversed, (b) a shared row's gradient taken from sample 0 instead of the sum over the batch, (c) the
    conjugation on the wrong factor of the cross, (d) gtheta formed with rot(gy; +theta).  (b) is defined for the three
    gradients of a row and (d) for gtheta only; (a) and (c) for all five."""
    import pytest

    n, batch, mux = 8, 2, ('y', 3, (6, 0, 4), (2,))
    rng = np.random.default_rng(17)
    fam, rev = ref.MuxBins(n, *mux), ref.MuxBins(n, mux[0], mux[1], mux[2][::-1], mux[3])
    (_, x), (_, u), (_, gy), (_, dx), (_, du) = (gauss(rng, (batch, 1 << n), DTYPES[dt]) for _ in range(5))
    a, c, th = (bin_rows(rng, batch, fam.count, True, real)[0] for real in (False, False, True))
    pair = lambda f, p, q: f.norms(p) * f.norms(q)  # noqa: E731

    def grads(f, sign=1.0):
        _, ga, gc = ref.binned_axpby_vjp(f, x, a, c, 'gate', gy)
        gx = f.rot(gy, -sign * th)
        return ga, gc, 0.5 * f.cross(gx, x).imag

    def swapped(f):                                     # conj(u) G v -> u conj(G v): G is Hermitian, so cross(v, u)
        return f.cross(gy, x, 'i'), f.cross(gy, x), 0.5 * f.cross(x, f.rot(gy, -th)).imag

    right = dict(zip(('ga', 'gc', 'gtheta'), grads(fam)))
    scale = {'ga': pair(fam, x, gy).sum(0), 'gc': pair(fam, x, gy).sum(0), 'gtheta': pair(fam, gy, x).sum(0)}
    wrong = {key: {'a': r.sum(0), 'b': right[key][0], 'c': w.sum(0)} for key, r, w in zip(right, grads(rev), swapped(fam))}
    wrong['gtheta']['d'] = grads(fam, sign=-1.0)[2].sum(0)
    right = {key: v.sum(0) for key, v in right.items()}
    right['cross'], scale['cross'] = fam.cross(u, x), pair(fam, u, x)
    wrong['cross'] = {'a': rev.cross(u, x), 'c': fam.cross(x, u)}
    right['cross tangent'] = ref.binned_cross_jvp(fam, u, x, du, dx)
    scale['cross tangent'] = pair(fam, du, x) + pair(fam, u, dx)
    wrong['cross tangent'] = {'a': ref.binned_cross_jvp(rev, u, x, du, dx), 'c': ref.binned_cross_jvp(fam, x, u, dx, du)}
    assert sorted(len(w) for w in wrong.values()) == [2, 2, 3, 3, 4]
    for key, want in right.items():
        close_reduction(torch.from_numpy(want), want, scale[key], dt, f'negative control {dt}: {key} as it is')
        rounded = want.astype(np.complex64 if np.iscomplexobj(want) else np.float32)   # (a rounding of 6e-8 passes in both)
        if dt == 'c64':
            close_reduction(torch.from_numpy(rounded), want, scale[key], dt, f'negative control {dt}: {key} rounded to single')
        for letter, bad in wrong[key].items():
            with pytest.raises(AssertionError):
                close_reduction(torch.from_numpy(np.ascontiguousarray(bad)), want, scale[key], dt,
                                f'negative control {dt}: {key} with ({letter})')
