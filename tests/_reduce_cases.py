"""The paths of the reduction kernels (csrc/dq_reduce.hip: expect_pauli_kernel / finish_kernel, inner_kernel, probs_kernel,
marginal_chunk_kernel, gate_grad_kernel, gate_grad_multi_kernel, expect_zmulti_mfma_kernel, scale_zsigns_mfma_kernel), one row
per path and shape -- TEST INFRASTRUCTURE ONLY; runs on whatever device it is given.

A row names ONE path (a key of `PATHS`: what the mirrors in `_launch_geometry` must say of its launch) at the smallest n that
reaches it with the row's own bits, or says in `note` why it is not.  test_reduce_paths_cpu.py proves both, and that every
path has a row in each precision in which it exists.  Every row runs with batch 3 (the per-sample offsets of the state, the
workspace and the result) unless its path is about the batch, and with two inputs:

  'exact'   amplitudes whose real and imaginary parts are seeded integers in {-2 .. 2}, not normalised (`scale_z_signs`:
            integer coefficients in [-3, 3]).  Every product and every sum is an integer far below 2^53 -- below 2^24 where
            the kernel works in float (`probs`, the per-thread partial sums of complex64 `gate_grad_multi`; asserted) -- so
            the result is exact whatever the order of the additions and of the atomics, and must equal the reference BIT FOR
            BIT (`torch.equal`): index mapping, signs, phases, bin order and tile membership judged with no margin.
  'random'  a seeded normalised Gaussian state, judged by the project's own figures (nothing here is measured):
            sums       |got - ref| <= tau S, S the same sum over absolute values; tau = `_handler_cases.TAU_SUM` (1e-12) for
                       every kernel that accumulates in double; complex64 `gate_grad_multi` keeps float partial sums:
                       tau = 2 (m + 2) u, u = 2^-24, m = iterations x pairs_per_thread from the mirror (the derivation of
                       test_grid_paths_gpu.py::test_gate_grad_multi_tile_loop);
            probs      works in the state's precision: |got - ref| <= 3 u ref elementwise (two rounded products and one
                       rounded sum), u = 2^-24 / 2^-53;
            scale_z_signs   per component |got - ref| <= (u_T + (K + 1) 2^-53) |a| sum_k |c_k|.

Negative controls, from reference tensors only (`corruptions`, `Z_CONTROLS`): each row shows that its 'random' criterion
rejects what a broken version of its path would give; the 'exact' criterion rejects any non-zero change and needs none.

On the CPU the rows run against `CpuTestBackend`, fed the state as stored but widened to complex128 (the double adds a
complex64 state in float32; the kernels add in double) and with its result rounded once to the kernel's output type.  The
double takes |psi|^2 through a square root, so where it does (`CPU_INEXACT`) an 'exact' input is judged on the CPU by the
'random' criterion; on the GPU every 'exact' run is bit for bit.

What this table does not reach: more than one tile per workgroup of gate_grad_multi (n >= 22) and the second iteration of
every grid-stride loop -- test_grid_paths_gpu.py runs those -- and `run` > 0 of the marginal kernel beyond its smallest
shape (test_grid_paths_gpu.py::test_marginal_chunk_runs)."""

from __future__ import annotations

import random
from dataclasses import dataclass

import torch

import _grid_refs as R
import _handler_cases as hc
import _launch_geometry as G
from deepquantum_amd import backend

C64, C128 = torch.complex64, torch.complex128
INF = float('inf')
KINDS = ('exact', 'random')
BATCH = 3
#: on the CPU the double forms these through abs() ** 2, a square root squared: not exact on integers
CPU_INEXACT = ('marginal', 'probs', 'expect_z_multi')


@dataclass(frozen=True)
class Row:
    path: str                 # key of PATHS
    kernel: str               # 'marginal', 'gate_grad', 'gate_grad_multi', 'expect_pauli', 'inner', 'probs'
    n: int                    # index bits; `inner`: the count itself (not a power of two)
    c128: bool
    args: tuple = ()          # marginal: the bits; gate_grad: (targets, controls); gate_grad_multi: ((target, controls), ..);
                              # expect_pauli: (xmask, zmask)
    batch: int = BATCH
    seed: int = 0
    note: str = ''            # why a smaller n reaches the same path and is not the row (empty: n is the smallest)

    @property
    def dtype(self):
        return C128 if self.c128 else C64

    @property
    def prec(self):
        return 'c128' if self.c128 else 'c64'

    @property
    def id(self):
        if self.kernel == 'marginal':
            a = 'w' + '.'.join(map(str, self.args))
        elif self.kernel == 'gate_grad':
            a = 't' + '.'.join(map(str, self.args[0])) + ('-c' + '.'.join(map(str, self.args[1])) if self.args[1] else '')
        elif self.kernel == 'gate_grad_multi':
            a = '_'.join(f't{t}' + ('c' + '.'.join(map(str, c)) if c else '') for t, c in self.args)
        elif self.kernel == 'expect_pauli':
            a = f'x{self.args[0]:x}-z{self.args[1]:x}'
        else:
            a = 'all'
        return f'{self.path}-{self.kernel}-n{self.n}-{a}-b{self.batch}-{self.prec}'

    def variants(self) -> list:
        """The argument tuples the row runs with: a marginal also with its bit list shuffled, two targets in both orders."""
        if self.kernel == 'marginal' and len(self.args) > 1:
            sh = list(self.args)
            rng = random.Random(len(sh) * 100 + self.n)
            while tuple(sh) == self.args:
                rng.shuffle(sh)
            return [self.args, tuple(sh)]
        if self.kernel == 'gate_grad' and len(self.args[0]) == 2:
            return [self.args, (self.args[0][::-1], self.args[1])]
        return [self.args]


# ---- what the mirrors say of a row ----------------------------------------------------------------------------------------------
def tile_geometry(c128: bool) -> tuple[int, int, int]:
    """gate_grad_multi: tile bits T, contiguous low bits L, gates per launch (dq_reduce.hip:811)."""
    return (10, 3, 4) if c128 else (11, 4, 8)


def _popc(v: int) -> int:
    return bin(v).count('1')


def valid(row: Row, n: int, args=None) -> bool:
    """The row's arguments name only bits below ``n`` (and leave a gate room)."""
    args = row.args if args is None else args
    if row.kernel == 'marginal':
        return all(b < n for b in args)
    if row.kernel == 'gate_grad':
        return all(b < n for b in args[0] + args[1])
    if row.kernel == 'gate_grad_multi':
        return all(b < n for t, c in args for b in (t,) + tuple(c))
    if row.kernel == 'expect_pauli':
        return (args[0] | args[1]) >> n == 0
    return True


def geo(row: Row, n: int | None = None, args=None) -> dict:
    """The mirror's account of the row's launch (``n``: of the same arguments at another size, for the floor test; ``args``:
    of another variant) plus the row's own facts."""
    n = row.n if n is None else n
    args = row.args if args is None else args
    assert valid(row, n, args)
    if row.kernel == 'marginal':
        g = G.marginal(n, list(args), row.batch, row.c128)
        g.update(nw=len(args), bits=list(args))
    elif row.kernel == 'gate_grad':
        t, c = args
        g = G.gate_grad(n, len(t), len(c))
        g.update(k=len(t), nc=len(c), t0=0 in t, top_t=n - 1 in t, below=any(q < min(t) for q in c),
                 above=any(q > max(t) for q in c), between=any(min(t) < q < max(t) for q in c))
    elif row.kernel == 'gate_grad_multi':
        tile, low, per = tile_geometry(row.c128)
        la = G.gate_grad_multi(n, row.c128, list(args))
        g = dict(launches=la, route=la[0]['route'], sizes=[len(x['gates']) for x in la], T=tile, L=low, per_call=per)
    elif row.kernel == 'expect_pauli':
        xm, zm = args
        g = G.expect_pauli(n, xm)
        g.update(xmask=xm, zmask=zm, ny=_popc(xm & zm), low=(xm & -xm).bit_length() - 1 if xm else None, nx=_popc(xm))
    elif row.kernel == 'inner':
        g = G.inner(n)
        g.update(count=n)
    else:
        g = G.probs(row.batch << n)
        g.update(count=row.batch << n)
    g.update(n=n, kernel=row.kernel, c128=row.c128, batch=row.batch)
    return g


def _live(pos) -> int:
    """Entries of a MargGeom position list that are not its pad (62)."""
    return sum(p != 62 for p in pos)


def _held(g) -> int:
    """How many of the four thread-held chunk bits 8 .. 11 the mirrored MargGeom fills."""
    return _live(g['geom']['pos'][8:12])


def _first_candidate(g) -> int:
    """The index bit the launcher hands out first above the contiguous run (dq_reduce.hip:650-655): the lowest unmeasured
    one, or, where all are measured, the one with the lowest outcome bit."""
    un = [b for b in range(g['low'], g['n']) if b not in g['bits']]
    return un[0] if un else next(b for b in reversed(g['bits']) if b >= g['low'])


def _first_served(g) -> bool:
    """Chunk-local bit 8, the first a thread holds itself, is served first (:663-668); without one, the first bit above the run."""
    pos = g['geom']['pos']
    return g['c'] == g['low'] or pos[8 if g['c'] > 8 else g['low']] == _first_candidate(g)


def _histogram_ok(g) -> bool:
    """Histogram bit t stands for a measured bit of the chunk and for that bit's place in the outcome, lowest first (:670-682)."""
    ge, bits = g['geom'], g['bits']
    lo = [(ge['pos'][ge['lo_x'][t]], ge['lo_out'][t]) for t in range(ge['nlo'])]
    return all(bits[len(bits) - 1 - o] == b for b, o in lo) and [o for _, o in lo] == sorted({o for _, o in lo})


def _marg(f):
    return lambda g: g['kernel'] == 'marginal' and _histogram_ok(g) and _first_served(g) and f(g)


def _gg(f):
    return lambda g: g['kernel'] == 'gate_grad' and f(g)


def _ggm(f):
    return lambda g: g['kernel'] == 'gate_grad_multi' and g['route'] == 'tile' and f(g, g['launches'])


def _ep(f):
    return lambda g: g['kernel'] == 'expect_pauli' and f(g)


def _ny(ny, blocks):
    return _ep(lambda g: g['xmask'] and g['ny'] == ny and g['blocks'] == blocks and g['n'] > 1)


#: path -> what `geo` must say of a row that claims it
PATHS = {
    # marginal_chunk_kernel / marginal_impl (dq_reduce.hip:634-692)
    'marg-all-contiguous': _marg(lambda g: _held(g) == 0 and g['c'] == g['low'] and g['geom']['pos'][:g['c']] == list(range(g['c']))),
    'marg-pass1-bits-only': _marg(lambda g: _held(g) == 0 and _live(g['geom']['pos'][g['low']:8]) == g['c'] - g['low'] > 0),
    'marg-thread-bits-partial': _marg(lambda g: 0 < _held(g) < 4 and 1 << g['geom']['c'] < 4096),      # (the nx guard is live)
    'marg-full-chunk-one-workgroup': _marg(lambda g: _held(g) == 4 and g['geom']['c'] == 12 and g['blocks'] == 1 and not g['cpos']),
    'marg-block-sum-exclusive': _marg(lambda g: g['nlo'] == 0 and g['exclusive'] and g['blocks'] > 1),
    'marg-histogram-atomics': _marg(lambda g: g['qmask'] == 0 and g['nlo'] > 0 and not g['exclusive'] and g['nhi'] == 0
                                    and g['blocks'] == 2 and g['run'] == 0),
    'marg-thread-bit-exclusive': _marg(lambda g: g['qmask'] != 0 and g['exclusive'] and g['blocks'] > 1),
    'marg-outside-bits-atomics': _marg(lambda g: g['nhi'] > 0 and not g['exclusive'] and g['blocks'] == 4 and g['run'] == 0),
    'marg-run': _marg(lambda g: g['run'] > 0),
    # gate_grad_kernel (k = 1, 2)
    'gg-one-group': _gg(lambda g: g['groups'] == 1),
    'gg-part-of-a-workgroup': _gg(lambda g: 1 < g['groups'] < 256),
    'gg-two-workgroups': _gg(lambda g: g['blocks'] == 2),
    'gg-target-bit0': _gg(lambda g: g['t0'] and g['groups'] > 1),
    'gg-target-top': _gg(lambda g: g['top_t'] and g['groups'] > 1),
    'gg-controls-around': _gg(lambda g: g['k'] == 2 and g['below'] and g['between'] and g['above'] and g['groups'] > 1),
    'gg-target-orders': _gg(lambda g: g['k'] == 2 and g['groups'] > 1),
    # gate_grad_multi_kernel and backend.gate_grad_multi
    'ggm-gate-by-gate': lambda g: g['kernel'] == 'gate_grad_multi' and g['route'] == 'gate_grad',
    'ggm-one-tile': _ggm(lambda g, la: len(la) == 1 and la[0]['ntiles'] == 1 and all(d['cout'] == 0 for d in la[0]['desc'])
                         and {g['L'] - 1, g['L'], g['T'] - 1, 0} <= {d['tbit'] for d in la[0]['desc']}),
    'ggm-control-outside': _ggm(lambda g, la: la[0]['ntiles'] == 2 and any(d['cout'] and d['cin'] for d in la[0]['desc'])
                                and any(d['cout'] and not d['cin'] for d in la[0]['desc'])),
    'ggm-top-above-outside': _ggm(lambda g, la: la[0]['ntiles'] == 2 and la[0]['outside'][0] < la[0]['tile_bits'][-1]
                                  and la[0]['outside'][0] > g['L']),
    'ggm-seven-high-outside-L': _ggm(lambda g, la: len(la) == 1 and len(la[0]['high_targets']) == 7 and la[0]['outside'] == [g['L']]),
    'ggm-split-by-high-targets': _ggm(lambda g, la: g['sizes'] == [7, 1] and len(la[0]['high_targets']) == 7),
    'ggm-split-by-gate-count': _ggm(lambda g, la: g['sizes'] == [g['per_call'], 1]),
    'ggm-repeated-target': _ggm(lambda g, la: len(la) == 1 and len({d['tbit'] for d in la[0]['desc']}) < len(la[0]['desc'])
                                and len({(d['tbit'], d['cin']) for d in la[0]['desc']}) == len(la[0]['desc'])),
    # expect_pauli_kernel / finish_kernel
    'ep-one-qubit': _ep(lambda g: g['n'] == 1 and (g['xmask'] or g['zmask'])),
    'ep-z-one-workgroup': _ep(lambda g: not g['xmask'] and g['zmask'] and g['blocks'] == 1 and g['n'] > 1),
    'ep-z-two-workgroups': _ep(lambda g: not g['xmask'] and g['zmask'] and g['blocks'] == 2),
    'ep-lowx-bit0': _ep(lambda g: g['low'] == 0 and g['nx'] >= 2),
    'ep-lowx-middle': _ep(lambda g: g['low'] is not None and 0 < g['low'] < g['n'] - 1),
    'ep-lowx-top': _ep(lambda g: g['low'] == g['n'] - 1 and g['n'] > 1),
    **{f'ep-ny{ny}-one-workgroup': _ny(ny, 1) for ny in range(4)},
    **{f'ep-ny{ny}-two-workgroups': _ny(ny, 2) for ny in range(4)},
    'ep-identity': _ep(lambda g: not g['xmask'] and not g['zmask']),
    # inner_kernel, probs_kernel
    'inner-one-element': lambda g: g['kernel'] == 'inner' and g['count'] == 1,
    'inner-part-of-a-workgroup': lambda g: g['kernel'] == 'inner' and 1 < g['count'] < 256,
    'inner-ragged-two-workgroups': lambda g: g['kernel'] == 'inner' and g['blocks'] == 2 and g['count'] % 256,
    'inner-ragged-four-workgroups': lambda g: g['kernel'] == 'inner' and g['blocks'] == 4 and g['count'] % 256,
    'probs-a-workgroup-and-a-half': lambda g: g['kernel'] == 'probs' and g['blocks'] == 2 and g['count'] % 256 == 128,
    'probs-part-of-a-wave': lambda g: g['kernel'] == 'probs' and g['count'] < 64,
}

#: paths that exist in one precision only
C64_ONLY = ('marg-run', 'ggm-seven-high-outside-L', 'ggm-split-by-high-targets')

ANY_N = 'the path does not depend on n: '


def _rows():
    out = []
    both = (False, True)

    def add(path, kernel, n, args=(), prec=both, **kw):
        for c128 in prec:
            a = args(c128) if callable(args) else args
            nn = n(c128) if callable(n) else n
            out.append(Row(path, kernel, nn, c128, a, seed=len(out), **kw))

    # ---- marginal: low = 6 (complex64) / 7 (complex128) contiguous bits, c = min(n, 12) ----
    m = lambda path, n, bits, **kw: add(path, 'marginal', n, tuple(bits), **kw)                  # noqa: E731
    m('marg-all-contiguous', 1, [0])
    m('marg-all-contiguous', 5, [4, 0])
    m('marg-all-contiguous', 7, [6], prec=[True])
    m('marg-all-contiguous', 7, [0, 6, 3], prec=[True])
    m('marg-pass1-bits-only', 7, [6], prec=[False])
    m('marg-pass1-bits-only', 7, [0, 6, 3], prec=[False])
    m('marg-pass1-bits-only', 8, [7], prec=[True])
    m('marg-pass1-bits-only', 8, [0, 7, 3], prec=[True])
    m('marg-thread-bits-partial', 9, [8])
    m('marg-thread-bits-partial', 10, [9, 8])
    m('marg-thread-bits-partial', 11, [0], note='n = 9 is the row above; n = 11 leaves one of the four thread-held bits out')
    m('marg-full-chunk-one-workgroup', 12, [11])
    m('marg-full-chunk-one-workgroup', 12, range(12))
    m('marg-full-chunk-one-workgroup', 12, range(11, -1, -1))
    m('marg-block-sum-exclusive', 13, [12])
    m('marg-block-sum-exclusive', 13, [7])
    m('marg-histogram-atomics', 13, [0])
    m('marg-thread-bit-exclusive', 13, [8, 9, 10, 11])
    m('marg-thread-bit-exclusive', 13, range(13))
    m('marg-thread-bit-exclusive', 13, range(12, -1, -1))
    m('marg-outside-bits-atomics', 14, [13])
    m('marg-outside-bits-atomics', 14, [0, 13])
    m('marg-run', 13, [0], prec=[False], batch=2048)
    # ---- gate_grad ----
    gg = lambda path, n, t, c=(), **kw: add(path, 'gate_grad', n, (tuple(t), tuple(c)), **kw)      # noqa: E731
    gg('gg-one-group', 1, [0])
    gg('gg-one-group', 2, [0, 1])
    gg('gg-one-group', 3, [2, 0], [1])
    gg('gg-part-of-a-workgroup', 2, [1])
    gg('gg-part-of-a-workgroup', 6, [4, 1], [2], note='n = 5 reaches it with four groups; n = 6 puts free bits below, between and above')
    gg('gg-two-workgroups', 10, [5])
    gg('gg-two-workgroups', 11, [3, 9])
    gg('gg-target-bit0', 3, [0], [2])
    gg('gg-target-bit0', 4, [0, 3], [2])
    gg('gg-target-top', 4, [3], [1])
    gg('gg-target-top', 5, [4, 1])
    gg('gg-controls-around', 7, [2, 4], [0, 3, 6])
    gg('gg-target-orders', 4, [1, 3])
    # ---- gate_grad_multi: T = 11, L = 4 (complex64); T = 10, L = 3 (complex128) ----
    T = lambda c: tile_geometry(c)[0]                                                              # noqa: E731
    L = lambda c: tile_geometry(c)[1]                                                              # noqa: E731
    ggm = lambda path, n, gates, **kw: add(path, 'gate_grad_multi', n, gates, **kw)                # noqa: E731
    one_tile = lambda c: ((0, ()), (L(c) - 1, (T(c) - 1,)), (L(c), (0, L(c) + 1)), (T(c) - 1, (L(c) - 1,)))      # noqa: E731
    ggm('ggm-gate-by-gate', lambda c: T(c) - 1, lambda c: tuple((t, tuple(q for q in ct if q < T(c) - 1)) for t, ct in one_tile(c)[:3]),
        note='every n below the tile goes gate by gate; this is the largest, the other side of the threshold of backend.py:491')
    ggm('ggm-one-tile', T, one_tile)
    ggm('ggm-control-outside', lambda c: T(c) + 1, lambda c: ((2, (T(c), 1)), (L(c) + 1, (T(c),)), (0, ())))
    ggm('ggm-top-above-outside', lambda c: T(c) + 1, lambda c: ((T(c), ()), (0, (T(c) - 1,)), (T(c), (T(c) - 1, 1))))
    ggm('ggm-seven-high-outside-L', 12, tuple((t, (4,) if t == 7 else ()) for t in range(5, 12)), prec=[False])
    ggm('ggm-split-by-high-targets', 12, tuple((t, ()) for t in range(4, 12)), prec=[False])
    ggm('ggm-split-by-gate-count', T, lambda c: tuple((t % T(c), ((t + 3) % T(c),) if t % 2 else ()) for t in range(tile_geometry(c)[2] + 1)))
    ggm('ggm-repeated-target', T, ((5, (0,)), (5, (1,)), (5, ()), (0, (5,))))
    # ---- expect_pauli ----
    ep = lambda path, n, x, z, **kw: add(path, 'expect_pauli', n, (x, z), **kw)                    # noqa: E731
    ep('ep-one-qubit', 1, 1, 0)
    ep('ep-one-qubit', 1, 1, 1)
    ep('ep-one-qubit', 1, 0, 1)
    ep('ep-z-one-workgroup', 2, 0, 0b11)
    ep('ep-z-one-workgroup', 8, 0, 0b101, note='n = 2 is the row above; n = 8 is one full workgroup')
    ep('ep-z-two-workgroups', 9, 0, 0b100010011)
    ep('ep-lowx-bit0', 3, 0b101, 0b010)
    ep('ep-lowx-middle', 3, 0b110, 0b001)
    ep('ep-lowx-middle', 10, 0b0100100000, 0b0000100001, note='n = 3 is the row above; here two workgroups and a Y on the lowest X bit')
    ep('ep-lowx-top', 3, 0b100, 0b011)
    ep('ep-lowx-top', 10, 1 << 9, 0b0110000001)
    for ny, (x, z) in enumerate([(0b011, 0b100), (0b011, 0b101), (0b011, 0b111), (0b111, 0b111)]):
        ep(f'ep-ny{ny}-one-workgroup', 3, x, z)
    top = 1 << 9
    for ny, (x, z) in enumerate([(top | 1, 0b10), (top | 1, top | 0b10), (top | 0b101, top | 0b1100), (top | 0b10101, top | 0b10100)]):
        ep(f'ep-ny{ny}-two-workgroups', 10, x, z)
    ep('ep-identity', 1, 0, 0)
    ep('ep-identity', 9, 0, 0, note=ANY_N + 'n = 9 has two workgroups')
    # ---- inner (n is the count), probs ----
    add('inner-one-element', 'inner', 1)
    add('inner-part-of-a-workgroup', 'inner', 255, note='every count from 2 on; 255 leaves exactly one thread idle')
    add('inner-ragged-two-workgroups', 'inner', 257)
    add('inner-ragged-four-workgroups', 'inner', 1000, note='769 is the smallest; 1000 = 3 * 256 + 232, neither a power of two nor a multiple of 64')
    add('probs-a-workgroup-and-a-half', 'probs', 7)
    add('probs-part-of-a-wave', 'probs', 1)
    return out


ROWS = _rows()


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def input_state(batch: int, size: int, dtype, kind: str, seed: int, device) -> torch.Tensor:
    """(batch, size), made on the host (the same on every device).  'exact': components in {-2 .. 2}; 'random': normalised."""
    g = torch.Generator().manual_seed(seed)
    if kind == 'exact':
        x = torch.view_as_complex(torch.randint(-2, 3, (batch, size, 2), generator=g).to(torch.float64))
    else:
        x = torch.view_as_complex(torch.randn(batch, size, 2, generator=g, dtype=torch.float64))
        x = x / x.norm(dim=-1, keepdim=True)
    return x.to(dtype).to(device).contiguous()


def row_inputs(row: Row, kind: str, device):
    size = row.n if row.kernel == 'inner' else 1 << row.n
    x = input_state(row.batch, size, row.dtype, kind, 7000 + 2 * row.seed, device)
    two = row.kernel in ('gate_grad', 'gate_grad_multi', 'inner')
    return x, (input_state(row.batch, size, row.dtype, kind, 7001 + 2 * row.seed, device) if two else None)


def _wide(t):
    """What the kernel under test is handed: the tensor itself on the GPU; on the CPU the same values in complex128."""
    return t if t is None or t.is_cuda else t.to(C128)


# ---- the kernels --------------------------------------------------------------------------------------------------------------
def run_kernel(row: Row, args, x, y) -> torch.Tensor:
    xs, ys = _wide(x), _wide(y)
    if row.kernel == 'marginal':
        return backend.marginal(xs, list(args))
    if row.kernel == 'gate_grad':
        return backend.gate_grad(xs, ys, list(args[0]), list(args[1]))
    if row.kernel == 'gate_grad_multi':
        return backend.gate_grad_multi(xs, ys, [(t, tuple(c)) for t, c in args])
    if row.kernel == 'expect_pauli':
        return backend.expect_pauli(xs, *args)
    if row.kernel == 'inner':
        return backend.inner(xs, ys)
    return backend.probs(xs).to(x.real.dtype)


# ---- references ---------------------------------------------------------------------------------------------------------------
def pauli_sum(psi, xmask: int, zmask: int, partner: int | None = None):
    """sum_i conj(psi_i) psi_{i ^ x} (-1)^popc((i ^ x) & z) as the kernel pairs it (dq_reduce.hip:57-82), complex128 (B,), and
    S.  ``partner``: the mask the pair partner is taken at (the negative control; default the X mask itself)."""
    y = psi.to(C128)
    i = torch.arange(psi.shape[-1], device=psi.device)
    if not xmask:
        p = R.probabilities(psi)
        return torch.complex((p * R.z_sign(i, zmask)).sum(-1), torch.zeros_like(p[:, 0])), p.sum(-1)
    low = (xmask & -xmask).bit_length() - 1
    i = i[((i >> low) & 1) == 0]
    k = i ^ (xmask if partner is None else partner)
    c = y[:, i].conj() * y[:, k]
    sk, si = R.z_sign(k, zmask), R.z_sign(i, zmask)
    val = torch.complex(((sk + si) * c.real).sum(-1), ((sk - si) * c.imag).sum(-1))
    return val, 2 * (y[:, i].abs() * y[:, k].abs()).sum(-1)


def pauli_value(s, ny: int):
    """Re(i^ny s), the four branches of finish_kernel (dq_reduce.hip:104-109)."""
    return [s.real, -s.imag, -s.real, s.imag][ny & 3].clone()


def multi_cross(x, y, gates):
    vals, ss = zip(*(R.cross(x, y, [t], list(c)) for t, c in gates))
    return torch.stack(vals, dim=1), torch.stack(ss, dim=1)


def reference(row: Row, args, x, y):
    """-> (ref, S): the value in float64 / complex128 and the same sum over absolute values (probs: the value itself)."""
    if row.kernel == 'marginal':
        ref = R.marginal(x, list(args))
        return ref, ref
    if row.kernel == 'gate_grad':
        return R.cross(x, y, list(args[0]), list(args[1]))
    if row.kernel == 'gate_grad_multi':
        return multi_cross(x, y, args)
    if row.kernel == 'expect_pauli':
        s, sa = pauli_sum(x, *args)
        return pauli_value(s, _popc(args[0] & args[1])), sa
    if row.kernel == 'inner':
        return R.inner(x, y)
    ref = R.probabilities(x)
    return ref, ref


# ---- criteria -----------------------------------------------------------------------------------------------------------------
def tau(row: Row, g: dict) -> float:
    if row.kernel == 'probs':
        return 3 * hc.U[row.c128]
    if row.kernel == 'gate_grad_multi' and not row.c128 and g['route'] == 'tile':
        m = max(la['iterations'] * la['pairs_per_thread'] for la in g['launches'])
        return 2 * (m + 2) * hc.U[False]
    return hc.TAU_SUM


def _as64(t):
    return t.to(C128) if t.is_complex() else t.to(torch.float64)


def ratio(got, ref, s, tau_) -> float:
    """max |got - ref| / (tau S); 0 / 0 counts as 0, anything else over 0 and a NaN as inf."""
    d = (_as64(got) - ref).abs()
    bound = tau_ * s
    r = torch.where((d == 0) & (bound == 0), torch.zeros_like(d), d / bound)
    return float(torch.nan_to_num(r, nan=INF).max())


def bits_equal(got, ref) -> bool:
    a, b = _as64(got), ref
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    return a.shape == b.shape and torch.equal(a, b)


def exact_headroom(row: Row, s) -> None:
    """The sums a kernel forms in float stay below 2^24 on the 'exact' input (S bounds every partial sum of a component)."""
    if row.kernel == 'probs' or (row.kernel == 'gate_grad_multi' and not row.c128):
        assert float(s.max()) < 2 ** 24, f'{row.id}: partial sums up to {float(s.max())}'
    assert float(s.max()) < 2 ** 50


# ---- negative controls --------------------------------------------------------------------------------------------------------
CONTROLS = ('marginal-outcome-bits-exchanged', 'marginal-last-chunk-dropped', 'gate_grad-last-group-dropped',
            'gate_grad-targets-exchanged', 'multi-outside-control-ignored', 'multi-outside-control-on-the-wrong-tile',
            'multi-last-group-dropped', 'pauli-ny-off-by-one', 'pauli-partner-at-lowbit', 'inner-tail-dropped',
            'probs-tail-unwritten')


def _last_group(x, y, n, t, c):
    """What the group with every free bit at 1 adds to cross(x, y, t, c): (B, D, D)."""
    a, r = R.cross_index(n, list(t), list(c), x.device)
    idx = a | r[-1]
    return y[:, idx].to(C128).unsqueeze(2) * x[:, idx].to(C128).conj().unsqueeze(1)


def corruptions(row: Row, g: dict, args, x, y, ref) -> list:
    """[(what, result)]: the reference as a broken version of the row's path would leave it."""
    out = []
    n = row.n
    if row.kernel == 'marginal':
        bits = list(args)
        if len(bits) >= 2:
            out.append((CONTROLS[0], R.marginal(x, [bits[1], bits[0]] + bits[2:])))
        # the chunk whose number is all ones: every index bit outside the chunk at 1 (the last workgroup's last chunk)
        om = sum(1 << p for p in g['cpos'])
        i = torch.arange(1 << n, device=x.device)
        keep = (i & om) != om if om else torch.zeros_like(i, dtype=torch.bool)
        xm = torch.where(keep, x, torch.zeros_like(x))
        out.append((CONTROLS[1], R.marginal(xm, bits)))
    elif row.kernel == 'gate_grad':
        t, c = args
        out.append((CONTROLS[2], ref - _last_group(x, y, n, t, c)))
        if len(t) == 2:
            out.append((CONTROLS[3], R.cross(x, y, list(t[::-1]), list(c))[0]))
    elif row.kernel == 'gate_grad_multi':
        bad = ref.clone()
        for gi, (t, c) in enumerate(args):
            bad[:, gi] -= _last_group(x, y, n, [t], c)
        out.append((CONTROLS[6], bad))
        if g['route'] == 'tile':
            ign, wrong, any_out = ref.clone(), ref.clone(), False
            for la in g['launches']:
                for gi, d in zip(la['gates'], la['desc']):
                    if d['cout']:
                        t, c = args[gi]
                        inside = [q for q in c if not (d['cout'] >> q) & 1]
                        ign[:, gi] = R.cross(x, y, [t], inside)[0]
                        wrong[:, gi] = ign[:, gi] - ref[:, gi]       # (one outside control: the tiles where it is 0)
                        any_out = True
            if any_out:
                out += [(CONTROLS[4], ign), (CONTROLS[5], wrong)]
    elif row.kernel == 'expect_pauli':
        xm, zm = args
        ny = _popc(xm & zm)
        s = pauli_sum(x, xm, zm)[0]
        out.append((CONTROLS[7], pauli_value(s, ny + 1)))
        if _popc(xm) >= 2:
            out.append((CONTROLS[8], pauli_value(pauli_sum(x, xm, zm, partner=xm & -xm)[0], ny)))
    elif row.kernel == 'inner':
        tail = n % 256
        if tail:
            out.append((CONTROLS[9], R.inner(x[:, : n - tail], y[:, : n - tail])[0]))
    else:
        bad = ref.reshape(-1).clone()
        bad[-(bad.numel() % 256 or 256):] = 0
        out.append((CONTROLS[10], bad.reshape(ref.shape)))
    return out


def run_row(row: Row, device) -> dict:
    """Runs the row on ``device`` with both inputs and every variant and asserts its path, its criteria and its negative
    controls; -> dict(ratio: the worst |got - ref| / (tau S) of the 'random' input, controls: the names it rejected)."""
    worst, seen = 0.0, set()
    on_gpu = torch.device(device).type == 'cuda'
    for args in row.variants():
        g = geo(row, args=args)
        assert PATHS[row.path](g), f'{row.id} {args}: the mirror does not say {row.path}: {g}'
        for kind in KINDS:
            x, y = row_inputs(row, kind, device)
            x0 = x.clone()
            ref, s = reference(row, args, x, y)
            got = run_kernel(row, args, x, y)
            assert torch.equal(torch.view_as_real(x), torch.view_as_real(x0)), f'{row.id}: the input changed'
            assert got.shape == ref.shape, (row.id, got.shape, ref.shape)
            r = ratio(got, ref, s, tau(row, g))
            if kind == 'exact':
                exact_headroom(row, s)
                if on_gpu or row.kernel not in CPU_INEXACT and not (row.kernel == 'expect_pauli' and not args[0]):
                    assert bits_equal(got, ref), f'{row.id} {args} (exact): not bit for bit, |got - ref| up to {float((_as64(got) - ref).abs().max())}'
                else:
                    assert r <= 1.0, f'{row.id} {args} (exact, by the bound): {r:.3e}'
                continue
            assert r <= 1.0, f'{row.id} {args} (random): worst |got - ref| / (tau S) = {r:.3e}'
            worst = max(worst, r)
            for what, bad in corruptions(row, g, args, x, y, ref):
                assert ratio(bad, ref, s, tau(row, g)) > 1.0, f'{row.id} {args}: the criterion does not see {what}'
                seen.add(what)
    return dict(ratio=worst, controls=seen)


# ---- the Z-string kernels on the matrix cores (n >= 8) ------------------------------------------------------------------------
Z_NS = (8, 9, 10, 11, 12)
Z_KS = {'sums': (16, 17, 32), 'scale': (1, 4, 5, 32), 'scale-two-launches': (33,)}
Z_WHAT = tuple(Z_KS)
Z_ROWS = [(n, c128, what) for what in Z_WHAT for n in Z_NS for c128 in (False, True)]
Z_IDS = [f'{what}-n{n}-{"c128" if c else "c64"}' for n, c, what in Z_ROWS]
Z_CONTROLS = ('z-slices-past-0-dropped', 'z-last-string-dropped')


def z_structured(n: int) -> list[int]:
    """The masks that isolate one factor of the kernels' sign decomposition: a bit below 4 is s_k(j); bits 4, 5 are
    s_k(16 q); bits 6, 7 the wave's share of i0; bits 8 .. 10 (complex128: 8, 9) the slice number (pu0 / pu1), the bits
    above them the workgroup; then all of them, none, and pairs that straddle the factors."""
    pairs = [(3, 4), (7, 8), (10, 11)]
    return [1 << p for p in range(n)] + [(1 << n) - 1, 0] + [1 << a | 1 << b for a, b in pairs if b < n]


def z_masks(n: int, k: int, rotated: bool) -> list[int]:
    """``k`` masks: the structured ones, a seeded fill up to 32 (33), as given or rotated by 16 places, cut to the first
    ``k``.  At K = 32 every structured mask sits once among the strings 0 .. 15 (acc0) and once among 16 .. 31 (acc1).  At
    K = 16 and 17 only acc0 (and string 16) is used: there the list as given holds the first 16 (17) structured masks and
    the rotated list the rest of them and the seeded fill -- at n = 12, with 17 structured masks, bits 10|11 is string 16
    as given and string 0 rotated -- so the structured masks meet acc1 at K = 32 alone."""
    rng = random.Random(31 * n)
    full = z_structured(n)
    full += [rng.randrange(1, 1 << n) for _ in range(max(32, k) - len(full))]
    if rotated:
        full = full[16:] + full[:16]
    return full[:k]


def z_inputs(n: int, c128: bool, k: int, kind: str, device):
    x = input_state(BATCH, 1 << n, C128 if c128 else C64, kind, 8000 + n, device)
    g = torch.Generator().manual_seed(100 * n + k)
    if kind == 'exact':
        coef = torch.randint(-3, 4, (BATCH, k), generator=g).to(torch.float64)
    else:
        coef = torch.randn(BATCH, k, generator=g, dtype=torch.float64)
    return x, coef.to(device)


def scale_bound(x, coef, c128: bool):
    """(u_T + (K + 1) 2^-53) |a| sum_k |c_k| per component: (B, 2^n, 2)."""
    k = coef.shape[1]
    f = hc.U[c128] + (k + 1) * 2.0 ** -53
    return f * torch.view_as_real(x).to(torch.float64).abs() * coef.abs().sum(-1).reshape(-1, 1, 1)


def _scale_ratio(got, ref, bound) -> float:
    d = (torch.view_as_real(got.to(C128)) - torch.view_as_real(ref)).abs()
    r = torch.where((d == 0) & (bound == 0), torch.zeros_like(d), d / bound)
    return float(torch.nan_to_num(r, nan=INF).max())


def run_z_row(n: int, c128: bool, what: str, device) -> dict:
    """One of `Z_WHAT` at ``n`` with the mask list as given and rotated, both inputs, batch 3: 'sums' expect_z_multi at K = 16,
    17, 32; 'scale' scale_z_signs at K = 1, 4, 5, 32 (one launch); 'scale-two-launches' at K = 33 (backend.scale_z_signs: 32 + 1
    strings, the launches added in complex128 whatever the state's precision).  -> dict(ratio: the worst ratio of
    the 'random' input to its bound, figures: [(what, ratio)], controls: the negative controls it rejected).  Every figure
    is printed before the first of them is judged."""
    on_gpu = torch.device(device).type == 'cuda'
    dtype = C128 if c128 else C64
    zg = G.expect_zmulti(n, c128)
    i = torch.arange(1 << n, device=device)
    figures, seen = [], set()
    for rotated in (False, True):
        for kind in KINDS:
            for k in Z_KS[what]:
                masks = z_masks(n, k, rotated)
                x, coef = z_inputs(n, c128, k, kind, device)
                tag = f'{what} n={n} K={k} {"rotated" if rotated else "as given"} {"c128" if c128 else "c64"}'
                if what == 'sums':
                    ref, s = R.expect_z_multi(x, masks)
                    got = backend.expect_z_multi(_wide(x), masks)
                    r = ratio(got, ref, s, hc.TAU_SUM)
                    if kind == 'exact' and on_gpu:
                        assert bits_equal(got, ref), f'{tag}: not bit for bit'
                    if kind == 'exact':
                        assert r <= 1.0, f'{tag} (exact, by the bound): {r:.3e}'
                        continue
                    figures.append((tag, r))
                    if zg['u'] > 1 and (1 << n) > 256:      # (n = 8 has no slice past u = 0)
                        xm = torch.where((i >> 8) % zg['u'] == 0, x, torch.zeros_like(x))
                        assert ratio(R.expect_z_multi(xm, masks)[0], ref, s, hc.TAU_SUM) > 1.0, Z_CONTROLS[0]
                        seen.add(Z_CONTROLS[0])
                    continue
                ref = R.scale_z_signs(x, masks, coef)
                got = backend.scale_z_signs(_wide(x), masks, coef).to(dtype)
                assert got.shape == x.shape
                if kind == 'exact':
                    assert float(ref.abs().max()) < 2 ** 24
                    assert bits_equal(got, ref), f'{tag}: not bit for bit'
                    continue
                bound = scale_bound(x, coef, c128)
                figures.append((tag, _scale_ratio(got, ref, bound)))
                if k > 1:
                    bad = R.scale_z_signs(x, masks[:-1], coef[:, :-1])
                    assert _scale_ratio(bad, ref, bound) > 1.0, Z_CONTROLS[1]
                    seen.add(Z_CONTROLS[1])
    for tag, r in figures:
        print(f'ZFIGURE {tag}: {r:.3e} of its bound')
    bad = [(tag, f'{r:.3e}') for tag, r in figures if not r <= 1.0]
    assert not bad, f'over the bound: {bad}'
    return dict(ratio=max(r for _, r in figures), figures=figures, controls=seen)
