"""The paths of the single-gate kernels behind `dq_apply_gate_*` (csrc/dq_gate.hip: apply_small_kernel, copy_uncontrolled_kernel,
apply_big_kernel; csrc/dq_dense.hip: apply_dense56_kernel, apply_dense_mfma_kernel), one row per path and shape -- TEST
INFRASTRUCTURE ONLY; runs on whatever device it is given.

A row names ONE path (a key of `PATHS`: what the mirrors `_launch_geometry.small_gate` / `.dense` must say of its launch) and
is the smallest n that reaches it, or says in `note` why it is not.  test_gate_paths_cpu.py proves both, and that every
route has a row.

Every row runs with two matrices:
  (a) 'unitary'  a seeded random unitary.  Elementwise |got - ref| <= tau S with S[r, c] = sum_j |U[r, j]| |x[j, c]|, taken in
                 float64 from the inputs as stored.  complex128: tau = 1e-12 (`_handler_cases.TAU_SUM`, the project's figure
                 for double accumulation).  complex64: tau = 2 (m + 2) u, u = 2^-24, m = 2 * 2^k the float additions behind
                 one component of an output; the factor 2 covers the complex modulus and a product that is rounded before
                 it is added (the small kernels' cfma; the matrix cores fuse).  Derived, not measured; DESIGN.md 4.2 holds
                 the measured ratios.
  (b) 'perm'     a seeded signed permutation, one entry of {1, -1, i, -i} per row and column: every product is exact, every
                 sum has one non-zero term, so the output equals the reference bit for bit (`torch.equal`) -- gather,
                 scatter, target order, sample split and tile mapping judged with no tolerance.
Both bit for bit: amplitudes whose controls are not all 1 equal the input (every output starts as NaN); for k <= 4 the
result in place equals the result out of place.

The reference is `_grid_refs.apply_gate` in complex128 (held against `oracle.apply_gate_bits` in test_gate_paths_cpu.py).

Negative controls, from reference tensors only (`corruptions`): the K chunk of 16 (complex128: 32) columns of U dropped for
the last row tile; the last column group / tile / workgroup left at its input; two targets exchanged in the matrix index;
where a column group spans samples, the sample of lane 0 read by the whole group; for the wide instantiation the second
amplitude of every pair left at its input.

What this table does not reach, and does not pretend to:
  - the grid-stride loop of apply_small_kernel: the grid is capped at 2^20 workgroups of 256, a second iteration needs more
    than 2^28 groups per sample (n >= 29: 4 GiB and more);
  - the non-temporal instantiations at their natural size (a state of 1 GiB): test_grid_paths_gpu.py runs those; here they
    run at small sizes under DQ_DENSE_NT=1 (the knob test).
"""

from __future__ import annotations

import functools
import hashlib
import itertools
import random
from dataclasses import dataclass

import torch

import _grid_refs as R
import _handler_cases as hc
import _launch_geometry as G
from deepquantum_amd import _lib, backend

C64, C128 = torch.complex64, torch.complex128
INF = float('inf')
KINDS = ('unitary', 'perm')


@dataclass(frozen=True)
class Row:
    path: str                 # key of PATHS (KNOB_ROWS: of the default environment)
    n: int
    targets: tuple            # targets[0] = matrix-index MSB
    controls: tuple = ()
    batch: int = 1
    c128: bool = False
    shared: bool = True       # ONE matrix for the batch (False: one per sample; needs batch >= 2)
    in_place: bool = False    # the launch the path speaks of (k <= 4 always runs both)
    valu: bool = False        # dq_set_dense_path(0)
    all_orders: bool = False  # every order of the targets
    seed: int = 0
    note: str = ''            # why a smaller n reaches the same path and is not the row (empty: n is the smallest)

    @property
    def k(self):
        return len(self.targets)

    @property
    def nc(self):
        return len(self.controls)

    @property
    def dtype(self):
        return C128 if self.c128 else C64

    @property
    def id(self):
        bits = 't' + '.'.join(map(str, self.targets)) + ('-c' + '.'.join(map(str, self.controls)) if self.controls else '')
        return (f'{self.path}-n{self.n}-{bits}-b{self.batch}-{"shared" if self.shared else "persample"}-'
                f'{"c128" if self.c128 else "c64"}')

    def variants(self):
        return list(itertools.permutations(self.targets)) if self.all_orders else [self.targets]


# ---- what the mirror says of a row --------------------------------------------------------------------------------------------
def geo(row: Row, n: int | None = None, **knobs) -> dict:
    """The mirror's account of the row's launch (``n``: of the same gate at another size, for the floor test: with no free
    bit left index bit 0 is used whatever the row says) plus the row's own facts.  ``knobs``: `_launch_geometry.dense`'s."""
    n = row.n if n is None else n
    k, nc = row.k, row.nc
    free = n - k - nc
    bit0 = 0 in row.targets or 0 in row.controls or free == 0
    if k <= 4:
        g = G.small_gate(n, k, nc, row.c128, bit0, row.in_place)
        g['kernel'] = 'small'
    elif row.valu:
        g = dict(kernel='valu', blocks=min(-(-(1 << n) // 256), 1 << 20))                  # dq_gate.hip:243-244
    else:
        g = G.dense(n, k, nc, row.batch, row.c128, row.shared, bit0, launch=True, **knobs)
        g['kernel'] = g['route']
    top = row.n - 1
    g.update(n=n, k=k, nc=nc, free=free, batch=row.batch, shared=row.shared, c128=row.c128, bit0_used=bit0,
             t0=0 in row.targets, c0=0 in row.controls, top_t=top in row.targets, top_c=top in row.controls,
             in_place=row.in_place, all_orders=row.all_orders, ncols=(row.batch if row.shared else 1) << free,
             ctrl_above=bool(row.controls) and max(row.controls) > max(row.targets),
             ctrl_below=bool(row.controls) and min(row.controls) < min(row.targets))
    return g


def _small(g):
    return g['kernel'] == 'small'


def _staged2(k, shared):
    return lambda g: (g['kernel'] == 'staged2' and g['k'] == k and g['grid'][1] == 1 << (k - 6) and g['shared'] == shared
                      and g['rows_fast'] == shared and g['free'] >= 1)


#: path -> what `geo` must say of a row that claims it
PATHS = {
    # apply_small_kernel
    'small-one-group': lambda g: _small(g) and g['free'] == 0 and g['groups'] == 1 and not g['wide'] and g['in_place'],
    'wide-one-pair': lambda g: _small(g) and g['wide'] and g['groups'] == 1 and g['nc'] == 0,
    'wide-one-pair-controlled': lambda g: _small(g) and g['wide'] and g['groups'] == 1 and g['nc'] == 1,
    'wide-many-workgroups': lambda g: _small(g) and g['wide'] and g['blocks'] > 1,
    'narrow-bit0-target': lambda g: _small(g) and g['k'] <= 3 and g['free'] >= 1 and g['t0'] and not g['wide'],
    'narrow-bit0-control': lambda g: _small(g) and g['k'] <= 3 and g['free'] >= 1 and g['c0'] and not g['wide'],
    'k4-bit0-free': lambda g: _small(g) and g['k'] == 4 and g['free'] >= 1 and not g['bit0_used'] and not g['wide'],
    'top-target': lambda g: _small(g) and g['top_t'] and g['free'] >= 1,
    'top-control': lambda g: _small(g) and g['top_c'] and g['free'] >= 1,
    'target-orders': lambda g: _small(g) and g['all_orders'] and g['k'] >= 2,
    'copy-then-controlled': lambda g: _small(g) and g['copy'] and g['nc'] == 2,
    'small-per-sample-matrix': lambda g: _small(g) and not g['shared'] and g['batch'] == 3,
    'small-shared-matrix': lambda g: _small(g) and g['shared'] and g['batch'] == 3,
    # apply_dense56_kernel, complex64
    'dense56-k5-one-group-per-sample': lambda g: (g['kernel'] == 'dense56' and g['k'] == 5 and not g['c128'] and g['ngroups'] == 1
                                                  and not g['shared']),
    'dense56-k5-group-spans-samples': lambda g: (g['kernel'] == 'dense56' and g['k'] == 5 and not g['c128'] and g['shared']
                                                 and g['col_shift'] == 1 and g['batch'] == 16 and g['ngroups'] == 1),
    'dense56-k5-ragged-groups': lambda g: (g['kernel'] == 'dense56' and g['k'] == 5 and not g['c128'] and g['ngroups'] > 4
                                           and g['ngroups'] % 4 != 0),
    'dense56-k6-one-group': lambda g: g['kernel'] == 'dense56' and g['k'] == 6 and g['ngroups'] == 1,
    'dense56-k6-three-groups': lambda g: g['kernel'] == 'dense56' and g['k'] == 6 and g['ngroups'] == 3,
    'dense56-control': lambda g: g['kernel'] == 'dense56' and g['nc'] >= 1,
    'bit0-target-staged1': lambda g: (g['kernel'] == 'staged1' and not g['c128'] and g['t0'] and g['ncols'] % 32 == 0
                                      and g['ncols'] <= 128),
    'bit0-target-staged2-k6': lambda g: g['kernel'] == 'staged2' and not g['c128'] and g['k'] == 6 and g['t0'] and g['ncols'] % 32 == 0,
    # apply_dense56_kernel, complex128
    'dense56-c128-lane-per-sample': lambda g: g['kernel'] == 'dense56' and g['c128'] and g['col_shift'] == 0 and g['batch'] == 16,
    'dense56-c128-bit0-target': lambda g: g['kernel'] == 'dense56' and g['c128'] and g['t0'] and g['free'] >= 1,
    'staged2-c128-k6': lambda g: g['kernel'] == 'staged2' and g['c128'] and g['k'] == 6 and g['ncols'] % 16 == 0,
    # apply_dense_mfma_kernel
    'staged1-partial-tile': lambda g: g['kernel'] == 'staged1' and g['ncols'] < 128,
    'staged1-two-tiles': lambda g: g['kernel'] == 'staged1' and g['grid'][0] == 2 and g['ncols'] % 128 != 0,
    **{f'staged2-k{k}-rows-fast': _staged2(k, True) for k in range(6, 11)},
    **{f'staged2-k{k}-per-sample': _staged2(k, False) for k in range(6, 11)},
    'staged2-n-equals-k-per-sample': lambda g: g['kernel'] == 'staged2' and g['free'] == 0 and not g['shared'] and g['ncols'] == 1,
    'staged2-n-equals-k-shared': lambda g: g['kernel'] == 'staged2' and g['free'] == 0 and g['shared'] and g['ncols'] == g['batch'],
    'staged2-ragged-columns': lambda g: g['kernel'] == 'staged2' and g['ncols'] > 64 and g['ncols'] % 64 != 0,
    'staged2-controls-around': lambda g: (g['kernel'] == 'staged2' and g['nc'] == 2 and g['ctrl_above'] and g['ctrl_below']
                                          and g['free'] >= 1),
    # apply_big_kernel
    'valu-k5': lambda g: g['kernel'] == 'valu' and g['k'] == 5 and g['nc'] == 2 and not g['shared'],
    'valu-k7': lambda g: g['kernel'] == 'valu' and g['k'] == 7 and g['nc'] == 2 and not g['shared'],
}

#: the routes of the launchers; every one is the kernel of some row (the census of test_gate_paths_cpu.py)
ROUTES = ('small-narrow', 'small-wide', 'dense56', 'staged1', 'staged2', 'valu')

ANY_N = 'the path does not depend on n: '


def _rows():
    out = []
    both = (False, True)

    def add(path, n, targets, controls=(), batch=1, prec=both, **kw):
        for c128 in prec:
            out.append(Row(path, n, tuple(targets), tuple(controls), batch, c128, seed=len(out), **kw))

    # ---- apply_small_kernel ----
    add('small-one-group', 1, [0], batch=2, in_place=True)
    add('small-one-group', 2, [0, 1], batch=2, in_place=True)
    add('small-one-group', 3, [1, 2, 0], batch=2, in_place=True)
    add('small-one-group', 4, [2, 0, 3, 1], batch=2, in_place=True)
    add('small-one-group', 3, [2, 0], [1], batch=2, in_place=True)
    add('wide-one-pair', 2, [1], prec=[False], batch=2, in_place=True)
    add('wide-one-pair', 3, [2, 1], prec=[False], batch=2, in_place=True)
    add('wide-one-pair', 4, [2, 3, 1], prec=[False], batch=2, in_place=True)
    add('wide-one-pair-controlled', 3, [1], [2], prec=[False], batch=2)
    add('wide-one-pair-controlled', 4, [1, 3], [2], prec=[False], batch=2)
    add('wide-one-pair-controlled', 5, [4, 1, 2], [3], prec=[False], batch=2)
    add('wide-many-workgroups', 11, [5], prec=[False])
    add('wide-many-workgroups', 12, [3, 9], prec=[False])
    add('wide-many-workgroups', 13, [12, 1, 6], prec=[False])
    add('narrow-bit0-target', 2, [0], batch=2)
    add('narrow-bit0-target', 4, [2, 0, 3], batch=2)
    add('narrow-bit0-control', 3, [2], [0], batch=2)
    add('narrow-bit0-control', 4, [1, 3], [0], batch=2)
    add('k4-bit0-free', 5, [3, 1, 4, 2], batch=2)
    add('top-target', 5, [4, 1], [2], batch=2, note=ANY_N + 'n = 5 leaves free bits below and between the gate\'s bits')
    add('top-control', 5, [1, 2], [4], batch=2, note=ANY_N + 'n = 5 leaves free bits below and between the gate\'s bits')
    add('target-orders', 6, [1, 4], all_orders=True, note=ANY_N + 'n = 6, where k = 4 still has two free bits')
    add('target-orders', 6, [0, 2, 5], all_orders=True, note=ANY_N + 'n = 6, where k = 4 still has two free bits')
    add('target-orders', 6, [1, 2, 3, 5], all_orders=True, note=ANY_N + 'n = 6, where k = 4 still has two free bits')
    add('copy-then-controlled', 12, [7, 2], [4, 10], batch=2,
        note='the copy runs at any n: n = 12 gives it 32 workgroups and the controlled writes more than one wave')
    add('small-per-sample-matrix', 5, [3, 1], batch=3, shared=False, note=ANY_N + 'n = 5: several groups per sample')
    add('small-shared-matrix', 5, [3, 1], batch=3, note=ANY_N + 'n = 5: several groups per sample')
    # ---- apply_dense56_kernel ----
    add('dense56-k5-one-group-per-sample', 10, [6, 2, 9, 4, 7], batch=2, shared=False, prec=[False])
    add('dense56-k5-group-spans-samples', 6, [3, 1, 5, 2, 4], batch=16, prec=[False])
    add('dense56-k5-ragged-groups', 10, [6, 2, 9, 4, 7], batch=5, prec=[False])
    add('dense56-k6-one-group', 11, [5, 1, 8, 3, 10, 6], prec=[False])
    add('dense56-k6-three-groups', 11, [5, 1, 8, 3, 10, 6], batch=3, prec=[False])
    add('dense56-control', 11, [6, 2, 9, 4, 7], [3], batch=2, shared=False, prec=[False])
    add('dense56-control', 10, [6, 2, 9, 4, 7], [3], batch=2, shared=False, prec=[True])
    add('bit0-target-staged1', 10, [6, 0, 9, 4, 7], prec=[False])
    add('bit0-target-staged2-k6', 11, [5, 0, 8, 3, 10, 6], prec=[False])
    add('dense56-c128-lane-per-sample', 5, [2, 0, 4, 1, 3], batch=16, prec=[True])
    add('dense56-c128-bit0-target', 9, [0, 3, 8, 5, 2], prec=[True])
    add('staged2-c128-k6', 10, [5, 1, 8, 3, 9, 6], prec=[True])
    # ---- apply_dense_mfma_kernel ----
    add('staged1-partial-tile', 5, [2, 0, 4, 1, 3])
    add('staged1-partial-tile', 7, [2, 0, 6, 1, 3], batch=3,
        note='n = 5 is the row above (one column); here 12 columns: neither one nor a multiple of 16')
    add('staged1-two-tiles', 10, [6, 0, 9, 4, 7], batch=5, prec=[False])        # 160 columns; bit 0 a target keeps dense56 away
    add('staged1-two-tiles', 8, [6, 0, 3, 4, 7], batch=21, prec=[True])        # 168: 160 is a multiple of 16 and would take dense56
    for k in range(6, 11):
        tg = list(range(k + 2))
        random.Random(k).shuffle(tg)
        why = 'n = k is the row staged2-n-equals-k; n = k + 2 gives every sample four columns, gathered from both sides of the targets'
        add(f'staged2-k{k}-rows-fast', k + 2, tg[:k], batch=3, note=why)
        add(f'staged2-k{k}-per-sample', k + 2, tg[:k], batch=2, shared=False, note=why)
    add('staged2-n-equals-k-per-sample', 7, [3, 6, 0, 5, 1, 4, 2], batch=3, shared=False)
    add('staged2-n-equals-k-shared', 7, [3, 6, 0, 5, 1, 4, 2], batch=3)
    add('staged2-ragged-columns', 12, [3, 6, 11, 5, 1, 4, 8], batch=3)
    add('staged2-controls-around', 11, [3, 6, 7, 5, 1, 4, 2], [0, 9], batch=2, shared=False,
        note='n = 10 reaches it with one free bit: n = 11 puts one between the targets and the upper control and one above it')
    # ---- apply_big_kernel ----
    add('valu-k5', 8, [6, 1, 4, 2, 7], [0, 5], batch=2, shared=False, valu=True,
        note='n = 7 has no free bit: one free bit puts controlled and uncontrolled amplitudes of two columns in a workgroup')
    add('valu-k7', 10, [6, 1, 4, 2, 7, 9, 0], [3, 8], batch=2, shared=False, valu=True,
        note='n = 9 has no free bit: one free bit puts controlled and uncontrolled amplitudes of two columns in a workgroup')
    return out


ROWS = _rows()


def route_of(g: dict) -> str:
    if g['kernel'] == 'small':
        return 'small-wide' if g['wide'] else 'small-narrow'
    return g['kernel']


# ---- the knob test ------------------------------------------------------------------------------------------------------------
def _knob_rows():
    t5, t6, t7 = [6, 2, 9, 4, 7], [5, 1, 8, 3, 10, 6], [3, 6, 11, 5, 1, 4, 8]
    t8, t10 = [3, 6, 9, 5, 1, 4, 8, 12], [3, 6, 9, 5, 1, 4, 8, 12, 2, 14]
    spec = [('dense56', 12, t5, (), 4, False, True), ('dense56', 12, t5, (), 2, True, True), ('dense56', 12, t6, (), 2, False, True),
            ('dense56', 10, t5, (), 2, False, False), ('staged1', 10, [6, 0, 9, 4, 7], (), 5, False, True),
            ('staged2', 12, t7, (), 3, False, True), ('staged2', 9, [3, 6, 7, 5, 1, 4, 8], (), 2, True, False),
            ('staged2', 15, t8, (), 2, False, True), ('staged2', 15, t8, (), 2, False, False),
            ('staged2', 16, t10, (), 2, False, True), ('staged2', 17, t10, (), 2, False, False),
            ('staged2', 16, t8, (13,), 1, False, True)]
    return [Row(p, n, tuple(t), tuple(c), b, c128, shared, seed=500 + i) for i, (p, n, t, c, b, c128, shared) in enumerate(spec)]


KNOB_ROWS = _knob_rows()
#: the settings of the knob test: one fresh process each; each is the whole environment change
KNOBS = [{'DQ_DENSE_NT': '1'}, {'DQ_DENSE_ROWS_FAST': '0'}, {'DQ_DENSE5_BLOCKS': '1'}, {'DQ_DENSE5': '0'}, {'DQ_DENSE_BIG': '1'},
         {'DQ_ZMULTI_MFMA': '0'}, {'DQ_PERMUTE_LDS': '0'}]
KNOB_NAMES = sorted({k for s in KNOBS for k in s})
#: settings that only change who does the work: the digest equals the parent's
SAME_DIGEST = ('DQ_DENSE_NT', 'DQ_DENSE_ROWS_FAST', 'DQ_DENSE5_BLOCKS')
_DENSE_KW = {'DQ_DENSE_NT': 'dense_nt', 'DQ_DENSE5': 'dense5', 'DQ_DENSE5_BLOCKS': 'dense5_blocks', 'DQ_DENSE_BIG': 'dense_big',
             'DQ_DENSE_ROWS_FAST': 'dense_rows_fast'}


def dense_knobs(env) -> dict:
    """The keywords of `_launch_geometry.dense` for the DQ_DENSE_* variables ``env`` holds (parsed like atoi)."""
    return {kw: int(env[name]) for name, kw in _DENSE_KW.items() if name in env}


#: (setting, path) -> what `geo` under the setting must say of some KNOB_ROW, and must not say of it by default
KNOB_PATHS = {
    ('DQ_DENSE_NT', 'nt-dense56-k5'): lambda g: g['kernel'] == 'dense56' and g['k'] == 5 and g['nt'],
    ('DQ_DENSE_NT', 'nt-dense56-k5-c128'): lambda g: g['kernel'] == 'dense56' and g['k'] == 5 and g['c128'] and g['nt'],
    ('DQ_DENSE_NT', 'nt-dense56-k6'): lambda g: g['kernel'] == 'dense56' and g['k'] == 6 and g['nt'],
    ('DQ_DENSE_NT', 'nt-staged1'): lambda g: g['kernel'] == 'staged1' and g['nt'],
    ('DQ_DENSE_NT', 'nt-staged2'): lambda g: g['kernel'] == 'staged2' and g['nt'] and not g['c128'],
    ('DQ_DENSE_NT', 'nt-staged2-c128'): lambda g: g['kernel'] == 'staged2' and g['nt'] and g['c128'],
    ('DQ_DENSE_ROWS_FAST', 'column-tiles-fast'): lambda g: g['kernel'] == 'staged2' and g['shared'] and not g['rows_fast'] and g['grid'][1] > 1,
    ('DQ_DENSE5_BLOCKS', 'one-workgroup-k5'): lambda g: g['kernel'] == 'dense56' and g['k'] == 5 and not g['c128'] and g['grid'][0] == 1 and g['iterations'] >= 3,
    ('DQ_DENSE5_BLOCKS', 'one-workgroup-k5-c128'): lambda g: g['kernel'] == 'dense56' and g['c128'] and g['grid'][0] == 1 and g['iterations'] >= 3,
    ('DQ_DENSE5_BLOCKS', 'one-workgroup-k6'): lambda g: g['kernel'] == 'dense56' and g['k'] == 6 and g['grid'][0] == 1 and g['iterations'] >= 2,
    ('DQ_DENSE5', 'dense56-off-staged1'): lambda g: g['kernel'] == 'staged1' and not g['bit0_used'] and g['ncols'] % 32 == 0 and not g['c128'],
    ('DQ_DENSE5', 'dense56-off-staged1-c128'): lambda g: g['kernel'] == 'staged1' and g['c128'] and g['ncols'] % 16 == 0,
    ('DQ_DENSE5', 'dense56-off-staged2-k6'): lambda g: g['kernel'] == 'staged2' and g['k'] == 6 and not g['c128'] and not g['bit0_used'] and g['ncols'] % 32 == 0,
    ('DQ_DENSE_BIG', 'big128-k8-shared'): lambda g: g['kernel'] == 'big128' and g['k'] == 8 and g['shared'] and g['rows_fast'] and g['nc'] == 0,
    ('DQ_DENSE_BIG', 'big128-k8-per-sample'): lambda g: g['kernel'] == 'big128' and g['k'] == 8 and not g['shared'] and not g['rows_fast'],
    ('DQ_DENSE_BIG', 'big128-k10-shared'): lambda g: g['kernel'] == 'big128' and g['k'] == 10 and g['shared'] and g['grid'][1] == 8,
    ('DQ_DENSE_BIG', 'big128-k10-per-sample'): lambda g: g['kernel'] == 'big128' and g['k'] == 10 and not g['shared'] and g['grid'] == (1, 8, 2),
    ('DQ_DENSE_BIG', 'big128-control'): lambda g: g['kernel'] == 'big128' and g['nc'] == 1,
}


# ---- inputs -------------------------------------------------------------------------------------------------------------------
UNITS = (1, -1, 1j, -1j)


def input_state(row: Row, device) -> torch.Tensor:
    """(batch, 2^n) in the row's precision, normalised, from the row's seed (made on the host: the same on every device)."""
    g = torch.Generator().manual_seed(9000 + row.seed)
    x = torch.view_as_complex(torch.randn(row.batch, 1 << row.n, 2, generator=g, dtype=torch.float64))
    return (x / x.norm(dim=-1, keepdim=True)).to(row.dtype).to(device)


@functools.lru_cache(maxsize=None)
def _unitary(k: int, nb: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(100 * k + nb)
    a = torch.view_as_complex(torch.randn(nb, 1 << k, 1 << k, 2, generator=g, dtype=torch.float64))
    return torch.linalg.qr(a)[0]


@functools.lru_cache(maxsize=None)
def _signed_perm(k: int, nb: int) -> torch.Tensor:
    rng = random.Random(200 * k + nb)
    d = 1 << k
    m = torch.zeros(nb, d, d, dtype=C128)
    for b in range(nb):
        cols = rng.sample(range(d), d)
        for r, c in enumerate(cols):
            m[b, r, c] = rng.choice(UNITS)
    return m


def matrices(row: Row, kind: str, device) -> torch.Tensor:
    """(1 or batch, D, D) in the row's precision."""
    nb = 1 if row.shared else row.batch
    assert row.shared or nb >= 2, 'a single matrix is a shared matrix'
    m = _unitary(row.k, nb) if kind == 'unitary' else _signed_perm(row.k, nb)
    return m.to(row.dtype).to(device)


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def run_kernel(row: Row, x, u, targets, controls, in_place: bool) -> torch.Tensor:
    """`backend.apply_gate` on the device of ``x``; out of place into an output that starts as NaN."""
    if in_place:
        st = x.clone()
        return backend.apply_gate(st, u, targets, controls, out=st)
    out = torch.full_like(x, float('nan'))
    if row.valu and x.is_cuda:
        lib = _lib.load()
        _lib.check(lib.dq_set_dense_path(0), 'dq_set_dense_path')
        try:
            backend.apply_gate(x, u, targets, controls, out=out)
        finally:
            _lib.check(lib.dq_set_dense_path(1), 'dq_set_dense_path')
        return out
    return backend.apply_gate(x, u, targets, controls, out=out)


def digest(*tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(torch.view_as_real(t).cpu().numpy().tobytes())
    return h.hexdigest()


# ---- criteria -----------------------------------------------------------------------------------------------------------------
def tau(row: Row) -> float:
    return hc.TAU_SUM if row.c128 else 2 * (2 * (1 << row.k) + 2) * hc.U[False]


def _bits_equal(a, b) -> bool:
    return torch.equal(torch.view_as_real(a), torch.view_as_real(b))


def controlled_mask(row: Row, device) -> torch.Tensor:
    cm = sum(1 << c for c in row.controls)
    return (torch.arange(1 << row.n, device=device) & cm) == cm


def reference(row: Row, x, u, targets):
    """-> dict(out, xm, ym, s): `_grid_refs.apply_gate` and S, the same product over absolute values."""
    out, xm, ym = R.apply_gate(x, u, list(targets), list(row.controls))
    s = R.apply_gate(x.abs().to(C128), u.abs().to(C128), list(targets), list(row.controls))[0].real
    return dict(out=out, xm=xm, ym=ym, s=s)


def ratio(row: Row, kind: str, got, ref, x) -> float:
    """inf unless the amplitudes outside the controls' 1-subspace equal the input bit for bit; 'perm': 0 if the rest equals
    the reference bit for bit, else inf; 'unitary': max |got - ref| / (tau S) over the rest, inf for a NaN."""
    on = controlled_mask(row, x.device)
    if not _bits_equal(got[:, ~on].to(C128), x[:, ~on].to(C128)):
        return INF
    if kind == 'perm':
        return 0.0 if _bits_equal(got.to(C128), ref['out']) else INF
    r = (got.to(C128) - ref['out']).abs()[:, on] / (tau(row) * ref['s'][:, on])
    return float(torch.nan_to_num(r, nan=INF).max())


def _scatter(row: Row, x, ym, targets) -> torch.Tensor:
    """The state whose controlled slice, as the (B, D, columns) matrix of the targets, is ``ym``; the rest is the input."""
    out = x.to(C128, copy=True)
    view = R.gate_matrix_view(out, list(targets), list(row.controls))
    view.copy_(ym.reshape(view.shape))
    return out


def corruptions(row: Row, g: dict, x, u, ref, targets) -> list:
    """[(what, state)]: the reference as a broken version of the row's path would leave it."""
    out = []
    xm, ym = ref['xm'], ref['ym']                     # (B, D, 2^free)
    uc = u.to(C128)
    d, free = 1 << row.k, g['free']
    if g['kernel'] in ('dense56', 'staged1', 'staged2', 'big128'):
        # the K chunk holding the largest entry of the last row tile's first row, dropped for that row tile
        kc = 32 if row.c128 else 16
        r0 = d - g['row_tile']
        j0 = int(uc[0, r0].abs().argmax()) // kc * kc
        bad = ym.clone()
        bad[:, r0:] -= uc[:, r0:, j0:j0 + kc] @ xm[:, j0:j0 + kc]
        out.append(('k-chunk', _scatter(row, x, bad, targets)))
    # the last column group / tile / workgroup left at its input
    if g['kernel'] == 'small':
        per = 256 * (2 if g['wide'] else 1)
        lo, hi, samples = (g['blocks'] - 1) * per, 1 << free, [row.batch - 1]
        cols = [(s, torch.arange(lo, hi)) for s in samples]
    elif g['kernel'] == 'valu':
        cols = None
    else:
        tile = g['col_tile']
        c = torch.arange((g['ncols'] - 1) // tile * tile, g['ncols'])
        if row.shared:
            cols = [(int(s), (c[(c >> free) == s] & ((1 << free) - 1))) for s in torch.unique(c >> free)]
        else:
            cols = [(row.batch - 1, c)]
    if cols is None:
        bad = ref['out'].clone()
        bad[-1, -256:] = x[-1, -256:].to(C128)
    else:
        badm = ym.clone()
        for s, w in cols:
            badm[s][:, w] = xm[s][:, w]
        bad = _scatter(row, x, badm, targets)
    out.append(('last-tile', bad))
    if row.k >= 2:
        sw = (targets[1], targets[0]) + tuple(targets[2:])
        out.append(('targets-swapped', R.apply_gate(x, u, list(sw), list(row.controls))[0]))
    if g['kernel'] == 'dense56' and row.shared and g['col_shift'] < g['col_group'].bit_length() - 1 and row.batch > 1:
        # the first column group reads the sample of its lane 0 in every lane
        c = torch.arange(min(g['col_group'], g['ncols']))
        s, w = c >> free, c & ((1 << free) - 1)
        badm = ym.clone()
        wrong = uc[0] @ xm[int(s[0])]
        for si, wi in zip(s.tolist(), w.tolist()):
            badm[si][:, wi] = wrong[:, wi]
        out.append(('sample-of-lane-0', _scatter(row, x, badm, targets)))
    if g['kernel'] == 'small' and g['wide']:
        on = controlled_mask(row, x.device) & ((torch.arange(1 << row.n, device=x.device) & 1) == 1)
        bad = ref['out'].clone()
        bad[:, on] = x[:, on].to(C128)
        out.append(('second-of-pair', bad))
    return out


def run_row(row: Row, device, check_path=True, **knobs) -> dict:
    """Runs the row on ``device`` with both matrices and asserts its path, its criteria and its negative controls; ->
    dict(ratio: the worst |got - ref| / (tau S) of matrix (a), digest: of every result, route)."""
    g = geo(row, **knobs)
    if check_path and row.path in PATHS:
        assert PATHS[row.path](g), f'{row.id}: the mirror does not say {row.path}: {g}'
    elif check_path:                                  # (a knob row: its path is its kernel in the default environment)
        assert geo(row)['kernel'] == row.path, f'{row.id}: the mirror does not say {row.path}: {geo(row)}'
    x = input_state(row, device)
    x0 = x.clone()
    worst, results = 0.0, []
    for targets in row.variants():
        for kind in KINDS:
            u = matrices(row, kind, device)
            ref = reference(row, x, u, targets)
            got = run_kernel(row, x, u, targets, row.controls, in_place=False)
            assert _bits_equal(x, x0), f'{row.id}: the input changed'
            r = ratio(row, kind, got, ref, x)
            assert r <= 1.0, f'{row.id} {targets} ({kind}): worst |got - ref| / (tau S) = {r:.3e}'
            if kind == 'unitary':
                worst = max(worst, r)
            if row.k <= 4:
                again = run_kernel(row, x, u, targets, row.controls, in_place=True)
                assert _bits_equal(again, got), f'{row.id} {targets} ({kind}): in place differs from out of place'
            results.append(got)
            for what, bad in corruptions(row, g, x, u, ref, targets):
                assert ratio(row, kind, bad, ref, x) > 1.0, f'{row.id} {targets} ({kind}): the criterion does not see corruption {what}'
    return dict(ratio=worst, digest=digest(*results), route=route_of(g))


# ---- the Z-string loop kernels and permute_bits (the small things of the knob test) -------------------------------------------
Z_NS, Z_KS, Z_KNOB_NS, Z_BATCH = (1, 4, 7), (1, 2, 31, 32, 33), (8, 13), 3


def check_z_strings(n: int, nstrings: int, c128: bool, device) -> dict:
    """`backend.expect_z_multi` and `backend.scale_z_signs` against `_grid_refs`: sums within 1e-12 S, amplitudes by TAU_AMP of
    test_grid_paths_gpu.py (per sample, relative to max |ref|); one string with coefficient 1: bit for bit."""
    from test_grid_paths_gpu import TAU_AMP, TAU_SUM

    dtype = C128 if c128 else C64
    rng = random.Random(1000 * n + nstrings)
    masks = [(1 << n) - 1] + [rng.randrange(0, 1 << n) for _ in range(nstrings - 1)]
    g = torch.Generator().manual_seed(77 * n + nstrings)
    x = torch.view_as_complex(torch.randn(Z_BATCH, 1 << n, 2, generator=g, dtype=torch.float64))
    x = (x / x.norm(dim=-1, keepdim=True)).to(dtype).to(device).contiguous()
    if nstrings == 1:
        coef = torch.ones(Z_BATCH, 1, dtype=torch.float64, device=device)
    else:
        coef = torch.randn(Z_BATCH, nstrings, generator=g, dtype=torch.float64).to(device)
    got = backend.expect_z_multi(x, masks)
    ref, s = R.expect_z_multi(x, masks)
    assert got.shape == ref.shape and got.dtype == torch.float64
    rs = float(((got - ref).abs() / s).max())
    assert rs <= TAU_SUM, f'expect_z_multi n={n} K={nstrings}: max |got - ref| / S = {rs:.3e}'
    # (negative control: the last amplitude's terms dropped)
    i = torch.tensor([(1 << n) - 1], device=device)
    delta = torch.stack([R.probabilities(x[:, -1:]).sum(-1) * R.z_sign(i, z) for z in masks], dim=1).reshape(ref.shape)
    assert bool((delta.abs() > TAU_SUM * s).all()), 'expect_z_multi: the criterion does not see a dropped amplitude'
    out = backend.scale_z_signs(x, masks, coef)
    want = R.scale_z_signs(x, masks, coef)
    scale = want.abs().amax(dim=1)
    ra = float(((out.to(C128) - want).abs().amax(dim=1) / scale).max())
    assert ra <= TAU_AMP[dtype], f'scale_z_signs n={n} K={nstrings}: max |got - ref| / max |ref| = {ra:.3e}'
    assert bool(((x[:, -1].to(C128) - want[:, -1]).abs() > TAU_AMP[dtype] * scale).all()) or nstrings == 1, \
        'scale_z_signs: the criterion does not see an amplitude left at its input'
    if nstrings == 1:
        sign = R.z_sign(torch.arange(1 << n, device=device), masks[0]).to(x.real.dtype)
        assert torch.equal(out, x * sign), f'scale_z_signs n={n}: one string with coefficient 1 is a sign flip, bit for bit'
    return dict(sums=rs / TAU_SUM, amps=ra / TAU_AMP[dtype], digest=digest(got.to(C128), out))


def index_test_permutations(n: int) -> list:
    """The permutations of test_kernels_gpu.py::test_permute_bits_against_index_arithmetic at ``n`` index bits."""
    rng = random.Random(n)
    perms = [list(range(n)), rng.sample(range(n), n), [0] + [1 + q for q in rng.sample(range(n - 1), n - 1)],
             list(range(1, n)) + [0], [q for q in range(n) if q not in (n - 3, n - 2)] + [n - 3, n - 2],
             list(range(n))[::-1], [n - 1] + list(range(n - 1)), [1, 0] + list(range(2, n))]
    perms += [rng.sample(range(n), n) for _ in range(5 if n <= 17 else 1)]
    return perms


PERMUTE_NL, PERMUTE_BATCH = 13, 2


def lds_permutations(c128: bool) -> list:
    """Those of them that take the LDS kernel by default at nl = 13."""
    return [p for p in index_test_permutations(PERMUTE_NL) if G.permute(PERMUTE_NL, p, PERMUTE_BATCH, c128)['variant'] == 'lds']


def check_permute(c128: bool, device, lds: bool) -> str:
    """`backend.permute_bits` at nl = 13 on the permutations that take the LDS kernel by default: bit for bit the index
    gather, whichever kernel the environment (``lds``: DQ_PERMUTE_LDS is not 0) gives them."""
    dtype = C128 if c128 else C64
    g = torch.Generator().manual_seed(13)
    x = torch.view_as_complex(torch.randn(PERMUTE_BATCH, 1 << PERMUTE_NL, 2, generator=g, dtype=torch.float64)).to(dtype).to(device)
    perms = lds_permutations(c128)
    assert len(perms) >= 5
    outs = []
    for p in perms:
        variant = G.permute(PERMUTE_NL, p, PERMUTE_BATCH, c128, lds=lds)['variant']
        assert variant == ('lds' if lds else ('tiled_pair' if not c128 and p[0] == 0 else 'tiled')), (p, variant)
        out = torch.full_like(x, float('nan'))
        backend.permute_bits(x, p, out=out)
        assert torch.equal(out, x[:, R.src_index(PERMUTE_NL, p, device)]), p
        outs.append(out)
    return digest(*outs)


def knob_run(device, env) -> list:
    """What the knob test runs under one environment ``env`` (the parent: its own, with none of `KNOB_NAMES` set): every
    KNOB_ROW judged by `run_row` with the mirror under the DQ_DENSE_* knobs of ``env``, the Z-string kernels at n = 1 .. 13
    and permute_bits; -> [(what, digest)].  Every check asserts for itself."""
    out = []
    knobs = dense_knobs(env)
    for row in KNOB_ROWS:
        res = run_row(row, device, check_path=False, **knobs)
        out.append((f'{row.id} [{geo(row, **knobs)["kernel"]}, {res["ratio"]:.1e} of the bound]', res['digest']))
    for c128 in (False, True):
        for n in Z_NS + Z_KNOB_NS:
            for k in Z_KS:
                out.append((f'z-strings n={n} K={k} {"c128" if c128 else "c64"}', check_z_strings(n, k, c128, device)['digest']))
        lds = not ('DQ_PERMUTE_LDS' in env and int(env['DQ_PERMUTE_LDS']) == 0)
        out.append((f'permute_bits {"c128" if c128 else "c64"}', check_permute(c128, device, lds)))
    return out
