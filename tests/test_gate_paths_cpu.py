"""The paths of the single-gate kernels without a GPU: the mirrors `_launch_geometry.small_gate` and `.dense` on both sides of
every condition of the launchers (csrc/dq_gate.hip: the wide instantiation; csrc/dq_dense.hip: dense56 / staged1 / the
128 x 128 tile / staged2) and under each DQ_DENSE_* knob; that every row of `_gate_cases.ROWS` reaches the path it claims,
that every path, route and knob-selected route has a row, and that a row is the smallest n of its path or says why not;
the references against the oracle; every row on the CPU backend under the criteria that judge the kernels in
test_gate_paths_gpu.py; and every negative control rejected."""

from collections import Counter

import pytest
import torch

import _gate_cases as gc
import _grid_refs as R
import _launch_geometry as G
from _cpu_backend import CpuTestBackend
from deepquantum_amd import backend
from oracle import statevec_oracle as oracle

ALL = gc.ROWS + gc.KNOB_ROWS


# ---- the mirrors on both sides of every condition ----------------------------------------------------------------------------
def test_small_gate_mirror_conditions():
    """dq_gate.hip:198: complex64, k <= 3, a free bit, index bit 0 neither target nor control."""
    wide = G.small_gate(4, 2, 1, False, False, True)
    assert wide == dict(wide=True, groups=1, blocks=1, iterations=1, copy=False)
    assert not G.small_gate(4, 2, 1, True, False, True)['wide']                  # complex128
    assert not G.small_gate(4, 2, 1, False, True, True)['wide']                  # bit 0 used
    assert not G.small_gate(3, 2, 1, False, True, True)['wide']                  # no free bit (bit 0 is then used)
    assert G.small_gate(5, 3, 0, False, False, True)['wide'] and not G.small_gate(6, 4, 0, False, False, True)['wide']      # k = 4
    assert G.small_gate(17, 3, 12, False, False, True)['wide'] and not G.small_gate(17, 3, 13, False, False, True)['wide']  # k + nc = 16
    # the group count halves when wide; 256 groups (pairs) per workgroup
    assert G.small_gate(12, 2, 0, False, False, True)['groups'] == 512 and G.small_gate(12, 2, 0, False, True, True)['groups'] == 1024
    assert G.small_gate(11, 2, 0, False, False, True)['blocks'] == 1 and G.small_gate(12, 2, 0, False, False, True)['blocks'] == 2
    assert G.small_gate(10, 2, 0, True, False, True)['blocks'] == 1 and G.small_gate(11, 2, 0, True, False, True)['blocks'] == 2
    # the grid's cap: a second iteration from 2^28 groups on
    assert G.small_gate(30, 1, 0, False, False, True)['iterations'] == 1 and G.small_gate(30, 1, 0, True, False, True)['iterations'] == 2
    # dq_gate.hip:188: the copy runs out of place with controls only
    assert [G.small_gate(6, 2, nc, False, False, ip)['copy'] for nc in (0, 1) for ip in (False, True)] == [False, False, True, False]


def test_dense_mirror_conditions():
    """dq_dense.hip:399 (dense56), :414 (staged1), :421 (the 128 x 128 tile), else staged2."""
    d = lambda *a, **kw: G.dense(*a, launch=True, **kw)                          # noqa: E731
    # :399, term by term: D, the column count a multiple of the column group, bit 0 (complex64)
    assert d(10, 5, 0, 1, False, True, False)['route'] == 'dense56' and d(9, 5, 0, 1, False, True, False)['route'] == 'staged1'
    assert d(9, 5, 0, 1, True, True, False)['route'] == 'dense56' and d(8, 5, 0, 1, True, True, False)['route'] == 'staged1'
    assert d(10, 5, 0, 1, False, True, True)['route'] == 'staged1' and d(9, 5, 0, 1, True, True, True)['route'] == 'dense56'
    assert d(11, 6, 0, 1, False, True, False)['route'] == 'dense56' and d(11, 6, 0, 1, False, True, True)['route'] == 'staged2'
    assert d(11, 6, 0, 1, True, True, False)['route'] == 'staged2'               # complex128 k = 6: always staged
    assert d(12, 7, 0, 1, False, True, False)['route'] == 'staged2'
    assert d(9, 5, 0, 2, False, True, False)['route'] == 'dense56' and d(9, 5, 0, 2, False, False, False)['route'] == 'staged1'     # a shared matrix: the batch is columns
    # the dense56 launch: groups, the grid, what one pass of it covers
    g = d(10, 5, 0, 5, False, True, False)
    assert (g['ngroups'], g['grid'], g['per_pass'], g['iterations'], g['col_shift']) == (5, (2, 1, 1), 8, 1, 5)
    g = d(10, 5, 0, 5, False, False, False)
    assert (g['ngroups'], g['grid'], g['col_shift']) == (1, (1, 5, 1), -1)
    g = d(11, 6, 0, 3, False, True, False)
    assert (g['ngroups'], g['grid'], g['per_pass']) == (3, (2, 1, 1), 4)
    # :414-:434, the staged grids
    assert d(10, 5, 0, 5, False, True, True)['grid'] == (2, 1, 1) and d(10, 5, 0, 4, False, True, True)['grid'] == (1, 1, 1)
    assert d(10, 5, 0, 5, False, False, True)['grid'] == (1, 1, 5)
    for k in range(6, 11):
        assert d(k + 2, k, 0, 3, True, True, False)['grid'] == (1, 1 << (k - 6), 1)
        assert d(k + 2, k, 0, 3, True, False, False)['grid'] == (1, 1 << (k - 6), 3)
    assert d(13, 7, 0, 1, False, True, False)['grid'][0] == 1 and d(14, 7, 0, 1, False, True, False)['grid'][0] == 2
    assert d(12, 7, 0, 3, False, True, False)['rows_fast'] and not d(12, 7, 0, 3, False, False, False)['rows_fast']
    assert not d(10, 5, 0, 5, False, True, True)['rows_fast']                    # staged1 never sets the flag
    # the default call is what it was: no launch keys
    assert set(G.dense(12, 7, 0, 3, False, True, False)) == {'route', 'nt', 'iterations'}


def test_dense_mirror_under_each_knob():
    d = lambda *a, **kw: G.dense(*a, launch=True, **kw)                          # noqa: E731
    # DQ_DENSE_NT: 0 / 1 force, unset (and a negative value) leave the 1-GiB rule
    assert d(10, 5, 0, 1, False, True, False, dense_nt=1)['nt'] and not d(27, 5, 0, 1, False, True, False, dense_nt=0)['nt']
    assert d(27, 5, 0, 1, False, True, False, dense_nt=-1)['nt'] and not d(26, 5, 0, 1, False, True, False, dense_nt=-1)['nt']
    # DQ_DENSE5 = 0: never dense56
    assert d(10, 5, 0, 1, False, True, False, dense5=0)['route'] == 'staged1'
    assert d(9, 5, 0, 1, True, True, False, dense5=0)['route'] == 'staged1'
    assert d(11, 6, 0, 1, False, True, False, dense5=0)['route'] == 'staged2'
    # DQ_DENSE5_BLOCKS: a cap on the workgroups (0 and below: the resident grid)
    g = d(12, 5, 0, 4, False, True, False, dense5_blocks=1)
    assert (g['ngroups'], g['grid'], g['per_pass'], g['iterations']) == (16, (1, 1, 1), 4, 4)
    assert d(12, 5, 0, 4, False, True, False, dense5_blocks=0)['grid'] == (4, 1, 1)
    assert d(12, 5, 0, 4, False, True, False, dense5_blocks=3)['iterations'] == 2
    assert d(12, 6, 0, 2, False, True, False, dense5_blocks=1)['iterations'] == 2
    # DQ_DENSE_BIG, :421 term by term: complex64, k >= 8, the knob, the column count a multiple of 128
    assert d(15, 8, 0, 1, False, True, False, dense_big=1)['route'] == 'big128'
    assert d(15, 8, 0, 1, False, True, False)['route'] == 'staged2'
    assert d(15, 8, 0, 1, True, True, False, dense_big=1)['route'] == 'staged2'
    assert d(14, 7, 0, 1, False, True, False, dense_big=1)['route'] == 'staged2'
    assert d(14, 8, 0, 1, False, True, False, dense_big=1)['route'] == 'staged2' and d(14, 8, 0, 2, False, True, False, dense_big=1)['route'] == 'big128'
    g = d(17, 10, 0, 2, False, False, False, dense_big=1)
    assert (g['grid'], g['rows_fast'], g['row_tile'], g['col_tile']) == ((1, 8, 2), False, 128, 128)
    assert d(16, 10, 0, 2, False, True, False, dense_big=1)['rows_fast']
    # DQ_DENSE_ROWS_FAST = 0
    assert not d(12, 7, 0, 3, False, True, False, dense_rows_fast=0)['rows_fast']
    assert d(16, 10, 0, 2, False, True, False, dense_big=1, dense_rows_fast=0)['rows_fast']      # (the 128 x 128 tile does not ask)
    # the knobs as the environment spells them
    assert gc.dense_knobs({'DQ_DENSE_NT': '1', 'DQ_DENSE5_BLOCKS': '1', 'PATH': 'x'}) == dict(dense_nt=1, dense5_blocks=1)


def test_permute_mirror_under_the_lds_knob():
    for c128 in (False, True):
        perms = gc.lds_permutations(c128)
        assert len(perms) >= 5
        for p in perms:
            off = G.permute(gc.PERMUTE_NL, p, gc.PERMUTE_BATCH, c128, lds=False)
            assert off['variant'] == ('tiled_pair' if not c128 and p[0] == 0 else 'tiled') and off['blocks'] in (4, 8)
    ident = list(range(13))
    assert G.permute(13, ident, 1, False, lds=False) == G.permute(13, ident, 1, False)      # (never the LDS kernel: the knob changes nothing)
    assert G.permute(11, list(range(1, 11)) + [0], 1, False, lds=False)['variant'] == 'elementwise'


# ---- the rows: paths, census, floors --------------------------------------------------------------------------------------------
def test_row_ids_are_unique():
    assert len({r.id for r in ALL}) == len(ALL)
    for r in ALL:
        bits = r.targets + r.controls
        assert len(set(bits)) == len(bits) and all(0 <= b < r.n for b in bits), r.id
        assert r.shared or r.batch >= 2, r.id


@pytest.mark.parametrize('row', gc.ROWS, ids=[r.id for r in gc.ROWS])
def test_every_row_reaches_its_path(row):
    assert gc.PATHS[row.path](gc.geo(row)), (row.id, gc.geo(row))


def test_census_every_path_and_route_has_a_row():
    claimed = Counter(r.path for r in gc.ROWS)
    assert set(claimed) == set(gc.PATHS), set(gc.PATHS) ^ set(claimed)
    for c128 in (False, True):
        routes = {gc.route_of(gc.geo(r)) for r in gc.ROWS if r.c128 == c128}
        assert routes == set(gc.ROUTES) - ({'small-wide'} if c128 else set()), (c128, routes)
    # what the issue names in both precisions has a row in both
    both = [p for p in gc.PATHS if not any(s in p for s in ('wide', 'dense56-k', 'bit0-target-staged', 'c128'))]
    for p in both:
        assert {r.c128 for r in gc.ROWS if r.path == p} == {False, True}, p
    # every order of the targets for k = 2, 3, 4
    assert sorted((r.k, len(r.variants())) for r in gc.ROWS if r.path == 'target-orders' and not r.c128) == [(2, 2), (3, 6), (4, 24)]
    # the largest row is k = 10 at n = 12
    assert max((r.k, r.n) for r in gc.ROWS) == (10, 12) and max(r.n for r in gc.ROWS) == 13


def test_census_every_knob_selected_route_has_a_knob_row():
    default = [gc.geo(r) for r in gc.KNOB_ROWS]
    assert {g['kernel'] for g in default} == {'dense56', 'staged1', 'staged2'} and not any(g['nt'] for g in default)
    for r, g in zip(gc.KNOB_ROWS, default):
        assert g['kernel'] == r.path, r.id
    assert {name for name, _ in gc.KNOB_PATHS} == {k for k in gc.KNOB_NAMES if k.startswith('DQ_DENSE')}
    for (name, path), pred in gc.KNOB_PATHS.items():
        setting = next(s for s in gc.KNOBS if name in s)
        under = [gc.geo(r, **gc.dense_knobs(setting)) for r in gc.KNOB_ROWS]
        hit = [i for i, g in enumerate(under) if pred(g)]
        assert hit, f'no knob row reaches {path} under {setting}'
        assert not any(pred(default[i]) for i in hit), f'{path} is reached without {setting}'
    # the 128 x 128 rows: complex64, k = 8 and 10, a column count that is a multiple of 128
    big = [g for g in (gc.geo(r, dense_big=1) for r in gc.KNOB_ROWS) if g['kernel'] == 'big128']
    assert {g['k'] for g in big} == {8, 10} and all(g['ncols'] % 128 == 0 and not g['c128'] for g in big)
    # the settings that only change who does the work leave every route as it is
    for setting in gc.KNOBS:
        name = next(iter(setting))
        if name in gc.SAME_DIGEST:
            assert [gc.geo(r, **gc.dense_knobs(setting))['kernel'] for r in gc.KNOB_ROWS] == [g['kernel'] for g in default]


@pytest.mark.parametrize('row', gc.ROWS, ids=[r.id for r in gc.ROWS])
def test_every_row_is_the_smallest_n_of_its_path_or_says_why(row):
    smaller = [n for n in range(row.k + row.nc, row.n) if gc.PATHS[row.path](gc.geo(row, n=n))]
    if row.note:
        assert smaller, f'{row.id}: the note is stale, no smaller n reaches {row.path}'
    else:
        assert not smaller, f'{row.id}: n = {smaller} reach {row.path} too'


# ---- the references against the oracle ----------------------------------------------------------------------------------------
UP_TO_13 = [r for r in ALL if r.n <= 13]       # (the knob rows above run the same reference code on larger states)


@pytest.mark.parametrize('row', UP_TO_13, ids=[r.id for r in UP_TO_13])
def test_reference_agrees_with_the_oracle(row):
    x = gc.input_state(row, 'cpu').to(torch.complex128)
    for targets in row.variants()[:6]:
        for kind in gc.KINDS:
            u = gc.matrices(row, kind, 'cpu').to(torch.complex128)
            ref = R.apply_gate(x, u, list(targets), list(row.controls))[0]
            want = oracle.apply_gate_bits(x, u, list(targets), list(row.controls))
            assert float((ref - want).abs().max()) < 1e-13, (row.id, targets, kind)


# ---- every row on the CPU backend, every negative control rejected --------------------------------------------------------------
@pytest.fixture()
def cpu():
    backend.set_test_backend(CpuTestBackend())
    yield
    backend.set_test_backend(None)


@pytest.mark.parametrize('row', gc.ROWS, ids=[r.id for r in gc.ROWS])
def test_row_on_the_cpu_backend(row, cpu):
    """`run_row` asserts the path, criteria (a) and (b), the bit-for-bit properties and that every corruption is rejected."""
    res = gc.run_row(row, 'cpu')
    assert res['ratio'] <= 1.0


@pytest.mark.parametrize('setting', [{}] + [s for s in gc.KNOBS if gc.dense_knobs(s)], ids=lambda s: '-'.join(f'{k}={v}' for k, v in s.items()) or 'default')
def test_knob_rows_on_the_cpu_backend(setting, cpu):
    """The knob rows under the criteria and with the negative controls of the tile sizes each setting selects."""
    for row in gc.KNOB_ROWS:
        assert gc.run_row(row, 'cpu', check_path=False, **gc.dense_knobs(setting))['ratio'] <= 1.0


def test_every_negative_control_has_a_row():
    seen = Counter()
    for row in gc.ROWS:
        g = gc.geo(row)
        x = gc.input_state(row, 'cpu')
        u = gc.matrices(row, 'unitary', 'cpu')
        ref = gc.reference(row, x, u, row.targets)
        for what, bad in gc.corruptions(row, g, x, u, ref, row.targets):
            assert gc.ratio(row, 'unitary', bad, ref, x) > 1.0, (row.id, what)
            seen[what] += 1
        assert gc.ratio(row, 'unitary', ref['out'].to(row.dtype), ref, x) <= 1.0     # (the reference itself, rounded once, passes)
    assert set(seen) == {'k-chunk', 'last-tile', 'targets-swapped', 'sample-of-lane-0', 'second-of-pair'}, seen


def test_the_small_things_on_the_cpu_backend(cpu):
    """The checks the knob child makes of the Z-string kernels and of permute_bits hold for the CPU backend (the Z sums in
    complex128 only: the CPU double adds a complex64 state's probabilities in float32, the kernels in double)."""
    for n in gc.Z_NS + gc.Z_KNOB_NS:
        for k in gc.Z_KS:
            res = gc.check_z_strings(n, k, True, 'cpu')
            assert res['sums'] <= 1.0 and res['amps'] <= 1.0
    for c128 in (False, True):
        gc.check_permute(c128, 'cpu', lds=True)
