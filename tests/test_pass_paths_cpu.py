"""The launch paths of the wave-tile pass kernel without a GPU: the mirror of `wave_launch` (`_launch_geometry.wave_pass`) on
both sides of every threshold and against the library's own tile count; the grid's index arithmetic as a bijection onto
batch x tiles for every row of the case table (`_pass_cases.ROWS`); that every row reaches the paths it claims, at full
size, and is the smallest shape where it says so; what the older cases of this kernel reach; and every row shrunk to
n <= 14 on the CPU backend against the references that judge the kernel in test_pass_paths_gpu.py, those references
themselves against the oracle."""

from collections import Counter

import numpy as np
import pytest
import torch

import _grid_refs as R
import _handler_cases as hc
import _launch_geometry as G
import _pass_cases as pc
import _wave_emulator as emu
from deepquantum_amd import fusion
from oracle import statevec_oracle as oracle

PREC = pytest.mark.parametrize('c128', [False, True], ids=['c64', 'c128'])


# ---- the mirror on both sides of every boundary ----------------------------------------------------------------------------
@PREC
def test_two_tiles_per_wave_from_16384_tiles_on(c128):
    m = pc.tile_bits(c128)
    for n, batch in ((m + 14, 1), (m + 10, 16), (m + 7, 128), (m, 16384)):
        at = G.wave_pass(n, batch, c128, grad=True)
        assert at['tiles'] * batch == 16384 and at['tpw'] == 2 and at['grid_x'] == max(1, at['tiles'] // 8)
        assert at['second_stride'] == at['grid_x'] * 4
        for kw in (dict(only_expz=True), dict(ext=True)):
            assert G.wave_pass(n, batch, c128, grad=True, **kw)['tpw'] == 2
        assert G.wave_pass(n, batch, c128)['tpw'] == 1                            # a plain launch: DQ_WAVE_TPW defaults to 1
        below = G.wave_pass(n, batch // 2, c128, grad=True) if batch > 1 else G.wave_pass(n - 1, 1, c128, grad=True)
        assert below['tiles'] * max(1, batch // 2) == 8192 and below['tpw'] == 1 and below['second_stride'] is None
    assert G.wave_pass(m + 16, 1, c128, grad=True)['tpw'] == 2                    # (the cap: never more than two)


@PREC
def test_xcd_numbers_and_regrouping_from_eight_workgroups_on(c128):
    m = pc.tile_bits(c128)
    for batch in (1, 3, 5):
        four, eight = G.wave_pass(m + 4, batch, c128), G.wave_pass(m + 5, batch, c128)
        assert (four['grid_x'], four['xcd'], four['regroup']) == (4, 0, False)
        assert (eight['grid_x'], eight['xcd'], eight['regroup']) == (8, 31, False)
        four, eight = G.wave_pass(m + 4, batch, c128, shared_input=True), G.wave_pass(m + 5, batch, c128, shared_input=True)
        assert (four['grid_x'], four['xcd'], four['regroup']) == (4, 0, False)
        assert (eight['grid_x'], eight['xcd'], eight['regroup']) == (8, 0, True)   # a shared input switches the XCD numbers off
    # known-zero and held bits outside the tile shrink the tile count and move the threshold with it
    assert G.wave_pass(m + 8, 2, c128, zero_bits_outside=3)['xcd'] == 31 and G.wave_pass(m + 8, 2, c128, zero_bits_outside=3)['grid_x'] == 8
    assert G.wave_pass(m + 8, 2, c128, zero_bits_outside=4)['xcd'] == 0 and G.wave_pass(m + 8, 2, c128, zero_bits_outside=4)['grid_x'] == 4
    assert G.wave_pass(m + 8, 2, c128, slice_bits=2)['tiles'] == 64 and G.wave_pass(m + 8, 2, c128, slice_bits=2, zero_bits_outside=1)['tiles'] == 32
    # two tiles per wave halve the grid: the threshold of the XCD numbers is met at the halved grid
    assert G.wave_pass(m + 14, 1, c128, grad=True)['grid_x'] == 2048 and G.wave_pass(m + 14, 1, c128, grad=True)['xcd'] == 31


@PREC
def test_streaming_from_one_gib_on(c128):
    n = 26 if c128 else 27
    at, below = G.wave_pass(n, 1, c128), G.wave_pass(n - 1, 1, c128)
    assert at['nt_loads'] and at['nt_stores'] and not below['nt_loads'] and not below['nt_stores']
    assert not G.wave_pass(n - 4, 15, c128)['nt_stores'] and G.wave_pass(n - 4, 16, c128)['nt_stores']       # one sample less than 1 GiB
    sh = G.wave_pass(n - 4, 16, c128, shared_input=True)
    assert sh['nt_stores'] and not sh['nt_loads'] and sh['regroup']                                          # the shared input stays cacheable


@PREC
def test_idle_waves_below_four_tiles(c128):
    m = pc.tile_bits(c128)
    assert [G.wave_pass(m + d, 2, c128, grad=True)['idle_waves'] for d in (0, 1, 2, 3)] == [3, 2, 0, 0]
    assert all(G.wave_pass(m + d, 2, c128, grad=True)['grid_x'] == 1 for d in (0, 1, 2))


# ---- the rows: tile counts against the library, paths, floors -------------------------------------------------------------------
@pytest.fixture(scope='module')
def planned():
    return {row.id: (row, pc.plan(row)) for row in pc.ROWS + pc.KNOB_ROWS}


def test_every_path_has_an_exact_row_per_precision():
    for is128 in (False, True):
        exact = {p for r in pc.ROWS if r.is128 == is128 and r.kind == 'exact' for p in r.paths}
        assert exact >= {'A', 'A1', 'B', 'C', 'D', 'D2', 'E', 'EH', 'F', 'Fs', 'ADF', 'G', 'H8', 'H4'}, exact
    assert len({r.id for r in pc.ROWS}) == len(pc.ROWS)


def test_rows_reach_their_paths_and_the_mirror_counts_the_librarys_tiles(planned):
    """At full size: scheduling and the descriptor hook need no GPU.  `tiles` of the mirror against the zext word of
    `dq_wave_descriptor` for every pass of every row (plain and zero-extended; the hook takes no held bits, so a slice's
    count is only held against :385-390 by hand above); every path a row names is reached by one of its passes; a `floor`
    path is not reached with one qubit less (same flags, from the mirror)."""
    ext_seen = 0
    for row, pl in planned.values():
        info = pc.step_info(row, pl)
        for g in info:
            assert g['tiles'] == g['lib_tiles'], (row.id, g['tiles'], g['lib_tiles'])
            ext_seen += g['ext']
        for p in row.paths:
            assert any(pc.PATHS[p](g) for g in info), (row.id, p)
        for p in row.floor:
            for g in (g for g in info if pc.PATHS[p](g)):
                less = dict(g)
                less.update(G.wave_pass(row.n - 1, row.batch, row.is128, grad=row.reducing, only_expz=g['only_expz'], ext=g['ext'],
                                        shared_input=g['regroup'] or (row.shared and g is info[0]), zero_bits_outside=g['zero_bits']))
                assert not pc.PATHS[p](less), (row.id, p)
        if row.mode == 'expz':
            assert all(pl.ops[i].kind != 'expz' for st in pl.steps[:-1] for i in st.ops)
    assert ext_seen >= 4


def test_zero_extended_and_plain_descriptors_count_tiles_as_the_mirror_does():
    from test_wave_cpu import random_ops

    for is128, n in ((False, 17), (False, 20), (True, 16), (True, 19)):
        ops, _ = random_ops(n, 120, n)
        geom = fusion.default_geometry(is128)
        geom.plan_min_bits = 11
        geom.permute_store = True
        for st in fusion.schedule(ops, n, geom):
            d = st.desc
            tile = set(range(d.L)) | {d.high_pos[i] for i in range(d.h)}
            outside = [p for p in range(n - 1, -1, -1) if p not in tile]
            for nz in range(0, len(outside) + 1):
                kz = sum(1 << p for p in outside[:nz])
                kz_in = kz | (1 << d.high_pos[0])                       # a known-zero bit INSIDE the tile does not count
                for mask in (kz, kz_in):
                    assert 1 << (emu.descriptor(d, n, mask).zext & 63) == G.wave_pass(n, 1, is128, zero_bits_outside=nz)['tiles']


# ---- the grid as a bijection ---------------------------------------------------------------------------------------------------
def _is_bijection(geo, batch):
    seen = Counter(G.wave_grid_visits(geo, batch))
    return len(seen) == batch * geo['tiles'] and set(seen.values()) == {1} and \
        all(0 <= s < batch and 0 <= t < geo['tiles'] for s, t in seen)


def test_the_grid_visits_every_tile_of_every_sample_once(planned):
    """The kernel's index arithmetic (:138-175) re-done in Python from the mirror, for every pass of every row: the
    (sample, tile) pairs the grid visits are batch x tiles, each once.  And the test tells: with the mirror's `xcd` or
    `second_stride` altered the same walk is no bijection."""
    done = {}
    for row, pl in planned.values():
        for g in pc.step_info(row, pl):
            key = (row.batch, g['tiles'], g['tpw'], g['grid_x'], g['xcd'], g['regroup'], g['second_stride'])
            if key not in done:
                done[key] = _is_bijection(g, row.batch)
            assert done[key], (row.id, key)
    assert len(done) >= 20
    kinds = {(k[2], k[4], k[5]) for k in done}
    assert {(1, 0, False), (1, 31, False), (2, 31, False), (2, 0, False), (1, 0, True)} <= kinds, kinds
    # altered by hand
    two = G.wave_pass(26, 1, False, grad=True)
    assert _is_bijection(two, 1)
    assert not _is_bijection(dict(two, second_stride=two['second_stride'] // 2), 1)
    assert not _is_bijection(dict(two, second_stride=two['second_stride'] * 2), 1)
    odd = G.wave_pass(12 + 4, 1, False)                                  # grid.x = 4: the XCD line must not run
    assert _is_bijection(odd, 1) and not _is_bijection(dict(odd, xcd=31), 1)
    sh = G.wave_pass(17, 3, False, shared_input=True)
    assert _is_bijection(sh, 3) and not _is_bijection(dict(sh, regroup=False, xcd=31, grid_x=12, tiles=32), 3)


def test_regrouping_puts_the_samples_of_a_tile_group_next_to_each_other():
    """:141-146 for a batch that is no power of two, from the walk of `wave_grid_visits` (workgroups in dispatch order, four
    waves each): workgroups 8 b k .. 8 b (k + 1) - 1 are exactly the b samples of tile groups 8 k .. 8 k + 7, and the b
    workgroups of one tile group lie eight apart, i.e. on one XCD of the round robin."""
    for batch in (3, 5):
        geo = G.wave_pass(17, batch, False, shared_input=True)
        assert geo['regroup'] and geo['tpw'] == 1
        visits = G.wave_grid_visits(geo, batch)                  # (by, bx, wave) order: four entries per workgroup
        wgs = [(visits[4 * i][0], visits[4 * i][1] // 4) for i in range(len(visits) // 4)]      # (sample, tile group) by dispatch number
        assert len(wgs) == batch * geo['grid_x']
        for k in range(geo['grid_x'] // 8):
            run = wgs[8 * batch * k: 8 * batch * (k + 1)]
            assert sorted(run) == sorted((s_, g_) for s_ in range(batch) for g_ in range(8 * k, 8 * k + 8))
            for g_ in range(8 * k, 8 * k + 8):
                where = [i for i, w in enumerate(run) if w[1] == g_]
                assert len({i % 8 for i in where}) == 1 and where == list(range(where[0], where[0] + 8 * batch, 8))


def test_what_the_knobs_change_in_the_knob_rows(planned):
    """The knob test on the GPU compares results only.  Here: what every setting changes in the launches of its two rows,
    from the mirror with the setting applied -- so a setting that is meant to move a launch to another path is known to do
    so at these shapes -- and every such grid is still a bijection."""
    red, fwd = pc.KNOB_ROWS
    geos = {}
    for row in (red, fwd):
        info = pc.step_info(row, planned[row.id][1])
        for ki, knob in enumerate([{}] + pc.KNOBS):
            geos[row.mode, ki - 1] = [G.wave_pass(row.n, row.batch, row.is128, grad=row.reducing, only_expz=g['only_expz'], ext=g['ext'],
                                                  env=knob) for g in info]
            for g in geos[row.mode, ki - 1]:
                assert _is_bijection(g, row.batch), (row.id, knob)
    at = lambda mode, knob: geos[mode, pc.KNOBS.index(knob)]                                           # noqa: E731
    assert all((g['tpw'], g['grid_x'], g['xcd']) == (2, 512, 31) for g in geos['grad', -1])             # the defaults
    assert all((g['tpw'], g['grid_x'], g['xcd']) == (1, 256, 31) for g in geos['fwd', -1])
    for v in range(4):
        for mode in ('grad', 'fwd'):
            assert all((g['nt_loads'], g['nt_stores']) == (bool(v & 1), bool(v & 2)) for g in at(mode, {'DQ_WAVE_NT': str(v)}))
    assert all(g['xcd'] == 0 for mode in ('grad', 'fwd') for g in at(mode, {'DQ_WAVE_XCD': '0'}))
    assert all(g['xcd'] == 2 for mode in ('grad', 'fwd') for g in at(mode, {'DQ_WAVE_XCD': '2'}))      # the xv != 31 branch of :157
    assert all(g['xcd'] == 7 for g in at('grad', {'DQ_WAVE_XCD': '64'}))                               # grid.x = 512 = 8 * 64
    assert all(g['xcd'] == 0 for g in at('fwd', {'DQ_WAVE_XCD': '64'}))                                # grid.x = 256: the mapping is off
    assert all((g['tpw'], g['grid_x']) == (2, 128) for g in at('fwd', {'DQ_WAVE_TPW': '2'}))
    assert all(g['tpw'] == 2 for g in at('grad', {'DQ_WAVE_TPW': '2'}))                                # (not read by a reducing launch)
    assert all((g['tpw'], g['grid_x']) == (1, 1024) for g in at('grad', {'DQ_WAVE_GRAD_TPW': '1'}))
    assert all((g['tpw'], g['grid_x'], g['second_stride']) == (8, 128, 512) for g in at('grad', {'DQ_WAVE_GRAD_TPW': '8'}))
    assert all((g['tpw'], g['xcd']) == (2, 0) for g in at('grad', {'DQ_WAVE_XCD_TPW': '0'}))
    # DQ_WAVE_EXPZ_TPW is the cap of passes without a DQ_FG_GRAD record: every pass of the reducing row has one
    assert not any(g['only_expz'] for g in pc.step_info(red, planned[red.id][1]))
    assert at('grad', {'DQ_WAVE_EXPZ_TPW': '1'}) == geos['grad', -1]


# ---- what the older cases reach --------------------------------------------------------------------------------------------------
def test_what_the_older_cases_of_this_kernel_reach():
    """The parameters of the tests that ran this kernel before this file, through the mirror."""
    # test_kernels_gpu.py::test_fused_pass_with_one_shared_input_state as it was: no grid of eight workgroups
    for is128, n, b in ((False, 15, 3), (False, 16, 16), (True, 14, 5), (False, 13, 4), (True, 11, 2)):
        assert not G.wave_pass(n, b, is128, shared_input=True)['regroup']
    # ... and the two shapes added to it
    for is128, n, b in ((False, 17, 3), (True, 16, 5)):
        assert G.wave_pass(n, b, is128, shared_input=True)['regroup']
    # test_wave_gpu.py::test_wave_batched_matrices_and_one_shared_input_state: complex64 never, complex128 at (16, 16) only
    got = {(is128, n, b): G.wave_pass(n, b, is128, shared_input=True)['regroup']
           for is128 in (False, True) for n, b in ((15, 3), (16, 16), (13, 4), (12, 5))}
    assert [k for k, v in got.items() if v] == [(True, 16, 16)]
    # _helpers.check_grad_records (n <= 15), check_fused_sweep (pair states up to n = 21, batch 2) and
    # test_sweep_passes_with_their_records_in_device_memory_on_gpu (n <= 15): one tile per wave
    for is128 in (False, True):
        for n, b in ((15, 2), (21, 2), (17, 3)):
            assert G.wave_pass(n, b, is128, grad=True)['tpw'] == 1
        for n in (13, 14, 15):
            assert G.wave_pass(n, 2, is128, grad=True, ext=True)['tpw'] == 1
    # test_z_string_expectations_from_the_registers_on_gpu: n = 21, batch 2
    assert G.wave_pass(21, 2, False, grad=True, only_expz=True)['tpw'] == 1
    assert G.wave_pass(21, 2, True, grad=True, only_expz=True)['tpw'] == 1
    # check_grad_records at n = m, m + 1 reaches G
    assert G.wave_pass(12, 2, False, grad=True)['idle_waves'] == 3 and G.wave_pass(11, 2, True, grad=True)['idle_waves'] == 3


# ---- the references, proven before they judge ---------------------------------------------------------------------------------------
@PREC
@pytest.mark.parametrize('mode', ['grad', 'expz'])
def test_references_against_the_oracle_and_numpy(mode, c128):
    """`_pass_cases.reference` (torch, pass order) against the oracle applying the caller's order gate by gate, and its sums
    against `_handler_cases.grad_sums` / a float64 parity sum in numpy; the tile's share against a masked state."""
    n = 13
    row = pc.Row((), n, 2, c128, 'round', mode, 5)
    pl = pc.plan(row)
    info = pc.step_info(row, pl)
    x = pc.input_state(row, 'cpu')
    ref = pc.reference(row, pl, x, info)
    mats = pl.src_mats.to(torch.complex128)
    cur = x.to(torch.complex128)
    want = np.full((2, pl.nrows + 1, 8), np.nan)
    for op in pl.ops:
        v = cur.numpy()
        if op.kind == 'grad':
            want[:, op.mode & fusion.GRAD_ROW_MASK] = hc.grad_components(hc.grad_sums(v, op.targets[0], op.targets[1], op.controls),
                                                                         op.mode >> fusion.GRAD_VARIANT_SHIFT)
        elif op.kind == 'expz':
            idx = np.arange(1 << n)
            par = sum(((idx >> q) & 1) for q in op.controls) & 1
            want[:, op.mode, 0] = ((v.real ** 2 + v.imag ** 2) * (1.0 - 2.0 * par)).sum(-1)
        else:
            d = 1 << op.k
            cur = oracle.apply_gate_bits(cur, mats[op.mat:op.mat + d * d].reshape(d, d), list(op.targets), list(op.controls))
    assert (ref['out'] - cur).abs().max().item() < 1e-13
    if mode == 'expz':            # (the sums of a sweep are taken in pass order, where commuting gates may have moved past a record)
        assert np.array_equal(np.isnan(want), torch.isnan(ref['acc']).numpy())
        assert np.nanmax(np.abs(want - ref['acc'].numpy())) < 1e-13
    else:
        again = pc.reference(row, pl, x, info, order=list(range(len(pl.ops))))
        assert np.array_equal(np.isnan(want), torch.isnan(again['acc']).numpy())
        assert np.nanmax(np.abs(want - again['acc'].numpy())) < 1e-13
    assert bool((ref['drop'][0] != 0).any()) and bool((ref['drop'][1:] == 0).all())
    assert float((ref['bound'][~torch.isnan(ref['acc'])]).min()) > 0


def test_a_tiles_share_of_the_sums_is_the_sum_over_the_tile():
    n = 14
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 1 << n, generator=g, dtype=torch.float64) + 1j * torch.randn(2, 1 << n, generator=g, dtype=torch.float64)
    blk = [13, 5]
    for tile in range(4):
        idx, free = R.tile_indices(n, blk, tile, 'cpu')
        assert idx.numel() == 1 << 12 and bool((((idx >> 13) & 1) == (tile & 1)).all()) and bool((((idx >> 5) & 1) == (tile >> 1)).all())
        masked = torch.zeros_like(x)
        masked[:, idx] = x[:, idx]
        for t, s, ctl in ((7, 0, ()), (12, 0, (3,)), (4, 0, (13,)), (9, 0, (5, 2))):
            a, _ = R.tile_grad_sums(x, idx, free, t, s, ctl)
            b, _ = R.grad_sums(masked, t, s, ctl)
            assert (a - b).abs().max().item() < 1e-12
    total = sum(R.tile_grad_sums(x, *R.tile_indices(n, blk, t, 'cpu'), 7, 0, (13,))[0] for t in range(4))
    assert (total - R.grad_sums(x, 7, 0, (13,))[0]).abs().max().item() < 1e-11


# ---- every row, shrunk, on the CPU backend -----------------------------------------------------------------------------------------
SHRUNK = list({pc.shrunk(r).id: pc.shrunk(r) for r in pc.ROWS}.values())


@pytest.mark.parametrize('row', SHRUNK, ids=[r.id for r in SHRUNK])
def test_rows_shrunk_on_the_cpu_backend(cpu_backend, row):
    """The same seeded gate lists, criteria and negative controls as on the GPU, at n <= 14 through the descriptor
    interpreter (tests/_cpu_backend.py): the rows' references and bounds are sound before they judge the kernel."""
    res = pc.run_row(row, 'cpu', check_paths=False)
    assert res['state'] <= 1.0 and (res['sums'] is None or res['sums'] <= 1.0)
