"""The paths of the reduction kernels (csrc/dq_reduce.hip) without a GPU: the mirrors `_launch_geometry.marginal` (the whole
MargGeom), `.gate_grad_multi`, `.expect_zmulti` and `.scale_zsigns_waves` on both sides of the conditions they stand for;
that every row of `_reduce_cases.ROWS` reaches the path it claims (in every variant it runs), that every path has a row in
each precision in which it exists, and that a row is the smallest n of its path or says why not; the references against
the oracle; every row on the CPU backend under the criteria that judge the kernels in test_reduce_paths_gpu.py, every
negative control rejected and reached; a Python emulation of marginal_chunk_kernel driven by the mirrored geometry, bit for
bit against `_grid_refs.marginal`; and the tiles of gate_grad_multi adding up to the explicit cross."""

import random
from collections import Counter

import numpy as np
import pytest
import torch

import _grid_refs as R
import _launch_geometry as G
import _reduce_cases as rc
from _cpu_backend import CpuTestBackend
from deepquantum_amd import backend

IDS = [r.id for r in rc.ROWS]
MARGINAL_ROWS = [r for r in rc.ROWS if r.kernel == 'marginal']
MULTI_ROWS = [r for r in rc.ROWS if r.kernel == 'gate_grad_multi']


# ---- the mirrors on both sides of their conditions -------------------------------------------------------------------------
def test_marginal_mirror_conditions():
    """dq_reduce.hip:634-692, the numbers read off the launcher by hand."""
    # :637: the contiguous run is 6 bits for complex64, 7 for complex128, n below it
    assert [G.marginal(n, [0], 3, False)['low'] for n in (5, 6, 7)] == [5, 6, 6]
    assert [G.marginal(n, [0], 3, True)['low'] for n in (6, 7, 8)] == [6, 7, 7]
    g = G.marginal(7, [6], 3, False)['geom']
    assert g['pos'] == [0, 1, 2, 3, 4, 5, 6] + [62] * 5 and g['lo_x'][0] == 6 and g['nlo'] == 1 and g['qmask'] == 0
    # :663-668: the thread-held bits 8 .. 11 take the first candidates (unmeasured ones), then the bits low .. 7
    g64, g128 = G.marginal(10, [9, 8], 3, False), G.marginal(10, [9, 8], 3, True)
    assert g64['geom']['pos'] == [0, 1, 2, 3, 4, 5, 8, 9, 6, 7, 62, 62] and g64['qmask'] == 0
    assert g128['geom']['pos'] == [0, 1, 2, 3, 4, 5, 6, 9, 7, 8, 62, 62] and g128['qmask'] == 2
    assert g64['geom']['lo_x'][:2] == [6, 7] and g64['geom']['lo_out'][:2] == [0, 1] and g64['exclusive']
    # the full chunk with everything measured: a 32 KiB histogram, all four thread-held bits measured
    for bits in (list(range(12)), list(range(11, -1, -1))):
        g = G.marginal(12, bits, 3, False)
        assert (g['nlo'], g['qmask'], g['lds_bytes'], g['blocks'], g['exclusive']) == (12, 15, 32768, 1, True)
    # n = 13 [7]: bit 7 is the one bit outside the chunk in both precisions
    for c128 in (False, True):
        g = G.marginal(13, [7], 3, c128)
        assert g['chunk_bits'] == [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12] and g['nlo'] == 0 and g['exclusive'] and g['blocks'] == 2
        assert g['geom']['hi_pos'][0] == 7 and g['geom']['hi_out'][0] == 0 and g['geom']['hi_pos'][1] == 63
    assert G.marginal(13, [8, 9, 10, 11], 3, False)['qmask'] == 8 and G.marginal(13, [8, 9, 10, 11], 3, True)['qmask'] == 12
    # :683 / :691: exclusive store against atomics; `run` is cut until 2048 workgroups are left
    g = G.marginal(13, [0], 3, False)
    assert (g['run'], g['run_bits'], g['blocks'], g['exclusive'], g['nlo'], g['qmask']) == (0, 1, 2, False, 1, 0)
    assert [G.marginal(13, [0], b, False)['run'] for b in (2047, 2048)] == [0, 1]
    assert G.marginal(13, [0], 2048, False)['blocks'] == 1
    g = G.marginal(14, [13], 3, False)
    assert (g['blocks'], g['run'], g['nlo'], g['nhi'], g['exclusive'], g['cpos']) == (4, 0, 0, 1, False, [12, 13])
    assert len(g['geom']['cpos']) == 28 and g['geom']['cpos'][:3] == [12, 13, 63]


def test_gate_grad_multi_mirror_conditions():
    """backend.py:491 (gate by gate below the tile), :498-506 (the two ways a launch is split) and dq_reduce.hip:829-878."""
    for c128 in (False, True):
        tile, low, per = rc.tile_geometry(c128)
        assert G.gate_grad_multi(tile - 1, c128, [(0, ()), (1, ())]) == [dict(route='gate_grad', gates=[0]), dict(route='gate_grad', gates=[1])]
        la = G.gate_grad_multi(tile, c128, [(0, ())] * (per + 1))
        assert [x['gates'] for x in la] == [list(range(per)), [per]] and la[0]['route'] == 'tile'
        la = G.gate_grad_multi(tile + 1, c128, [(tile, (tile - 1, 1))])[0]       # the top bit gathered: bit T - 1 falls outside
        assert la['outside'] == [tile - 1] and la['high_sorted'] == list(range(low, tile - 1)) + [tile]
        assert la['desc'] == [dict(tbit=tile - 1, cin=2, cout=1 << (tile - 1))]
    la = G.gate_grad_multi(12, False, [(t, ()) for t in range(4, 12)])
    assert [x['gates'] for x in la] == [list(range(7)), [7]] and la[0]['outside'] == [11] and la[1]['outside'] == [10]
    la = G.gate_grad_multi(12, False, [(t, ()) for t in range(5, 12)])
    assert len(la) == 1 and la[0]['outside'] == [4] and la[0]['high_sorted'] == list(range(5, 12))


def test_z_string_mirror_conditions():
    """Which slices of which workgroup lie inside the state (expect_zmulti_mfma_kernel) and which waves of
    scale_zsigns_mfma_kernel have no work."""
    z = lambda n, c128: G.expect_zmulti(n, c128)                                # noqa: E731
    assert z(8, False)['slices'] == [[0]] and z(9, False)['slices'] == [[0, 1]] and z(10, False)['slices'] == [[0, 1, 2, 3]]
    assert z(11, False)['slices'] == [list(range(8)), []] and z(11, False)['idle_blocks'] == [1]      # the second workgroup: no work at all
    assert z(12, False)['idle_blocks'] == [2, 3]
    assert z(8, True)['slices'] == [[0]] and z(9, True)['slices'] == [[0, 1]] and z(10, True)['slices'] == [[0, 1, 2, 3]]
    assert z(11, True)['slices'] == [[0, 1, 2, 3]] * 2 and z(12, True)['idle_blocks'] == []
    for n in (9, 10):
        assert any(len(s) < z(n, False)['u'] for s in z(n, False)['slices'])    # slices past the end
    assert G.scale_zsigns_waves(8)['idle_waves'] == [(0, 1), (0, 2), (0, 3)]
    assert G.scale_zsigns_waves(9)['idle_waves'] == [(0, 2), (0, 3)]
    assert all(G.scale_zsigns_waves(n)['idle_waves'] == [] for n in (10, 11, 12))
    # the masks of the rows: every structured mask among the strings 0 .. 15 once and among 16 .. 31 once
    for n in rc.Z_NS:
        plain, rot = rc.z_masks(n, 32, False), rc.z_masks(n, 32, True)
        assert sorted(plain) == sorted(rot) and len(rc.z_masks(n, 33, True)) == 33
        for m in rc.z_structured(n):
            assert {plain.index(m) < 16, rot.index(m) < 16} == {True, False}, (n, m)
        assert sorted(rc.Z_KS) == ['scale', 'scale-two-launches', 'sums'] and len(rc.Z_ROWS) == 30
        assert all(m >> n == 0 for m in plain)


# ---- the rows: ids, paths, census, floors --------------------------------------------------------------------------------------
def test_row_ids_are_unique_and_well_formed():
    assert len(set(IDS)) == len(IDS)
    for r in rc.ROWS:
        assert r.kernel in ('marginal', 'gate_grad', 'gate_grad_multi', 'expect_pauli', 'inner', 'probs') and r.path in rc.PATHS
        assert r.batch == rc.BATCH or r.path == 'marg-run', r.id
        for args in r.variants():
            assert rc.valid(r, r.n, args), r.id
        if r.kernel == 'marginal':
            assert len(set(r.args)) == len(r.args) >= 1
        if r.kernel == 'gate_grad':
            assert len(set(r.args[0] + r.args[1])) == len(r.args[0] + r.args[1]) and len(r.args[0]) in (1, 2)
        if r.kernel == 'gate_grad_multi':
            assert all(t not in c and len(set(c)) == len(c) for t, c in r.args)


@pytest.mark.parametrize('row', rc.ROWS, ids=IDS)
def test_every_row_reaches_its_path(row):
    for args in row.variants():
        g = rc.geo(row, args=args)
        assert rc.PATHS[row.path](g), (row.id, args, g)
    if row.kernel == 'marginal' and len(row.args) > 1:
        assert len(row.variants()) == 2 and sorted(row.variants()[1]) == sorted(row.args)
    if row.kernel == 'gate_grad' and len(row.args[0]) == 2:
        assert [v[0] for v in row.variants()] == [row.args[0], row.args[0][::-1]]


def test_census_every_path_has_a_row_in_each_precision():
    claimed = Counter(r.path for r in rc.ROWS)
    assert set(claimed) == set(rc.PATHS), set(rc.PATHS) ^ set(claimed)
    for p in rc.PATHS:
        assert {r.c128 for r in rc.ROWS if r.path == p} == ({False} if p in rc.C64_ONLY else {False, True}), p
    # what the table is made for, by name
    marg = {(r.n, r.args) for r in MARGINAL_ROWS if not r.c128}
    assert {(12, tuple(range(12))), (12, tuple(range(11, -1, -1))), (13, tuple(range(13))), (13, (7,)), (14, (0, 13))} <= marg
    assert sorted(r.n for r in rc.ROWS if r.kernel == 'inner' and not r.c128) == [1, 255, 257, 1000]
    assert max(r.batch << r.n for r in rc.ROWS if r.kernel != 'inner') * 8 == 128 << 20       # the largest input: 128 MiB
    for c128 in (False, True):
        one = next(r for r in MULTI_ROWS if r.path == 'ggm-gate-by-gate' and r.c128 == c128)
        assert one.n == rc.tile_geometry(c128)[0] - 1


@pytest.mark.parametrize('row', rc.ROWS, ids=IDS)
def test_every_row_is_the_smallest_n_of_its_path_or_says_why(row):
    smaller = [n for n in range(1, row.n) if rc.valid(row, n) and rc.PATHS[row.path](rc.geo(row, n=n))]
    if row.note:
        assert smaller, f'{row.id}: the note is stale, no smaller n reaches {row.path}'
    else:
        assert not smaller, f'{row.id}: n = {smaller} reach {row.path} too'


# ---- the references against the oracle ----------------------------------------------------------------------------------------
SMALL = [r for r in rc.ROWS if r.batch == rc.BATCH]


@pytest.mark.parametrize('row', SMALL, ids=[r.id for r in SMALL])
def test_reference_agrees_with_the_oracle(row):
    cpu = CpuTestBackend()
    x, y = (t if t is None else t.to(torch.complex128) for t in rc.row_inputs(row, 'random', 'cpu'))
    for args in row.variants():
        ref, s = rc.reference(row, args, x, y)
        if row.kernel == 'marginal':
            want = cpu.marginal(x, list(args))
        elif row.kernel == 'gate_grad':
            want = cpu.gate_grad(x, y, list(args[0]), list(args[1]))
        elif row.kernel == 'gate_grad_multi':
            want = torch.stack([cpu.gate_grad(x, y, [t], list(c)) for t, c in args], dim=1)
        elif row.kernel == 'expect_pauli':
            want = cpu.expect_pauli(x, *args)
            assert torch.allclose(ref, R.expect_pauli(x, *args)[0], rtol=0, atol=1e-13)
        elif row.kernel == 'inner':
            want = cpu.inner(x, y)
        else:
            want = cpu.probs(x)
        assert want.shape == ref.shape and float((want - ref).abs().max()) < 1e-13, (row.id, args)
        assert bool((s >= ref.abs() * (1 - 1e-12)).all())                      # S is an upper bound of the value


# ---- every row on the CPU backend, every negative control rejected and reached --------------------------------------------------
@pytest.fixture()
def cpu():
    backend.set_test_backend(CpuTestBackend())
    yield
    backend.set_test_backend(None)


@pytest.mark.parametrize('row', rc.ROWS, ids=IDS)
def test_row_on_the_cpu_backend(row, cpu):
    """`run_row` asserts the path, both criteria and that every corruption is rejected."""
    res = rc.run_row(row, 'cpu')
    assert res['ratio'] <= 1.0


@pytest.mark.parametrize('n,c128,what', rc.Z_ROWS, ids=rc.Z_IDS)
def test_z_row_on_the_cpu_backend(n, c128, what, cpu):
    """(The double forms all K strings at once: K = 33 is one rounding here, two launches on the GPU.)"""
    res = rc.run_z_row(n, c128, what, 'cpu')
    assert res['ratio'] <= 1.0
    assert res['controls'] == ({rc.Z_CONTROLS[1]} if what != 'sums' else {rc.Z_CONTROLS[0]} if n > 8 else set())


def test_every_negative_control_has_a_row():
    """From reference tensors only: every corruption is made by some row, and rejected by that row's criterion."""
    seen = Counter()
    for row in SMALL:
        for args in row.variants():
            g = rc.geo(row, args=args)
            x, y = rc.row_inputs(row, 'random', 'cpu')
            ref, s = rc.reference(row, args, x, y)
            for what, bad in rc.corruptions(row, g, args, x, y, ref):
                assert rc.ratio(bad, ref, s, rc.tau(row, g)) > 1.0, (row.id, what)
                seen[what] += 1
            rounded = ref.to(x.real.dtype) if row.kernel == 'probs' else ref
            assert rc.ratio(rounded, ref, s, rc.tau(row, g)) <= 1.0               # (the reference itself passes)
    assert set(seen) == set(rc.CONTROLS), set(rc.CONTROLS) ^ set(seen)


# ---- marginal_chunk_kernel in Python, driven by the mirrored geometry ------------------------------------------------------------
def emulate_marginal_chunk_kernel(psi: np.ndarray, n: int, nw: int, geo: dict) -> np.ndarray:
    """dq_reduce.hip:166-241 for every workgroup of the grid, the 256 threads as a vector: the same loops over the padded
    geometry (constant trip counts, no guards but the kernel's own), the same choice between the thread sum, the block sum
    and the histogram, and between the exclusive store and the add.  ``psi``: (B, 2^n) complex; -> (B, 2^nw) float64."""
    g = geo['geom']
    u = np.uint64
    nb = psi.shape[0]
    out = np.zeros((nb, 1 << nw))
    nloc, nx = 1 << g['nlo'], 1 << g['c']
    xt = np.arange(256, dtype=u)
    off_t = np.zeros(256, dtype=u)
    for i in range(8):
        off_t |= ((xt >> u(i)) & u(1)) << u(g['pos'][i])
    jt = np.zeros(256, dtype=u)
    for t in range(12):
        jt |= ((xt >> u(g['lo_x'][t])) & u(1)) << u(t)
    off_k = np.zeros(16, dtype=u)
    for k in range(16):
        for i in range(8, 12):
            off_k[k] |= u(((k >> (i - 8)) & 1) << g['pos'][i])
    rows = np.arange(nb)[:, None]
    for bx in range(geo['blocks']):
        hist = np.zeros((nb, nloc))
        s = np.zeros((nb, 256))
        base0 = None
        for ci in range(bx << g['run'], (bx + 1) << g['run']):
            base = 0
            for t in range(28):
                base |= ((ci >> t) & 1) << g['cpos'][t]
            if base0 is None:
                base0 = base
            for k in range(16):
                live = (xt | u(k << 8)) < u(nx)
                idx = np.where(live, off_t + off_k[k], u(0)) + u(base)      # (the sum wraps where a pad meets a pad: never live)
                a = psi[:, idx.astype(np.int64)]
                v = np.where(live[None, :], a.real * a.real + a.imag * a.imag, 0.0)
                if g['qmask'] == 0:
                    s += v
                else:
                    j = jt.copy()
                    for t in range(12):
                        j |= u(((k << 8) >> g['lo_x'][t]) & 1) << u(t)
                    np.add.at(hist, (rows, j[live].astype(np.int64)[None, :]), v[:, live])
        if g['qmask'] == 0:
            if g['nlo'] == 0:
                hist[:, 0] = s.sum(axis=1)
            else:
                np.add.at(hist, (rows, jt.astype(np.int64)[None, :]), s)
        hi = 0
        for t in range(40):
            hi |= ((base0 >> g['hi_pos'][t]) & 1) << g['hi_out'][t]
        j = np.arange(nloc, dtype=np.int64)
        o = np.full(nloc, hi, dtype=np.int64)
        for t in range(12):
            o |= ((j >> t) & 1) << g['lo_out'][t]
        if g['exclusive']:
            out[:, o] = hist
        else:
            np.add.at(out, (rows, o[None, :]), hist)
    return out


def _emulation_agrees(n, bits, batch, c128, seed):
    geo = G.marginal(n, list(bits), batch, c128)
    x = rc.input_state(2, 1 << n, torch.complex128, 'exact', seed, 'cpu')       # (samples are independent: two stand for the batch)
    got = emulate_marginal_chunk_kernel(x.numpy(), n, len(bits), geo)
    assert np.array_equal(got, R.marginal(x, list(bits)).numpy()), (n, bits, batch, c128, geo)


@pytest.mark.parametrize('row', MARGINAL_ROWS, ids=[r.id for r in MARGINAL_ROWS])
def test_marginal_emulation_on_every_row(row):
    for bits in row.variants():
        _emulation_agrees(row.n, bits, row.batch, row.c128, row.seed)


@pytest.mark.parametrize('n', range(1, 14))
def test_marginal_emulation_on_seeded_wire_sets(n):
    """Both precisions, batch 3 and 4096 (where `run` survives the cut), wire sets of every size class in seeded orders."""
    rng = random.Random(n)
    sets = [[0], [n - 1], list(range(n)), list(range(n - 1, -1, -1))]
    sets += [rng.sample(range(n), rng.randint(1, n)) for _ in range(4)]
    for c128 in (False, True):
        for batch in (3, 4096):
            for bits in sets:
                _emulation_agrees(n, bits, batch, c128, 100 * n + len(bits))
    assert n < 13 or G.marginal(13, [0], 4096, False)['run'] == 1


# ---- gate_grad_multi: the mirror's tiles add up to the explicit cross -----------------------------------------------------------
TILE_ROWS = [r for r in MULTI_ROWS if r.path != 'ggm-gate-by-gate']


@pytest.mark.parametrize('row', TILE_ROWS, ids=[r.id for r in TILE_ROWS])
def test_tiles_of_gate_grad_multi_add_up_to_the_cross(row):
    x, y = (t.to(torch.complex128) for t in rc.row_inputs(row, 'exact', 'cpu'))
    for la in G.gate_grad_multi(row.n, row.c128, list(row.args)):
        assert sorted(la['tile_bits'] + la['outside']) == list(range(row.n)) and la['ntiles'] == 1 << len(la['outside'])
        for gi, d in zip(la['gates'], la['desc']):
            t, c = row.args[gi]
            assert la['tile_bits'][d['tbit']] == t
            total = sum(R.tile_cross(x, y, la['tile_bits'], tile, t, c) for tile in range(la['ntiles']))
            assert torch.equal(torch.view_as_real(total), torch.view_as_real(R.cross(x, y, [t], list(c))[0])), (row.id, gi)
            # the tiles the kernel skips for this gate (dq_reduce.hip:767) are the ones that add nothing
            for tile in range(la['ntiles']):
                base = sum(((tile >> q) & 1) << p for q, p in enumerate(la['outside']))
                if base & d['cout'] != d['cout']:
                    assert not bool(R.tile_cross(x, y, la['tile_bits'], tile, t, c).abs().any())


# ---- the slices of backend._scale_z_signs_wide, the CPU double standing in for the complex128 kernel ---------------------------
@pytest.mark.parametrize('wide_bytes', [256 << 20, 16 << 13, 16 << 12, 16 << 9, 1])
def test_slices_of_the_wide_scale_path(wide_bytes, cpu, monkeypatch):
    """Whole samples per slice, one sample per slice, runs of 2^9 and 2^8 amplitudes of a sample: integer input, bit for bit."""
    n, k = 12, 70
    masks = (rc.z_masks(n, 33, True) + rc.z_masks(n, 33, False) + [0b101, 1 << 11, 0b111000000000, 1])[:k]
    x, coef = rc.z_inputs(n, False, k, 'exact', 'cpu')
    monkeypatch.setattr(backend, '_WIDE_BYTES', wide_bytes)
    got = backend._scale_z_signs_wide(x, masks, coef, n)
    assert got.dtype == torch.complex64 and rc.bits_equal(got, R.scale_z_signs(x, masks, coef))
