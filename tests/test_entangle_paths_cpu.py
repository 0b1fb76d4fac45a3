"""What test_entangle_paths_gpu.py stands on, checked without a GPU:

- the full mirror of the entanglement plan (_launch_geometry.entangle_passes / entangle_launch) against the older
  summary mirror, against the workspace size the built library reports for every row, and the census of the case table
  (_entangle_cases.py): every claim of every row true, every path covered in every instantiation it applies to;
- the tile addressing of the mirror: the tiles of a pass partition the state, and the shares of all tiles of all passes
  (_grid_refs.rdm1_tile_share, the negative control of the GPU rows) add up to the whole reduction;
- the references (_grid_refs.rdm1_exact, rdm1_cross, wire_sum) against explicit_rdm1_cross / explicit_wire_sum and the
  CPU test backend's gate_grad at n <= 10;
- the conditions on the exact inputs at every row's own shape, and that each kind of negative control is rejected by
  the exact and by the rounding criterion."""

import pytest
import torch

import _entangle_cases as T
import _grid_refs as R
import _launch_geometry as G
from _cpu_backend import CpuTestBackend
from _entangle_cases import CASES, PATHS, TAU_RDM1_C64, TAU_SUM
from deepquantum_amd import _lib, backend
from oracle import statevec_oracle as oracle
from test_entanglement_gpu import explicit_rdm1_cross, explicit_wire_sum
from test_grid_paths_gpu import TAU_AMP
from test_grid_paths_gpu import TAU_SUM as GRID_TAU_SUM

C64, C128 = torch.complex64, torch.complex128


# ---- the mirror ------------------------------------------------------------------------------------------------------------
def test_full_mirror_against_the_summary_and_the_library():
    lib = _lib.load()
    for n in range(1, 41):
        for c128 in (False, True):
            for cross in (False, True):
                plan = G.entangle_passes(n, c128, cross)
                ps = plan['passes']
                assert [p['ntiles'] for p in ps] == [p['ntiles'] for p in G.ent_plan(n, c128, cross)]
                assert plan['M'] == (11 if c128 and cross else 12) and plan['gmax'] == plan['M'] - (3 if c128 else 4)
                # every wire bit is settled exactly once; the gathered bits of a pass are consecutive from lo
                settled = sorted(wp for p in ps for wp, _, _ in p['settles'])
                assert settled == list(range(n)), (n, c128, cross)
                for p in ps:
                    assert p['gathered'] == p['m'] - p['s'] and p['jlo'] == (0 if p['first'] else p['s'])
                    assert all((via == 'reg') == (j >= 8) for _, j, via in p['settles'])
                    assert p['first'] or p['s'] >= (3 if c128 else 4)
                assert plan['diag'] == ['tile'] * plan['m0'] + ['tile_sums'] * (n - plan['m0'])
                assert plan['pad'] == ('sub_workgroup' if n < 8 else 'sub_tile' if n < plan['M'] else None)
                for batch in (1, 2, 3, 700, 2048, 65535):
                    if n > 30 and batch > 3:
                        continue
                    g = G.entangle_launch(n, batch, c128, cross)
                    e = G.entangle(n, batch, c128, cross)
                    assert [p['nwg'] for p in g['passes']] == e['nwg'] and [p['iterations'] for p in g['passes']] == e['iterations']
                    ws = 8 * (sum(batch * p['nwg'] * G.ENT_ROW for p in g['passes']) + (batch * ps[0]['ntiles'] * 2 if n > plan['m0'] else 0))
                    assert ws == G.rdm1_ws_bytes(n, batch, c128, cross) == lib.dq_rdm1_ws_bytes(n, batch, int(c128), int(cross))
                    for p in g['passes']:
                        if p['tiles_per_wg'] is not None:
                            assert sum(p['tiles_per_wg']) == p['ntiles'] and max(p['tiles_per_wg']) == p['iterations']
                            assert p['ragged'] == (len(set(p['tiles_per_wg'])) > 1)
                        assert p['last_tile_wg0'] % p['nwg'] == 0 and p['ntiles'] - p['nwg'] <= p['last_tile_wg0'] < p['ntiles']


def test_tiles_partition_the_state():
    for n, c128, cross in ((14, False, False), (13, True, True), (17, True, False), (21, False, True)):
        for p in G.entangle_passes(n, c128, cross)['passes']:
            seen = torch.zeros(1 << n, dtype=torch.int32)
            for o in range(p['ntiles']):
                idx = R.ent_tile_indices(p, G.ent_tile_base(p, o), 'cpu')
                seen[idx] += 1
                for l in (0, 1, (1 << p['m']) - 1, 0x2A5 & ((1 << p['m']) - 1)):          # noqa: E741
                    assert int(idx[l]) == G.ent_tile_index(p, G.ent_tile_base(p, o), l)
                    # local bit j is the wire bit the pass says it settles
                    for wp, j, _ in p['settles']:
                        assert ((int(idx[l]) >> wp) & 1) == ((l >> j) & 1)
            assert bool((seen == 1).all()), (n, c128, cross, p['lo'])


def test_case_table_reaches_what_it_claims():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    assert T.MAX_BATCH == backend.MAX_BATCH
    # the figures of the rounding criterion are the ones test_grid_paths_gpu.py uses for its third-pass case
    assert TAU_SUM == GRID_TAU_SUM == 1e-12 and TAU_RDM1_C64 == 2 * (8 + 2) * 2.0**-24
    lib = _lib.load()
    for c in CASES:
        g = T.launch(c)
        assert PATHS[c.path](c, g), c.name
        for key, want in c.claims.items():
            assert [p[key] for p in g['passes']] == want, (c.name, key, [p[key] for p in g['passes']], want)
        for lo, hi in T.slices(c.batch):                                 # the workspace of every launch, from the full mirror
            ps = G.entangle_launch(c.n, hi - lo, c.c128, c.cross)['passes']
            rows = sum((hi - lo) * p['nwg'] * G.ENT_ROW for p in ps)
            sums = (hi - lo) * ps[0]['ntiles'] * 2 if ps[0]['ntiles'] > 1 else 0
            assert lib.dq_rdm1_ws_bytes(c.n, hi - lo, int(c.c128), int(c.cross)) == 8 * (rows + sums) > 0, c.name
            assert 8 * (rows + sums) == G.rdm1_ws_bytes(c.n, hi - lo, c.c128, c.cross)
    for path, insts in T.APPLIES.items():
        for inst in insts:
            assert [c for c in CASES if c.path == path and c.inst == inst], (path, inst)
    assert set(T.APPLIES) == set(PATHS) == {c.path for c in CASES}
    have = {(c.path, c.inst): [] for c in CASES}
    for c in CASES:
        have[(c.path, c.inst)].append((c.n, c.batch))
    for key, shape in T.LISTED.items():
        assert shape in have[key], (key, shape, have[key])
    # a row reaches its own path only (the batch-slices rows, n = 2, are also smaller than a workgroup)
    for c in CASES:
        reached = [p for p, pred in PATHS.items() if pred(c, T.launch(c))]
        assert reached == ([c.path] if c.path != 'batch-slices' else ['pad-sub-workgroup', 'batch-slices']), c.name
    # the largest rows stay as listed
    assert max(c.n for c in CASES) == 22 and max(c.batch << c.n for c in CASES if c.c128) == 700 << 14


# ---- the references ----------------------------------------------------------------------------------------------------------
def _gauss(b, n, seed, dtype=C128):
    g = torch.Generator().manual_seed(seed)
    x = torch.view_as_complex(torch.randn(b, 1 << n, 2, generator=g, dtype=torch.float64))
    return (x / x.norm(dim=-1, keepdim=True)).to(dtype)


@pytest.mark.parametrize('n', [1, 2, 5, 9, 10])
def test_references_against_explicit_torch_and_the_cpu_backend(n):
    be = CpuTestBackend()
    samples = torch.arange(3)
    for x, y in ((_gauss(3, n, n), _gauss(3, n, n + 40)), (R.int_state(n, samples, 5, 1), R.int_state(n, samples, 5, 0))):
        for bra in (x, y):
            t = R.rdm1_exact(bra, y)
            tr, s = R.rdm1_cross(bra, y)
            want = explicit_rdm1_cross(bra, y)
            assert float((t - want).abs().max()) < 1e-12 * max(1.0, float(want.abs().max()))
            assert float((tr - t).abs().max()) < 1e-12 * max(1.0, float(want.abs().max())) and bool((t.abs() <= s + 1e-12).all())
            for k in range(n):                                           # (wire k = index bit n - 1 - k)
                assert float((t[:, k] - be.gate_grad(y, bra, [n - 1 - k], []).conj()).abs().max()) < 1e-12 * max(1.0, float(want.abs().max()))
        for mats in (torch.view_as_complex(torch.randn(3, n, 2, 2, 2, generator=torch.Generator().manual_seed(n), dtype=torch.float64)),
                     R.int_mats(n, 3, 9, 'cpu')):
            w = R.wire_sum(y, mats)
            scale = max(1.0, float(w.abs().max()))
            assert float((w - explicit_wire_sum(y, mats)).abs().max()) < 1e-12 * scale
            by_gates = sum(oracle.apply_gate_bits(y, mats[:, k], [n - 1 - k]) for k in range(n))
            assert float((w - by_gates).abs().max()) < 1e-12 * scale
            # the off-diagonal term of one wire: the sum with that wire's off-diagonal entries at zero lacks exactly it
            p = n - 1
            m0 = mats.clone()
            m0[:, n - 1 - p, 0, 1] = 0
            m0[:, n - 1 - p, 1, 0] = 0
            assert float((w[2] - R.wire_sum(y, m0)[2] - R.wire_offdiag(y[2], mats[2], p)).abs().max()) < 1e-12 * scale
    # integer inputs: integer-valued, equal to the einsum bit for bit
    x, y = R.int_state(n, samples, 5, 1), R.int_state(n, samples, 5, 0)
    t = R.rdm1_exact(x, y)
    assert torch.equal(t, explicit_rdm1_cross(x, y)) and torch.equal(torch.view_as_real(t), torch.view_as_real(t).round())
    mats = R.int_mats(n, 3, 9, 'cpu')
    w = R.wire_sum(y, mats)
    assert torch.equal(w, explicit_wire_sum(y, mats)) and float(torch.view_as_real(w).abs().max()) <= 16 * n
    assert torch.equal(w.to(C64).to(C128), w)                          # (the exact conversion of the complex64 rows)


def test_generator_depends_on_nothing_but_its_arguments():
    a = R.int_state(6, torch.arange(5), 3, 0)
    assert torch.equal(R.int_state(6, torch.tensor([4, 1]), 3, 0), a[[4, 1]])
    assert not torch.equal(R.int_state(6, torch.arange(5), 3, 1), a) and not torch.equal(R.int_state(6, torch.arange(5), 3, 0, 1), a)
    parts = torch.view_as_real(R.int_state(12, torch.arange(4), 11, 0))
    assert parts.min() == -2 and parts.max() == 2 and torch.equal(parts, parts.round())
    counts = torch.bincount((parts + 2).long().flatten(), minlength=5).double() / parts.numel()
    assert float((counts - 0.2).abs().max()) < 0.01
    m = R.int_mats(7, 50, 2, 'cpu')
    parts = torch.view_as_real(m)
    assert parts.min() >= -2 and parts.max() <= 2 and torch.equal(parts, parts.round())
    assert bool((m[:, :, 0, 1] != 0).all() and (m[:, :, 1, 0] != 0).all() and (m[:, :, 0, 1] != m[:, :, 1, 0]).all()
                and (m[:, :, 0, 0] != m[:, :, 1, 1]).all())


SHAPES = sorted({(c.n, c.batch, c.cross, c.seed) for c in CASES if c.kernel == 'rdm1'}, key=lambda s: (s[1] << s[0], s))


@pytest.mark.parametrize('n,batch,cross,seed', SHAPES, ids=lambda v: str(int(v)))
def test_exact_inputs_meet_their_conditions(n, batch, cross, seed):
    """At the row's own shape: per sample the T_k differ pairwise, T00 != T11, T01 != 0, and T01 != conj(T10) for a cross
    row.  The reference is recomputed here from the states alone."""
    bra, ket = R.exact_states(n, batch, seed, cross, 'cpu')
    assert (bra is ket) == (not cross) and ket.shape == (batch, 1 << n)
    parts = torch.view_as_real(ket)
    assert parts.min() >= -2 and parts.max() <= 2 and torch.equal(parts, parts.round())
    t = R.rdm1_exact(bra, ket)
    assert torch.equal(torch.view_as_real(t), torch.view_as_real(t).round()) and float(t.abs().max()) <= 8 * 2.0**n * 2**0.5
    assert bool(R.rdm1_inputs_ok(t, cross).all())
    # spelled out for the last sample
    tl = t[-1]
    for k in range(n):
        assert tl[k, 0, 0] != tl[k, 1, 1] and tl[k, 0, 1] != 0 and (not cross or tl[k, 0, 1] != tl[k, 1, 0].conj())
        assert all(not torch.equal(tl[k], tl[j]) for j in range(k))
    # the conditions are not vacuous: they reject a state with two equal wires / a real symmetric one
    sym = torch.ones(1, 1 << max(n, 2), dtype=C128)
    assert not bool(R.rdm1_inputs_ok(R.rdm1_exact(sym, sym), cross).any())


# ---- the negative controls ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,c128,cross', [(14, False, False), (14, False, True), (13, True, True), (14, True, False)])
def test_tile_shares_add_up_and_are_rejected(n, c128, cross):
    """The share of every tile of every pass, added up, is the whole reduction (exactly, on integer amplitudes); one tile's
    share missing fails torch.equal and, on a Gaussian state, the rounding criterion of the row's precision."""
    plan = G.entangle_launch(n, 700, c128, cross)
    bra, ket = R.exact_states(n, 1, 77, cross, 'cpu')
    whole = torch.zeros(n, 2, 2, dtype=C128)
    for i, p in enumerate(plan['passes']):
        for o in range(p['ntiles']):
            whole += R.rdm1_tile_share(bra[0], ket[0], plan, i, G.ent_tile_base(p, o), o)
    assert torch.equal(whole, R.rdm1_exact(bra, ket)[0])
    ket = _gauss(1, n, 3)
    bra = _gauss(1, n, 4) if cross else ket
    ref, s = R.rdm1_cross(bra, ket)
    tau = TAU_SUM if c128 else TAU_RDM1_C64
    case = next(c for c in CASES if c.path == 'tile-loop-ragged' and c.c128 == c128 and c.cross == cross and c.kernel == 'rdm1')
    for i, o, base in T.passes_of_control(case, plan):
        assert o == plan['passes'][i]['last_tile_wg0'] > 0
        delta = R.rdm1_tile_share(bra[0], ket[0], plan, i, base, o)
        assert bool((delta.abs() > tau * s[0]).any()), (i, o)
        ib, ik = R.exact_states(n, 1, 77, cross, 'cpu')
        assert bool(R.rdm1_tile_share(ib[0], ik[0], plan, i, base, o).abs().max() > 0)


@pytest.mark.parametrize('n', [5, 13])
def test_wire_sum_control_is_rejected(n):
    psi = _gauss(2, n, 8)
    mats = torch.view_as_complex(torch.randn(2, n, 2, 2, 2, generator=torch.Generator().manual_seed(n), dtype=torch.float64))
    ref = R.wire_sum(psi, mats)
    delta = R.wire_offdiag(psi[1], mats[1], n - 1)
    for dtype in (C64, C128):
        assert float(delta.abs().max()) > TAU_AMP[dtype] * float(ref[1].abs().max())
    ipsi, imats = R.int_state(n, torch.arange(2), 4), R.int_mats(n, 2, 4, 'cpu')
    assert float(R.wire_offdiag(ipsi[1], imats[1], n - 1).abs().max()) > 0
