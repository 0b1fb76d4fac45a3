"""What test_rdmk_paths_gpu.py stands on, checked without a GPU:

- the mirror of the k-wire cross reduction's plan (_launch_geometry.rdmk) against the workspace size the built library
  reports (``dq_rdmk_ws_bytes`` is a function of the tile slots and the contraction splits), the thresholds at which the
  complex64 flush is first followed by more chunks, and the claims of every row of the case table (_rdmk_cases.py);
- which of these paths the random-state cases of test_rdm_gpu.test_kernel_against_explicit_einsum reach (pinned: the table
  documents what that test covers and what it leaves to the new file);
- the references and their mutations (_grid_refs.cross, cross_columns, swap_tiles, conj_tile, f32_chain) against the CPU
  test backend at small n, and each mutation against the criterion it has to fail."""

import pytest
import torch

import _grid_refs as R
import _launch_geometry as G
import _rdmk_cases as T
from _cpu_backend import CpuTestBackend
from _rdmk_cases import TAU_C64, TAU_SUM
from deepquantum_amd import _lib
from test_rdm_gpu import _cases as einsum_cases


# ---- the mirror ----------------------------------------------------------------------------------------------------------
def test_plan_against_the_library():
    lib = _lib.load()
    for n in range(3, 35):
        for k in range(3, 11):
            for nc in (0, 1, 2):
                if n < k + nc:
                    continue
                for batch in (1, 2, 3, 16, 2048, 3000):
                    for c128 in (False, True):
                        for herm in (False, True):
                            g = G.rdmk(n, k, nc, batch, c128, herm)
                            assert lib.dq_rdmk_ws_bytes(n, k, nc, batch, int(c128), int(herm)) == g['ws_bytes'], \
                                (n, k, nc, batch, c128, herm)
                            assert g['nsplit'] * g['nch'] == g['chunks'] and g['ws_bytes'] == 16 * batch * g['nsplit'] * g['ntl'] * g['dt'] ** 2
                            assert g['chunks'] * g['kc'] == max(g['terms'], g['kc']) and g['pad_chunk'] == (g['terms'] < g['kc'])


def test_plan_geometry():
    # tiles: 16 x 16 up to k = 4 (rows padded at k = 3), 32 x 32 at k = 5, 64 x 64 from k = 6
    assert [G.rdmk(20, k, 0, 1, False, False)['tile'] for k in range(3, 11)] == [16, 16, 32, 64, 64, 64, 64, 64]
    assert [G.rdmk(20, k, 0, 1, False, False)['kc'] for k in (3, 5, 6)] == [64, 32, 16]
    assert G.rdmk(20, 3, 0, 1, False, False)['pad_rows'] and G.rdmk(20, 3, 0, 1, False, False)['dt'] == 8
    assert not any(G.rdmk(20, k, 0, 1, False, False)['pad_rows'] for k in range(4, 11))
    # tile slots: every tile, or the upper triangle
    assert [G.rdmk(20, k, 0, 1, False, False)['ntl'] for k in (6, 7, 8, 10)] == [1, 4, 16, 256]
    assert [G.rdmk(20, k, 0, 1, False, True)['ntl'] for k in (6, 7, 8, 10)] == [1, 3, 10, 136]
    # chunk bits padded when fewer rest bits than the chunk has
    assert G.rdmk(8, 3, 0, 1, False, False)['pad_chunk'] and not G.rdmk(9, 3, 0, 1, False, False)['pad_chunk']
    assert G.rdmk(9, 6, 0, 1, False, False)['pad_chunk'] and not G.rdmk(10, 6, 0, 1, False, False)['pad_chunk']


def test_flush_thresholds():
    """complex64: a flush inside the loop is followed by further chunks only when a split has more than 256 chunks.  For
    k <= 5 the splits double until 2048 workgroups, so that needs batch * 2^n >= 2^30 (2^29 at k = 3); k = 6 at batch 1
    gets there at n = 19.  complex128 never flushes."""
    for k, floor in ((3, 29), (4, 30), (5, 30)):
        first = None
        for n in range(k, 35):
            for nc in (0, 1, 2):
                if n < k + nc:
                    continue
                for batch in (1, 2, 3, 8, 16, 2048, 3000):
                    for herm in (False, True):
                        g = G.rdmk(n, k, nc, batch, False, herm)
                        assert not G.rdmk(n, k, nc, batch, True, herm)['flush_then_more']
                        if g['flush_then_more']:
                            assert batch << n >= 1 << floor, (n, k, nc, batch, herm, g)
                            first = min(first or (batch << n), batch << n)
        assert first == 1 << floor, (k, first)
    for herm in (False, True):
        assert not G.rdmk(18, 6, 0, 1, False, herm)['flush_then_more']
        g = G.rdmk(19, 6, 0, 1, False, herm)
        assert g['flush_then_more'] and (g['nsplit'], g['nch'], g['flushes']) == (1, 512, 2)
    # the shape class of the published table: n = 28, batch 16: 4096 / 2048 / 2048 chunks per split
    for k, nch in ((3, 4096), (4, 2048), (5, 2048)):
        g = G.rdmk(28, k, 0, 16, False, True)
        assert g['nch'] == nch and g['flushes'] == nch // 256 and g['flush_then_more'] and g['workgroups'] == 2048


def _plan(case):
    return G.rdmk(case.n, case.k, case.nc, case.batch, case.c128, case.herm)


def test_case_table_reaches_what_it_claims():
    names = [c.name for c in T.CASES]
    assert len(set(names)) == len(names)
    for c in T.CASES:
        g = _plan(c)
        for key, want in c.claims.items():
            assert g[key] == want, (c.name, key, g[key], want)
        assert len(set(c.targets) | set(c.controls)) == c.k + c.nc and max(c.targets + c.controls) < c.n
        assert list(c.targets) != sorted(c.targets) and list(c.targets) != sorted(c.targets, reverse=True), c.name
        assert 0 in c.targets + c.controls or c.n - 1 in c.targets + c.controls, c.name
        assert T.has_holes(c, g['chunk_bits']), c.name
        assert g['nsplit'] > 1 and not g['pad_chunk'], c.name
        if c.big:
            assert c.n == T.BIG_N and c.batch <= T.BIG_BATCH and not c.c128
        if c.c128 and c.rounding:
            assert g['terms'] <= 1 << 16, c.name
    by = lambda f: [c for c in T.CASES if f(c, _plan(c))]      # noqa: E731
    # index bit 0 as a target, as a control and as a chunk bit; the top bit as a target and as a control
    assert by(lambda c, g: 0 in c.targets) and by(lambda c, g: 0 in c.controls) and by(lambda c, g: 0 not in c.targets + c.controls)
    assert by(lambda c, g: c.n - 1 in c.targets) and by(lambda c, g: c.n - 1 in c.controls)
    # every tile size: a flush followed by more chunks on both routes (16 and 32: the four-wave reduction)
    for tile in (16, 32, 64):
        for herm in (False, True):
            assert by(lambda c, g: g['tile'] == tile and g['flush_then_more'] and c.herm == herm), (tile, herm)
    assert by(lambda c, g: g['pad_rows'] and g['flush_then_more'])
    # a control on index bit 0 and one on the top bit, on each small tile
    for tile in (16, 32):
        assert by(lambda c, g: g['tile'] == tile and c.controls == (0,))
        assert by(lambda c, g: g['tile'] == tile and c.controls == (c.n - 1,))
    # splits x tiles x batch at once, on both routes and in both precisions
    for herm in (False, True):
        for c128 in (False, True):
            assert by(lambda c, g: g['nsplit'] > 1 and g['ntl'] > 1 and c.batch > 1 and c.herm == herm and c.c128 == c128), (herm, c128)
    # the unflushed-chain condition sits on K = 2^23, on the padded 16 x 16 tile
    assert T.LARGEST_K.name == 't16-k3-herm' and _plan(T.LARGEST_K)['terms'] == 1 << 23
    # complex128 at large K stands on the exact criterion alone
    assert by(lambda c, g: c.c128 and not c.rounding and g['terms'] >= 1 << 22)


def test_what_the_einsum_cases_reach():
    """test_rdm_gpu.test_kernel_against_explicit_einsum (its seed is fixed): never a flush followed by more chunks on the
    16 x 16 or 32 x 32 tile, never contraction splits and several tiles at once."""
    plans = [(G.rdmk(n, len(tg), len(ctl), b, False, same), len(tg)) for n, tg, ctl, b, same in einsum_cases()]
    assert not any(g['flush_then_more'] for g, k in plans if k <= 5)
    assert max(g['nch'] for g, k in plans if k <= 4) <= 32
    assert max(g['nch'] for g, k in plans if k == 5) <= 256
    # the flush followed by more chunks: two cases, both k = 7 at n = 20 without a control, one split of 512 chunks
    assert [(k, g['nsplit'], g['nch']) for g, k in plans if g['flush_then_more']] == [(7, 1, 512)] * 2
    assert not any(g['nsplit'] > 1 and g['ntl'] > 1 for g, k in plans)
    assert any(g['nsplit'] > 1 for g, k in plans) and any(g['ntl'] > 1 for g, k in plans)
    assert any(g['pad_chunk'] for g, k in plans) and any(g['pad_rows'] for g, k in plans)


# ---- the references and their mutations ---------------------------------------------------------------------------------------
def _state(b, n, seed, dtype=torch.complex128):
    g = torch.Generator().manual_seed(seed)
    x = torch.view_as_complex(torch.randn(b, 1 << n, 2, generator=g, dtype=torch.float64))
    return (x / x.norm(dim=-1, keepdim=True)).to(dtype)


def _ints(b, n, seed, dtype=torch.complex128):
    g = torch.Generator().manual_seed(seed)
    return torch.view_as_complex(torch.randint(-2, 3, (b, 1 << n, 2), generator=g).to(torch.float64)).to(dtype)


SMALL = [  # (n, targets, controls): every tile size, padded rows and chunks, controls on bit 0 and the top bit
    (9, [8, 0, 4], []), (11, [3, 10, 0, 7], [5]), (12, [11, 2, 0, 6, 9], [1]), (12, [0, 5, 11, 3, 8, 1], []),
    (13, [12, 1, 6, 0, 9, 4, 10], [7]), (12, [4, 11, 0, 2, 9, 6, 1, 7], [5, 10]), (10, [1, 9, 3], [0, 8]),
]


@pytest.mark.parametrize('n,targets,controls', SMALL)
def test_references_against_the_cpu_backend(n, targets, controls):
    be = CpuTestBackend()
    x, y = _state(2, n, n), _state(2, n, n + 50)
    for a, b in ((x, y), (x, x)):
        ref, s = R.cross(a, b, targets, controls)
        want = be.gate_grad(a, b, targets, controls)
        assert float((ref - want).abs().max()) < 1e-13
        sa, _ = R.cross(a.abs().to(torch.complex128), b.abs().to(torch.complex128), targets, controls)
        assert float((s - sa.real).abs().max()) < 1e-13 and (ref.abs() <= s + 1e-15).all()
    # a dropped chunk: the reference less the columns of one chunk is the reduction of a state whose amplitudes at those
    # columns are zero; the plan of a shape with several splits gives the columns
    k, nc = len(targets), len(controls)
    geo = G.rdmk(n, k, nc, 2, False, False)
    geo = dict(geo, nsplit=2, nch=geo['chunks'] // 2) if geo['chunks'] > 1 else geo
    split, chunk = geo['nsplit'] - 1, geo['nch'] // 2
    first, count = R.chunk_columns(geo, split, chunk)
    ref, _ = R.cross(x, y, targets, controls)
    delta, sd = R.cross_columns(x, y, targets, controls, 1, first, count)
    a_idx, r_idx = R.cross_index(n, targets, controls, 'cpu')
    gone = (a_idx[:, None] | r_idx[None, first : first + count]).reshape(-1)
    rest = [p for p in range(n) if p not in targets and p not in controls]
    # (the kernel's order: chunk bits are the lowest rest bits, the split is the top of the chunk number)
    cb = geo['chunk_bits']
    number = split * geo['nch'] + chunk
    for i in gone.tolist()[:: max(1, len(gone) // 64)]:
        assert sum(((i >> p) & 1) << q for q, p in enumerate(rest[cb:])) == number
    y0 = y.clone()
    y0[1, gone] = 0
    assert float((R.cross(x, y0, targets, controls)[0][1] - (ref[1] - delta)).abs().max()) < 1e-13
    assert float((ref[0] - R.cross(x, y0, targets, controls)[0][0]).abs().max()) == 0.0
    assert (delta.abs() <= sd + 1e-15).all() and float(sd.min()) > 0
    # at these sizes one chunk is far more than 2 tau of S: both rounding criteria reject the reference without it
    s = R.cross(x, y, targets, controls)[1][1]
    assert (delta.abs() > TAU_C64 * s).any() and (delta.abs() > TAU_SUM * s).any()


@pytest.mark.parametrize('targets', [[4, 0, 7, 2, 9, 5, 1], [0, 3, 1], [9, 8, 7, 6, 5, 4, 3, 2]])
def test_internal_order_and_tile_mutations(targets):
    """The kernel's internal row bit q is the q-th lowest target: with sorted descending targets it is the caller's order.
    A swap of two tile blocks and the conjugation of an off-diagonal block are seen by torch.equal and by tau * S."""
    k = len(targets)
    assert R.internal_order(sorted(targets, reverse=True)) == list(range(1 << k))
    p = R.internal_order(targets)
    assert sorted(p) == list(range(1 << k))
    srt = sorted(targets)
    for i in (1, 5, (1 << k) - 2):
        bits = {srt[q] for q in range(k) if (i >> q) & 1}                       # the index bits internal row i sets
        assert p[i] == sum(1 << (k - 1 - j) for j, t in enumerate(targets) if t in bits)
    n = 10
    x, y = _state(1, n, 3), _state(1, n, 4)
    if k < 8:
        ref, s = R.cross(x, y, targets, [])
        ri, si = R.to_internal(ref, targets), R.to_internal(s, targets)
        # the same matrix from the sorted targets
        want, _ = R.cross(x, y, sorted(targets, reverse=True), [])
        assert torch.equal(ri, want)
        dt = min(1 << k, 4)
        for bad in (R.swap_tiles(ri, dt, (0, 1), (1, 0)), R.conj_tile(ri, dt, (0, 1))):
            assert not torch.equal(bad, ri)
            assert ((bad - ri).abs() > TAU_C64 * si).any() and ((bad - ri).abs() > TAU_SUM * si).any()
        assert torch.equal(R.swap_tiles(R.swap_tiles(ri, dt, (0, 1), (1, 1)), dt, (0, 1), (1, 1)), ri)


def test_exact_inputs_make_exact_references():
    """Integer amplitudes in -2 .. 2: the reference is integer-valued whatever the order of its sums, and one dropped chunk,
    two exchanged tile blocks or a conjugated off-diagonal block change it."""
    n, targets, controls = 13, [12, 3, 0, 8, 5], [10]
    x, y = _ints(2, n, 1), _ints(2, n, 2)
    geo = G.rdmk(n, 5, 1, 2, False, False)
    ref, s = R.cross(x, y, targets, controls)
    assert torch.equal(ref, ref.real.round() + 1j * ref.imag.round())
    assert torch.equal(ref, CpuTestBackend().gate_grad(x, y, targets, controls))
    delta, _ = R.cross_columns(x, y, targets, controls, 0, *R.chunk_columns(geo, geo['nsplit'] - 1, geo['nch'] - 1))
    assert not torch.equal(ref[0] - delta, ref[0])
    ri = R.to_internal(ref, targets)
    assert not torch.equal(R.swap_tiles(ri, 16, (0, 1), (1, 0)), ri) and not torch.equal(R.conj_tile(ri, 16, (0, 1)), ri)


def test_f32_chain_and_the_complex64_criterion():
    """The emulation of the documented accumulation (float32 chains of 4096 contraction indices, added in float64) stays
    inside TAU_C64 / 8 of S; the same chain never flushed is rejected by TAU_C64 at K = 2^21.  Small K: the chain equals a
    plain float64 sum to float32 rounding, and a window as long as K is the unflushed chain."""
    torch.manual_seed(5)
    y = torch.view_as_complex(torch.randn(3, 256, 2, dtype=torch.float32))
    x = torch.view_as_complex(torch.randn(3, 256, 2, dtype=torch.float32))
    want = (y.to(torch.complex128) * x.to(torch.complex128).conj()).sum(-1)
    s = (y.abs().double() * x.abs().double()).sum(-1)
    assert ((R.f32_chain(y, x, 64) - want).abs() <= 2e-6 * s).all()
    assert torch.equal(R.f32_chain(y, x, 256), R.f32_chain(y, x, None))
    # one wire set of the 16 x 16 tile at n = 24: K = 2^21; two diagonal and two off-diagonal elements
    n, targets = 24, [23, 0, 13]
    psi = _state(1, n, 8, torch.complex64)
    a, r = R.cross_index(n, targets, [], 'cpu')
    rows = psi[0][a[:, None] | r[None, :]]
    ye, xe = rows[[0, 7, 0, 3]], rows[[0, 7, 1, 5]]
    ref = (ye.to(torch.complex128) * xe.to(torch.complex128).conj()).sum(-1)
    s = (ye.abs().double() * xe.abs().double()).sum(-1)
    windowed = ((R.f32_chain(ye, xe, 4096) - ref).abs() / s).max().item()
    unflushed = ((R.f32_chain(ye, xe, None) - ref).abs() / s).max().item()
    print(f'f32 chain at K = 2^21: windows of 4096 {windowed:.3e} of S, never flushed {unflushed:.3e} of S')
    assert windowed <= TAU_C64 / 8
    assert unflushed > TAU_C64
