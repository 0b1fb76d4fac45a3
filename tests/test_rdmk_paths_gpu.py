"""The k-wire cross reduction (``dq_rdmk_cross_*``, dq_rdm.hip) path by path against plain complex128 references
(_grid_refs.cross) on the MI355X: the rows of _rdmk_cases.py, each asserted from the plan's mirror to reach its path.

Exact criterion (every row).  Amplitudes whose real and imaginary parts are integers in -2 .. 2, not normalised.  Every
partial sum in the kernel is then an integer: at most 4096 * 2 * 8 inside an f32 window (exact in f32), at most 2^R * 8 in
double (exact in f64).  The result does not depend on the order of the summation, on the flush, on the splits or on the
wave reduction, and neither does the reference (asserted integer-valued): ``torch.equal`` on real and imaginary parts.  A
dropped, doubled or misaddressed term at n = 26 fails it.

Rounding criterion (complex64 rows; complex128 rows with K <= 2^16).  Random normalised states:
|got - ref| <= tau * S elementwise, tau = TAU_SUM (complex128) or TAU_C64 (derived in _rdmk_cases.py from the documented
accumulation).  Each complex64 row runs that emulation (_grid_refs.f32_chain) on four elements of its own first sample
and holds it to TAU_C64 / 8; the row with the largest K also runs the chain without the flush and asserts that TAU_C64
rejects it.

Negative controls, on reference tensors only: the reference less one chunk of one split (the kernel's own order: chunk
bits are the lowest rest bits, the split is the top of the chunk number), two tile blocks exchanged, one off-diagonal
block conjugated.  The exact criterion sees each of them in every row that has the tiles.  The rounding criterion sees the
dropped chunk where its expected share of an element -- KC / K on the diagonal of a Hermitian row, sqrt(KC) / K where x
and gy are independent and the terms cancel -- is more than 2 * tau; the other rows print that it is not asserted (n = 26
without a control: Hermitian rows at 7.6e-6 and 1.5e-5, every cross row) and the exact criterion carries them.  Worst ratios are printed (``-s``)."""

from __future__ import annotations

import math

import pytest
import torch

import _grid_refs as R
import _launch_geometry as G
import _rdmk_cases as T
from _rdmk_cases import CASES, FLUSH_WINDOW, LARGEST_K, TAU_C64, TAU_SUM
from deepquantum_amd import backend

pytestmark = pytest.mark.gpu

DEV = 'cuda'
C64, C128 = torch.complex64, torch.complex128
ROUNDING = [c for c in CASES if c.rounding]


def _reach(case) -> dict:
    geo = G.rdmk(case.n, case.k, case.nc, case.batch, case.c128, case.herm)
    for key, want in case.claims.items():
        assert geo[key] == want, (case.name, key, geo[key], want)
    assert T.has_holes(case, geo['chunk_bits'])
    return geo


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _fill(out, kind, seed):
    """One sample at a time: no temporary larger than a sample."""
    real = torch.view_as_real(out)
    g = torch.Generator(device=DEV).manual_seed(seed)
    for b in range(out.shape[0]):
        if kind == 'ints':
            real[b] = torch.randint(-2, 3, real[b].shape, generator=g, device=DEV, dtype=torch.int8).to(real.dtype)
        else:
            real[b] = torch.randn(real[b].shape, generator=g, device=DEV, dtype=real.dtype)
            real[b] /= real[b].double().pow(2).sum().sqrt().to(real.dtype)
    return out


_BIG: dict = {}


def _big_inputs(kind):
    """The two (16, 2^26) complex64 inputs of the n = 26 rows, made once per kind and shared; one kind lives at a time."""
    if kind not in _BIG:
        _BIG.clear()
        torch.cuda.empty_cache()
        _BIG[kind] = tuple(_fill(torch.empty(T.BIG_BATCH, 1 << T.BIG_N, dtype=C64, device=DEV), kind, seed) for seed in (1, 2))
    return _BIG[kind]


@pytest.fixture(scope='module', autouse=True)
def _release_big_inputs():
    yield
    _BIG.clear()
    torch.cuda.empty_cache()


def _inputs(case, kind):
    if case.big:
        x, gy = _big_inputs(kind)
        x = x[: case.batch]
        return x, (x if case.herm else gy[: case.batch])
    dtype = C128 if case.c128 else C64
    seed = 100 + 2 * CASES.index(case)
    x = _fill(torch.empty(case.batch, 1 << case.n, dtype=dtype, device=DEV), kind, seed)
    return x, (x if case.herm else _fill(torch.empty_like(x), kind, seed + 1))


# ---- negative controls -------------------------------------------------------------------------------------------------------
def _dropped_chunk(case, geo, x, gy):
    """(sample, what one chunk adds, its S): the last sample and split; the chunk right behind the first flush where the
    loop has one, the last chunk otherwise."""
    sample, split = case.batch - 1, geo['nsplit'] - 1
    chunk = G.RDM_FLUSH if geo['flush_then_more'] else geo['nch'] - 1
    first, count = R.chunk_columns(geo, split, chunk)
    return (sample,) + R.cross_columns(x, gy, case.targets, case.controls, sample, first, count)


def _tile_mutations(case, geo, ref_internal):
    """Two tile blocks exchanged and one off-diagonal block conjugated (rows with more than one tile per side)."""
    if geo['nt'] == 1:
        return []
    nt, dt = geo['nt'], geo['dt']
    return [('two tile blocks exchanged', R.swap_tiles(ref_internal, dt, (0, nt - 1), (1, nt - 1))),
            ('an off-diagonal block conjugated', R.conj_tile(ref_internal, dt, (0, nt - 1)))]


# ---- the exact criterion -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_exact(case):
    geo = _reach(case)
    x, gy = _inputs(case, 'ints')
    got = backend.rdmk_cross(x, gy, list(case.targets), list(case.controls))
    assert got.dtype == C128 and got.shape == (case.batch, 1 << case.k, 1 << case.k)
    ref, s = R.cross(x, gy, case.targets, case.controls)
    rr, gr = torch.view_as_real(ref), torch.view_as_real(got)
    assert torch.equal(rr, rr.round()) and float(s.max()) <= 8.0 * geo['terms'] < 2.0 ** 53       # the reference is exact
    wrong = int((gr != rr).sum())
    print(f'{case.name}: K = 2^{int(math.log2(geo["terms"]))}, {geo["nsplit"]} splits x {geo["nch"]} chunks, {geo["ntl"]} tiles, '
          f'max |ref| {float(ref.abs().max()):.0f}: {wrong} of {rr.numel()} parts differ')
    assert torch.equal(gr, rr), f'{case.name}: {wrong} real / imaginary parts differ, worst by {float((gr - rr).abs().max())}'
    sample, delta, _ = _dropped_chunk(case, geo, x, gy)
    assert not torch.equal(ref[sample] - delta, ref[sample]), f'{case.name}: the dropped chunk adds nothing'
    ri = R.to_internal(ref, case.targets)
    for what, bad in _tile_mutations(case, geo, ri):
        assert not torch.equal(bad, ri), f'{case.name}: {what} goes unseen'


# ---- the rounding criterion ----------------------------------------------------------------------------------------------------
def _emulation(case, x, gy, window):
    """f32_chain on two diagonal and two off-diagonal elements of the first sample: worst |emulated - ref| / S."""
    d = 1 << case.k
    a, r = R.cross_index(case.n, case.targets, case.controls, DEV)
    rows, cols = [0, d - 1, 0, 3], [0, d - 1, 1, 5]
    ye, xe = gy[0][a[rows][:, None] | r[None, :]], x[0][a[cols][:, None] | r[None, :]]
    ref = (ye.to(C128) * xe.to(C128).conj()).sum(-1)
    s = (ye.abs().double() * xe.abs().double()).sum(-1)
    return float(((R.f32_chain(ye, xe, window) - ref).abs() / s).max())


@pytest.mark.parametrize('case', ROUNDING, ids=lambda c: c.name)
def test_rounding(case):
    geo = _reach(case)
    tau = TAU_SUM if case.c128 else TAU_C64
    assert not case.c128 or geo['terms'] <= 1 << 16
    x, gy = _inputs(case, 'rand')
    got = backend.rdmk_cross(x, gy, list(case.targets), list(case.controls))
    ref, s = R.cross(x, gy, case.targets, case.controls)
    err = (got - ref).abs()
    line = f'{case.name}: K = 2^{int(math.log2(geo["terms"]))}: kernel worst |got - ref| / S = {float((err / s).max()):.3e} (tau {tau:.0e})'
    if not case.c128:
        emulated = _emulation(case, x, gy, FLUSH_WINDOW)
        line += f'; f32 chain in windows of {FLUSH_WINDOW}: {emulated:.3e}'
        assert emulated <= TAU_C64 / 8, f'{case.name}: the emulation TAU_C64 is derived from is at {emulated:.3e} of S'
        if case is LARGEST_K:
            unflushed = _emulation(case, x, gy, None)
            line += f', never flushed: {unflushed:.3e}'
            assert unflushed > TAU_C64, f'{case.name}: an f32 chain over all K passes the criterion ({unflushed:.3e})'
    assert (err <= tau * s).all(), line
    # the dropped chunk
    sample, delta, _ = _dropped_chunk(case, geo, x, gy)
    seen = float((delta.abs() / s[sample]).max())
    share = (geo['kc'] if case.herm else math.sqrt(geo['kc'])) / geo['terms']
    if share > 2 * tau:
        assert (delta.abs() > tau * s[sample]).any(), f'{case.name}: the criterion does not see a dropped chunk ({seen:.3e} of S)'
        line += f'; a dropped chunk ({seen:.3e} of S) is rejected'
    else:
        line += f'; a dropped chunk is {seen:.3e} of S (expected share {share:.1e} <= 2 tau): left to the exact criterion'
    ri, si = R.to_internal(ref, case.targets), R.to_internal(s, case.targets)
    for what, bad in _tile_mutations(case, geo, ri):
        assert ((bad - ri).abs() > tau * si).any(), f'{case.name}: {what} goes unseen'
    print(line)

