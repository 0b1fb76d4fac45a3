"""The Gram and combine kernels on the MI355X (dq_gram_*, dq_combine_*) through ``backend``, against numpy complex128
(tests/_gram_ref.py).

Sizes.  ``backend.gram_geometry`` gives the kernel's geometry -- a lane's segment of 8 / 4 columns (complex64 / complex128),
a wave's share of 32 / 16 columns per step, a workgroup's unit of 512 / 256 columns per iteration, at most 1024 workgroups
per tile pair -- and ``_gram_ref.boundary_size`` turns a named boundary into its n when a test runs (nothing is loaded
while pytest collects), so that a change of the geometry moves the cases along: the minimum n (1 / 0: one 16-byte
vector); a row shorter than a lane's segment (n = 2 / 1); one on each side of
a wave's share and the share itself (4, 5, 6 / 3, 4, 5); one on each side of a unit (8, 9, 10 / 7, 8, 9), the upper one
being the first n with more than one workgroup; and the first n at which a workgroup of a single tile pair takes a second
grid-stride iteration (20 / 19).  With two tile pairs the workgroups per pair halve, so 33 x 17 rows at the n below that
stride a second time as well.  The combine kernel's wave takes 16 vectors and its unit is 64 vectors (128 / 64 columns): n =
4..8 of the same list lie around both.

Row counts: 1, 2, 3, 15, 16, 17, 31, 32, 33 on either side (one block, its edge, two blocks, the tile's edge, the next tile)
and 40 x 70 (2 x 3 tiles).  Every boundary n meets the small counts, every count meets the n up to 12; no operand holds more
than 2^25 amplitudes.

Exact rows: Gaussian integers with parts in {-1, 0, 1}, so every partial sum is an integer below 2^22, and coefficients from
{+-1, +-2, +-1/2, +-i}: Gram and combine equal the reference as numbers -- a wrong lane map, swapped re / im, a transposed
result, a missing conjugate, a dropped or doubled column show here.

Gaussian rows, Gram: per entry |err| <= (2^-53 2^n + (C + 2) 2^-24) sum_x |a_x| |b_x| for complex64, C the chain length of the
geometry export; complex128: 2^-53 (2 2^n + 1024 + 2) sum_x |a_x| |b_x| (``_gram_ref.gram_bound``).  The bound is not vacuous:
the reference without its largest term lies outside it for every entry at every n of the list up to 16 for complex64 (a
single term of 2^n Gaussian ones outweighs 1.5e-5 of their sum up to there; at n = 20 it no longer does) and at every n for
complex128; checked on the host with the reference alone.  Combine: (2 N + 2) u sum_j |c_mj| |s_jx| per element, and 1e-4 /
1e-10 of max |ref|.

What the docstrings promise about bits: two runs agree bit for bit; an entry of a Gram of up to 32 x 32 rows is the 1 x 1 Gram
of its two rows bit for bit; beyond a tile the bits of an entry depend on its two rows, n and the number of tile pairs -- an
entry of a 33 x 17 Gram keeps its bits when the rows are shuffled."""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from deepquantum_amd import _lib, backend
import _gram_ref as ref
from _gram_ref import NP, ROWS, TOL, TORCH, U_T

pytestmark = pytest.mark.gpu

DEVICE = 'cuda'
DTS = ('c64', 'c128')


@functools.lru_cache(maxsize=None)
def geometry(dt):
    return backend.gram_geometry(TORCH[dt])


#: (dtype, boundary): the names of ``_gram_ref.BOUNDARIES``; ``size`` turns one into its n through the geometry export
#: when the test runs (nothing is loaded while pytest collects)
CASES = [(dt, name) for dt in DTS for name in ref.BOUNDARIES]


def size(dt, where):
    return ref.boundary_size(geometry(dt), dt, where)
SMALL_PAIRS = ((1, 1), (3, 2), (5, 7))
#: every row count on either side
ALL_PAIRS = ((1, 1), (2, 3), (3, 2), (15, 17), (16, 16), (17, 15), (31, 33), (32, 32), (33, 31), (1, 33), (32, 1), (16, 2), (40, 70))


def pairs_of(n):
    return ALL_PAIRS if n <= 12 else SMALL_PAIRS + ((33, 17),) if n < 20 else SMALL_PAIRS


def test_the_cases_cover_the_row_counts_and_the_geometry():
    assert all(any(m == r for m, _ in ALL_PAIRS) and any(k == r for _, k in ALL_PAIRS) for r in ROWS)
    for dt in DTS:
        g = geometry(dt)
        sizes = [size(dt, name) for name in ref.BOUNDARIES]
        assert sizes == ref.boundary_sizes(g, dt) and sizes[0] == ref.NMIN[dt] and len(sizes) == 9, sizes
        assert g.tile_rows == 32 and 0 < g.chain <= 512 if dt == 'c64' else g.chain == 0      # a few hundred real terms
        assert sizes[-1] + 5 <= 25                      # 32 rows at the largest n: 2^25 amplitudes


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEVICE)


def host(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def operands(kind, dt, n, rows_a, rows_b):
    """(a, b) on the host and on the device; shared by the tests of a case and never written."""
    rng = np.random.default_rng([n, rows_a, rows_b, kind == 'int'])
    make = ref.integer_rows if kind == 'int' else ref.gaussian_rows
    a, b = make(rng, rows_a, n, dt), make(rng, rows_b, n, dt)
    return a, b, dev(a), dev(b)


# ---- exact rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt,where', CASES)
def test_gram_exact(dt, where):
    n = size(dt, where)
    for rows_a, rows_b in pairs_of(n):
        a, b, da, db = operands('int', dt, n, rows_a, rows_b)
        got = backend.gram(da, db)
        assert got.dtype == torch.complex128 and got.shape == (rows_a, rows_b)
        np.testing.assert_array_equal(host(got), ref.gram_ref(a, b), err_msg=f'gram {dt} n={n} {rows_a} x {rows_b}')
        np.testing.assert_array_equal(host(backend.gram(da, da)), ref.gram_ref(a, a), err_msg=f'self-gram {dt} n={n} {rows_a}')


@pytest.mark.parametrize('dt,where', CASES)
def test_combine_exact(dt, where):
    n = size(dt, where)
    for rows_out, rows_in in pairs_of(n):
        s, _, ds, _ = operands('int', dt, n, rows_in, rows_out)
        coef = ref.exact_coefs(np.random.default_rng([n, rows_out, rows_in]), rows_out, rows_in)
        got = backend.combine(ds, dev(coef))
        assert got.dtype == TORCH[dt] and got.shape == (rows_out, 1 << n)
        np.testing.assert_array_equal(host(got), ref.combine_ref(coef, s).astype(NP[dt]),
                                      err_msg=f'combine {dt} n={n} {rows_out} <- {rows_in}')


@pytest.mark.parametrize('dt', DTS)
def test_combine_loops_over_chunks_of_input_rows(dt):
    """More input rows than the 64 whose coefficients LDS holds at a time: 65, 150 (three chunks, the last one partial)."""
    n = 7
    for rows_out, rows_in in ((3, 65), (45, 150)):
        rng = np.random.default_rng([rows_out, rows_in])
        s = ref.integer_rows(rng, rows_in, n, dt)
        coef = (rng.integers(-1, 2, (rows_out, rows_in)) + 1j * rng.integers(-1, 2, (rows_out, rows_in))).astype(np.complex128)
        np.testing.assert_array_equal(host(backend.combine(dev(s), dev(coef))), ref.combine_ref(coef, s).astype(NP[dt]))


# ---- Gaussian rows --------------------------------------------------------------------------------------------------------
def gram_bound(dt, n, a, b):
    g = geometry(dt)
    return ref.gram_bound(n, dt, g.chain, g.max_blocks, ref.gram_abs(a, b))


@pytest.mark.parametrize('dt,where', CASES)
def test_gram_gaussian_within_the_bound(dt, where):
    n = size(dt, where)
    for rows_a, rows_b in SMALL_PAIRS + ((33, 17),) if n <= 16 else SMALL_PAIRS:
        a, b, da, db = operands('gauss', dt, n, rows_a, rows_b)
        want, bound = ref.gram_ref(a, b), gram_bound(dt, n, a, b)
        err = np.abs(host(backend.gram(da, db)) - want)
        print(f'gram {dt} n={n} {rows_a} x {rows_b}: max err / bound = {(err / bound).max():.3e}')
        assert (err <= bound).all(), f'gram {dt} n={n} {rows_a} x {rows_b}: {(err / bound).max():.3e} of the bound'
        if rows_a <= 7 and (dt == 'c128' or n <= 16):     # (not vacuous: module docstring)
            assert (ref.gram_largest_term(a, b) > bound).all()
        # gram(b, a) is gram(a, b)^H, within the bound of both
        back = host(backend.gram(db, da))
        assert (np.abs(back - want.conj().T) <= bound.T).all()
        assert (np.abs(back.conj().T - host(backend.gram(da, db))) <= bound).all()


@pytest.mark.parametrize('dt,where', CASES)
def test_combine_gaussian_within_the_bound(dt, where):
    n = size(dt, where)
    for rows_out, rows_in in SMALL_PAIRS + ((17, 33), (33, 16)) if n <= 12 else SMALL_PAIRS:
        s, _, ds, _ = operands('gauss', dt, n, rows_in, rows_out)
        coef = ref.gaussian_coefs(np.random.default_rng([n, rows_out, rows_in, 7]), rows_out, rows_in)
        want = ref.combine_ref(coef, s)
        bound = (2 * rows_in + 2) * U_T[dt] * ref.combine_abs(coef, s)
        err = np.abs(host(backend.combine(ds, dev(coef))) - want)
        print(f'combine {dt} n={n} {rows_out} <- {rows_in}: max err / bound = {(err / np.maximum(bound, 1e-300)).max():.3e}')
        assert (err <= bound).all(), f'combine {dt} n={n} {rows_out} <- {rows_in}'
        assert err.max() <= TOL[dt] * np.abs(want).max()


# ---- the self-Gram --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt,where', CASES)
def test_self_gram_is_exactly_hermitian(dt, where):
    n = size(dt, where)
    for rows in (1, 3, 17, 33, 70) if n <= 12 else (3, 17):
        a, _, da, _ = operands('gauss', dt, n, rows, 1)
        got = backend.gram(da, da)
        assert torch.equal(got, got.mH.resolve_conj()), f'{dt} n={n} {rows}: G == G^H bit for bit'
        assert (got.imag.diagonal() == 0).all()
        other = backend.gram(da, da.clone())
        bound = gram_bound(dt, n, a, a)
        assert (np.abs(host(got) - host(other)) <= bound).all()
        assert (np.abs(host(got) - ref.gram_ref(a, a)) <= bound).all()
        # the real parts and the strict upper triangle are the same sums in the same order (the diagonal's imaginary
        # part is rounding noise there and exactly 0 here)
        iu = np.triu_indices(rows, 1)
        assert np.array_equal(host(got).real, host(other).real) and np.array_equal(host(got)[iu], host(other)[iu])


# ---- reproducibility ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt,where', CASES)
def test_bits_do_not_depend_on_the_run_or_the_other_rows(dt, where):
    n = size(dt, where)
    a, b, da, db = operands('gauss', dt, n, 5, 7)
    first = backend.gram(da, db)
    assert torch.equal(first, backend.gram(da, db))
    for i, j in ((0, 0), (4, 6), (2, 5)):
        alone = backend.gram(da[i:i + 1], db[j:j + 1])
        assert torch.equal(alone[0, 0], first[i, j]), f'{dt} n={n}: entry ({i}, {j}) of 5 x 7 against the 1 x 1 Gram'
    # one tile pair whatever the blocks: 17 x 32 rows hold the same entries
    if n <= 12:
        a2, b2, da2, db2 = operands('gauss', dt, n, 17, 32)
        wide = backend.gram(da2, db2)
        assert torch.equal(wide[:16, :16], backend.gram(da2[:16], db2[:16]))
        assert torch.equal(wide[16:, 30:], backend.gram(da2[16:], db2[30:]))
    if n <= 16:
        # beyond a tile: the same number of tile pairs, the rows shuffled
        a3, b3, da3, db3 = operands('gauss', dt, n, 33, 17)
        pa, pb = torch.randperm(33, generator=torch.Generator().manual_seed(n)), torch.randperm(17, generator=torch.Generator().manual_seed(n + 1))
        tiled = backend.gram(da3, db3)
        assert torch.equal(tiled, backend.gram(da3, db3))
        shuffled = backend.gram(da3[pa.to(DEVICE)].contiguous(), db3[pb.to(DEVICE)].contiguous())
        assert torch.equal(shuffled, tiled[pa.to(DEVICE)][:, pb.to(DEVICE)])
    c = dev(ref.gaussian_coefs(np.random.default_rng(n), 3, 5))
    assert torch.equal(backend.combine(da, c).view(torch.float64 if dt == 'c128' else torch.float32),
                       backend.combine(da, c).view(torch.float64 if dt == 'c128' else torch.float32))


# ---- non-interference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('rows_out', [3, 17, 33])
def test_combine_writes_only_out(dt, rows_out):
    for n in (ref.NMIN[dt], 2, 6, 9):
        s, _, ds, _ = operands('gauss', dt, n, 5, 1)
        coef = ref.gaussian_coefs(np.random.default_rng(rows_out), rows_out, 5)
        buf = torch.full((rows_out + 2, 1 << n), 7.0 - 3.0j, dtype=TORCH[dt], device=DEVICE)
        before = ds.clone()
        out = backend.combine(ds, dev(coef), out=buf[1:rows_out + 1])
        assert out.data_ptr() == buf[1].data_ptr()
        assert (buf[0] == 7.0 - 3.0j).all() and (buf[rows_out + 1] == 7.0 - 3.0j).all(), 'the guard rows stay untouched'
        assert torch.equal(ds, before)
        assert torch.equal(out, backend.combine(ds, dev(coef)))


# ---- host refusals of the raw entry points --------------------------------------------------------------------------------
def refused(rc, *words):
    msg = _lib.load().dq_last_error().decode()
    assert rc < 0 and all(w in msg for w in words), (rc, msg)


@pytest.mark.parametrize('dt', DTS)
def test_host_refusals(dt):
    """Each returns a negative code and a dq_last_error text; nothing is launched (the buffers keep their contents)."""
    lib = _lib.load()
    c128 = int(dt == 'c128')
    gram, combine = getattr(lib, f'dq_gram_{dt}'), getattr(lib, f'dq_combine_{dt}')
    n, rows = 5, 3
    a = torch.ones(rows + 1, 1 << n, dtype=TORCH[dt], device=DEVICE)
    b = torch.ones(rows + 1, 1 << n, dtype=TORCH[dt], device=DEVICE)
    out = torch.full((rows, rows, 2), 5.0, dtype=torch.float64, device=DEVICE)
    need = lib.dq_gram_ws_bytes(n, rows, rows, c128)
    assert need == 32 * 32 * 16
    ws = torch.full((need // 8,), 5.0, dtype=torch.float64, device=DEVICE)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    refused(gram(None, p(b), n, rows, rows, p(out), p(ws), need, None), 'dq_gram', 'null pointer')
    refused(gram(p(a), p(b), n, rows, rows, None, p(ws), need, None), 'null pointer')
    refused(gram(p(a), p(b), n, rows, rows, p(out), None, need, None), 'null pointer')
    refused(gram(p(a, 8), p(b), n, rows, rows, p(out), p(ws), need, None), '16-byte aligned')
    refused(gram(p(a), p(b, 8), n, rows, rows, p(out), p(ws), need, None), '16-byte aligned')
    refused(gram(p(a), p(b), n, rows, rows, p(out), p(ws), need - 1, None), 'workspace', 'dq_gram_ws_bytes')
    refused(gram(p(a), p(b), 41, rows, rows, p(out), p(ws), need, None), 'n=41 out of range')
    refused(gram(p(a), p(b), ref.NMIN[dt] - 1, rows, rows, p(out), p(ws), need, None), 'out of range')
    refused(gram(p(a), p(b), n, 0, rows, p(out), p(ws), need, None), 'rows')
    refused(gram(p(a), p(b), n, rows, 65535 * 32 + 1, p(out), p(ws), need, None), 'rows')
    refused(gram(p(a), p(b), n, rows, rows, p(a), p(ws), need, None), 'overlap')
    assert lib.dq_gram_ws_bytes(41, 1, 1, c128) == -1 and lib.dq_gram_ws_bytes(n, 0, 1, c128) == -1
    assert lib.dq_gram_ws_bytes(ref.NMIN[dt] - 1, 1, 1, c128) == -1
    coef = torch.ones(rows, rows, dtype=torch.complex128, device=DEVICE)
    refused(combine(None, p(coef), p(b), n, rows, rows, None), 'dq_combine', 'null pointer')
    refused(combine(p(a), None, p(b), n, rows, rows, None), 'null pointer')
    refused(combine(p(a), p(coef), None, n, rows, rows, None), 'null pointer')
    refused(combine(p(a, 8), p(coef), p(b), n, rows, rows, None), '16-byte aligned')
    refused(combine(p(a), p(coef), p(b, 8), n, rows, rows, None), '16-byte aligned')
    refused(combine(p(a), p(coef, 8), p(b), n, rows, rows, None), 'coef', '16-byte aligned')
    refused(combine(p(a), p(coef), p(b), 41, rows, rows, None), 'n=41 out of range')
    refused(combine(p(a), p(coef), p(b), n, 0, rows, None), 'rows')
    refused(combine(p(a), p(coef), p(a), n, rows, rows, None), 'in and out overlap', 'out of place only')
    row = (1 << n) * a.element_size()
    refused(combine(p(a), p(coef), p(a, row), n, rows, rows, None), 'in and out overlap')       # a shifted overlap
    refused(combine(p(a), p(coef), p(a, rows * row - 16), n, 1, rows, None), 'in and out overlap')  # the last vector
    refused(combine(p(a), p(coef), p(coef), n, 1, 1, None), 'coef and out overlap')
    torch.cuda.synchronize()
    assert (a == 1).all() and (b == 1).all() and (out == 5.0).all() and (ws == 5.0).all() and (coef == 1).all()


def test_wrapper_slices_wide_batches(monkeypatch):
    """Rows beyond ``backend.GRAM_MAX_ROWS`` go through several launches: the same numbers (exact rows)."""
    monkeypatch.setattr(backend, 'GRAM_MAX_ROWS', 32)
    a, b, da, db = operands('int', 'c64', 6, 40, 70)
    np.testing.assert_array_equal(host(backend.gram(da, db)), ref.gram_ref(a, b))
    coef = ref.exact_coefs(np.random.default_rng(3), 70, 40)
    np.testing.assert_array_equal(host(backend.combine(da, dev(coef))), ref.combine_ref(coef, a).astype(np.complex64))
