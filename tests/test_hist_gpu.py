"""The binned cost reduction and its cotangent on the MI355X (dq_cost_hist_*, dq_apply_binned_*) against the complex128
torch reference of _hist_ref.py.

Geometry under test (csrc/dq_hist.hip): a unit is 2^11 complex64 / 2^10 complex128 amplitudes, so n = 12 .. 15 is 2 .. 32
units per sample.  `all` streams the table and flushes every unit, `line3` keeps one bin per slot for the whole loop,
`above` has table bits only in the unit's part of sub().  V = 1 / 2 / 37 / 1024 run 64, 64, 8 and 1 copies per wave.

Acceptance, as tests/test_diag_gpu.py has it for cost_cross and apply_cost: per bin |out - ref| <= (2^-53 2^n + u_T) *
sum |terms of the bin|, u_T = 2^-24 / 2^-53; max |out - ref| <= tol * max |ref| with tol = 1e-4 / 1e-10 for the pass."""

import functools

import pytest
import torch

from deepquantum_amd import _lib, backend
from _hist_ref import binned_ref, hist_ref

pytestmark = pytest.mark.gpu

DTYPES = {'c64': torch.complex64, 'c128': torch.complex128}
TOL = {'c64': 1e-4, 'c128': 1e-10}
U_T = {'c64': 2.0**-24, 'c128': 2.0**-53}
CASES = {       # name: (n, batch, bits, controls)
    'all': (12, 3, tuple(range(11, -1, -1)), ()),
    'line3': (13, 1, (2, 0, 1), ()),
    'straddle': (14, 3, (4, 3, 2), ()),
    'above': (15, 1, (14, 12, 13), ()),
    'reversed': (12, 1, tuple(range(12)), ()),
    'ctrl_low': (13, 3, (6, 5, 11, 2), (0,)),
    'ctrl_high': (13, 1, (6, 5, 11, 2), (12,)),
}


@functools.lru_cache(maxsize=None)
def state(n, batch, dt, seed):
    g = torch.Generator().manual_seed(7919 * n + 31 * batch + seed)
    psi = torch.randn(batch, 1 << n, dtype=torch.complex128, generator=g).to(DTYPES[dt])
    return psi.cuda(), psi.to(torch.complex128)


def check(dt, n, batch, bits, controls, table, nbins):
    ket, kr = state(n, batch, dt, 0)
    bra, br = state(n, batch, dt, 5)
    tab = backend.bin_table(table, ket, nbins)
    for b_dev, b_ref in ((ket, kr), (bra, br)):
        out = backend.cost_hist(b_dev, ket, tab, nbins, bits, controls)
        ref, mass = hist_ref(b_ref, kr, table, nbins, n, bits, controls)
        assert out.dtype == torch.complex128 and out.shape == (batch, nbins)
        err, bound = (out.cpu() - ref).abs(), (2.0**-53 * 2.0**n + U_T[dt]) * mass
        print(f'cost_hist {dt}: worst err / bound = {(err / bound.clamp_min(1e-300)).max():.3e}')
        assert (err <= bound).all()
        again = backend.cost_hist(b_dev, ket, tab, nbins, bits, controls)
        assert torch.equal(torch.view_as_real(out), torch.view_as_real(again))
        if b_dev is ket:
            assert (out.imag == 0).all()
    g = torch.randn(batch, nbins, dtype=torch.complex128, generator=torch.Generator().manual_seed(nbins))
    ref = binned_ref(kr, g, table, n, bits, controls)
    for in_place in (False, True):
        src = ket.clone()
        out = backend.apply_binned(src, g.cuda(), tab, bits, controls, out=src if in_place else None)
        assert (out.data_ptr() == src.data_ptr()) == in_place
        err = (out.cpu().to(torch.complex128) - ref).abs().max()
        print(f'apply_binned {dt}: err / (tol * max|ref|) = {err / (TOL[dt] * ref.abs().max()):.3e}')
        assert err <= TOL[dt] * ref.abs().max()


@pytest.mark.parametrize('nbins', [1, 2, 37, 'max'])
@pytest.mark.parametrize('case', sorted(CASES))
@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_hist_and_binned_against_the_reference(dt, case, nbins):
    n, batch, bits, controls = CASES[case]
    nbins = backend.cost_hist_max_bins() if nbins == 'max' else nbins
    table = torch.randint(0, nbins, (1 << len(bits),), generator=torch.Generator().manual_seed(len(bits) + nbins))
    check(dt, n, batch, bits, controls, table, nbins)


@pytest.mark.parametrize('kind', ['one_bin', 'each_bin_once'])
@pytest.mark.parametrize('dt', ['c64', 'c128'])
def test_extreme_bin_tables(dt, kind):
    """Every entry in one bin (every lane of a copy meets every other: the longest run of rounds), and 1024 bins used once
    each over 10 scattered wires."""
    bits = (11, 0, 9, 3, 10, 5, 1, 7, 2, 6)
    if kind == 'one_bin':
        check(dt, 12, 1, bits, (), torch.full((1024,), 36), 37)
    else:
        check(dt, 12, 3, bits, (), torch.randperm(1024, generator=torch.Generator().manual_seed(3)), 1024)


def test_bad_arguments_are_refused_by_name_without_a_launch():
    lib, ia = _lib.load(), _lib.int_array
    x = torch.zeros(2, 32, dtype=torch.complex64, device='cuda')
    tab = torch.zeros(8, dtype=torch.int16, device='cuda')
    out = torch.zeros(64, dtype=torch.float64, device='cuda')
    ws = torch.zeros(256, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    xp, tp, op, wp = (v.data_ptr() for v in (x, tab, out, ws))
    bits, none = ia((2, 1, 0)), ia(())

    def hist(bra=xp, ket=xp, V=4, n=5, k=3, nc=0, wsb=2048):
        return lib.dq_cost_hist_c64(bra, ket, tp, V, n, bits, k, none, nc, 1, op, wp, wsb, None)

    def binned(src=xp, dst=xp, V=4, n=5, k=3, nc=0):
        return lib.dq_apply_binned_c64(src, dst, tp, op, V, n, bits, k, none, nc, 1, None)

    for call, word in ((lambda: hist(V=0), b'V=0'), (lambda: hist(V=backend.cost_hist_max_bins() + 1), b'V='),
                       (lambda: hist(bra=None), b'null'), (lambda: hist(n=2), b'exceeds'), (lambda: hist(wsb=8), b'workspace'),
                       (lambda: binned(V=0), b'V=0'), (lambda: binned(dst=None), b'null'), (lambda: binned(n=2), b'exceeds'),
                       (lambda: binned(dst=xp + 16), b'overlap')):
        assert call() == -1 and word in lib.dq_last_error(), lib.dq_last_error()
    assert lib.dq_cost_hist_ws_bytes(5, 1, 0, 0, 0) == -1 and lib.dq_cost_hist_ws_bytes(5, 1, 0, 0, 4) == 4 * 16
    with pytest.raises(ValueError, match=r'\[0, 4\)'):
        backend.bin_table(torch.tensor([0, 4]), x, 4)
    torch.cuda.synchronize()
    assert not x.any() and not out.any()
