"""``dq_apply_collapse_*`` and ``dq_measure_draw`` on the GPU, path by path, against the numpy complex128 reference of
``_collapse_ref.py``.  A unit is 2^11 complex64 / 2^10 complex128 amplitudes, a 128-byte line 16 / 8 of them.

Tolerances: with scale 1 the result is the reference bit for bit; otherwise each component is within
``1.5 eps |s| |amp|`` -- one rounding of s to the state's precision, one of the product; everything outside the kept
slice is exactly 0; in-place FULL equals out-of-place FULL bit for bit.  The draw: on a dyadic table every partial sum is
exact in any order, so outcomes equal the reference's exactly."""

import numpy as np
import pytest
import torch

import _collapse_ref as ref
from deepquantum_amd import backend

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(torch.complex64, id='c64'), pytest.param(torch.complex128, id='c128')]
MAPS = [pytest.param('full', False, id='full'), pytest.param('full', True, id='fullT'), pytest.param('drop', False, id='drop'),
        pytest.param('drop', True, id='dropT')]
# (n, measured bits, x table, random z): x is None, or a mask that is and-ed into random values ('reset': scatter(o))
CASES = [
    pytest.param(4, [2], 0xF, True, id='below_a_unit'),
    pytest.param(13, [0], 0x1001, True, id='bit0_x_bit0'),
    pytest.param(13, [2], 0xE, False, id='inside_the_line_x_low'),
    pytest.param(14, [10], 0x3800, True, id='unit_boundary_c128_x_high'),
    pytest.param(14, [11], 0x3801, True, id='unit_boundary_c64_x_high_and_bit0'),
    pytest.param(13, [12], None, True, id='top_bit_no_x'),
    pytest.param(13, [0], None, False, id='bit0_no_masks'),
    pytest.param(14, [13, 0, 11], 'reset', True, id='k3_scattered_reset'),
    pytest.param(14, [3, 10, 0], 0x3FFF, True, id='k3_scattered_x_random'),
]
B = 3


def records(rng, psi, n, bits, xmask, zrand):
    """Outcomes that differ over the samples, the last forced onto the least likely one, and their masks."""
    k = len(bits)
    idx = np.arange(1 << n)
    marg = np.stack([np.bincount(ref.sub(idx, bits), weights=np.abs(p) ** 2, minlength=1 << k) for p in psi])
    o = np.array([int(np.argmax(marg[0])), int(rng.integers(1 << k)), int(np.argmin(marg[2]))])
    if xmask == 'reset':
        x = np.array([sum(((v >> (k - 1 - j)) & 1) << p for j, p in enumerate(bits)) for v in o])
    else:
        x = None if xmask is None else rng.integers(1 << n, size=B) & xmask | (xmask & 1)
    z = rng.integers(1 << n, size=B) if zrand else np.zeros(B, dtype=np.int64)
    return o, x, z, marg[np.arange(B), o] ** -0.5


@pytest.mark.parametrize('n,bits,xmask,zrand', CASES)
@pytest.mark.parametrize('layout,transpose', MAPS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_collapse_paths(dtype, layout, transpose, n, bits, xmask, zrand):
    rng = np.random.default_rng(n * 100 + len(bits))
    k = len(bits)
    psi = rng.standard_normal((B, 1 << n)) + 1j * rng.standard_normal((B, 1 << n))
    o, x, z, s = records(rng, psi, n, bits, xmask, zrand)
    nin = n - k if (layout, transpose) == ('drop', True) else n
    state = torch.from_numpy(psi[:, :1 << nin]).to(dtype).cuda().contiguous()
    held = state.cpu().numpy().astype(np.complex128)
    eps = float(torch.finfo(dtype).eps)
    dev = lambda a: None if a is None else torch.from_numpy(np.asarray(a, dtype=np.int64)).cuda()      # noqa: E731
    for scale in (np.ones(B), s):
        rec = backend.collapse_rec(dev(o), torch.from_numpy(scale).cuda(), dev(x), dev(z))
        got = backend.collapse(state, bits, rec, layout, transpose)
        out = got.cpu().numpy().astype(np.complex128)
        sr = scale.astype(np.float32).astype(np.float64) if dtype == torch.complex64 else scale
        for b in range(B):
            want = ref.collapse(held[b], n, bits, int(o[b]), 0 if x is None else int(x[b]), int(z[b]), sr[b], layout, transpose)
            assert out[b].shape == want.shape
            assert np.all(out[b][want == 0] == 0), 'outside the kept slice'
            if scale[0] == 1.0 and scale[-1] == 1.0:
                assert np.array_equal(out[b], want)
            else:
                for part in (np.real, np.imag):
                    assert np.all(np.abs(part(out[b]) - part(want)) <= 1.5 * eps * np.abs(part(want)))
        if layout == 'full' and x is None:
            same = state.clone()
            assert backend.collapse(same, bits, rec, layout, transpose, out=same) is same and torch.equal(same, got)
    if layout == 'full' and x is not None:
        with pytest.raises(ValueError, match='overlaps'):
            backend.collapse(state, bits, rec, layout, transpose, out=state)


def dyadic_table(k):
    rng = np.random.default_rng(k)
    counts = rng.multinomial(1024, rng.dirichlet(np.full(1 << k, 0.3)))
    counts[rng.integers(1 << k, size=max(1, (1 << k) // 4))] = 0
    counts[int(np.argmax(counts))] += 1024 - counts.sum()
    return counts / 1024.0


@pytest.mark.parametrize('k', [3, 10])
def test_draw_on_a_dyadic_table_is_exact(k):
    p = dyadic_table(k)
    assert p.sum() == 1.0 and (p == 0).any()
    c = np.cumsum(p)
    u = np.unique(np.concatenate([[0.0, 1.0 - 2.0 ** -53], c[c < 1.0], np.nextafter(c, 0.0)]))
    want = np.array([ref.draw(p, v)[0] for v in u])
    assert np.all(p[want] > 0)
    fx = torch.arange(1 << k).cuda() * 3
    rec = backend.measure_draw(torch.from_numpy(np.tile(p, (len(u), 1))).cuda(), torch.from_numpy(u).cuda(), fx=fx)
    o = rec.outcome.cpu().numpy()
    assert np.array_equal(o, want)
    assert np.array_equal(rec.xmask.cpu().numpy(), 3 * want) and not rec.zmask.any()
    assert np.array_equal(rec.prob.cpu().numpy(), p[want])
    np.testing.assert_allclose(rec.scale.cpu().numpy(), p[want] ** -0.5, rtol=9e-16)      # (a rounding each of sqrt, 1 / and **)


def test_draw_on_a_random_table_and_forced_outcomes():
    rng = np.random.default_rng(5)
    k, b = 10, 64
    p = rng.random((b, 1 << k)) * (rng.random((b, 1 << k)) > 0.2)
    u = rng.random(b)
    want = []
    for row, v in zip(p, u):
        o, c = ref.draw(row, v)
        assert np.abs(c - v * c[-1]).min() >= 1e-9 * c[-1]         # (the condition under which the order of the sums cannot matter)
        want.append(o)
    probs = torch.from_numpy(p).cuda()
    rec = backend.measure_draw(probs, torch.from_numpy(u).cuda())
    assert np.array_equal(rec.outcome.cpu().numpy(), want)
    np.testing.assert_allclose(rec.prob.cpu().numpy(), p[np.arange(b), want] / p.sum(-1), rtol=1e-13)
    live, dead = int(np.flatnonzero(p[1] > 0)[3]), int(np.flatnonzero(p[2] == 0)[0])
    forced = torch.full((b,), -1, dtype=torch.int64)
    forced[1], forced[2] = live, dead
    again = backend.measure_draw(probs, torch.from_numpy(u).cuda(), forced=forced.cuda())
    o = again.outcome.cpu().numpy()
    assert o[1] == live and o[2] == dead and np.array_equal(np.delete(o, [1, 2]), np.delete(want, [1, 2]))
    assert again.scale[2].item() == 0.0 and again.prob[2].item() == 0.0
    assert again.scale[1].item() == pytest.approx(p[1, live] ** -0.5, rel=9e-16)
    assert torch.equal(rec.data, backend.measure_draw(probs, torch.from_numpy(u).cuda()).data)      # reproducible
