"""The jump kernels on the MI355X (dq_apply_jump_*, dq_jump_cross_*) against their formulas in complex128 torch: a loop over
the n bit positions on an index ``arange``.

Geometry under test (csrc/dq_jump.hip): a unit is 1024 vectors -- 2^11 complex64 / 2^10 complex128 amplitudes.  The factor
of an amplitude is a per-lane register (the bits below the unit size: bit 0 of complex64 is the element of the vector,
then eight lane bits and two unroll bits) times the unit's factor from three LDS tables of 8 bits each.  So per
precision: n = 3 is less than a unit, n = 11 / 10 exactly one, n = 13 / 12 has two high bits, n = 21 / 20 a high bit in
the second LDS table.  Every case runs at batch 3 with a record per sample, plain and transposed.

Acceptance.  Factors +-1 with scale 1: bit for bit.  Otherwise an output amplitude is one product of at most n + 1
rounded real factors and a scale: max |out - ref| <= 4 (n + 3) eps max |ref| (the 4 covers the table products, rounded
once more per group).  jump_cross: the bound of ``tests/test_diag_gpu.py`` for ``cost_cross``,
|out - ref| <= (2^-53 2^n + u_T) sum_i |w_i| |bra_i| |ket_i| with u_T = 2^-24 / 2^-53; two runs are bitwise equal."""

import pytest
import torch

from deepquantum_amd import backend

pytestmark = pytest.mark.gpu

SHAPES = [pytest.param(torch.complex64, n, id=f'c64-n{n}') for n in (3, 11, 13, 21)] + \
         [pytest.param(torch.complex128, n, id=f'c128-n{n}') for n in (3, 10, 12, 20)]
BATCH = 3


def unit_bits(dtype):
    return 11 if dtype == torch.complex64 else 10


def gaussian(n, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + n)
    return torch.randn(BATCH, 1 << n, dtype=torch.complex128, generator=g).to(dtype).cuda()


def turned(a, m):
    """i^m a per sample, by swapping and negating parts: exact in a's own precision."""
    r = torch.view_as_real(a)
    re, im = r[..., 0], r[..., 1]
    m = m[:, None]
    out = torch.stack([torch.where(m == 0, re, torch.where(m == 1, -im, torch.where(m == 2, -re, im))),
                       torch.where(m == 0, im, torch.where(m == 1, re, torch.where(m == 2, -im, -re)))], dim=-1)
    return torch.view_as_complex(out.contiguous())


def reference(x, factors, xmask, phase, scale, transpose, wide=True):
    """The map as the header states it, from the output index q: source q ^ x, factors at the source (transposed: at q).
    ``wide``: in complex128; otherwise in x's own precision (exact for factors +-1 and scale 1)."""
    n = factors.shape[1]
    q = torch.arange(1 << n, device=x.device)[None]
    src = q ^ xmask[:, None]
    at = q if transpose else src
    f = torch.ones(x.shape[0], 1 << n, dtype=torch.float64, device=x.device)
    for p in range(n):
        f = f * torch.gather(factors[:, p, :], 1, ((at >> p) & 1).expand(x.shape[0], -1))
    a = torch.gather(x.to(torch.complex128) if wide else x, 1, src)
    return turned(a * (scale[:, None] * f).to(a.real.dtype), (-phase if transpose else phase) & 3)


def record(case, n, dtype):
    """(factors, xmask, phase, scale, exact) of BATCH samples, each its own."""
    g = torch.Generator().manual_seed(100 * CASES.index(case) + n)
    lane, high, top = min(4, n - 1), min(unit_bits(dtype), n - 1), n - 1
    factors = torch.ones(BATCH, n, 2, dtype=torch.float64)
    xmask = torch.zeros(BATCH, dtype=torch.int64)
    phase = torch.zeros(BATCH, dtype=torch.int64)
    scale = torch.ones(BATCH, dtype=torch.float64)
    if case == 'pauli':                                     # x, y, z or nothing per wire; x on bit 0, a lane bit and the top bit
        z = torch.randint(0, 1 << n, (BATCH,), generator=g)
        xmask = torch.randint(0, 1 << n, (BATCH,), generator=g) | 1 | (1 << lane) | (1 << top)
        for p in range(n):
            factors[:, p, 1] = 1.0 - 2.0 * ((z >> p) & 1)
        phase = torch.tensor([bin(int(v)).count('1') % 4 for v in xmask & z])          # one i per Y
    elif case != 'identity':                                # damping on all wires, an exact zero somewhere
        factors = 0.3 + 0.7 * torch.rand(BATCH, n, 2, dtype=torch.float64, generator=g)
        scale = 0.5 + torch.rand(BATCH, dtype=torch.float64, generator=g)
        phase = torch.arange(BATCH) % 4
        where = {'zero_bit0': 0, 'zero_lane': lane, 'zero_high': high, 'zero_top': top, 'jump_top': top}[case]
        for b in range(BATCH):
            factors[b, where, 0 if case == 'jump_top' else b & 1] = 0.0       # (on either value of the bit)
        if case == 'jump_top':                              # sqrt(g) |0><1|: the zero and the flip on one wire
            xmask[:] = 1 << top
    return [t.cuda() for t in (factors, xmask, phase, scale)] + [case in ('identity', 'pauli')]


CASES = ['identity', 'pauli', 'zero_bit0', 'zero_lane', 'zero_high', 'zero_top', 'jump_top']


@pytest.mark.parametrize('transpose', [False, True], ids=['plain', 'transposed'])
@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('dtype,n', SHAPES)
def test_jump_apply(dtype, n, case, transpose):
    x = gaussian(n, dtype)
    factors, xmask, phase, scale, exact = record(case, n, dtype)
    out = backend.jump_apply(x, factors, xmask, phase, scale, transpose=transpose)
    if exact:
        assert torch.equal(out, x if case == 'identity' else reference(x, factors, xmask, phase, scale, transpose, wide=False))
        return
    ref = reference(x, factors, xmask, phase, scale, transpose)
    tol = 4 * (n + 3) * torch.finfo(x.real.dtype).eps
    err = (out.to(torch.complex128) - ref).abs().max().item() / ref.abs().max().item()
    print(f'jump_apply {case} n={n} {dtype}: err / tol = {err / tol:.3e}')
    assert err <= tol
    assert not out[ref == 0].any()                          # what an exact zero kills is exactly zero


@pytest.mark.parametrize('dtype,n', SHAPES)
def test_jump_apply_in_place(dtype, n):
    x = gaussian(n, dtype)
    factors, _, phase, scale, _ = record('zero_high', n, dtype)
    unread = torch.full((BATCH,), 5, dtype=torch.int64, device='cuda')                 # may_flip=False: xmask is not read
    ref = reference(x, factors, torch.zeros_like(unread), phase, scale, False)
    out = backend.jump_apply(x, factors, unread, phase, scale, may_flip=False, out=x)
    assert out is x
    assert (x.to(torch.complex128) - ref).abs().max().item() <= 4 * (n + 3) * torch.finfo(x.real.dtype).eps * ref.abs().max().item()
    with pytest.raises(ValueError, match='out of place only'):
        backend.jump_apply(x, factors, unread, phase, scale, out=x)


@pytest.mark.parametrize('same', [True, False], ids=['weight', 'cross'])
@pytest.mark.parametrize('case', ['random', 'zero_bit0', 'zero_high', 'zero_top'])
@pytest.mark.parametrize('dtype,n', SHAPES)
def test_jump_cross(dtype, n, case, same):
    ket = gaussian(n, dtype)
    bra = ket if same else gaussian(n, dtype, seed=5)
    weights = record(case, n, dtype)[0] ** 2 if case != 'random' else \
        torch.rand(BATCH, n, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(n)).cuda() + 0.5
    out = backend.jump_cross(bra, ket, weights)
    i = torch.arange(1 << n, device='cuda')[None]
    w = torch.ones(BATCH, 1 << n, dtype=torch.float64, device='cuda')
    for p in range(n):
        w = w * torch.gather(weights[:, p, :], 1, ((i >> p) & 1).expand(BATCH, -1))
    terms = w * bra.to(torch.complex128).conj() * ket.to(torch.complex128)
    bound = (2.0**-53 * 2.0**n + (2.0**-24 if dtype == torch.complex64 else 2.0**-53)) * terms.abs().sum(-1)
    err = (out - terms.sum(-1)).abs()
    print(f'jump_cross {case} n={n} {dtype}: worst err / bound = {(err / bound).max().item():.3e}')
    assert out.dtype == torch.complex128 and out.shape == (BATCH,)
    assert (err <= bound).all()
    if same:
        assert (out.imag == 0).all()
    assert torch.equal(torch.view_as_real(out), torch.view_as_real(backend.jump_cross(bra, ket, weights)))
