"""The kernels' large-grid paths against plain complex128 / float64 references (_grid_refs.py) on the MI355X.

Every launcher changes path with size: above a grid cap workgroups loop over their work, apply_dense56_kernel prefetches
the next column group, the entanglement kernels run a third tile pass, marginals sum runs of chunks, states of 1 GiB or
more take non-temporal instantiations.  Each case here runs a kernel at the smallest shape that reaches one such path --
asserted from the launch-geometry mirrors of _launch_geometry.py -- and compares it with a reference built from torch
tensor operations on the device.

Criteria (absolute tolerances mean nothing at these sizes: a typical amplitude at n = 27 is 8.6e-5):
- amplitude outputs, per sample: max |got - ref| <= TAU_AMP * max |ref|;
- reductions: |got - ref| <= tau * S elementwise, S the same sum over the absolute values of its terms; tau = 1e-12 for
  the kernels that accumulate in double from exactly upcast inputs (only the order of the summation differs);
- data movement: bit for bit.
Each case also builds a NEGATIVE CONTROL: a copy of the reference corrupted the way a broken large-grid path would corrupt
it (the terms of one workgroup's last loop iteration dropped, a column group only a second iteration writes left at its
input value, two wires' blocks swapped), and asserts that the criterion rejects it.  That runs on the reference tensors
only.  The worst measured ratio of every case is printed (``-s``)."""

from __future__ import annotations

import itertools
import random

import pytest
import torch

import _grid_refs as R
import _launch_geometry as G
from deepquantum_amd import backend
from test_entanglement_gpu import explicit_wire_sum
from test_rdm_gpu import explicit_cross

pytestmark = pytest.mark.gpu

DEV = 'cuda'
C64, C128 = torch.complex64, torch.complex128
#: rounding of the amplitude kernels relative to max |ref|: estimated 1e-7 (complex64) / 1e-16 (complex128) at these sizes
TAU_AMP = {C64: 1e-5, C128: 1e-12}
TAU_SUM = 1e-12
IDS = {C64: 'c64', C128: 'c128'}


def rand_state(b, n, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    real = torch.float32 if dtype == C64 else torch.float64
    x = torch.view_as_complex(torch.randn(b, 1 << n, 2, generator=g, device=DEV, dtype=real))
    return (x / x.norm(dim=-1, keepdim=True)).contiguous()


def rand_unitary(k, b, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    a = torch.view_as_complex(torch.randn(b, 1 << k, 1 << k, 2, generator=g, device=DEV, dtype=torch.float64))
    return torch.linalg.qr(a)[0].to(dtype)


def report(what, ratio, tau):
    print(f'{what}: worst ratio {ratio:.3e} (criterion {tau:.1e})')


# ---- criteria ------------------------------------------------------------------------------------------------------------
CHUNK = 1 << 24


def amp_ratios(got, ref):
    """Per sample max |got - ref| / max |ref| (in chunks: no temporary of a whole 1-GiB state)."""
    err = torch.zeros(ref.shape[0], dtype=torch.float64, device=ref.device)
    scale = torch.zeros_like(err)
    for lo in range(0, ref.shape[1], CHUNK):
        r = ref[:, lo : lo + CHUNK]
        err = torch.maximum(err, (got[:, lo : lo + CHUNK].to(r.dtype) - r).abs().amax(dim=1).double())
        scale = torch.maximum(scale, r.abs().amax(dim=1).double())
    return err / scale, scale


def check_amps(got, ref, dtype, what):
    ratio, scale = amp_ratios(got, ref)
    report(what, float(ratio.max()), TAU_AMP[dtype])
    assert (ratio <= TAU_AMP[dtype]).all(), f'{what}: max |got - ref| / max |ref| = {ratio.tolist()}'
    return scale


def rejects_amps(bad_part, ref_part, scale, dtype, what):
    """The negative control: a corrupted share of one sample (the rest equal to the reference) fails the amplitude
    criterion of that sample (``scale`` = its max |ref|)."""
    assert float((bad_part.to(ref_part.dtype) - ref_part).abs().max()) > TAU_AMP[dtype] * float(scale), \
        f'{what}: the criterion does not see the corruption'


def check_sum(got, ref, s, tau, what):
    err = (got - ref).abs()
    report(what, float((err / s).max()), tau)
    assert (err <= tau * s).all(), f'{what}: max |got - ref| / S = {float((err / s).max()):.3e}'


def rejects_sum(delta, s, tau, what, every=False):
    """The negative control of a reduction: dropping terms that sum to ``delta`` fails the criterion (somewhere, or at
    every element with ``every``)."""
    hit = delta.abs() > tau * s
    assert (hit.all() if every else hit.any()), f'{what}: the criterion does not see the dropped terms'


# ---- dense gates: apply_dense56_kernel and the staged MFMA kernels ------------------------------------------------------------
def _dense_case(x, u, targets, controls, shared, dtype, what, geo):
    """Out of place against the gather / matmul / scatter reference; amplitudes whose controls are not all 1 bit for bit;
    the negative control leaves the column group (dense56) or column tile (staged kernels) that workgroup 0 handles in its
    second iteration (resp. the last tile) at its input value."""
    n = x.shape[-1].bit_length() - 1
    b = x.shape[0]
    got = backend.apply_gate(x, u, targets, controls)
    assert got.data_ptr() != x.data_ptr()
    ref, xm, ym = R.apply_gate(x, u, targets, controls)
    colbits = n - len(targets) - len(controls)
    if geo['route'] == 'dense56':
        width, first = geo['col_group'], geo['per_pass'] * geo['col_group']       # the first group of the second pass
    else:
        width = 128 if geo['route'] == 'staged1' else 64
        first = ((b if shared else 1) << colbits) - width
    sample, col = (first >> colbits, first & ((1 << colbits) - 1)) if shared else (b - 1, first)
    bad, good = xm[sample, :, col : col + width].clone(), ym[sample, :, col : col + width].clone()
    del xm, ym
    scale = check_amps(got, ref, dtype, what)
    rejects_amps(bad, good, scale[sample], dtype, what)
    del ref
    if controls:
        vg, ax = R.bit_view(got, set(controls))
        vx, _ = R.bit_view(x, set(controls))
        for bits in itertools.product((0, 1), repeat=len(controls)):
            if all(bits):
                continue
            idx = [slice(None)] * vg.ndim
            for c, v in zip(controls, bits):
                idx[ax[c]] = v
            assert torch.equal(vg[tuple(idx)], vx[tuple(idx)]), f'{what}: uncontrolled amplitudes changed'
    del got


DENSE = [  # (k, n, batch, shared U, controls, dtype)
    (5, 21, 4, True, 1, C64),
    (5, 22, 2, False, 0, C64),
    (5, 21, 2, True, 1, C128),
    (5, 21, 2, False, 0, C128),
    (6, 22, 2, True, 1, C64),
    (6, 22, 2, False, 0, C64),
]


@pytest.mark.parametrize('k,n,batch,shared,nc,dtype', DENSE,
                         ids=[f'k{c[0]}-n{c[1]}-b{c[2]}-{"shared" if c[3] else "per_sample"}-c{c[4]}-{IDS[c[5]]}' for c in DENSE])
def test_dense56_second_iteration(k, n, batch, shared, nc, dtype):
    rng = random.Random(100 * n + 10 * k + batch)
    lo = 0 if dtype == C128 else 1             # (complex64: bit 0 must be a column bit for the 16-byte accesses)
    bits = [n - 1] + rng.sample(range(lo, n - 1), k + nc - 1)
    rng.shuffle(bits)
    targets, controls = bits[:k], bits[k:]
    geo = G.dense(n, k, nc, batch, dtype == C128, shared, 0 in bits)
    assert geo['route'] == 'dense56' and geo['iterations'] >= 2 and not geo['nt'], geo
    x = rand_state(batch, n, dtype, seed=n + k)
    u = rand_unitary(k, 1 if shared else batch, dtype, seed=k)
    _dense_case(x, u if not shared else u[0], targets, controls, shared, dtype, f'dense k={k} n={n} b={batch}', geo)


def test_dense_streaming_complex64_1gib():
    """One 1-GiB complex64 state (n = 27): k = 5 away from bit 0 (dense56, non-temporal), k = 5 with bit 0 among the targets
    (staged kernel WM = 1, non-temporal), k = 8 with one control (staged WM = 2, non-temporal, and the copy of the
    uncontrolled amplitudes loops)."""
    n = 27
    x = rand_state(1, n, C64, seed=27)
    cases = [([26, 3, 17, 9, 1], [], 'dense56'), ([4, 0, 22, 11, 7], [], 'staged1'),
             ([26, 0, 5, 13, 2, 20, 9, 15], [24], 'staged2')]
    for i, (targets, controls, route) in enumerate(cases):
        geo = G.dense(n, len(targets), len(controls), 1, False, True, 0 in targets + controls)
        assert geo['route'] == route and geo['nt'], geo
        if route == 'dense56':
            assert geo['iterations'] >= 2
        if controls:
            assert G.copy_uncontrolled(n, 1)['iterations'] >= 2
        u = rand_unitary(len(targets), 1, C64, seed=50 + i)[0]
        _dense_case(x, u, targets, controls, True, C64, f'dense n=27 k={len(targets)} {route}', geo)
        torch.cuda.empty_cache()


def test_dense_streaming_complex128_1gib():
    """One 1-GiB complex128 state (n = 26): k = 5 (dense56, non-temporal, bit 0 a target) and k = 6 (staged WM = 2)."""
    n = 26
    x = rand_state(1, n, C128, seed=26)
    for i, (targets, route) in enumerate((([0, 25, 7, 14, 3], 'dense56'), ([21, 1, 25, 8, 0, 16], 'staged2'))):
        geo = G.dense(n, len(targets), 0, 1, True, True, 0 in targets)
        assert geo['route'] == route and geo['nt'], geo
        u = rand_unitary(len(targets), 1, C128, seed=60 + i)[0]
        _dense_case(x, u, targets, [], True, C128, f'dense n=26 c128 k={len(targets)} {route}', geo)
        torch.cuda.empty_cache()


def test_small_controlled_gate_copy_loop():
    """k = 2 with a control, out of place, over 2^25 amplitudes: the copy of the uncontrolled amplitudes loops (VALU route
    of apply_small_kernel); the negative control zeroes uncontrolled amplitudes of the copy's second iteration."""
    n, batch = 25, 1
    assert G.copy_uncontrolled(n, batch)['iterations'] >= 2
    x = rand_state(batch, n, C64, seed=25)
    u = rand_unitary(2, 1, C64, seed=2)[0]
    targets, controls = [3, n - 1], [0]
    got = backend.apply_gate(x, u, targets, controls)
    ref, _xm, _ym = R.apply_gate(x, u, targets, controls)
    del _xm, _ym
    check_amps(got, ref, C64, 'k=2 controlled n=25')
    unc = (torch.arange(1 << n, device=DEV) & 1) == 0
    assert torch.equal(got[:, unc], x[:, unc])
    lo = G.copy_uncontrolled(n, batch)['blocks'] * 256            # the first amplitude the second iteration copies
    bad = got[:, lo : lo + 256].clone()
    bad[:, ::2] = 0
    assert not torch.equal(bad[:, ::2], x[:, lo : lo + 256 : 2])


# ---- gate gradients ----------------------------------------------------------------------------------------------------------
GRAD = [(1, 20, 2, 0), (2, 22, 2, 1)]     # (k, n, batch, controls)


@pytest.mark.parametrize('dtype', [C64, C128], ids=['c64', 'c128'])
@pytest.mark.parametrize('k,n,batch,nc', GRAD, ids=[f'k{c[0]}-n{c[1]}' for c in GRAD])
def test_gate_grad_loop(k, n, batch, nc, dtype):
    geo = G.gate_grad(n, k, nc)
    assert geo['iterations'] >= 4, geo
    rng = random.Random(n)
    bits = rng.sample(range(n), k + nc)
    targets, controls = bits[:k], bits[k:]
    x, gy = rand_state(batch, n, dtype, seed=1), rand_state(batch, n, dtype, seed=2)
    got = backend.gate_grad(x, gy, targets, controls)
    ref = explicit_cross(x, gy, targets, controls)
    s = explicit_cross(x.abs(), gy.abs(), targets, controls).real
    check_sum(got, ref, s, TAU_SUM, f'gate_grad k={k} n={n}')
    # negative control: the groups workgroup 0 handles in its last iteration
    first = (geo['iterations'] - 1) * geo['blocks'] * 256
    xm = R.gate_matrix_view(x, targets, controls).reshape(batch, 1 << k, -1)[:, :, first : first + 256].to(C128)
    ym = R.gate_matrix_view(gy, targets, controls).reshape(batch, 1 << k, -1)[:, :, first : first + 256].to(C128)
    rejects_sum(ym @ xm.mH, s, TAU_SUM, f'gate_grad k={k} n={n}')


def _multi_gates(n):
    return [(0, ()), (2, (5,)), (n - 1, (0,)), (n - 1, ()), (3, (n - 2,)), (11, (1, 17)), (7, (n - 1,)), (0, (n - 1,)),
            (15, ()), (16, (3,)), (2, ()), (12, (13, 14))]


@pytest.mark.parametrize('n,dtype', [(22, C64), (21, C128)], ids=['c64-n22', 'c128-n21'])
def test_gate_grad_multi_tile_loop(n, dtype):
    """Several launches (more gates than one holds), targets below L, repeated targets, the top bit, controls inside and
    outside the tile; each gate against the explicit reference (not against gate_grad).  Complex64 keeps per-thread float
    partials (dq_reduce.hip, T acc[GM][8]): a thread adds at most m = (tiles per workgroup) x (pairs per tile and thread)
    terms in float before the double reduction, so its error is bounded by about (m + 2) u S per component, u = 2^-24;
    tau = 2 (m + 2) u covers both components of a complex entry."""
    c128 = dtype == C128
    gates = _multi_gates(n)
    launches = G.gate_grad_multi(n, c128, gates)
    assert len(launches) >= 2 and all(la['iterations'] >= 2 for la in launches), launches
    m = max(la['iterations'] * la['pairs_per_thread'] for la in launches)
    tau = TAU_SUM if c128 else 2 * (m + 2) * 2.0**-24
    batch = 2
    x, gy = rand_state(batch, n, dtype, seed=3), rand_state(batch, n, dtype, seed=4)
    got = backend.gate_grad_multi(x, gy, gates)
    assert got.shape == (batch, len(gates), 2, 2)
    for la in launches:
        for gi in la['gates']:
            t, c = gates[gi]
            ref = explicit_cross(x, gy, [t], c)
            s = explicit_cross(x.abs(), gy.abs(), [t], c).real
            check_sum(got[:, gi], ref, s, tau, f'gate_grad_multi n={n} gate {gi} {gates[gi]}')
            # negative control: the first tile of the second iteration whose controls outside the tile are 1
            outside = [p for p in range(n) if p not in la['tile_bits']]
            cout = [outside.index(q) for q in c if q in outside]
            tile = next(tt for tt in range(la['blocks'], la['ntiles']) if all((tt >> q) & 1 for q in cout))
            rejects_sum(R.tile_cross(x, gy, la['tile_bits'], tile, t, c), s, tau, f'gate_grad_multi gate {gi}')


# ---- reductions ----------------------------------------------------------------------------------------------------------------
def _pauli_strings(n):
    top = 1 << (n - 1)
    return [(1 | top, 0),                                      # ny = 0, X on bit 0 and the top bit
            (1 | top | 1 << 5, 1 << 5 | 1 << 8),               # ny = 1
            (1 << 3 | top, 1 << 3),                            # ny = 1, lowest X bit 3
            (1 | top | 1 << 5 | 1 << 9, 1 << 5 | 1 << 9),      # ny = 2
            (1 | top | 0b1110, 0b1110 | 1 << 12),              # ny = 3
            (0, 1 | 1 << 7 | top)]                             # Z only


@pytest.mark.parametrize('dtype', [C64, C128], ids=['c64', 'c128'])
def test_expect_pauli_and_inner_loops(dtype):
    n, batch = 22, 2
    x, y = rand_state(batch, n, dtype, seed=5), rand_state(batch, n, dtype, seed=6)
    assert {bin(xm & zm).count('1') % 4 for xm, zm in _pauli_strings(n) if xm} == {0, 1, 2, 3}
    for xmask, zmask in _pauli_strings(n):
        geo = G.expect_pauli(n, xmask)
        assert geo['iterations'] >= 2, geo
        got = backend.expect_pauli(x, xmask, zmask)
        ref, s = R.expect_pauli(x, xmask, zmask)
        check_sum(got, ref, s, TAU_SUM, f'expect_pauli n={n} x={xmask:#x} z={zmask:#x}')
        # negative control: the items of workgroup 0's last iteration (pairs (i, i ^ x) for X / Y strings)
        g = (geo['iterations'] - 1) * geo['blocks'] * 256 + torch.arange(256, device=DEV)
        if xmask:
            low = (xmask & -xmask).bit_length() - 1
            i = ((g >> low) << (low + 1)) | (g & ((1 << low) - 1))
            i = torch.cat([i, i ^ xmask])
        else:
            i = g
        yc = x.to(C128)
        delta = (yc[:, i].conj() * yc[:, i ^ xmask] * R.z_sign(i ^ xmask, zmask)).sum(-1)
        delta = (delta * 1j ** bin(xmask & zmask).count('1')).real
        rejects_sum(delta, s, TAU_SUM, f'expect_pauli x={xmask:#x}', every=True)
    geo = G.inner(1 << n)
    assert geo['iterations'] >= 2
    got = backend.inner(x, y)
    ref, s = R.inner(x, y)
    check_sum(got, ref, s, TAU_SUM, f'inner n={n}')
    lo = (geo['iterations'] - 1) * geo['blocks'] * 256
    rejects_sum((x[:, lo : lo + 256].to(C128).conj() * y[:, lo : lo + 256].to(C128)).sum(-1), s, TAU_SUM, 'inner', every=True)


@pytest.mark.parametrize('dtype', [C64, C128], ids=['c64', 'c128'])
@pytest.mark.parametrize('nstrings', [1, 17, 40])
def test_scale_z_signs_loop(nstrings, dtype):
    n, batch = 22, 2
    geo = G.scale_zsigns(n)
    assert geo['iterations'] >= 2, geo
    rng = random.Random(nstrings)
    masks = [0b1011 | 1 << (n - 1)] + [rng.randrange(1, 1 << n) for _ in range(nstrings - 1)]
    x = rand_state(batch, n, dtype, seed=7)
    if nstrings == 1:
        coef = torch.ones(batch, 1, dtype=torch.float64, device=DEV)
    else:
        coef = torch.randn(batch, nstrings, generator=torch.Generator(device=DEV).manual_seed(8), device=DEV, dtype=torch.float64)
    got = backend.scale_z_signs(x, masks, coef)
    ref = R.scale_z_signs(x, masks, coef)
    scale = check_amps(got, ref, dtype, f'scale_z_signs n={n} K={nstrings}')
    if nstrings == 1:
        sign = R.z_sign(torch.arange(1 << n, device=DEV), masks[0]).to(x.real.dtype)
        assert torch.equal(got, x * sign)
    # negative control: workgroup 0's 1024 amplitudes of the second iteration left at their input value
    lo = geo['blocks'] * geo['chunk']
    for b in range(batch):
        rejects_amps(x[b, lo : lo + 1024], ref[b, lo : lo + 1024], scale[b], dtype, 'scale_z_signs')


@pytest.mark.parametrize('n,dtype', [(22, C128), (23, C64)], ids=['c128-n22', 'c64-n23'])
def test_expect_z_multi_second_iteration(n, dtype):
    geo = G.expect_zmulti(n, dtype == C128)
    assert geo['iterations'] >= 2, geo
    rng = random.Random(n)
    masks = [1, 1 << (n - 1), (1 << n) - 1] + [rng.randrange(1, 1 << n) for _ in range(37)]      # two launches (32 + 8)
    x = rand_state(2, n, dtype, seed=9)
    got = backend.expect_z_multi(x, masks)
    ref, s = R.expect_z_multi(x, masks)
    check_sum(got, ref, s, TAU_SUM, f'expect_z_multi n={n}')
    lo = (geo['iterations'] - 1) * geo['blocks'] * geo['window']       # workgroup 0's window in its last iteration
    i = lo + torch.arange(geo['window'], device=DEV)
    p = R.probabilities(x[:, lo : lo + geo['window']])
    delta = torch.stack([(p * R.z_sign(i, z)).sum(-1) for z in masks], dim=1)
    rejects_sum(delta, s, TAU_SUM, 'expect_z_multi', every=True)


MARG = [(24, 1), (22, 4)]


@pytest.mark.parametrize('dtype', [C64, C128], ids=['c64', 'c128'])
@pytest.mark.parametrize('n,batch', MARG, ids=[f'n{m[0]}-b{m[1]}' for m in MARG])
def test_marginal_chunk_runs(n, batch, dtype):
    x = rand_state(batch, n, dtype, seed=10)
    for bits in ([n - 1], [n - 1, 3, n - 2], [n - 1, n - 2, n - 3, 12, 5, 0, 17, 9]):
        geo = G.marginal(n, bits, batch, dtype == C128)
        assert geo['run'] > 0, (bits, geo)
        got = backend.marginal(x, bits)
        ref = R.marginal(x, bits)
        check_sum(got, ref, ref, TAU_SUM, f'marginal n={n} b={batch} bits={bits}')
        # negative control: the last chunk of workgroup 0's run
        ci = (1 << geo['run']) - 1
        base = sum(((ci >> t) & 1) << p for t, p in enumerate(geo['cpos']))
        a = torch.arange(1 << len(geo['chunk_bits']), device=DEV)
        e = torch.full_like(a, base)
        for q, p in enumerate(geo['chunk_bits']):
            e |= ((a >> q) & 1) << p
        o = R.outcome_index(n, bits, DEV)[e]
        delta = torch.zeros_like(ref).index_add_(1, o, R.probabilities(x[:, e]))
        rejects_sum(delta, ref, TAU_SUM, f'marginal bits={bits}')


@pytest.mark.parametrize('n,batch,dtype', [(25, 1, C64), (24, 2, C128)], ids=['c64-n25', 'c128-n24-b2'])
def test_probs_loop(n, batch, dtype):
    geo = G.probs(batch << n)
    assert geo['iterations'] >= 2, geo
    x = rand_state(batch, n, dtype, seed=11)
    got = backend.probs(x)
    ref = R.probabilities(x)
    scale = check_amps(got, ref, dtype, f'probs n={n}')
    lo = geo['blocks'] * 256 - (batch - 1) * (1 << n)              # the second iteration's first element, in the last sample
    rejects_amps(torch.zeros(256, dtype=torch.float64, device=DEV), ref[-1, lo : lo + 256], scale[-1], dtype, 'probs')


# ---- entanglement kernels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [C64, C128], ids=['c64', 'c128'])
def test_entanglement_third_pass(dtype):
    """rdm1_cross(psi, psi), rdm1_cross(phi, psi) (complex128 cross: the 11-bit tile) and apply_wire_sum at n = 23, batch
    2: three passes, two tiles per workgroup; wire by wire."""
    n, batch = 23, 2
    c128 = dtype == C128
    for cross in (False, True):
        e = G.entangle(n, batch, c128, cross)
        assert e['passes'] == 3 and min(e['iterations']) >= 2, e
    psi, phi = rand_state(batch, n, dtype, seed=12), rand_state(batch, n, dtype, seed=13)
    # complex64: a tile's (at most 8) pair products along one bit are summed in float before the double accumulation
    # (dq_entangle.hip, file header) -- about (8 + 2) u S per component, u = 2^-24; doubled for a complex entry
    tau = TAU_SUM if c128 else 2 * (8 + 2) * 2.0**-24
    for bra, what in ((psi, 'rdm1'), (phi, 'rdm1 cross')):
        got = backend.rdm1_cross(bra, psi)
        ref, s = R.rdm1_cross(bra, psi)
        for k in range(n):
            check_sum(got[:, k], ref[:, k], s[:, k], tau, f'{what} n={n} wire {k}')
        bad = ref.clone()
        bad[:, [n - 2, n - 1]] = ref[:, [n - 1, n - 2]]               # two wires of the third pass swapped
        rejects_sum(bad - ref, s, tau, what)
    g = torch.Generator(device=DEV).manual_seed(14)
    mats = torch.view_as_complex(torch.randn(batch, n, 2, 2, 2, generator=g, device=DEV, dtype=torch.float64))
    got = backend.apply_wire_sum(psi, mats)
    ref = explicit_wire_sum(psi, mats)
    scale = check_amps(got, ref, dtype, f'wire_sum n={n}')
    del got, ref
    # negative control: wire n - 2's matrix applied in the slot of wire n - 1 (the difference of the two sums)
    k = n - 1
    delta = torch.einsum('bac,bics->bias', (mats[:, n - 2] - mats[:, k]), psi.to(C128).reshape(batch, 1 << k, 2, -1))
    for b in range(batch):
        rejects_amps(delta[b], torch.zeros_like(delta[b]), scale[b], dtype, 'wire_sum')


# ---- relayout ------------------------------------------------------------------------------------------------------------------
def _perms(n):
    """The permutations of test_kernels_gpu.py::test_permute_bits_against_index_arithmetic."""
    rng = random.Random(n)
    return [list(range(n)), rng.sample(range(n), n), [0] + [1 + q for q in rng.sample(range(n - 1), n - 1)],
            list(range(1, n)) + [0], [q for q in range(n) if q not in (n - 3, n - 2)] + [n - 3, n - 2],
            list(range(n))[::-1], [n - 1] + list(range(n - 1)), [1, 0] + list(range(2, n)), rng.sample(range(n), n)]


def _check_permute(x, perm, what):
    nl = x.shape[-1].bit_length() - 1
    geo = G.permute(nl, perm, x.shape[0], x.dtype == C128)
    assert geo['iterations'] >= 2, (what, geo)
    out = backend.permute_bits(x, perm)
    want = x[:, R.src_index(nl, perm, DEV)]
    assert torch.equal(out, want), (what, perm)
    # negative control: the first 1024 outputs of the second pass over the tiles left unwritten
    lo = geo['blocks'] * 1024
    bad = want[:, lo : lo + 1024].clone().zero_()
    assert not torch.equal(bad, want[:, lo : lo + 1024])
    return geo


@pytest.mark.parametrize('dtype', [C64, C128], ids=['c64', 'c128'])
def test_permute_bits_loops(dtype):
    nl = 24
    x = rand_state(1, nl, dtype, seed=15)
    variants = {_check_permute(x, perm, f'nl={nl}')['variant'] for perm in _perms(nl)}
    assert variants == ({'tiled', 'lds'} | ({'tiled_pair'} if dtype == C64 else set())), variants


def test_permute_bits_streaming_1gib():
    nl = 27
    rng = random.Random(nl)
    perm = [0, 3, 1, 4, 2] + rng.sample(range(5, nl), nl - 5)
    x = rand_state(1, nl, C64, seed=16)
    geo = _check_permute(x, perm, 'nl=27')
    assert geo['variant'] == 'tiled_pair' and geo['nt'], geo


@pytest.mark.parametrize('dtype', [C64, C128], ids=['c64', 'c128'])
def test_pack_unpack_loops(dtype):
    nl, mask = 26, 1 << 13
    geo = G.pack(nl, mask)
    assert geo['iterations'] >= 2, geo
    amps = rand_state(1, nl, dtype, seed=17)
    half = 1 << (nl - 1)
    lo = geo['blocks'] * 256                                       # the second iteration's first packed amplitude
    for value in (0, mask):
        idx = R.expand_index(nl, mask, value, DEV)
        got = backend.pack(amps, mask, value)
        want = amps[:, idx]
        assert torch.equal(got, want)
        assert not torch.equal(want[:, lo : lo + 256].clone().zero_(), want[:, lo : lo + 256])     # (negative control)
        xs, ys = rand_state(1, nl - 1, dtype, seed=18), rand_state(1, nl - 1, dtype, seed=19)
        dst = amps.clone()
        backend.unpack_axpby(dst, xs, None, None, mask, value)
        want = amps.clone()
        want[:, idx] = xs
        assert torch.equal(dst, want)
        coef = torch.tensor([[0.5 - 0.25j, -2.0 + 1.5j]], dtype=dtype, device=DEV)
        backend.unpack_axpby(dst, xs, ys, coef, mask, value)
        want = amps.to(C128)
        want[:, idx] = coef[:, 0:1].to(C128) * xs.to(C128) + coef[:, 1:2].to(C128) * ys.to(C128)
        scale = check_amps(dst, want, dtype, f'unpack_axpby nl={nl} value={value}')
        rejects_amps(xs[0, lo : lo + 256], want[0, idx[lo : lo + 256]], scale[0], dtype, 'unpack_axpby')     # (left as unpacked before)
        assert idx.numel() == half
