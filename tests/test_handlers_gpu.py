"""Every handler body of the wave-tile kernel (csrc/dq_wave.hip, csrc/dq_wave_asm*.inc) on the MI355X, one minimal pass per
handler id (`_handler_cases.cases`: found by search, counted by `_handler_census`, proven complete on the CPU by
test_handler_census_cpu.py), against a complex128 reference that applies the same precision-rounded matrices gate by gate
with plain index arithmetic (`_handler_cases.reference`).  One pytest case per (family, precision); a failure names the
handler, the configuration and the worst ratio.

Criteria (u = 2^-24 / 2^-53; every tau below is derived in `_handler_cases`, next to the constant, none is tuned):
- DATA MOVEMENT IS BIT FOR BIT: a pass whose records only move amplitudes (X, trips, swaps; no arithmetic record, so the
  deferred factor is exactly 1) equals index arithmetic on the input, `torch.equal`.
- ARITHMETIC, ELEMENTWISE AND RELATIVE TO WHAT WAS SUMMED: |got_i - ref_i| <= tau S_i with S = |U_G| .. |U_1| |x| (the same
  gates applied to absolute values) and tau = sqrt 2 gamma_r, r the roundings a real component passes through summed over
  the pass's arithmetic records (`roundings`: 2k for a length-k complex dot product, k where the matrix is promised real,
  2 for a diagonal; Hadamard 1 + 2, deferred Rx 3 + 2, and 2 for the multiplication by the pass's factor).
- AMPLITUDES A CONTROL EXCLUDES ARE UNTOUCHED, bit for bit (lane, register and outside controls alike).
- REDUCTIONS (DQ_FG_GRAD, DQ_FG_EXPZ): the accumulator is pre-filled with 0.5 (it is added to); a row no record names and
  the components the header promises untouched (include/dq_hip.h, DQ_FG_GRAD) stay exactly 0.5; formed components
  |got - ref| <= tau S, S the same sum over absolute values; tau = 1e-12 for complex128 (double accumulation, order only),
  2 (m + 2) u resp. (m + 2) u for complex64 with m the float additions in front of the promotion to double (`M_GRAD`,
  `M_EXPZ`), plus twice the amplitude bound of the records in front.
NEGATIVE CONTROLS, from reference tensors only: for every case the corruptions a plausible generator bug would produce
(`corruptions`: the gate on the neighbouring bit, imaginary parts dropped / one sign flipped, a lane or outside control
ignored, the two index bits of a 4x4 matrix swapped, a diagonal's phases exchanged, the neighbouring variant's sums, a
parity ignored) are each shown to be REJECTED by the case's criterion.  The worst measured ratio of every family is
printed (``-s``); the table is in DESIGN.md 4.0."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import _handler_cases as hc
import _handler_census as census
from deepquantum_amd import backend, fusion
from deepquantum_amd.fusion import PrimOp

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FAMILIES = [(nm, is128) for is128 in (False, True) for nm, _, _ in census.families(is128)]


def cdt(is128):
    return torch.complex128 if is128 else torch.complex64


# ---- criteria (numpy, on host copies: the states are 2^13 or 2^14 amplitudes) ------------------------------------------------------
def amp_ratio(got, want, tau, is128):
    """max |got - ref| / (tau S); with tau = 0 (nothing rounds): 0 if bit for bit equal, else inf."""
    if tau == 0:
        ndt = np.complex128 if is128 else np.complex64
        return 0.0 if np.array_equal(got.astype(ndt), want['out'].astype(ndt)) else float('inf')
    assert (want['abs'] > 0).all()
    return float((np.abs(got.astype(np.complex128) - want['out']) / (tau * want['abs'])).max())


def acc_ratio(acc, ref, ref_abs, tau):
    """Rows of the accumulator (pre-filled with 0.5): inf unless exactly the components the reference forms changed."""
    formed = ~np.isnan(ref)
    if not np.all(acc[~formed] == 0.5):
        return float('inf')
    return float((np.abs(acc[formed] - 0.5 - ref[formed]) / (tau * ref_abs[formed])).max())


# ---- negative controls --------------------------------------------------------------------------------------------------
def _op_under_test(case):
    fam = census.family(case.hid, case.is128)[0]
    kind = {'GRAD': 'grad', 'EXPZ': 'expz', 'DIAG1': 'diag', 'DIAG2': 'diag'}.get(fam, 'x' if fam in census.MOVES else 'gen')
    idx = [i for i, op in enumerate(case.cfg.ops) if op.kind == kind]
    return (idx[-1] if idx else len(case.cfg.ops) - 1), fam


def corruptions(case, refm):
    """[(what, ops, matrices)]: the case as a plausible generator bug would compute it."""
    geom = fusion.default_geometry(case.is128)
    oi, fam = _op_under_test(case)
    op = case.cfg.ops[oi]
    slots = {b for s, _ in case.cfg.rounds for b in s}
    out = []

    def with_op(what, new, mats=refm):
        ops = list(case.cfg.ops)
        ops[oi] = new
        out.append((what, ops, mats))

    def clone(**kw):
        d = dict(kind=op.kind, targets=op.targets, controls=op.controls, mat=op.mat, mode=op.mode, pos=0, order=op.order)
        d.update(kw)
        return PrimOp(**d)

    if op.targets:
        used = set(op.targets) | set(op.controls)
        t = op.targets[0]
        near = next(b for d in (1, -1, 2, -2, 3, -3) for b in [t + d] if 0 <= b < geom.m and b not in used)
        with_op(f'the gate on index bit {near} instead of {t}', clone(targets=(near,) + op.targets[1:]))
    lane_c = tuple(c for c in op.controls if c < geom.m and c not in slots)
    out_c = tuple(c for c in op.controls if c >= geom.m)
    if op.kind != 'expz':
        if lane_c:
            with_op('lane control ignored', clone(controls=tuple(c for c in op.controls if c not in lane_c)))
        if out_c:
            with_op('outside control ignored', clone(controls=tuple(c for c in op.controls if c not in out_c)))
    if op.kind in ('gen', 'diag'):
        d = 1 << op.k
        blk = refm[:, op.mat:op.mat + d * d].reshape(-1, d, d).copy()
        bad = refm.copy()
        if op.kind == 'diag':
            i, j = (0, 1) if op.k == 1 else (1, 2)
            blk[:, [i, j], [i, j]] = blk[:, [j, i], [j, i]]
            what = 'the phases of the two halves exchanged' if op.k == 1 else 'the two index bits of the diagonal swapped'
        elif np.abs(blk.imag).max() > 0:
            blk, what = blk.real.astype(np.complex128), 'imaginary parts of the matrix dropped'
        else:
            blk[:, 0, d - 1] *= -1
            what = 'the sign of one entry of the real matrix flipped'
        bad[:, op.mat:op.mat + d * d] = blk.reshape(-1, d * d)
        with_op(what, op, bad)
    if op.kind == 'gen' and op.k == 2:
        with_op('the two index bits of the 4x4 matrix swapped (w6 inverted)', clone(targets=op.targets[::-1]))
    if op.kind == 'grad':
        variant = op.mode >> fusion.GRAD_VARIANT_SHIFT
        with_op('the sums of the neighbouring variant', clone(mode=(op.mode & fusion.GRAD_ROW_MASK) | (((variant + 1) % 5) << fusion.GRAD_VARIANT_SHIFT)))
    if op.kind == 'expz':
        z = op.controls
        for what, drop in (('tile parity ignored', out_c), ('lane parity ignored', lane_c), ('register signs ignored', tuple(c for c in z if c in slots))):
            if drop:
                with_op(what, clone(controls=tuple(c for c in z if c not in drop)))
    return out


# ---- one case ---------------------------------------------------------------------------------------------------------------
def run_case(case):
    """-> (ratio of the amplitudes, ratio of the reductions or None); asserts the criteria and their negative controls."""
    is128, cfg = case.is128, case.cfg
    src, refm = hc.matrices(case)
    step, km, stride = hc.kernel_inputs(case, src)
    assert case.hid in {r.hid for r in census.ids(step.desc, cfg.n, is128)}, case.name
    x = hc.state(case)
    xd = torch.from_numpy(x).to(cdt(is128)).to(DEV)
    out = torch.full_like(xd, float('nan'))
    acc = torch.full((2, cfg.nrows + 1, 8), 0.5, dtype=torch.float64, device=DEV) if cfg.nrows else None
    backend.apply_fused(xd, km.to(DEV).reshape(-1), stride, step.desc, out=out, grads=acc)
    got = out.cpu().numpy()
    want = hc.reference(case, x, refm)
    tau = hc.tau_amplitudes(case)
    assert (tau == 0) == all(op.kind in ('x', 'grad', 'expz') for op in cfg.ops)
    ratio = amp_ratio(got, want, tau, is128)
    assert ratio <= 1.0, f'{case.name}: max |got - ref| / (tau |U||x|) = {ratio:.3e}, tau = {tau:.3e}'
    if cfg.wpos is None and not want['touched'].all():
        keep = ~want['touched']
        assert np.array_equal(got[:, keep], xd.cpu().numpy()[:, keep]), f'{case.name}: amplitudes a control excludes changed'
    aratio = None
    if cfg.nrows:
        kind = 'expz' if any(op.kind == 'expz' for op in cfg.ops) else 'grad'
        atau = hc.tau_reduction(case, kind)
        a = acc.cpu().numpy()
        assert np.all(a[:, cfg.nrows] == 0.5), f'{case.name}: a row no record names changed'
        aratio = acc_ratio(a[:, :cfg.nrows], want['acc'], want['acc_abs'], atau)
        assert aratio <= 1.0, f'{case.name}: reduction, max |got - ref| / (tau S) = {aratio:.3e}, tau = {atau:.3e}'
    # negative controls: the criterion rejects each corruption (computed from reference tensors only)
    bad = corruptions(case, refm)
    assert bad, case.name
    seen = 0
    for what, ops, mats in bad:
        wrong = hc.reference(case, x, mats, ops)
        rejected = amp_ratio(wrong['out'], want, tau, is128) > 1.0
        if cfg.nrows:
            rejected = rejected or acc_ratio(np.where(np.isnan(wrong['acc']), 0.5, wrong['acc'] + 0.5), want['acc'], want['acc_abs'], atau) > 1.0
        assert rejected, f'{case.name}: the criterion does not see "{what}"'
        seen += 1
    assert seen > 0
    return ratio, aratio


@pytest.mark.parametrize('fam,is128', FAMILIES, ids=[f'{nm}-{"c128" if p else "c64"}' for nm, p in FAMILIES])
def test_handler_family_against_complex128(fam, is128):
    mine = [c for c in hc.cases(is128) if census.family(c.hid, is128)[0] == fam]
    ids_ = {c.hid for c in mine}
    lo, hi = next((lo, hi) for nm, lo, hi in census.families(is128) if nm == fam)
    assert ids_ | set(hc.unreachable(is128)) >= set(range(lo, hi))
    worst, worst_acc, where = 0.0, None, ''
    for c in mine:
        r, ar = run_case(c)
        if r >= worst:
            worst, where = r, c.name
        if ar is not None:
            worst_acc = ar if worst_acc is None else max(worst_acc, ar)
    red = '' if worst_acc is None else f'; reductions {worst_acc:.3f} of their tau'
    print(f'\n{fam} {"c128" if is128 else "c64"}: {len(mine)} cases, {len(ids_)} ids; worst |got - ref| / (tau S) = {worst:.3f} ({where}){red}')


# ---- zero-extended loads ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('is128', [False, True], ids=['c64', 'c128'])
def test_zero_extended_loads_bit_by_bit(is128):
    """dq_apply_fused_zext_*: every gathered index bit of a pass (register slots and lane bits of the load layout: which is
    read from bits 8..13 / 16..21 of the descriptor's zext word) and one index bit outside the tile declared known-zero in
    turn, on an input that is zero there.  The output equals the plain launch bit for bit where the pass writes; NaN in the
    halves that must not be read changes nothing; for the bit outside the tile `out` keeps a sentinel where the header says
    nothing is written (include/dq_hip.h)."""
    geom = fusion.default_geometry(is128)
    m, L, R, vb = geom.m, geom.min_low, geom.slots, geom.vb
    n = m + 1
    o = hc._Ops()
    a, b, c, d = o.gen(m - 1, (), 0), o.gen(m - 2, (L,), 3), o.x(m - 3, (m,)), o.diag([L + 1], ())
    cfg = hc.Config('zero-extended loads', n, o.ops, [([m - 1, m - 2, m - 3], [a, b, c, d])])
    case = hc.Case(0, cfg, is128, batched=True, seed=4242)
    src, _ = hc.matrices(case)
    step, km, stride = hc.kernel_inputs(case, src)
    kd = km.to(DEV).reshape(-1)
    x = torch.from_numpy(hc.state(case)).to(cdt(is128)).to(DEV)
    idx = torch.arange(1 << n, device=DEV)
    kinds = set()
    for p in list(range(L, m)) + [m]:
        one = ((idx >> p) & 1).bool()
        x0 = x.clone()
        x0[:, one] = 0
        plain = torch.empty_like(x0)
        backend.apply_fused(x0, kd, stride, step.desc, out=plain)
        sentinel = complex(-7.0, 3.0)
        outs = []
        for fill in (0.0, float('nan')):
            xin = x0.clone()
            xin[:, one] = complex(fill, fill)
            out = torch.full_like(x0, sentinel)
            backend.apply_fused(xin, kd, stride, step.desc, out=out, known_zero=1 << p)
            outs.append(out)
        ntile, dead_slots, dead_lanes = census.zext_word(step.desc, n, 1 << p)
        if p < m:
            assert ntile == n - m and bin(dead_slots).count('1') + bin(dead_lanes).count('1') == 1, (p, dead_slots, dead_lanes)
            kinds.add('slot' if dead_slots else 'lane')
            written = torch.ones(1 << n, dtype=torch.bool, device=DEV)
        else:
            assert ntile == n - m - 1 and not dead_slots and not dead_lanes
            kinds.add('outside')
            written = ~one
            assert bool((outs[0][:, one] == sentinel).all()), f'bit {p}: a skipped tile was written'
        for out in outs:
            assert torch.equal(torch.view_as_real(out[:, written]), torch.view_as_real(plain[:, written])), f'known-zero bit {p}'
        assert torch.equal(torch.view_as_real(outs[0]), torch.view_as_real(outs[1])), f'bit {p}: the halves that must not be read were read'
    assert kinds == {'slot', 'lane', 'outside'}, kinds
    with pytest.raises(RuntimeError):           # the contiguous low bits are refused
        backend.apply_fused(x, kd, stride, step.desc, out=torch.empty_like(x), known_zero=1)
