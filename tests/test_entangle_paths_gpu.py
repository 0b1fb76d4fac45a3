"""The one-wire entanglement kernels (dq_entangle.hip: ``rdm1_pass_kernel`` x 4, ``rdm1_finish_kernel``,
``wire_sum_pass_kernel`` x 2) path by path on the MI355X: the rows of _entangle_cases.py, each asserted from the plan's
mirror (_launch_geometry.entangle_launch) to reach its path, through ``backend.rdm1_cross`` / ``backend.apply_wire_sum``.

Exact criterion (every row).  Amplitudes, and wire-sum operators, whose real and imaginary parts are integers in
-2 .. 2 (_grid_refs.exact_states / int_state / int_mats: a counter-based generator, the same numbers in both precisions
and on any device).  Every float32 intermediate of the kernels is then an integer that float32 holds -- a tile's at most
8 pair products along one bit sum to at most 64, a wire-sum output to at most 16 n -- and every double one is below 2^53:
``torch.equal`` with the wire-by-wire complex128 reference, whatever the order of the sums.  The rdm1 inputs are chosen
(asserted here and, at every row's shape, in test_entangle_paths_cpu.py) so that per sample the T_k differ pairwise,
T00 != T11, T01 != 0 and, cross, T01 != conj(T10): exchanged wires, components or states cannot pass.

Rounding criterion (every row).  Gaussian normalised states.  rdm1: wire by wire |got - ref| <= tau S (check_sum), S from
_grid_refs.rdm1_cross, tau = TAU_SUM (complex128) or TAU_RDM1_C64; wire_sum: check_amps with TAU_AMP.  A same-state call
must also give T10 == conj(T01) bit for bit in every sample, which only the same-state instantiation promises (the
batch-slices rows: in every slice).

Negative controls, on reference tensors only, against both criteria: rdm1 -- per pass, what the tile that workgroup 0
takes in its last iteration adds (last sample); wire_sum -- the off-diagonal term of the last gathered wire (last sample).
Every rdm1 call runs twice and must repeat bit for bit.  Worst ratios are printed (``-s``)."""

from __future__ import annotations

import pytest
import torch

import _entangle_cases as T
import _grid_refs as R
import _launch_geometry as G
from _entangle_cases import CASES, PATHS, TAU_RDM1_C64, TAU_SUM
from deepquantum_amd import _lib, backend
from test_grid_paths_gpu import check_amps, check_sum, rand_state, rejects_amps, rejects_sum, report

pytestmark = pytest.mark.gpu

DEV = 'cuda'
C64, C128 = torch.complex64, torch.complex128
RDM1 = [c for c in CASES if c.kernel == 'rdm1']
WIRE_SUM = [c for c in CASES if c.kernel == 'wire_sum']
SENTINEL = -7.25


def _reach(case) -> dict:
    """The row's claims from the mirror; returns the mirror of the launch that holds the LAST sample."""
    geo = T.launch(case)
    assert PATHS[case.path](case, geo), case.name
    for key, want in case.claims.items():
        assert [p[key] for p in geo['passes']] == want, (case.name, key)
    assert T.MAX_BATCH == backend.MAX_BATCH
    lo, hi = T.slices(case.batch)[-1]
    return G.entangle_launch(case.n, hi - lo, case.c128, case.cross)


def _rdm1_twice(bra, ket):
    got, again = backend.rdm1_cross(bra, ket), backend.rdm1_cross(bra, ket)
    assert got.dtype == C128 and got.shape == (ket.shape[0], R._nbits(ket), 2, 2)
    assert torch.equal(torch.view_as_real(got), torch.view_as_real(again)), 'rdm1_cross does not repeat bit for bit'
    return got


def _same_route(case, got):
    if not case.cross:
        assert torch.equal(got[:, :, 1, 0], got[:, :, 0, 1].conj()), f'{case.name}: T10 is not conj(T01) bit for bit'


# ---- rdm1 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', RDM1, ids=lambda c: c.name)
def test_rdm1_exact(case):
    geo = _reach(case)
    dtype = C128 if case.c128 else C64
    bra, ket = R.exact_states(case.n, case.batch, case.seed, case.cross, DEV)
    y = ket.to(dtype)
    x = bra.to(dtype) if case.cross else y
    assert torch.equal(y.to(C128), ket) and (x is y) == (not case.cross)
    got = _rdm1_twice(x, y)
    ref = R.rdm1_exact(bra, ket)
    rr, gr = torch.view_as_real(ref), torch.view_as_real(got)
    assert torch.equal(rr, rr.round()) and float(rr.abs().max()) <= 8.0 * 2.0**case.n        # the reference is exact
    assert bool(R.rdm1_inputs_ok(ref, case.cross).all()), f'{case.name}: the inputs do not tell wires, components or states apart'
    wrong = int((gr != rr).sum())
    print(f'{case.name}: max |ref| {float(ref.abs().max()):.0f}: {wrong} of {rr.numel()} parts differ')
    assert torch.equal(gr, rr), f'{case.name}: {wrong} real / imaginary parts differ, worst by {float((gr - rr).abs().max())}'
    _same_route(case, got)
    for i, o, base in T.passes_of_control(case, geo):
        delta = R.rdm1_tile_share(bra[-1], ket[-1], geo, i, base, o)
        assert not torch.equal(ref[-1] - delta, ref[-1]), f'{case.name}: tile {o} of pass {i} adds nothing'


@pytest.mark.parametrize('case', RDM1, ids=lambda c: c.name)
def test_rdm1_rounding(case):
    geo = _reach(case)
    dtype = C128 if case.c128 else C64
    tau = TAU_SUM if case.c128 else TAU_RDM1_C64
    y = rand_state(case.batch, case.n, dtype, seed=21)
    x = rand_state(case.batch, case.n, dtype, seed=22) if case.cross else y
    got = _rdm1_twice(x, y)
    ref, s = R.rdm1_cross(x, y)
    report(case.name, float(((got - ref).abs() / s).max()), tau)
    for k in range(case.n):
        check_sum(got[:, k], ref[:, k], s[:, k], tau, f'{case.name} wire {k}')
    _same_route(case, got)
    for i, o, base in T.passes_of_control(case, geo):
        delta = R.rdm1_tile_share(x[-1], y[-1], geo, i, base, o)
        rejects_sum(delta, s[-1], tau, f'{case.name}: tile {o} of pass {i}')


# ---- wire_sum ----------------------------------------------------------------------------------------------------------------
def _last_gathered_bit(case, geo) -> int:
    p = geo['passes'][-1]['settles'][-1][0]
    assert p == case.n - 1
    return p


@pytest.mark.parametrize('case', WIRE_SUM, ids=lambda c: c.name)
def test_wire_sum_exact(case):
    geo = _reach(case)
    dtype = C128 if case.c128 else C64
    psi = R.int_state(case.n, torch.arange(case.batch, device=DEV), case.seed)
    mats = R.int_mats(case.n, case.batch, case.seed, DEV)
    x = psi.to(dtype)
    assert torch.equal(x.to(C128), psi)
    got = backend.apply_wire_sum(x, mats)
    assert got.dtype == dtype and got.shape == x.shape and got.data_ptr() != x.data_ptr()
    ref = R.wire_sum(psi, mats)
    rr = torch.view_as_real(ref)
    assert torch.equal(rr, rr.round()) and float(rr.abs().max()) <= 16 * case.n          # exact, and float32 holds it
    gr = torch.view_as_real(got.to(C128))
    wrong = int((gr != rr).sum())
    print(f'{case.name}: max |ref| part {float(rr.abs().max()):.0f}: {wrong} of {rr.numel()} parts differ')
    assert torch.equal(gr, rr), f'{case.name}: {wrong} real / imaginary parts differ, worst by {float((gr - rr).abs().max())}'
    delta = R.wire_offdiag(psi[-1], mats[-1], _last_gathered_bit(case, geo))
    assert not torch.equal(ref[-1] - delta, ref[-1]), f'{case.name}: the off-diagonal term adds nothing'


@pytest.mark.parametrize('case', WIRE_SUM, ids=lambda c: c.name)
def test_wire_sum_rounding(case):
    geo = _reach(case)
    dtype = C128 if case.c128 else C64
    psi = rand_state(case.batch, case.n, dtype, seed=23)
    g = torch.Generator(device=DEV).manual_seed(24)
    mats = torch.view_as_complex(torch.randn(case.batch, case.n, 2, 2, 2, generator=g, device=DEV, dtype=torch.float64))
    got = backend.apply_wire_sum(psi, mats)
    ref = R.wire_sum(psi, mats)
    scale = check_amps(got, ref, dtype, case.name)
    delta = R.wire_offdiag(psi[-1], mats[-1], _last_gathered_bit(case, geo))
    rejects_amps(ref[-1] - delta, ref[-1], scale[-1], dtype, case.name)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _refused(lib, rc, word, what):
    msg = lib.dq_last_error().decode()
    assert rc == -1 and word in msg, f'{what}: status {rc}, message {msg!r}'              # DQ_ERR_ARG


def test_rdm1_refusals_launch_nothing():
    """DQ_ERR_ARG with a message from dq_rdm1_cross_* before any launch: the output and the workspace keep their sentinel."""
    lib = _lib.load()
    n, batch = 13, 2
    for suffix, dtype in (('c64', C64), ('c128', C128)):
        fn = getattr(lib, f'dq_rdm1_cross_{suffix}')
        ket = torch.ones(batch, 1 << n, dtype=dtype, device=DEV)
        bra = torch.ones_like(ket)
        need = lib.dq_rdm1_ws_bytes(n, batch, int(dtype == C128), 1)
        need_same = lib.dq_rdm1_ws_bytes(n, batch, int(dtype == C128), 0)
        assert need == G.rdm1_ws_bytes(n, batch, dtype == C128, True) and need_same == G.rdm1_ws_bytes(n, batch, dtype == C128, False)
        out = torch.full((batch, n, 2, 2, 2), SENTINEL, dtype=torch.float64, device=DEV)
        ws = torch.full((need // 8 + 16,), SENTINEL, dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        b, k, o, w = bra.data_ptr(), ket.data_ptr(), out.data_ptr(), ws.data_ptr()
        bad = 'bad argument'
        for what, args, word in (
                ('n = 0', (b, k, 0, batch, o, w, need), bad), ('n = 41', (b, k, 41, batch, o, w, need), bad),
                ('batch 0', (b, k, n, 0, o, w, need), bad), ('batch 65536', (b, k, n, 65536, o, w, need), bad),
                ('null bra', (None, k, n, batch, o, w, need), bad), ('null ket', (b, None, n, batch, o, w, need), bad),
                ('null out', (b, k, n, batch, None, w, need), bad), ('null workspace', (b, k, n, batch, o, None, need), 'workspace'),
                ('workspace 8 bytes short', (b, k, n, batch, o, w, need - 8), 'workspace'),
                ('same state, workspace 8 bytes short', (k, k, n, batch, o, w, need_same - 8), 'workspace')):
            _refused(lib, fn(*args, None), word, f'dq_rdm1_cross_{suffix}, {what}')
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all()), suffix


def test_wire_sum_refusals_launch_nothing():
    """DQ_ERR_ARG with a message from dq_apply_wire_sum_* before any launch: ``out`` keeps its sentinel, and a state that
    ``out`` aliases, wholly or in part, is left as it was."""
    lib = _lib.load()
    n, batch = 13, 2
    dim = 1 << n
    for suffix, dtype in (('c64', C64), ('c128', C128)):
        fn = getattr(lib, f'dq_apply_wire_sum_{suffix}')
        buf = torch.arange(3 * dim, device=DEV).to(dtype)                   # psi = its first two samples
        before = buf.clone()
        out = torch.full((batch, dim), SENTINEL, dtype=dtype, device=DEV)
        mats = torch.ones(batch, n, 2, 2, 2, dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        size = buf.element_size()
        p, o, m = buf.data_ptr(), out.data_ptr(), mats.data_ptr()
        bad = 'bad argument'
        for what, args, word in (
                ('n = 0', (p, o, m, 0, batch), bad), ('n = 41', (p, o, m, 41, batch), bad),
                ('batch 0', (p, o, m, n, 0), bad), ('batch 65536', (p, o, m, n, 65536), bad),
                ('null psi', (None, o, m, n, batch), bad), ('null out', (p, None, m, n, batch), bad),
                ('null mats', (p, o, None, n, batch), bad),
                ('out == psi', (p, p, m, n, batch), 'alias'),
                ('out overlaps the second sample of psi', (p, p + dim * size, m, n, batch), 'alias'),
                ('psi overlaps the second sample of out', (p + dim * size, p, m, n, batch), 'alias'),
                ('out half a sample into psi', (p, p + dim * size // 2, m, n, batch), 'alias')):
            _refused(lib, fn(*args, None), word, f'dq_apply_wire_sum_{suffix}, {what}')
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and torch.equal(buf, before), suffix
