"""Every handler body of the wave-tile kernel has a directed case, and the cases are right before a GPU sees them.

`_handler_cases.cases` holds one minimal pass per handler id (found by a bounded search over hand-chosen rounds, counted by
`_handler_census`).  Here, without a GPU: the ids the cases reach, united with the ids the translator provably never emits
(`_handler_cases.unreachable`, each with its citation), are ALL ids of the generated kernel -- a body added later fails
this until it has a case --; every case runs through the emulator (the library's own records) against the complex128
reference of `_handler_cases.reference`; and a report (``-s``) says which ids the random corpora of the other tests reach."""

import os

import numpy as np
import pytest

import _handler_cases as hc
import _handler_census as census
import _wave_emulator as emu
from deepquantum_amd import fusion

PREC = pytest.mark.parametrize('is128', [False, True], ids=['c64', 'c128'])
TOL = {False: 2e-6, True: 1e-12}          # the emulator's bars of test_wave_cpu.py, relative to max |ref|

#: feature values every family has to show in some case (the paths inside a body: `_handler_census.features`)
CTL = {'lane_ctl', 'no_lane_ctl', 'out_ctl', 'no_out_ctl'}
G2 = CTL | {'partial_mask', 'full_mask', 'w6=0', 'w6=1'}
REQUIRED = {
    'GEN_C': CTL, 'X_C': CTL, 'X_R1': CTL, 'GEN_R': CTL | {'partial_mask'}, 'X_R': CTL | {'partial_mask'},
    'DIAG1': CTL | {'selB=none', 'selB=lane', 'selB=tile', 'masked', 'unmasked'},
    'DIAG2': CTL | {'selA=none', 'selA=lane', 'selA=tile', 'selB=none', 'selB=lane', 'selB=tile', 'masked', 'unmasked'},
    'GRAD': CTL | {'partial_mask', 'full_mask'},
    'EXPZ': {'reg_signs', 'lane_parity', 'tile_parity', 'no_reg_signs', 'no_lane_parity', 'no_tile_parity', 'all_three'},
    'GEN2': G2, 'GEN2R': G2, 'GEN2X': G2, 'GEN2XC': G2,
}


@PREC
def test_every_handler_id_has_a_directed_case_or_a_cited_reason(is128):
    g = emu.gen(is128)
    cases = hc.cases(is128)
    reached = {c.hid for c in cases}
    dead = hc.unreachable(is128)
    # the citations, against the translator's text: the two statements that emit a swap record name slot 0, the third use of
    # swap_id is the index offset, and there is no fourth (the two one-line definitions aside)
    with open(os.path.join(emu.ROOT, 'deepquantum_amd', 'csrc', 'dq_wave.hip')) as f:
        text = f.read()
    translate = text[text.index('static int wave_translate('):text.index('static int wave_launch(')]
    for stmt in hc.SWAP_SITES + (hc.SWAP_OFFSET_USE,):
        assert translate.count(stmt) == 1, stmt
        assert all(stmt in why for why in dead.values())
    assert translate.count('swap_id(') == 3 and text.count('swap_id(') == 5, 'the translator gained or lost a use of swap_id: revisit UNREACHABLE'
    assert not reached & set(dead), [census.name(h, is128) for h in sorted(reached & set(dead))]
    missing = sorted(set(range(g.NIDS)) - reached - set(dead))
    assert not missing, 'handler ids without a directed case: ' + ', '.join(f'{h} ({census.name(h, is128)})' for h in missing)
    for c in cases:          # every case contains the id it stands for, per the library's own translation
        step, _ = hc.build(c.cfg, is128)
        assert c.hid in {r.hid for r in census.ids(step.desc, c.cfg.n, is128)}, c.name
        assert c.cfg.n - fusion.default_geometry(is128).m in (1, 2)
    print(f'\n{"complex128" if is128 else "complex64"}: NIDS = {g.NIDS}, directed cases reach {len(reached)}, UNREACHABLE = {len(dead)}')
    for why in sorted(set(dead.values())):
        print('  unreachable: ' + ', '.join(f'{h} {census.name(h, is128)}' for h in sorted(dead) if dead[h] == why) + f'\n    {why}')


@PREC
def test_the_name_table_follows_the_generator(is128):
    g = emu.gen(is128)
    names = [census.name(h, is128) for h in range(g.NIDS)]
    assert len(set(names)) == g.NIDS
    assert any(nm.startswith('GEN2X ') for nm in names) == hasattr(g, 'ID_GEN2X')
    assert sum(nm.startswith('GRAD ') for nm in names) == g.GRAD_VARIANTS * (g.R - 1)
    assert sum(nm.startswith('TRIP mask') for nm in names) == len(g.TRIP_MASKS)
    assert names[g.ID_GEN_U + 2 * g.R + 3] == 'GEN_U mode=2 slot=3' and names[g.ID_X_R1] == 'X_R1 q=0 c=1'


@PREC
def test_the_cases_of_a_family_show_every_path_inside_its_bodies(is128):
    cases = hc.cases(is128)
    shown, batched = {}, {}
    for c in cases:
        fam = census.family(c.hid, is128)[0]
        for r in c.records:
            if r.hid == c.hid:
                shown.setdefault(fam, set()).update(r.features)
        has_matrix = any(op.kind in ('gen', 'diag') for op in c.cfg.ops)
        batched[fam] = batched.get(fam, False) or (c.batched and has_matrix)
    fams = {nm for nm, _, _ in census.families(is128)}
    for fam, need in REQUIRED.items():
        if fam in fams:
            assert need <= shown[fam], (fam, sorted(need - shown[fam]))
    for fam in fams - set(census.MOVES) - {'GRAD', 'EXPZ'}:
        assert batched[fam], f'{fam}: no case with per-sample matrices'
    if not is128:        # both forms of the deferred Rx block { f, it, -, flag } run
        flags = set()
        for c in cases:
            if census.name(c.hid, is128).startswith('GEN_U mode=2'):
                src, _ = hc.matrices(c)
                step, km, _ = hc.kernel_inputs(c, src)
                assert fusion.deferred_rx(step.desc.gates[0])
                flags |= {float(v) for v in km[:, step.desc.gates[0].mat + 3].real}
        assert flags == {0.0, 1.0}


@PREC
def test_reductions_sit_behind_deferred_factors(is128):
    """Every GRAD variant and EXPZ has a case whose pass holds a Hadamard record and (complex64) a deferred Rx in front of the
    reduction, so that the |factor|^2 of the reduction bodies runs on hardware."""
    g = emu.gen(is128)
    behind = {}
    for c in hc.cases(is128):
        fam = census.family(c.hid, is128)[0]
        if fam not in ('GRAD', 'EXPZ'):
            continue
        at = [r.hid for r in c.records].index(c.hid)
        modes = {(r.hid - g.ID_GEN_U) // g.R for r in c.records[:at] if r.family == 'GEN_U'}
        key = ('GRAD', (c.hid - g.ID_GRAD) // (g.R - 1)) if fam == 'GRAD' else ('EXPZ', 0)
        behind.setdefault(key, set()).update(modes)
        if not is128 and 2 in modes:
            step, _ = hc.build(c.cfg, is128)
            assert any(fusion.deferred_rx(step.desc.gates[i]) for i in range(len(c.cfg.ops))), c.name
    want = {3} if is128 else {2, 3}
    keys = [('GRAD', v) for v in range(g.GRAD_VARIANTS)] + [('EXPZ', 0)]
    assert all(want <= behind.get(k, set()) for k in keys), {k: behind.get(k) for k in keys}


def run_on_emulator(case):
    src, refm = hc.matrices(case)
    step, km, stride = hc.kernel_inputs(case, src)
    x = hc.state(case)
    want = hc.reference(case, x, refm)
    acc = np.zeros((2, max(1, case.cfg.nrows), 8))
    dt = np.complex128 if case.is128 else np.complex64
    got = emu.run_pass(step.desc, case.cfg.n, x.astype(dt), km.numpy(), stride, grads=acc if case.cfg.nrows else None)
    return got, acc, want


@PREC
def test_every_directed_case_on_the_emulator_against_complex128(is128):
    worst = 0.0
    for c in hc.cases(is128):
        got, acc, want = run_on_emulator(c)
        err = np.abs(got - want['out']).max() / np.abs(want['out']).max()
        worst = max(worst, err)
        assert err < TOL[is128], (c.name, err)
        if c.cfg.nrows:
            ref = want['acc']
            formed = ~np.isnan(ref)
            assert formed.any() and np.all(acc[:, :c.cfg.nrows][~formed] == 0.0), c.name
            aerr = np.abs(acc[:, :c.cfg.nrows][formed] - ref[formed]).max()
            assert aerr < TOL[is128] * max(1.0, np.abs(ref[formed]).max()), (c.name, aerr)
    print(f'\n{"complex128" if is128 else "complex64"}: {len(hc.cases(is128))} directed cases on the emulator, worst error / max |ref| = {worst:.2e}')


def _corpus_ids(is128):
    """Handler ids of the random corpora of test_wave_gpu.py / test_kernels_gpu.py (their sizes and seeds)."""
    from test_fusion_cpu import random_ops as mixed_ops
    from test_wave_cpu import long_sweep_ops, long_sweep_steps, random_ops

    def steps_for(ops, n, permute):
        geom = fusion.default_geometry(is128)
        geom.permute_store, geom.plan_min_bits = permute, 11
        return fusion.schedule(ops, n, geom)

    seen = set()

    def add(steps, n, ext=False):
        for st in steps:
            if isinstance(st, fusion.FusedStep):
                seen.update(r.hid for r in (census.ids_ext if ext else census.ids)(st.desc, n, is128))

    for n, ng, seed in [(12, 60, 0), (13, 120, 1), (14, 200, 2), (15, 300, 3), (17, 300, 4), (19, 400, 5)]:
        add(steps_for(random_ops(n, ng, seed)[0], n, False), n)
    for n, ng, seed in [(14, 150, 5), (16, 260, 4), (18, 300, 6), (20, 400, 7)]:
        add(steps_for(random_ops(n, ng, seed)[0], n, True), n)
    kinds = ('gen', 'x', 'diag', 'gen2', 'gen2', 'gen2real', 'gen2x', 'gen2x', 'gen2xc', 'gen2xc', 'diag2')
    for n, ng, seed, perm in [(12, 60, 0, False), (14, 150, 1, True), (17, 250, 2, True), (20, 300, 3, True)]:
        add(steps_for(mixed_ops(n, ng, seed, kinds=kinds)[0], n, perm), n)
    from test_kernels_gpu import handler_ops

    for n in ((12, 15) if is128 else (13, 16)):
        for seed in (0, 1):
            add(fusion.schedule(handler_ops(n, 150, seed)[0], n, fusion.default_geometry(is128)), n)
    for n, seed in [(13, 0), (14, 4), (15, 5)]:
        add(long_sweep_steps(long_sweep_ops(n, 400, seed)[0], n, is128), n, ext=True)
    return seen


@PREC
def test_report_what_the_random_corpora_reach(is128):
    """Reported, not asserted: the measured size of the gap the directed cases close."""
    g = emu.gen(is128)
    seen = _corpus_ids(is128)
    directed = {c.hid for c in hc.cases(is128)}
    never = sorted(set(range(g.NIDS)) - seen)
    print(f'\n{"complex128" if is128 else "complex64"}: the random corpora reach {len(seen)} of {g.NIDS} handler ids; '
          f'{len(directed - seen)} are reached by the directed cases only:')
    for h in never:
        print(f'  {h:3d} {census.name(h, is128)}{"" if h in directed else "  (unreachable: no case)"}')
    assert seen <= set(range(g.NIDS))
