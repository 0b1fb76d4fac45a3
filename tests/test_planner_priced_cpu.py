"""The priced pass planner without a GPU: the library's pass-cost function (dq_wave_pass_cost) against counts taken from the
generators' handler bodies record by record, the bytes it says a pass moves against what the emulator reads and writes,
the native beam search (dq_dag_plan) against the Python search it replaces, priced plans under the emulator against the
complex128 oracle, and the headline: modelled step time and planning time of the chosen schedule against the count-driven
one (what the planner chose before it knew prices)."""

import ctypes as C
import random
import time

import numpy as np
import pytest
import torch

import bench
from deepquantum_amd import _lib, backend, executor, fusion

import _wave_emulator as emu
from test_wave_cpu import random_ops, reference


def hrc_ops(n, ngates, seed):
    """Hadamard / Rx / CNOT gates on random wires, as the headline circuit has them."""
    rng = random.Random(seed)
    ops, mats, off = [], [], 0
    for _ in range(ngates):
        kind = rng.choice(['h', 'rx', 'cnot'])
        if kind == 'cnot':
            c, t = rng.sample(range(n), 2)
            ops.append(fusion.PrimOp('x', (t,), (c,), off, 0))
            m = torch.tensor([[0, 1], [1, 0]], dtype=torch.complex128)
        elif kind == 'h':
            ops.append(fusion.PrimOp('gen', (rng.randrange(n),), (), off, 3))
            m = torch.tensor([[1, 1], [1, -1]], dtype=torch.complex128) * (2 ** -0.5)
        else:
            th = rng.random() * 6.28
            ops.append(fusion.PrimOp('gen', (rng.randrange(n),), (), off, 2))
            m = torch.tensor([[np.cos(th / 2), -1j * np.sin(th / 2)], [-1j * np.sin(th / 2), np.cos(th / 2)]], dtype=torch.complex128)
        mats.append(m.reshape(-1))
        off += 4
    return ops, torch.cat(mats)


def headline_ops(n, depth=40, seed=1234):
    """The benchmark's circuit as the executor hands it to the scheduler (adjacent one-qubit gates merged)."""
    prims = []
    for op in bench.random_circuit_spec(n, depth, seed):
        if op[0] == 'cnot':
            prims.append(executor.Prim('x', None, (n - 1 - op[2],), (n - 1 - op[1],), 0))
        else:
            prims.append(executor.Prim('gen', None, (n - 1 - op[1],), (), 3 if op[0] == 'h' else 2))
    groups, order, _multi, _levels = executor._merge_structure(prims)
    merged = []
    for kind, idx in order:
        if kind == 's':
            continue
        merged.append(prims[idx] if kind == 'p' else executor.Prim('gen', None, prims[groups[idx][0][0]].targets, (), groups[idx][1]))
    return [fusion.PrimOp(p.kind, p.targets, p.controls, 4 * i, p.mode) for i, p in enumerate(merged)]


def generator_counts(is128):
    """{handler id: VALU instructions a wave executes}, counted here from the generator's bodies by the rule of the pass-cost
    model: lines that start with v_; a handler with controls pays two more for its exec mask; masked bodies whole; of the
    two variants of a complex64 deferred Rx body one runs (half the lines less the shared factor update)."""
    g = emu.gen(is128)
    out = {}
    for i, (ctl, lines) in g.handlers().items():
        v = sum(1 for ln in lines if ln.lstrip().startswith('v_'))
        if not is128 and g.ID_GEN_U + 12 <= i < g.ID_GEN_U + 18:
            v = v // 2 - 1
        out[i] = v + (2 if ctl else 0)
    return g, out


def records_valu(desc, n, is128, kz=0):
    """The count of a pass, record by record as the kernel walks them (a layout change is two records; the second holds
    addresses, no handler id)."""
    g, counts = generator_counts(is128)
    kp = emu.descriptor(desc, n, kz)
    total, i, nrec = 0, 0, kp.nrec_bytes // 32
    while i < nrec:
        hid = kp.rec[i][0]
        i += 2 if g.ID_TRIP0 <= hid < g.ID_SWAP else 1
        total += counts.get(hid, 0)
    return total, kp


def pass_cost(desc, n, kz=0):
    v, b = C.c_int64(-1), C.c_double(-1.0)
    assert _lib.load().dq_wave_pass_cost(C.byref(desc), n, kz, C.addressof(v), C.addressof(b)) == 0
    return v.value, b.value


def _geom(is128):
    geom = fusion.default_geometry(is128)
    geom.permute_store = True
    geom.plan_min_bits = 12
    return geom


@pytest.mark.parametrize('is128', [False, True], ids=['c64', 'c128'])
def test_exported_table_is_the_generators(is128):
    lib = _lib.load()
    g, counts = generator_counts(is128)
    assert [lib.dq_wave_handler_valu(int(is128), i) for i in range(g.NIDS)] == [counts.get(i, 0) for i in range(g.NIDS)]
    assert g.handler_valu() == [counts.get(i, 0) for i in range(g.NIDS)]
    assert lib.dq_wave_handler_valu(int(is128), g.NIDS) == -1 and lib.dq_wave_handler_valu(int(is128), -1) == -1
    assert sum(counts.values()) > 10000


@pytest.mark.parametrize('is128', [False, True], ids=['c64', 'c128'])
@pytest.mark.parametrize('n', [13, 14, 15, 16])
def test_pass_cost_is_the_generator_count_record_by_record(cpu_backend, n, is128):
    ops, _mats = hrc_ops(n, 40 * n, 100 + n)
    steps = fusion.schedule(ops, n, _geom(is128))
    assert len(steps) >= 2 and all(isinstance(s, fusion.FusedStep) for s in steps)
    elem = 16 if is128 else 8
    seen = 0
    for st in steps:
        want, _kp = records_valu(st.desc, n, is128)
        valu, nbytes = pass_cost(st.desc, n)
        assert valu == want and valu > 0
        assert nbytes == 2.0 * elem * (1 << n)          # a full pass reads and writes the state once
        seen += valu
    assert seen > 1000


@pytest.mark.parametrize('is128', [False, True], ids=['c64', 'c128'])
def test_pass_cost_with_known_zero_bits(cpu_backend, is128):
    """n = 14 behind |0..0>: the count under every pass's mask, and the bytes against the emulator -- what it WRITES (an
    output full of a sentinel) plus what it READS (its load loop: the pieces and lanes the descriptor's zext word leaves)."""
    n = 14
    dtype = torch.complex128 if is128 else torch.complex64
    ops, mats = hrc_ops(n, 300, 7)
    mats = mats.to(dtype)
    steps = fusion.schedule(ops, n, _geom(is128))
    masks = fusion.zero_state_masks(steps, n)
    assert masks is not None and sum(1 for k in masks if k) >= 2
    km = fusion.kernel_matrices(steps, ops, mats)
    elem = 16 if is128 else 8
    cur = np.zeros((1, 1 << n), dtype=np.complex128 if is128 else np.complex64)
    cur[0, 0] = 1
    sentinel = complex(7.0, -7.0)
    idx = np.arange(1 << n, dtype=np.int64)
    for st, kz in zip(steps, masks):
        want, kp = records_valu(st.desc, n, is128, kz)
        valu, nbytes = pass_cost(st.desc, n, kz)
        assert valu == want
        src = cur.copy()
        src[0][(idx & kz) != 0] = complex(float('nan'), float('nan'))      # (nothing known to be zero is read)
        out = np.full_like(cur, sentinel)
        emu.run_pass(st.desc, n, src, km.numpy(), 0, known_zero=kz, out=out)
        written = int(np.count_nonzero(out[0] != sentinel))
        assert not np.isnan(out[0][out[0] != sentinel]).any()
        ntiles = 1 << (kp.zext & 63)
        dead_slots, dead_lanes = (kp.zext >> 8) & 63, (kp.zext >> 16) & 63
        pieces = sum(1 for piece in range(32) if not ((piece << (0 if is128 else 1)) & dead_slots))
        lanes = sum(1 for lane in range(64) if not (lane & dead_lanes))
        read = ntiles * pieces * lanes * (1 if is128 else 2)
        assert nbytes == float(elem * (written + read)), (kz, written, read)
        cur = np.where(out == sentinel, 0, out)
    assert masks[-1] == 0 and pass_cost(steps[-1].desc, n)[1] == 2.0 * elem * (1 << n)


def test_pass_cost_and_planner_refuse_bad_arguments():
    lib = _lib.load()
    assert lib.dq_dag_plan(None, None, None, None, 0, None, 0, None) == -1 and b'null' in lib.dq_last_error()
    assert lib.dq_wave_pass_cost(None, 14, 0, None, None) == -1 and b'null' in lib.dq_last_error()
    d = _lib.DqFusedPass()
    d.m, d.slots = 13, 4
    assert lib.dq_wave_pass_cost(C.byref(d), 14, 0, None, None) < 0


@pytest.mark.parametrize('n,seeds', [(16, (20250929, 20250930, 7)), (20, (20250929, 20250931)), (28, (20250929, 20250934))])
def test_native_beam_reproduces_the_python_search(n, seeds):
    """Pricing off: the tile lists of `_plan_tiles`, seed for seed -- the randomised branches draw from the same generator."""
    ops = headline_ops(n)
    geom = fusion.default_geometry(False)
    L = geom.min_low
    for seed in seeds:
        for free_low in (0, L):
            for width, branch, far in ((4, 3, None), (8, 4, None), (1, 3, None), (4, 3, (19, 2))):
                dag = fusion._Dag(ops, n)
                a = fusion._plan_tiles(dag, set(range(L)), geom.m - L, geom.max_gates, width, branch, seed, far, free_low=free_low)
                b = fusion._plan_tiles_native(dag, set(range(L)), geom.m - L, geom.max_gates, width, branch, seed, far, free_low=free_low)
                assert a == b, (seed, free_low, width, branch, far)
                assert len(a) >= 3


def priced_steps(ops, n, geom, free_low, rate, seed=20250929):
    """A schedule from a PRICED plan, whether or not `schedule` would prefer it."""
    L = geom.min_low
    dag = fusion._Dag(ops, n)
    price = fusion._Price(n, geom.m, geom.vb == 0, None, rate)
    plan = fusion._plan_tiles_native(dag, set(range(L)), geom.m - L, geom.max_gates, 4, 3, seed, None,
                                     free_low=L if free_low else 0, price=price)
    assert price.estimate > 0
    return fusion._schedule_planned(ops, n, geom, 4, None, free_low, list(plan))


@pytest.mark.parametrize('is128', [False, True], ids=['c64', 'c128'])
@pytest.mark.parametrize('n,ngates,seed,free_low,rate,hrc', [(13, 120, 1, True, None, False), (14, 200, 2, False, None, True),
                                                            (15, 300, 3, True, 2e-4, True), (16, 260, 4, True, None, False),
                                                            (14, 150, 5, True, 1e-3, False)])
def test_priced_plans_run_under_the_emulator(cpu_backend, n, ngates, seed, free_low, rate, hrc, is128):
    dtype = torch.complex128 if is128 else torch.complex64
    ops, mats = hrc_ops(n, ngates, seed) if hrc else random_ops(n, ngates, seed)
    mats = mats.to(dtype)
    steps = priced_steps(ops, n, _geom(is128), free_low, rate)
    if steps is None:        # (free low bits: a plan may turn out infeasible; the other family always works out)
        steps = priced_steps(ops, n, _geom(is128), False, rate)
    assert steps is not None and all(isinstance(s, fusion.FusedStep) for s in steps)
    assert sorted(oi for s in steps for oi in s.ops) == list(range(len(ops)))
    km = fusion.kernel_matrices(steps, ops, mats)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 1 << n, generator=g, dtype=torch.float64) + 1j * torch.randn(2, 1 << n, generator=g, dtype=torch.float64)
    x = (x / x.norm(dim=-1, keepdim=True)).to(dtype)
    ref = reference(x, ops, mats)
    cur_d, cur_e = x.clone(), x.numpy().copy()
    tol = 1e-12 if is128 else 2e-6
    for st in steps:
        nxt = torch.empty_like(cur_d)
        backend.apply_fused(cur_d, km, 0, st.desc, out=nxt)
        cur_d = nxt
        cur_e = emu.run_pass(st.desc, n, cur_e, km.numpy(), 0)
        assert np.abs(cur_e - cur_d.numpy()).max() < tol
    assert (cur_d - ref).abs().max().item() < 10 * tol
    assert np.abs(cur_e - ref.numpy()).max() < 10 * tol


def test_schedule_keeps_the_cheapest_by_the_model(cpu_backend):
    """With prices the choice is never worse than the count-driven one by the model (that one is a candidate), for a few
    circuits at n = 20; and it is a schedule of the same gates."""
    n = 20
    for seed in (1, 2):
        ops, _mats = hrc_ops(n, 500, seed)
        geom = fusion.default_geometry(False)
        geom.permute_store = True
        a = fusion.schedule(ops, n, geom)
        geom.plan_priced = False
        b = fusion.schedule(ops, n, geom)
        assert fusion.modelled_ms(a, n)[0] <= fusion.modelled_ms(b, n)[0]
        assert sorted(oi for s in a for oi in s.ops) == list(range(len(ops)))


def _headline_geometry():
    geom = fusion.default_geometry(False)
    geom.permute_store = True
    geom.plan_width, geom.plan_branch, geom.plan_restarts = 8, 4, 6       # (executor.make_plan for states this big)
    return geom


def test_headline_modelled_time_and_planning_time(monkeypatch):
    """n = 28, depth 40, batch 16: the chosen schedule's modelled step time is strictly below that of the count-driven
    schedule, and planning takes no longer than it did with the search in Python (profiles/r07/planner_priced.txt)."""
    n = 28
    ops = headline_ops(n)
    t0 = time.perf_counter()
    new = fusion.schedule(ops, n, _headline_geometry())
    t_new = time.perf_counter() - t0
    geom = _headline_geometry()
    geom.plan_priced = False
    monkeypatch.setattr(fusion, '_plan_tiles_native', lambda *a, **k: fusion._plan_tiles(*a, **k))
    t0 = time.perf_counter()
    old = fusion.schedule(ops, n, geom)
    t_old = time.perf_counter() - t0
    ms_new, ms_old = fusion.modelled_ms(new, n, None, 16)[0], fusion.modelled_ms(old, n, None, 16)[0]
    print(f'modelled ms per step: {ms_new:.2f} (priced) {ms_old:.2f} (count-driven); planning {t_new:.2f} s against {t_old:.2f} s')
    assert len(old) == 19
    assert ms_new < ms_old
    assert t_new <= t_old
