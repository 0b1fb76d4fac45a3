"""Dry run (no data, no GPU) of one rank's schedule of a sharded circuit: the commutation-DAG order, the remaps, and the
fused passes of every local stretch with their gate counts -- what `bench.py --rehearse-rank` runs, for sizing the
exchange schedule offline.  usage: python tools/dist_schedule_dry.py [n] [g = log2 ranks] [rank] [--place]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from deepquantum_amd import distributed as D, executor, fusion, schedule


def gate_prims(n, depth=40, seed=1234):
    prims = []
    for op in bench.random_circuit_spec(n, depth, seed):
        if op[0] == 'cnot':
            prims.append(executor.Prim('x', None, (n - 1 - op[2],), (n - 1 - op[1],), 0))
        else:
            prims.append(executor.Prim('gen', None, (n - 1 - op[1],), (), 3 if op[0] == 'h' else 2))
    return prims


def merged(prims):
    groups, order, multi, levels = executor._merge_structure(prims)
    out = []
    for kind, idx in order:
        if kind == 's':          # (a scalar product rides on another gate's matrix: executor._merge_structure)
            continue
        out.append(prims[idx] if kind == 'p' else executor.Prim('gen', None, prims[groups[idx][0][0]].targets, (), groups[idx][1]))
    return out


def stretches(n, g, rank, prims, place=False):
    """[(localized prims of the stretch, out_perm of the remap behind it or None)] for rank ``rank``."""
    L = n - g
    knobs = D._knobs(True)
    st = schedule.structure(prims)
    ph = list(schedule.initial_placement(st, n, L, 0, False, knobs)) if place else list(range(n))
    order = schedule.order_indices(st, tuple(ph), n, L, 0, knobs)
    prims, st = [prims[j] for j in order], tuple(st[j] for j in order)
    out, pending, i = [], [], 0
    while i < len(prims):
        loc = D._localize_at(L, rank, D._translate(prims[i], ph))
        if loc == 'exchange':
            _, _, out_perm = schedule.relabel(ph, schedule.plan_remap(ph, st, i, n, L, 0, knobs), L)
            out.append((pending, out_perm))
            pending = []
            continue
        if loc is not None:
            pending.append(loc)
        i += 1
    out.append((pending, None))
    return out


def plan_stretch(prims, L, out_perm):
    prims = merged(prims)
    plan = executor.make_plan(prims, L, False, True, out_perm, amps=1 << L)
    steps = [s for s in plan.steps if isinstance(s, fusion.FusedStep)]
    return [len(s.ops) for s in steps], len(prims)


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    n = int(args[0]) if args else 34
    g = int(args[1]) if len(args) > 1 else 3
    rank = int(args[2]) if len(args) > 2 else 1
    prims = gate_prims(n)
    st = stretches(n, g, rank, prims, place='--place' in sys.argv)
    total = 0
    for k, (pending, out_perm) in enumerate(st):
        passes, ng = plan_stretch(pending, n - g, out_perm) if pending else ([], 0)
        total += len(passes)
        print(f'stretch {k}: {len(pending)} gates ({ng} after merging) -> {len(passes)} passes {passes}' + ('' if out_perm is not None else '  (last)'))
    print('passes', total, 'remaps', len(st) - 1)
