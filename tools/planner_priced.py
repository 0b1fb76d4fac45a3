"""The headline's schedule with and without prices (no GPU needed): modelled step time of the count-driven schedule (the
planner's choice before it knew prices: fewest passes, then least moved behind |0..0>, then fewest layout changes) and of the
schedule `fusion.schedule` keeps now (the cheapest by the pass-cost model among the count-driven and the priced plans), pass by
pass, and the planning time of both.  usage: python tools/planner_priced.py [n depth batch] > profiles/rNN/planner_priced.txt"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import bench
from deepquantum_amd import executor, fusion


def ops_of(n, depth, seed=1234):
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


def geometry(priced):
    geom = fusion.default_geometry(False)
    geom.permute_store = True
    geom.plan_width, geom.plan_branch, geom.plan_restarts = 8, 4, 6       # (executor.make_plan for states this big)
    geom.plan_priced = priced
    return geom


if __name__ == '__main__':
    n, depth, batch = (int(a) for a in sys.argv[1:4]) if len(sys.argv) >= 4 else (28, 40, 16)
    ops = ops_of(n, depth)
    print(f'n = {n}, depth {depth}, batch {batch}, complex64: {len(ops)} gates after merging')
    native = fusion._plan_tiles_native
    fusion._plan_tiles_native = lambda *a, **k: fusion._plan_tiles(*a, **k)       # the planner before: the beam search in Python
    t0 = time.perf_counter()
    steps = fusion.schedule(ops, n, geometry(False))
    print(f'count-driven selection with the beam search in Python (the planner before): {len(steps)} passes, planning '
          f'{time.perf_counter() - t0:.2f} s on the same machine')
    fusion._plan_tiles_native = native
    for priced in (False, True):
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            steps = fusion.schedule(ops, n, geometry(priced))
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        ms, rows = fusion.modelled_ms(steps, n, None, batch)
        masks = fusion.zero_state_masks(steps, n) or [0] * len(steps)
        print(f'\n{"priced selection" if priced else "count-driven selection"}: {len(steps)} passes, modelled {ms:.2f} ms per step, '
              f'planning {best:.2f} s (best of 3, native beam search)')
        for i, (st, kz, (valu, nbytes, pms)) in enumerate(zip(steps, masks, rows)):
            print(f'pass {i:2d}: gates {len(st.ops):3d} trips {st.ntranspose}  valu {valu:5d}  known-zero bits {bin(kz).count("1"):2d}  '
                  f'{nbytes / 2 ** 30:6.2f} GiB moved  modelled {pms:6.2f} ms')
