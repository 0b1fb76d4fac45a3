"""Diagonal operators on the MI355X (dq_apply_diag_*, dq_apply_cost_*, dq_cost_cross_*), each
against a kernel of the parent library with the same traffic shape, timed in the same process on the same buffers.

1. Full width (bits = n-1 .. 0), complex64 n = 28 and complex128 n = 27 at batch 4:
   apply_diag, PHASE and SCALE out of place -- bytes = state read + state written + table read -- against
   ``dq_scale_zsigns_*`` with one string (state read + state written); a gathered PHASE (k = 12 scattered bits, a table
   that stays in cache) shows what the gather costs; complex128 has that row twice, in flight and through a table of
   phases (the two sides of the switch in ``backend.apply_cost``), and a sweep over n = 12 .. 24 of the same pair at
   batch 1 shows where the switch belongs.
2. ``cost_cross`` with bra == ket (state read + table read) and bra != ket against ``dq_expect_pauli_*`` with a Z mask
   (state read).
3. One QAOA cost layer on K_24 and K_28, un-batched complex64, end to end through ``QubitCircuit`` without autograd:
   route A = hlayer, one rzz per edge, rxlayer; route B = hlayer, cost_phase(ising_cost), rxlayer; with the number of
   launches each takes (fused passes; route B: the passes of its two stretches plus the diagonal pass).

Every point: one warm-up call, then the median of ``reps`` calls between device events; the rows of a group, yardstick
included, take turns within every repetition.  The box is recorded first.

usage: python tools/bench_diag.py [--quick] [--out FILE]
"""
import json
import os
import platform
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deepquantum_amd as dq  # noqa: E402
from deepquantum_amd import backend, executor, qmath  # noqa: E402


def timed(f, reps):
    return timed_group({'f': f}, reps)['f']


def timed_group(fns, reps):
    """Median, min and max ms of every function of ``fns``: one warm-up call each, then ``reps`` rounds in which they take
    turns (what drifts over the run -- clocks, the other tenants of the host -- then hits all of them alike)."""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            ts[name].append(a.elapsed_time(b))
    return {name: (sorted(v)[len(v) // 2], min(v), max(v)) for name, v in ts.items()}


def row(rows, name, dtype, n, batch, t, nbytes, base=None):
    med, lo, hi = t
    r = {'what': name, 'dtype': str(dtype)[6:], 'n': n, 'batch': batch, 'ms': round(med, 4), 'ms_min': round(lo, 4),
         'ms_max': round(hi, 4), 'bytes': nbytes, 'TB_per_s': round(nbytes / med / 1e9, 3)}
    if base is not None:
        r['time_over_yardstick'] = round(med / base, 3)
    rows.append(r)
    print(f"{name:<32} {r['dtype']:<10} n={n} b={batch}  {med:9.4f} ms  [{lo:.4f}, {hi:.4f}]  {r['TB_per_s']:6.3f} TB/s"
          + (f"  x{r['time_over_yardstick']:.3f} of the yardstick" if base is not None else ''), flush=True)
    return med


def forced(route, f):
    """``f`` with the table / in-flight switch of ``backend.apply_cost`` held on one side (where the table route exists)."""
    def g():
        keep = backend.PHASE_TABLE_MAX_BITS, backend.PHASE_TABLE_MIN_QUBITS
        backend.PHASE_TABLE_MAX_BITS, backend.PHASE_TABLE_MIN_QUBITS = (-1, keep[1]) if route == 'in flight' else (keep[0], 0)
        try:
            return f()
        finally:
            backend.PHASE_TABLE_MAX_BITS, backend.PHASE_TABLE_MIN_QUBITS = keep
    return g


def kernels(rows, dtype, n, batch, reps):
    """Every row allocates its output as the yardsticks do (``scale_z_signs`` has no ``out``), except the in-place one."""
    real = torch.float32 if dtype == torch.complex64 else torch.float64
    esz = 8 if dtype == torch.complex64 else 16
    psi = torch.randn(batch, 1 << n, dtype=dtype, device='cuda')
    psi /= psi.norm(dim=-1, keepdim=True)
    other = torch.randn(batch, 1 << n, dtype=dtype, device='cuda')
    sbytes = psi.numel() * esz
    full = list(range(n - 1, -1, -1))
    cost = torch.randn(1 << n, dtype=real, device='cuda')
    diag = torch.exp(1j * cost.to(torch.float64)).to(dtype)
    t = torch.linspace(0.3, 1.7, batch, dtype=torch.float64, device='cuda')
    s = torch.complex(t, -t)
    coef = torch.ones(batch, 1, dtype=torch.float64, device='cuda')
    gbits = [n - 1, n - 3, n - 6, n - 8, 10, 9, 8, 6, 5, 4, 1, 0]
    small, dsmall = cost[:1 << len(gbits)].contiguous(), diag[:1 << len(gbits)].contiguous()
    rbits = list(range(n))
    tb = cost.numel() * esz // 2
    yard = 'scale_zsigns K=1 (yardstick)'
    apply = {
        yard: (lambda: backend.scale_z_signs(psi, [5], coef), 2 * sbytes),
        'apply_diag full': (lambda: backend.apply_diag(psi, diag, full), 2 * sbytes + 2 * tb),
        'PHASE full': (lambda: backend.apply_cost(psi, cost, t, full, (), 'phase'), 2 * sbytes + tb),
        'SCALE full': (lambda: backend.apply_cost(psi, cost, s, full, (), 'scale'), 2 * sbytes + tb),
        'PHASE full in place': (lambda: backend.apply_cost(other, cost, t, full, (), 'phase', out=other), 2 * sbytes + tb),
        'PHASE k=12 gathered, in flight': (forced('in flight', lambda: backend.apply_cost(psi, small, t, gbits, (), 'phase')), 2 * sbytes),
        'apply_diag k=12 gathered': (lambda: backend.apply_diag(psi, dsmall, gbits), 2 * sbytes),
        'PHASE bit-reversed k=n': (lambda: backend.apply_cost(psi, cost, t, rbits, (), 'phase'), 2 * sbytes + tb),
    }
    if dtype == torch.complex128:
        apply['PHASE k=12 gathered, via table'] = (forced('via table', lambda: backend.apply_cost(psi, small, t, gbits, (), 'phase')),
                                                   2 * sbytes)
    eyard = 'expect_pauli Z (yardstick)'
    reduce = {
        eyard: (lambda: backend.expect_pauli(psi, 0, 1 << 5), sbytes),
        'cost_cross bra == ket': (lambda: backend.cost_cross(psi, psi, cost, full), sbytes + tb),
        'cost_cross bra != ket': (lambda: backend.cost_cross(other, psi, cost, full), 2 * sbytes + tb),
        'cost_cross k=12 gathered': (lambda: backend.cost_cross(psi, psi, small, gbits), sbytes),
    }
    with torch.no_grad():
        for group, first in ((apply, yard), (reduce, eyard)):
            ts = timed_group({k: v[0] for k, v in group.items()}, reps)
            base = None
            for name, (_, nbytes) in group.items():
                med = row(rows, name, dtype, n, batch, ts[name], nbytes, base)
                base = med if name == first else base
    del psi, other, cost, diag
    torch.cuda.empty_cache()


def switch_sweep(rows, reps):
    """complex128 PHASE with a small table (k = 8 scattered bits), un-batched, in flight against via a table of phases, taking
    turns: where the three launches of the table route stop costing more than the double-precision sine and cosine."""
    dtype, k = torch.complex128, 8
    for n in (12, 14, 16, 18, 19, 20, 21, 22, 24):
        psi = torch.randn(1, 1 << n, dtype=dtype, device='cuda')
        bits = [n - 1, n - 3, n - 4, 6, 5, 3, 1, 0]
        cost = torch.randn(1 << k, dtype=torch.float64, device='cuda')
        t = torch.tensor([0.7], dtype=torch.float64, device='cuda')
        f = lambda: backend.apply_cost(psi, cost, t, bits, (), 'phase')  # noqa: E731
        with torch.no_grad():
            ts = timed_group({'in flight': forced('in flight', f), 'via table': forced('via table', f)}, reps)
        base = row(rows, 'PHASE k=8, in flight', dtype, n, 1, ts['in flight'], 2 * psi.numel() * 16)
        row(rows, 'PHASE k=8, via table', dtype, n, 1, ts['via table'], 2 * psi.numel() * 16, base)
        del psi


def qaoa(rows, n, reps):
    edges = [(i, j) for i in range(n) for j in range(i + 1, n)]
    table = qmath.ising_cost(n, [(1.0, list(e)) for e in edges], device='cuda')
    launches = {}
    real_run = executor.run

    def counting_run(*a, **k):
        r = real_run(*a, **k)
        launches['n'] = launches.get('n', 0) + executor.LAST_RUN['passes'] + executor.LAST_RUN['singles']
        return r

    res = {}
    for route in 'AB':
        cir = dq.QubitCircuit(n)
        cir.hlayer()
        if route == 'A':
            for e in edges:
                cir.rzz(list(e), inputs=2 * 0.37)
        else:
            cir.cost_phase(table, inputs=0.37)
        cir.rxlayer(inputs=[1.22] * n)
        cir.to('cuda')
        with torch.no_grad():
            executor.run = counting_run
            try:
                cir()
                launches.clear()
                cir()
                count = launches.get('n', 0) + (1 if route == 'B' else 0)
            finally:
                executor.run = real_run
            t = timed(lambda: cir(), reps)
            res[route] = cir().reshape(-1).clone()
        r = {'what': f'QAOA layer K_{n} route {route}', 'dtype': 'complex64', 'n': n, 'batch': 1, 'ms': round(t[0], 3),
             'ms_min': round(t[1], 3), 'ms_max': round(t[2], 3), 'launches': count, 'gates': len(cir.operators)}
        rows.append(r)
        print(f"{r['what']:<28} {t[0]:9.3f} ms  [{t[1]:.3f}, {t[2]:.3f}]  launches {count}  operators {len(cir.operators)}", flush=True)
        del cir
    err = (res['A'] - res['B']).abs().max().item()
    rows.append({'what': f'QAOA layer K_{n} routes differ by', 'max_abs': err, 'largest_amplitude': res['A'].abs().max().item()})
    print(f'  routes differ by {err:.3e} (largest amplitude {res["A"].abs().max().item():.3e})', flush=True)
    torch.cuda.empty_cache()


def main():
    quick = '--quick' in sys.argv
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    assert torch.cuda.is_available(), 'bench_diag.py measures on the GPU: there is no fallback'
    prop = torch.cuda.get_device_properties(0)
    box = {'device': prop.name, 'cus': prop.multi_processor_count, 'memory_GiB': round(prop.total_memory / 2**30, 1),
           'devices_visible': torch.cuda.device_count(), 'torch': torch.__version__, 'hip': torch.version.hip,
           'host': platform.processor() or platform.machine()}
    print('box:', json.dumps(box), flush=True)
    rows = []
    reps = 5 if quick else 11
    points = ((torch.complex64, 22, 4), (torch.complex128, 21, 4)) if quick else ((torch.complex64, 28, 4), (torch.complex128, 27, 4))
    for dtype, n, batch in points:
        kernels(rows, dtype, n, batch, reps)
    switch_sweep(rows, 5 if quick else 31)
    for n in ((16, 18) if quick else (24, 28)):
        qaoa(rows, n, 3 if quick else 7)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as fh:
            json.dump({'box': box, 'rows': rows}, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
