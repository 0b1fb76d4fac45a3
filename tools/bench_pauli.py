"""Pauli-string kernels on the MI355X (dq_apply_pauli_axpby_*, dq_pauli_cross_*), each against a
kernel of the parent library with the same traffic, timed in the same process on the same buffers.

1. ``apply_pauli_axpby`` out of place, complex64 n = 28 and complex128 n = 27 at batch 4 -- bytes = state read + state
   written -- for xmask = 0 (a Z string), bit 0 (inside the 16-byte vector for complex64), a bit inside a unit of 1024
   vectors, the top bit, all ones, and the top-bit row in place, against ``dq_scale_zsigns_*`` with one string (state
   read + state written).
2. ``pauli_cross`` with bra == ket (state read) and bra != ket (two states read) against ``dq_expect_pauli_*`` with a Z
   mask (state read).
3. One rotation exp(-i theta/2 P) of weight 12 and of weight 28 at n = 28, un-batched complex64, end to end through
   ``QubitCircuit`` without autograd: route A = the hand decomposition (basis change, CNOT ladder, rz, undone) through
   fused passes; route B = ``cir.pauli_rot``; with the number of launches each takes: every device kernel of one
   forward, counted in a profiler trace of it (taken apart from the timed calls), and beside it how many of them are
   passes over the state (fused passes, single gates, the Pauli pass).

Every point: one warm-up call, then the median of ``reps`` calls between device events; the rows of a group, yardstick
included, take turns within every repetition.  The box is recorded first.

usage: python tools/bench_pauli.py [--quick] [--out FILE]
"""
import json
import os
import platform
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deepquantum_amd as dq  # noqa: E402
from deepquantum_amd import backend, executor  # noqa: E402


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
    print(f"{name:<34} {r['dtype']:<10} n={n} b={batch}  {med:9.4f} ms  [{lo:.4f}, {hi:.4f}]  {r['TB_per_s']:6.3f} TB/s"
          + (f"  x{r['time_over_yardstick']:.3f} of the yardstick" if base is not None else ''), flush=True)
    return med


def kernels(rows, dtype, n, batch, reps):
    """Every row allocates its output as the yardstick does (``scale_z_signs`` has no ``out``), except the in-place one."""
    esz = 8 if dtype == torch.complex64 else 16
    psi = torch.randn(batch, 1 << n, dtype=dtype, device='cuda')
    psi /= psi.norm(dim=-1, keepdim=True)
    other = torch.randn(batch, 1 << n, dtype=dtype, device='cuda')
    sbytes = psi.numel() * esz
    t = torch.linspace(0.3, 1.7, batch, dtype=torch.float64, device='cuda')
    a, c = torch.complex(torch.cos(t), 0 * t), torch.complex(0 * t, -torch.sin(t))
    coef = torch.ones(batch, 1, dtype=torch.float64, device='cuda')
    top, ones, z = 1 << (n - 1), (1 << n) - 1, 1 << 5 | 1 << (n - 2)
    yard = 'scale_zsigns K=1 (yardstick)'
    apply = {
        yard: (lambda: backend.scale_z_signs(psi, [1 << 5], coef), 2 * sbytes),
        'axpby xmask = 0 (Z string)': (lambda: backend.apply_pauli_axpby(psi, 0, z, a, c), 2 * sbytes),
        'axpby xmask bit 0': (lambda: backend.apply_pauli_axpby(psi, 1, z, a, c), 2 * sbytes),
        'axpby xmask bit 1': (lambda: backend.apply_pauli_axpby(psi, 2, z, a, c), 2 * sbytes),
        'axpby xmask bit 7 (inside a unit)': (lambda: backend.apply_pauli_axpby(psi, 1 << 7, z, a, c), 2 * sbytes),
        'axpby xmask top bit': (lambda: backend.apply_pauli_axpby(psi, top, z, a, c), 2 * sbytes),
        'axpby xmask all ones': (lambda: backend.apply_pauli_axpby(psi, ones, z, a, c), 2 * sbytes),
        'axpby xmask top bit, in place': (lambda: backend.apply_pauli_axpby(other, top, z, a, c, out=other), 2 * sbytes),
        'axpby top bit, control on n-3': (lambda: backend.apply_pauli_axpby(psi, top, 1 << 5, a, c, (n - 3,)), 2 * sbytes),
    }
    eyard = 'expect_pauli Z (yardstick)'
    reduce = {
        eyard: (lambda: backend.expect_pauli(psi, 0, 1 << 5), sbytes),
        'pauli_cross bra == ket, Z string': (lambda: backend.pauli_cross(psi, psi, 0, z), sbytes),
        'pauli_cross bra == ket, top bit': (lambda: backend.pauli_cross(psi, psi, top, z), sbytes),
        'pauli_cross bra == ket, all ones': (lambda: backend.pauli_cross(psi, psi, ones, z), sbytes),
        'pauli_cross bra != ket, top bit': (lambda: backend.pauli_cross(other, psi, top, z), 2 * sbytes),
        'pauli_cross bra != ket, bit 0': (lambda: backend.pauli_cross(other, psi, 1, z), 2 * sbytes),
    }
    with torch.no_grad():
        for group, first in ((apply, yard), (reduce, eyard)):
            ts = timed_group({k: v[0] for k, v in group.items()}, reps)
            base = None
            for name, (_, nbytes) in group.items():
                med = row(rows, name, dtype, n, batch, ts[name], nbytes, base)
                base = med if name == first else base
    del psi, other
    torch.cuda.empty_cache()


def count_kernels(f):
    """The device kernels one call of ``f`` launches, counted in the profiler's trace of that call: every kernel, the
    element-wise ones on one-element tensors included (copies and fills done by the runtime are not kernels)."""
    from torch.profiler import ProfilerActivity, profile

    f()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        f()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    count = sum(1 for name in names if not name.lower().startswith(('memcpy', 'memset')))
    assert count > 0, 'the profiler recorded no device kernel'
    return count


def by_hand(cir, letters, wires, theta):
    """exp(-i theta/2 P) = B^dagger L^dagger rz(theta) L B: the basis change B (h for x, sdg then h for y) and the CNOT
    ladder L onto the last wire of the string."""
    for ch, w in zip(letters, wires):
        if ch == 'y':
            cir.sdg(w)
        if ch in 'xy':
            cir.h(w)
    for p, q in zip(wires[:-1], wires[1:]):
        cir.cnot(p, q)
    cir.rz(wires[-1], inputs=theta)
    for p, q in reversed(list(zip(wires[:-1], wires[1:]))):
        cir.cnot(p, q)
    for ch, w in zip(letters, wires):
        if ch in 'xy':
            cir.h(w)
        if ch == 'y':
            cir.s(w)


def rotation(rows, n, weight, reps):
    wires = list(range(n)) if weight == n else sorted(list(range(0, n, 2))[:weight // 2] + list(range(n - 1, 0, -2))[:weight - weight // 2])
    letters = ('xyzzyx' * n)[:weight]
    theta = 0.83
    passes = {}
    real_run = executor.run

    def counting_run(*a, **k):
        r = real_run(*a, **k)
        passes['n'] = passes.get('n', 0) + executor.LAST_RUN['passes'] + executor.LAST_RUN['singles']
        return r

    res = {}
    for route in 'AB':
        cir = dq.QubitCircuit(n)
        cir.hlayer()
        cir.rylayer(inputs=[0.1 * (i + 1) for i in range(n)])
        if route == 'A':
            by_hand(cir, letters, wires, theta)
        else:
            cir.pauli_rot(letters, wires=wires, inputs=theta)
        cir.to('cuda')
        with torch.no_grad():
            executor.run = counting_run
            try:
                cir()
                passes.clear()
                cir()
                count = passes.get('n', 0) + sum(isinstance(op, dq.PauliRot) for op in cir.operators)
            finally:
                executor.run = real_run
            kernels = count_kernels(lambda: cir())
            t = timed_group({'f': lambda: cir()}, reps)['f']
            res[route] = cir().reshape(-1).clone()
        r = {'what': f'weight-{weight} rotation route {route}', 'dtype': 'complex64', 'n': n, 'batch': 1, 'ms': round(t[0], 3),
             'ms_min': round(t[1], 3), 'ms_max': round(t[2], 3), 'launches': kernels, 'state_passes': count, 'gates': len(cir.operators)}
        rows.append(r)
        print(f"{r['what']:<30} {t[0]:9.3f} ms  [{t[1]:.3f}, {t[2]:.3f}]  launches {kernels} (of them passes over the state: {count})  "
              f"operators {len(cir.operators)}", flush=True)
        del cir
    err = (res['A'] - res['B']).abs().max().item()
    rows.append({'what': f'weight-{weight} rotation routes differ by', 'max_abs': err, 'largest_amplitude': res['A'].abs().max().item()})
    print(f'  routes differ by {err:.3e} (largest amplitude {res["A"].abs().max().item():.3e})', flush=True)
    del res
    torch.cuda.empty_cache()


def main():
    quick = '--quick' in sys.argv
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    assert torch.cuda.is_available(), 'bench_pauli.py measures on the GPU: there is no fallback'
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
    n = 18 if quick else 28
    for weight in (12, n):
        rotation(rows, n, weight, 3 if quick else 7)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as fh:
            json.dump({'box': box, 'rows': rows}, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
