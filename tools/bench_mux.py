"""Multiplexed one-qubit gates on the MI355X (dq_apply_mux_*).

1. Kernel rows, complex64 n = 28 and complex128 n = 27 at batch 4, against two yardsticks timed in the same process on the
   same buffers, which both move the same state bytes: ``dq_apply_diag_*`` out of place, and ``dq_apply_pauli_axpby_*`` in
   GATE mode with ``xmask = 1 << target`` (the same pairs, no table) out of place and in place.  P = log2 of the pairs of
   a unit (11 / 10).  Rows: RY and U tables with k = 4 and k = 10 (the table stays in cache); the target low, across the
   unit and high; select bits on both sides of the target and of the unit; bit 0 as a select; one control (low, and high:
   half of the units are skipped); complex64 with the target at bit 0; in place against out of place; and k = n - 1 for
   RY and U, where the table streams with the state -- those rows are reported against the bytes actually moved, state
   plus table.
2. End to end through ``QubitCircuit`` without autograd, complex64, un-batched: the eigenvalue-rotation loop of
   ``ansatz.HHL`` as it is built today (X flips, one ``ry`` controlled on all counting wires, X flips back, for every
   register value) against one ``ucry``, at ncount = 8, 10, 12 on 1 + ncount + 1 wires (``--loop-only`` times the loop
   alone and uses nothing this gate added, so that it also runs on an older checkout); ``cir.any`` of the block-diagonal
   matrix on 10 wires at n = 26 against ``cir.multiplexer`` with k = 9; ``prepare_state`` of a 2^20-entry vector on 20
   of 26 wires.

3. The trainable rotations (``--cross-only`` runs these alone): ``dq_mux_cross_*``, the binned reduction behind the angle
   gradients, at the same sizes against ``dq_pauli_cross_*`` with ``xmask = 1 << target`` on the same buffers -- k = 4 and
   k = 10 with the selects low, high and across the unit, k = n - 1, ``bra is ket``, a high control -- and a forward plus
   backward of a trainable ``ucry`` (k = 9, n = 26) against a forward plus backward of ``cir.pauli_rot('y')`` on the same
   target.

Every point: one warm-up call, then the median of ``reps`` calls between device events; the rows of a group, yardsticks
included, take turns within every repetition.  The box is recorded first.

usage: python tools/bench_mux.py [--quick] [--loop-only] [--cross-only] [--out FILE]
"""
import json
import math
import os
import platform
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deepquantum_amd as dq  # noqa: E402
from deepquantum_amd import backend  # noqa: E402


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


def row(rows, name, dtype, n, batch, t, nbytes, bases=None):
    med, lo, hi = t
    r = {'what': name, 'dtype': str(dtype)[6:], 'n': n, 'batch': batch, 'ms': round(med, 4), 'ms_min': round(lo, 4),
         'ms_max': round(hi, 4), 'bytes': nbytes, 'TB_per_s': round(nbytes / med / 1e9, 3)}
    text = ''
    for key, base in (bases or {}).items():
        r[key] = round(med / base, 3)
        text += f'  x{r[key]:.3f} {key[10:]}'
    rows.append(r)
    print(f"{name:<58} {r['dtype']:<10} n={n} b={batch} {med:9.4f} ms [{lo:.4f}, {hi:.4f}] {r['TB_per_s']:6.3f} TB/s{text}", flush=True)
    return med


def tables(kind, k, dtype, seed):
    """2^k random rotations as rows (c, s), or random unitaries u00 u01 u10 u11, in the state's precision on the device."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    real = torch.float32 if dtype == torch.complex64 else torch.float64
    half = torch.rand(1 << k, generator=g, device='cuda', dtype=real) * (2 * math.pi)
    c, s = torch.cos(half), torch.sin(half)
    if kind == 'ry':
        return torch.stack([c, s], dim=-1).contiguous()
    ph = torch.exp(1j * torch.rand(1 << k, 2, generator=g, device='cuda', dtype=real) * (2 * math.pi)).to(dtype)
    a, b = c * ph[:, 0], s * ph[:, 1]
    return torch.stack([a, -b.conj(), b, a.conj()], dim=-1).reshape(-1, 2, 2).contiguous()


def kernels(rows, dtype, n, batch, reps):
    esz = 8 if dtype == torch.complex64 else 16
    p = 11 if dtype == torch.complex64 else 10
    psi = torch.randn(batch, 1 << n, dtype=dtype, device='cuda')
    out = torch.empty_like(psi)
    work = psi.clone()                                  # the in-place rows run on a buffer of their own
    sbytes = psi.numel() * esz
    diag = torch.exp(1j * torch.linspace(0, 3, 8, dtype=torch.float64)).to(dtype).cuda()
    lo_t, mid_t, hi_t = 3, p, n - 2
    k10_low = tuple(q for q in range(11, -1, -1) if q != lo_t)[:10]
    cases = {
        # name: (kind, target, bits, controls, in place)
        'RY k=4, target low, selects on both sides': ('ry', lo_t, (n - 1, p + 1, 6, 1), (), False),
        'RY k=4, target at the top bit of a unit': ('ry', mid_t, (n - 1, p + 1, 6, 1), (), False),
        'RY k=4, target high': ('ry', hi_t, (n - 1, p + 1, 6, 1), (), False),
        'RY k=4, target high, in place': ('ry', hi_t, (n - 1, p + 1, 6, 1), (), True),
        'RY k=4, target low, in place': ('ry', lo_t, (n - 1, p + 1, 6, 1), (), True),
        'RY k=4, bit 0 a select': ('ry', lo_t, (n - 1, p + 1, 6, 0), (), False),
        'RY k=4, target at bit 0': ('ry', 0, (n - 1, p + 1, 6, 1), (), False),
        'RY k=4, one low control': ('ry', lo_t, (n - 1, p + 1, 6, 1), (5,), False),
        'RY k=4, one high control, in place (half the units skipped)': ('ry', lo_t, (p + 1, 6, 1, 2), (n - 1,), True),
        'RY k=10, low selects (lane bits)': ('ry', lo_t, k10_low, (), False),
        'RY k=10, high selects (unit bits)': ('ry', lo_t, tuple(range(n - 1, n - 11, -1)), (), False),
        'RY k=10, selects across the unit, target across': ('ry', mid_t, tuple(range(p + 6, p, -1)) + tuple(range(p - 1, p - 5, -1)), (), False),
        'U k=4, target low, selects on both sides': ('u', lo_t, (n - 1, p + 1, 6, 1), (), False),
        'U k=4, target at the top bit of a unit': ('u', mid_t, (n - 1, p + 1, 6, 1), (), False),
        'U k=4, target high': ('u', hi_t, (n - 1, p + 1, 6, 1), (), False),
        'U k=4, target high, in place': ('u', hi_t, (n - 1, p + 1, 6, 1), (), True),
        'U k=4, bit 0 a select': ('u', lo_t, (n - 1, p + 1, 6, 0), (), False),
        'U k=4, target at bit 0': ('u', 0, (n - 1, p + 1, 6, 1), (), False),
        'U k=4, one low control': ('u', lo_t, (n - 1, p + 1, 6, 1), (5,), False),
        'U k=10, low selects (lane bits)': ('u', lo_t, k10_low, (), False),
        'U k=10, high selects (unit bits)': ('u', lo_t, tuple(range(n - 1, n - 11, -1)), (), False),
        'RY k=n-1, target low (table streams)': ('ry', lo_t, tuple(q for q in range(n - 1, -1, -1) if q != lo_t), (), False),
        'RY k=n-1, target high (table streams)': ('ry', hi_t, tuple(q for q in range(n - 1, -1, -1) if q != hi_t), (), False),
        'RY k=n-1, target high, in place': ('ry', hi_t, tuple(q for q in range(n - 1, -1, -1) if q != hi_t), (), True),
        'U k=n-1, target low (table streams)': ('u', lo_t, tuple(q for q in range(n - 1, -1, -1) if q != lo_t), (), False),
        'U k=n-1, target high (table streams)': ('u', hi_t, tuple(q for q in range(n - 1, -1, -1) if q != hi_t), (), False),
    }
    yd = 'apply_diag out of place (yardstick)'
    fns = {yd: lambda: backend.apply_diag(psi, diag, (5, n - 2, 2), out=out)}
    pauli = {}
    for t in (0, lo_t, mid_t, hi_t):
        for inplace in (False, True):
            name = f"pauli axpby GATE xmask=1<<{t}{', in place' if inplace else ''} (yardstick)"
            pauli[(t, inplace)] = name
            fns[name] = (lambda t=t, i=inplace: backend.apply_pauli_axpby(work if i else psi, 1 << t, 0, 0.6, 0.8j,
                                                                          out=work if i else out))
    tabs = {}
    for i, (name, (kind, t, bits, controls, inplace)) in enumerate(cases.items()):
        key = (kind, len(bits))
        if key not in tabs:
            tabs[key] = tables(kind, len(bits), dtype, 100 + i)
        tab = tabs[key]
        fns[name] = (lambda tab=tab, kd=kind, t=t, b=bits, c=controls, i=inplace:
                     backend.apply_mux(work if i else psi, tab, kd, t, b, c, out=work if i else out))
    with torch.no_grad():
        ts = timed_group(fns, reps)
    base = row(rows, yd, dtype, n, batch, ts[yd], 2 * sbytes)
    pbase = {}
    for key, name in pauli.items():
        pbase[key] = row(rows, name, dtype, n, batch, ts[name], 2 * sbytes, {'time_over_diag': base})
    for name, (kind, t, bits, controls, inplace) in cases.items():
        tab = tabs[(kind, len(bits))]
        tbytes = tab.numel() * tab.element_size()
        moved = 2 * sbytes + (tbytes if len(bits) == n - 1 else 0)
        if controls and max(controls) >= p + 2 and inplace:
            moved = sbytes                              # half of the units are neither read nor written
        row(rows, name, dtype, n, batch, ts[name], moved, {'time_over_diag': base, 'time_over_pauli': pbase[(t, inplace)]})
        rows[-1]['table_bytes'] = tbytes
    del psi, out, work, tabs
    torch.cuda.empty_cache()


def cross_kernels(rows, dtype, n, batch, reps):
    """``dq_mux_cross_*`` (the binned reduction behind the angle gradients) against ``dq_pauli_cross_*`` with
    ``xmask = 1 << target`` on the same buffers, which makes the same reads and returns one number per sample."""
    esz = 8 if dtype == torch.complex64 else 16
    p = 11 if dtype == torch.complex64 else 10
    ket = torch.randn(batch, 1 << n, dtype=dtype, device='cuda')
    bra = torch.randn(batch, 1 << n, dtype=dtype, device='cuda')
    sbytes = ket.numel() * esz
    t = 3
    low = tuple(q for q in range(11, -1, -1) if q != t)
    across = tuple(range(p + 6, p, -1)) + tuple(range(p - 1, p - 5, -1))
    cases = {
        # name: (bits, controls, bra is ket)
        'cross k=4, selects low': (low[-4:], (), False),
        'cross k=10, selects low': (low[:10], (), False),
        'cross k=4, selects high': (tuple(range(n - 1, n - 5, -1)), (), False),
        'cross k=10, selects high': (tuple(range(n - 1, n - 11, -1)), (), False),
        'cross k=4, selects across the unit': (across[3:7], (), False),
        'cross k=10, selects across the unit': (across, (), False),
        'cross k=n-1': (tuple(q for q in range(n - 1, -1, -1) if q != t), (), False),
        'cross k=4, selects low, bra is ket': (low[-4:], (), True),
        'cross k=10, selects across the unit, bra is ket': (across, (), True),
        'cross k=4, selects low, one high control': (low[-4:], (n - 1,), False),
    }
    yards = {(False, ()): 'pauli_cross xmask=1<<3 (yardstick)', (True, ()): 'pauli_cross xmask=1<<3, bra is ket (yardstick)',
             (False, (n - 1,)): 'pauli_cross xmask=1<<3, one high control (yardstick)'}
    fns = {name: (lambda s=same, c=controls: backend.pauli_cross(ket if s else bra, ket, 1 << t, 0, c))
           for (same, controls), name in yards.items()}
    for name, (bits, controls, same) in cases.items():
        fns[name] = lambda b=bits, c=controls, s=same: backend.mux_cross(ket if s else bra, ket, 'y', t, b, c)
    with torch.no_grad():
        ts = timed_group(fns, reps)
    moved = lambda same, controls: (1 if same else 2) * sbytes // (2 if controls else 1)  # noqa: E731
    base = {key: row(rows, name, dtype, n, batch, ts[name], moved(*key)) for key, name in yards.items()}
    for name, (bits, controls, same) in cases.items():
        row(rows, name, dtype, n, batch, ts[name], moved(same, controls), {'time_over_pauli_cross': base[(same, controls)]})
    del ket, bra
    torch.cuda.empty_cache()


def trainable_ucry(rows, n, k, reps):
    """Forward plus backward of a trainable ``ucry`` with k select wires against a forward plus backward of
    ``cir.pauli_rot('y')`` on the same target (one rotation and one cross), complex64, un-batched, from |0..0> behind a
    layer of Hadamards."""
    res = {}
    for name in ("pauli_rot('y') forward + backward", f'trainable ucry k={k} forward + backward'):
        cir = dq.QubitCircuit(n)
        cir.hlayer()
        if name.startswith('pauli'):
            cir.pauli_rot('y', wires=[n - 3])
        else:
            cir.ucry(wires=list(range(k)) + [n - 3], requires_grad=True)
        cir.observable(n - 3)
        cir.to('cuda')

        def step(c=cir):
            c.zero_grad(set_to_none=True)
            c()
            c.expectation().sum().backward()

        res[name] = (cir, step)
    ts = timed_group({name: step for name, (_, step) in res.items()}, reps)
    names = list(res)
    circuit_row(rows, f'n = {n}: {names[0]}', res[names[0]][0], ts[names[0]])
    circuit_row(rows, f'n = {n}: {names[1]}', res[names[1]][0], ts[names[1]],
                {'time_over_pauli_rot': round(ts[names[1]][0] / ts[names[0]][0], 3)})
    print(f'  x{ts[names[1]][0] / ts[names[0]][0]:.3f} pauli_rot', flush=True)
    del res
    torch.cuda.empty_cache()


def circuit_row(rows, what, cir, t, extra=None):
    r = {'what': what, 'dtype': 'complex64', 'qubits': cir.nqubit, 'operators': len(cir.operators), 'ms': round(t[0], 3),
         'ms_min': round(t[1], 3), 'ms_max': round(t[2], 3)}
    r.update(extra or {})
    rows.append(r)
    print(f"{what:<62} qubits {cir.nqubit:3d}  operators {len(cir.operators):6d}  {t[0]:10.3f} ms  [{t[1]:.3f}, {t[2]:.3f}]",
          flush=True)


def hhl_loop(ncount):
    """The eigenvalue rotation of ``ansatz.HHL``, gate for gate, and nothing else of it: wire 0 the ancilla, wires
    1 .. ncount the counting register (its least significant bit on wire 1), one more wire for |b>."""
    cir = dq.QubitCircuit(1 + ncount + 1)
    cir.hlayer()
    counting = list(range(1, ncount + 1))
    for value in range(2**ncount):
        zeros = [1 + j for j in range(ncount) if not (value >> j) & 1]
        for w in zeros:
            cir.x(w)
        cir.ry(0, inputs=2 * torch.pi * value / 2**ncount, controls=counting)
        for w in zeros:
            cir.x(w)
    return cir


def hhl_rotation(rows, ncount, reps, loop_only):
    res = {}
    with torch.no_grad():
        for name in ('the loop of HHL',) + (() if loop_only else ('one ucry',)):
            t0 = time.perf_counter()
            if name == 'one ucry':
                cir = dq.QubitCircuit(1 + ncount + 1)
                cir.hlayer()
                cir.ucry([2 * torch.pi * v / 2**ncount for v in range(2**ncount)], wires=list(range(ncount, 0, -1)) + [0])
            else:
                cir = hhl_loop(ncount)
            cir.to('cuda')
            built = time.perf_counter() - t0
            t = timed_group({'f': lambda c=cir: c()}, reps)['f']
            circuit_row(rows, f'HHL rotation, ncount = {ncount}: {name}', cir, t, {'ncount': ncount, 'build_s': round(built, 2)})
            res[name] = cir().reshape(-1).clone()
            del cir
    if len(res) == 2:
        a, b = res.values()
        err = (a - b).abs().max().item()
        rows.append({'what': f'HHL rotation, ncount = {ncount}: routes differ by', 'max_abs': err, 'largest_amplitude': a.abs().max().item()})
        print(f'  routes differ by {err:.3e} (largest amplitude {a.abs().max().item():.3e})', flush=True)
    torch.cuda.empty_cache()


def dense_against_multiplexer(rows, n, k, reps):
    blocks = tables('u', k, torch.complex64, 5).cpu()
    wires = list(range(n - k - 3, n - 2))
    res = {}
    with torch.no_grad():
        for name in ('cir.any of the block-diagonal matrix', 'cir.multiplexer'):
            cir = dq.QubitCircuit(n)
            cir.hlayer()
            cir.rylayer(inputs=[0.1 * (i + 1) for i in range(n)])
            if name == 'cir.multiplexer':
                cir.multiplexer(blocks, wires=wires)
            else:
                cir.any(torch.block_diag(*blocks), wires=wires)
            cir.to('cuda')
            t = timed_group({'f': lambda c=cir: c()}, reps)['f']
            circuit_row(rows, f'k = {k} on n = {n}: {name}', cir, t)
            res[name] = cir().reshape(-1).clone()
            del cir
    a, b = res.values()
    err = (a - b).abs().max().item()
    rows.append({'what': f'k = {k} routes differ by', 'max_abs': err, 'largest_amplitude': a.abs().max().item()})
    print(f'  routes differ by {err:.3e} (largest amplitude {a.abs().max().item():.3e})', flush=True)
    torch.cuda.empty_cache()


def prepare(rows, n, k, reps):
    g = torch.Generator().manual_seed(9)
    phi = torch.randn(1 << k, dtype=torch.float64, generator=g) + 1j * torch.randn(1 << k, dtype=torch.float64, generator=g)
    wires = list(range(3, 3 + k))
    with torch.no_grad():
        t0 = time.perf_counter()
        cir = dq.QubitCircuit(n)
        cir.prepare_state(phi, wires=wires)
        cir.to('cuda')
        built = time.perf_counter() - t0
        t = timed_group({'f': lambda: cir()}, reps)['f']
        got = cir().reshape(1 << 3, 1 << k, -1)[0, :, 0].to(torch.complex128).cpu()
    err = (got - phi / phi.norm()).abs().max().item()
    circuit_row(rows, f'prepare_state of 2^{k} entries on {k} of {n} wires', cir, t,
                {'build_s': round(built, 2), 'max_abs_error': err, 'largest_amplitude': (phi / phi.norm()).abs().max().item()})
    print(f'  reaches the vector to {err:.3e} (largest amplitude {(phi / phi.norm()).abs().max().item():.3e})', flush=True)
    torch.cuda.empty_cache()


def main():
    quick = '--quick' in sys.argv
    loop_only = '--loop-only' in sys.argv
    cross_only = '--cross-only' in sys.argv
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    assert torch.cuda.is_available(), 'bench_mux.py measures on the GPU: there is no fallback'
    prop = torch.cuda.get_device_properties(0)
    box = {'device': prop.name, 'cus': prop.multi_processor_count, 'memory_GiB': round(prop.total_memory / 2**30, 1),
           'devices_visible': torch.cuda.device_count(), 'torch': torch.__version__, 'hip': torch.version.hip,
           'host': platform.processor() or platform.machine()}
    print('box:', json.dumps(box), flush=True)
    rows = []
    reps = 5 if quick else 11
    points = ((torch.complex64, 22, 4), (torch.complex128, 21, 4)) if quick else ((torch.complex64, 28, 4), (torch.complex128, 27, 4))
    if not loop_only:
        for dtype, n, batch in points:
            cross_kernels(rows, dtype, n, batch, reps)
        trainable_ucry(rows, 16 if quick else 26, 9, 3 if quick else 7)
    if not loop_only and not cross_only:
        for dtype, n, batch in points:
            kernels(rows, dtype, n, batch, reps)
        dense_against_multiplexer(rows, 16 if quick else 26, 9, 3 if quick else 7)
        prepare(rows, 16 if quick else 26, 10 if quick else 20, 3 if quick else 7)
    for ncount in () if cross_only else ((4, 6) if quick else (8, 10, 12)):
        hhl_rotation(rows, ncount, 3 if quick else 5, loop_only)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as fh:
            json.dump({'box': box, 'rows': rows}, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
