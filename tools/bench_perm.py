"""Basis-state permutations on the MI355X (dq_apply_permutation_*), each against
``dq_apply_diag_*`` run out of place at the same n and batch -- it moves the same bytes, state read + state written, and
is the yardstick the diagonal and the Pauli kernels were measured with -- timed in the same process on the same buffers.

1. Per path class, complex64 n = 28 and complex128 n = 27 at batch 4, seeded random bijections (u = the unit boundary,
   ``dq_permutation_local_bits``):
   LOCAL (every table bit below u; bit 0 free, bit 0 a table bit, all u low bits), the same tables through GATHER (the
   evidence for what ``DQ_PERM_AUTO`` picks), GATHER with all table bits high, GATHER with bit 0 free and table bits on
   both sides of u, GATHER with bit 0 a table bit, a controlled permutation, and a table of 2^20 entries over the 20 low
   bits (a modular multiplication's shape).
2. End to end through ``QubitCircuit`` without autograd, complex64, un-batched: a controlled ``modmul`` (one pass, nreg
   wires plus the control) against ``ControlledUa`` of the same a and N (2 nreg + 3 wires with its control) on the input
   |1>|x = 1>, the ``modmul`` both on its own small register and embedded in a register as large as ``ControlledUa``'s;
   and ``cir.any`` of the 0/1 matrix at k = 10 against ``cir.permutation`` of the same table.

Every point: one warm-up call, then the median of ``reps`` calls between device events; the rows of a group, yardstick
included, take turns within every repetition.  The box is recorded first.

usage: python tools/bench_perm.py [--quick] [--out FILE]
"""
import json
import os
import platform
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deepquantum_amd as dq  # noqa: E402
from deepquantum_amd import backend, qmath  # noqa: E402


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
    print(f"{name:<44} {r['dtype']:<10} n={n} b={batch}  {med:9.4f} ms  [{lo:.4f}, {hi:.4f}]  {r['TB_per_s']:6.3f} TB/s"
          + (f"  x{r['time_over_yardstick']:.3f} of the yardstick" if base is not None else ''), flush=True)
    return med


def bijection(k, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(1 << k, generator=g).to(torch.int32).cuda()


def kernels(rows, dtype, n, batch, reps):
    esz = 8 if dtype == torch.complex64 else 16
    u = backend.permutation_local_bits(dtype)
    psi = torch.randn(batch, 1 << n, dtype=dtype, device='cuda')
    out = torch.empty_like(psi)
    sbytes = psi.numel() * esz
    diag = torch.exp(1j * torch.linspace(0, 3, 8, dtype=torch.float64)).to(dtype).cuda()
    kbig = min(20, n - 2)
    cases = {
        # name: (bits, controls, path)
        'LOCAL bit 0 free, k=4': ((u - 1, 6, 3, 1), (), 'local'),
        'GATHER on the same': ((u - 1, 6, 3, 1), (), 'gather'),
        'LOCAL bit 0 a table bit, k=4': ((u - 1, 6, 3, 0), (), 'local'),
        'GATHER on the same (bit 0)': ((u - 1, 6, 3, 0), (), 'gather'),
        f'LOCAL all {u} low bits': (tuple(range(u - 1, -1, -1)), (), 'local'),
        f'GATHER on the same ({u} low bits)': (tuple(range(u - 1, -1, -1)), (), 'gather'),
        'LOCAL k=4, control on n-3': ((u - 1, 6, 3, 1), (n - 3,), 'local'),
        'GATHER all table bits high, k=8': (tuple(range(n - 1, n - 9, -1)), (), 'gather'),
        'GATHER bit 0 free, bits on both sides of u': ((n - 1, u + 1, u, u - 1, u - 2, 3), (), 'gather'),
        'GATHER bit 0 a table bit': ((n - 1, u, 3, 0), (), 'gather'),
        'GATHER k=8 high, control on bit 4': (tuple(range(n - 1, n - 9, -1)), (4,), 'gather'),
        f'GATHER {kbig} low bits (a 2^{kbig} table), control on top': (tuple(range(kbig - 1, -1, -1)), (n - 1,), 'gather'),
    }
    yard = 'apply_diag out of place (yardstick)'
    fns = {yard: lambda: backend.apply_diag(psi, diag, (5, n - 2, 2), out=out)}
    for i, (name, (bits, controls, path)) in enumerate(cases.items()):
        src = bijection(len(bits), 100 + i)
        fns[name] = (lambda s=src, b=bits, c=controls, p=path: backend.apply_permutation(psi, s, b, c, out=out, path=p))
    with torch.no_grad():
        ts = timed_group(fns, reps)
    base = row(rows, yard, dtype, n, batch, ts[yard], 2 * sbytes)
    for name in cases:
        row(rows, name, dtype, n, batch, ts[name], 2 * sbytes, base)
    del psi, out
    torch.cuda.empty_cache()


def circuit_row(rows, what, cir, t, extra=None):
    r = {'what': what, 'dtype': 'complex64', 'qubits': cir.nqubit, 'operators': len(cir.operators), 'ms': round(t[0], 3),
         'ms_min': round(t[1], 3), 'ms_max': round(t[2], 3)}
    r.update(extra or {})
    rows.append(r)
    print(f"{what:<58} qubits {cir.nqubit:3d}  operators {len(cir.operators):6d}  {t[0]:10.3f} ms  [{t[1]:.3f}, {t[2]:.3f}]",
          flush=True)


def modular_multiplication(rows, mod, a, reps):
    """|c>|x> -> |c>|a^c x mod N>: ControlledUa on 2 nreg + 3 wires against one permutation pass."""
    nreg = mod.bit_length()
    nq = 2 * nreg + 3
    circuits = {}
    for name, width in (('ControlledUa', nq), ('modmul, register of its own', nreg + 1), ('modmul, in the register of ControlledUa', nq)):
        cir = dq.QubitCircuit(width)
        cir.x(0)                                        # the control is set
        cir.x(nreg)                                     # x = 1
        if name == 'ControlledUa':
            cir.add(dq.ControlledUa(nq, a, mod, [1, nreg], list(range(nreg + 1, 2 * nreg + 3)), controls=[0]))
        else:
            cir.modmul(a, mod, wires=list(range(1, nreg + 1)), controls=[0])
        circuits[name] = cir
    res = {}
    with torch.no_grad():
        for name, cir in circuits.items():
            cir.to('cuda')
            t = timed_group({'f': lambda c=cir: c()}, reps)['f']
            # |1>|x = 1> -> |1>|a mod N>: the outcome of the first nreg + 1 wires with the largest probability
            p = (cir().reshape(1 << (nreg + 1), -1).abs() ** 2).sum(dim=1)
            res[name] = (int(p.argmax()) & ((1 << nreg) - 1), p.max().item())
            circuit_row(rows, f'controlled x -> {a} x mod {mod}: {name}', cir, t,
                        {'mod': mod, 'a': a, 'x_out_for_x_in_1': res[name][0], 'its_probability': round(res[name][1], 6)})
    print(f'  |1>|1> -> |1>|x>, x (probability) per route: {res}; a mod N = {a % mod}', flush=True)
    del circuits
    torch.cuda.empty_cache()


def dense_against_permutation(rows, n, k, reps):
    g = torch.Generator().manual_seed(5)
    perm = torch.randperm(1 << k, generator=g)
    m = torch.zeros(1 << k, 1 << k, dtype=torch.complex64)
    m[perm, torch.arange(1 << k)] = 1
    wires = list(range(n - k - 2, n - 2))
    res = {}
    with torch.no_grad():
        for name in ('cir.any of the 0/1 matrix', 'cir.permutation'):
            cir = dq.QubitCircuit(n)
            cir.hlayer()
            cir.rylayer(inputs=[0.1 * (i + 1) for i in range(n)])
            if name == 'cir.permutation':
                cir.permutation(perm, wires=wires)
            else:
                cir.any(m, wires=wires)
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


def main():
    quick = '--quick' in sys.argv
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    assert torch.cuda.is_available(), 'bench_perm.py measures on the GPU: there is no fallback'
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
    dense_against_permutation(rows, 16 if quick else 26, 10, 3 if quick else 7)
    # the largest modulus for which ControlledUa's register (2 nreg + 3 wires) fits comfortably: 12 bits, 27 wires
    mod, a = (13, 7) if quick else (4093, 1234)
    assert qmath.modmul_table(a, mod, mod.bit_length()) is not None
    modular_multiplication(rows, mod, a, 3 if quick else 5)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as fh:
            json.dump({'box': box, 'rows': rows}, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
