"""SELECT over Pauli strings on the MI355X (dq_apply_select_pauli_*), each case against
``dq_apply_permutation_*`` on its gather path over the same table bits -- out of place as well, one read and one write of
the state, the same traffic -- timed in the same process on the same buffers.

1. Per case, complex64 n = 28 and complex128 n = 27 at batch 4, seeded random strings over the free bits (u = the unit
   boundary, ``dq_select_pauli_unit_bits``):
   UNIFORM (every select bit at or above u; k = 7 on the top bits, the same under a control), LANE (select bits below u
   with bit 0 free; bits on both sides of u), SPLIT (bit 0 a select bit; complex128 runs the same bits through LANE), and
   the two low-bit cases again with diagonal strings (x = 0: no vector leaves its place), which separates the kernel's
   table loads and arithmetic from the access pattern of strings that flip bits anywhere in the register.
2. End to end through ``QubitCircuit`` without autograd, complex64, un-batched, 28 wires = 7 select + 21 system wires: the
   Heisenberg chain ``sum J (XX + YY + ZZ)`` on 21 wires in a field ``h sum Z`` -- 60 + 21 = 81 strings -- as one
   ``cir.select_pauli`` against the loop the package offered before: one controlled ``cir.pauli_rot(pi)`` per string
   between X gates for the zero bits of s, and one ``cir.diagonal`` on the select wires for the phases.  And one
   ``cir.block_encode`` of the same chain.

Every point: one warm-up call, then the median of ``reps`` calls between device events; the rows of a group, yardstick
included, take turns within every repetition.  The box is recorded first.

usage: python tools/bench_select.py [--quick] [--out FILE]
"""
import json
import math
import os
import platform
import sys

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


def row(rows, name, dtype, n, batch, t, nbytes, base=None):
    med, lo, hi = t
    r = {'what': name, 'dtype': str(dtype)[6:], 'n': n, 'batch': batch, 'ms': round(med, 4), 'ms_min': round(lo, 4),
         'ms_max': round(hi, 4), 'bytes': nbytes, 'TB_per_s': round(nbytes / med / 1e9, 3)}
    if base is not None:
        r['time_over_permutation_gather'] = round(med / base, 3)
    rows.append(r)
    print(f"{name:<58} {r['dtype']:<10} n={n} b={batch}  {med:9.4f} ms  [{lo:.4f}, {hi:.4f}]  {r['TB_per_s']:6.3f} TB/s"
          + (f"  x{r['time_over_permutation_gather']:.3f} of the permutation" if base is not None else ''), flush=True)
    return med


def random_table(n, bits, controls, seed, flips=True):
    """2^k random strings over the free bits with random powers of i; ``flips=False``: diagonal strings (x = 0), so that
    every vector is its own partner -- the kernel's table loads and arithmetic without the gather's access pattern."""
    g = torch.Generator().manual_seed(seed)
    free = sum(1 << p for p in range(n) if p not in bits and p not in controls)
    draw = lambda: int(torch.randint(0, 1 << 62, (1,), generator=g)) & free
    return backend.SelectTable(n, [(draw() if flips else 0, draw(), int(torch.randint(0, 4, (1,), generator=g)))
                                   for _ in range(1 << len(bits))])


def kernels(rows, dtype, n, batch, reps):
    esz = 8 if dtype == torch.complex64 else 16
    u = backend.select_pauli_unit_bits(dtype)
    psi = torch.randn(batch, 1 << n, dtype=dtype, device='cuda')
    out = torch.empty_like(psi)
    sbytes = psi.numel() * esz
    cases = {
        # name: (bits, controls)
        'UNIFORM k=7 on the top bits': (tuple(range(n - 1, n - 8, -1)), ()),
        'UNIFORM k=7 on the top bits, control on bit 4': (tuple(range(n - 1, n - 8, -1)), (4,)),
        'UNIFORM k=2 at u, u + 1': ((u + 1, u), ()),
        'LANE k=4 below u, bit 0 free': ((u - 1, 6, 3, 1), ()),
        'LANE bits on both sides of u': ((n - 1, u + 1, u, u - 1, u - 2, 3), ()),
        'bit 0 a select bit (complex64: SPLIT, complex128: LANE)': ((n - 1, u, 3, 0), ()),
        'k=4 below u with bit 0 (complex64: SPLIT, complex128: LANE)': ((u - 1, 6, 3, 0), ()),
        'LANE k=4 below u, bit 0 free, diagonal strings': ((u - 1, 6, 3, 1), ()),
        'k=4 below u with bit 0, diagonal strings': ((u - 1, 6, 3, 0), ()),
    }
    fns = {}
    for i, (name, (bits, controls)) in enumerate(cases.items()):
        words = random_table(n, bits, controls, 200 + i, flips='diagonal' not in name).on('cuda')[0]
        src = torch.randperm(1 << len(bits), generator=torch.Generator().manual_seed(300 + i)).to(torch.int32).cuda()
        fns[name] = (lambda w=words, b=bits, c=controls: backend.apply_select_pauli(psi, w, b, c, out=out))
        fns[name + ' / permutation'] = (lambda s=src, b=bits, c=controls: backend.apply_permutation(psi, s, b, c, out=out, path='gather'))
    with torch.no_grad():
        ts = timed_group(fns, reps)
    for name in cases:
        base = row(rows, name + ' / permutation (gather)', dtype, n, batch, ts[name + ' / permutation'], 2 * sbytes)
        row(rows, name, dtype, n, batch, ts[name], 2 * sbytes, base)
    del psi, out
    torch.cuda.empty_cache()


def chain_in_a_field(m):
    return [[1.0, f'{p}{w}{p}{w + 1}'] for w in range(m - 1) for p in 'xyz'] + [[0.5, f'z{w}'] for w in range(m)]


def circuit_row(rows, what, cir, t, extra=None):
    r = {'what': what, 'dtype': 'complex64', 'qubits': cir.nqubit, 'operators': len(cir.operators), 'ms': round(t[0], 3),
         'ms_min': round(t[1], 3), 'ms_max': round(t[2], 3)}
    r.update(extra or {})
    rows.append(r)
    print(f"{what:<58} qubits {cir.nqubit:3d}  operators {len(cir.operators):6d}  {t[0]:10.3f} ms  [{t[1]:.3f}, {t[2]:.3f}]",
          flush=True)


def end_to_end(rows, m, k, reps):
    """SELECT of the chain's strings on k select wires (the first k of the register) and m system wires behind them."""
    n = k + m
    ham = dq.PauliSum(chain_in_a_field(m), m)
    select, system = list(range(k)), list(range(k, n))
    assert ham.select_bits <= k
    pi = torch.tensor(math.pi, dtype=torch.float64)

    def front(cir):
        cir.hlayer()
        cir.rylayer(inputs=[0.1 * (i + 1) for i in range(n)])

    one = dq.QubitCircuit(n)
    front(one)
    one.select_pauli(ham, wires=select, system_wires=system)
    loop = dq.QubitCircuit(n)
    front(loop)
    phases = []
    for s, (h, xmask, zmask) in enumerate(ham.terms):
        wires = [w for w in range(m) if (xmask | zmask) >> (m - 1 - w) & 1]
        letters = ''.join('y' if (xmask & zmask) >> (m - 1 - w) & 1 else 'x' if xmask >> (m - 1 - w) & 1 else 'z' for w in wires)
        zeros = [select[j] for j in range(k) if not (s >> (k - 1 - j)) & 1]
        for w in zeros:
            loop.x(w)
        loop.pauli_rot(letters, wires=[system[w] for w in wires], inputs=pi, controls=select)      # exp(-i pi/2 P) = -i P
        for w in zeros:
            loop.x(w)
        phases.append(1j if h > 0 else -1j)
    loop.diagonal(torch.tensor(phases + [1] * ((1 << k) - len(phases)), dtype=torch.cfloat), wires=select)
    block = dq.QubitCircuit(n)
    front(block)
    lam = block.block_encode(ham, wires=select, system_wires=system)
    res = {}
    with torch.no_grad():
        for name, cir in (('cir.select_pauli', one), ('loop of controlled pauli_rot(pi), X flips, a diagonal', loop),
                          ('cir.block_encode', block)):
            cir.to('cuda')
            t = timed_group({'f': lambda c=cir: c()}, reps)['f']
            circuit_row(rows, f'{ham.nterms} strings, {k} select + {m} system wires: {name}', cir, t,
                        {'strings': ham.nterms, 'select_wires': k, 'system_wires': m, 'lam': lam})
            res[name] = cir().reshape(-1).clone()
            cir.to('cpu')
            torch.cuda.empty_cache()
    a, b = res['cir.select_pauli'], res['loop of controlled pauli_rot(pi), X flips, a diagonal']
    err = (a - b).abs().max().item()
    rows.append({'what': 'select_pauli and the loop differ by', 'max_abs': err, 'largest_amplitude': a.abs().max().item()})
    print(f'  routes differ by {err:.3e} (largest amplitude {a.abs().max().item():.3e})', flush=True)


def main():
    quick = '--quick' in sys.argv
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    assert torch.cuda.is_available(), 'bench_select.py measures on the GPU: there is no fallback'
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
    end_to_end(rows, 9 if quick else 21, 6 if quick else 7, 3 if quick else 5)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as fh:
            json.dump({'box': box, 'rows': rows}, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
