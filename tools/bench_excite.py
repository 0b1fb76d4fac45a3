"""Excitation kernels on the MI355X (dq_apply_excite_axpby_*, dq_excite_cross_*), each against one
full ``dq_apply_pauli_axpby_*`` pass timed in the same process on the same buffers.

1. The gate in place, complex64 n = 28 and complex128 n = 27 at batch 4, singles and doubles with the fixed bits (a) all
   above the 128-byte line, (b) straddling it, (c) all at the bottom, each with 0 and 2 controls.  Beside the time ratio
   stands the byte ratio of the model: 128-byte lines that hold an end of a pair / all lines.
2. ``excite_cross`` with bra == ket and bra != ket against ``pauli_cross`` of a full string.
3. One single and one double at n = 28, un-batched complex64, end to end through ``QubitCircuit`` without autograd: route
   A = ``cir.pauli_evolution`` of the 2 / 8 Pauli strings of K; route B = ``cir.single_excitation`` /
   ``cir.double_excitation`` (out of place there: a copy of the state, then the sparse launch).
4. A UCCSD layer (n = 22, 2 electrons: 40 singles, 190 doubles) the same two ways.

Every point: one warm-up call, then the median of ``reps`` calls between device events; the rows of a group, yardstick
included, take turns within every repetition.  The box is recorded first.  The output goes to profiles/excite/.

usage: python tools/bench_excite.py [--quick] [--out FILE]
"""
import itertools
import json
import os
import platform
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import deepquantum_amd as dq  # noqa: E402
from deepquantum_amd import backend  # noqa: E402
from deepquantum_amd.gate import excitation_masks  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAULIS = {'i': np.eye(2, dtype=complex), 'x': np.array([[0, 1], [1, 0]], dtype=complex), 'y': np.array([[0, -1j], [1j, 0]]),
          'z': np.diag([1.0 + 0j, -1.0])}


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


def line_fraction(xmask, controls, line_bits):
    """Lines that hold an end of a pair / all lines: every fixed bit at or above the line halves the lines of one end, and
    the two ends lie in different lines when xmask has a bit there."""
    fixed = xmask | sum(1 << c for c in controls)
    above = bin(fixed >> line_bits).count('1')
    return (2 if xmask >> line_bits else 1) / 2**above


def kernels(rows, dtype, n, batch, reps):
    esz = 8 if dtype == torch.complex64 else 16
    line_bits = 7 - (3 if esz == 8 else 4)              # amplitudes of a 128-byte line: 16 / 8
    psi = torch.randn(batch, 1 << n, dtype=dtype, device='cuda')
    psi /= psi.norm(dim=-1, keepdim=True)
    other = torch.randn(batch, 1 << n, dtype=dtype, device='cuda')
    sbytes = psi.numel() * esz
    t = torch.linspace(0.3, 1.7, batch, dtype=torch.float64, device='cuda')
    a, c = torch.complex(torch.cos(t), 0 * t), torch.complex(0 * t, -torch.sin(t))
    ones = (1 << n) - 1
    yard = 'pauli_axpby all ones, in place (yardstick)'
    places = {
        'single above the line': (n - 1, n - 2), 'single straddling': (2, n - 1), 'single at the bottom': (0, 1),
        'double above the line': (n - 1, n - 2, n - 3, n - 4), 'double straddling': (1, 2, n - 2, n - 1),
        'double at the bottom': (0, 1, 2, 3),
    }
    group = {yard: (lambda: backend.apply_pauli_axpby(psi, ones, 0, a, c, out=psi), 1.0)}
    for name, bits in places.items():
        xmask = sum(1 << b for b in bits)
        amask = sum(1 << b for b in bits[:len(bits) // 2])
        zmask = 1 << 6 | 1 << (n - 8)
        for controls in ((), (n - 6, 10)):
            spec = (xmask, amask, zmask, 0, controls)
            label = f'{name}, {len(controls)} controls'
            group[label] = ((lambda spec=spec: backend.apply_excite_rot(psi, spec, t, out=psi)),
                            line_fraction(xmask, controls, line_bits))
    with torch.no_grad():
        ts = timed_group({k: v[0] for k, v in group.items()}, reps)
    base = ts[yard][0]
    for name, (_, frac) in group.items():
        med, lo, hi = ts[name]
        r = {'what': name, 'dtype': str(dtype)[6:], 'n': n, 'batch': batch, 'ms': round(med, 4), 'ms_min': round(lo, 4),
             'ms_max': round(hi, 4), 'bytes': int(2 * sbytes * frac), 'TB_per_s': round(2 * sbytes * frac / med / 1e9, 3),
             'time_ratio': round(med / base, 4), 'byte_ratio': frac}
        rows.append(r)
        print(f"{name:<44} {r['dtype']:<10} n={n} b={batch}  {med:9.4f} ms  [{lo:.4f}, {hi:.4f}]  {r['TB_per_s']:6.3f} TB/s  "
              f"time x{r['time_ratio']:.4f}  bytes x{frac:.4f}", flush=True)
    # the cross
    top4 = sum(1 << b for b in places['double above the line'])
    spec = (top4, top4 >> 2 & top4, 1 << 6, 0)
    cyard = 'pauli_cross all ones, bra == ket (yardstick)'
    cross = {
        cyard: (lambda: backend.pauli_cross(psi, psi, ones, 0), 1.0),
        'pauli_cross all ones, bra != ket': (lambda: backend.pauli_cross(other, psi, ones, 0), 2.0),
        'excite_cross double above, bra == ket': (lambda: backend.excite_cross(psi, psi, spec), 1 / 8),
        'excite_cross double above, bra != ket': (lambda: backend.excite_cross(other, psi, spec), 2 / 8),
        'excite_cross single at the bottom, bra == ket': (lambda: backend.excite_cross(psi, psi, (3, 1, 1 << 6, 0)), 1.0),
    }
    with torch.no_grad():
        ts = timed_group({k: v[0] for k, v in cross.items()}, reps)
    base = ts[cyard][0]
    for name, (_, frac) in cross.items():
        med, lo, hi = ts[name]
        r = {'what': name, 'dtype': str(dtype)[6:], 'n': n, 'batch': batch, 'ms': round(med, 4), 'ms_min': round(lo, 4),
             'ms_max': round(hi, 4), 'bytes': int(sbytes * frac), 'TB_per_s': round(sbytes * frac / med / 1e9, 3),
             'time_ratio': round(med / base, 4), 'byte_ratio': frac}
        rows.append(r)
        print(f"{name:<44} {r['dtype']:<10} n={n} b={batch}  {med:9.4f} ms  [{lo:.4f}, {hi:.4f}]  {r['TB_per_s']:6.3f} TB/s  "
              f"time x{r['time_ratio']:.4f}  bytes x{frac:.4f}", flush=True)
    del psi, other
    torch.cuda.empty_cache()


def strings_of(n, create, annihilate):
    """K = E - E^dagger as a Hamiltonian for ``pauli_evolution``: exp(theta K) = exp(-i H theta).  In index terms K is the
    qubit excitation on the listed wires times Z on the wires of zmask times (-1)^negate, so the strings come from the
    dense 4^m-dimensional qubit K alone."""
    listed = list(create) + list(annihilate)
    m2 = len(listed)
    _, _, zmask, negate = excitation_masks(n, create, annihilate)
    i0 = sum(1 << (m2 - 1 - j) for j in range(len(create), m2))                 # the annihilated wires occupied
    i1 = (1 << m2) - 1 - i0
    k = np.zeros((1 << m2, 1 << m2))
    k[i1, i0], k[i0, i1] = 1.0, -1.0
    tail = ''.join(f'z{w}' for w in range(n) if (zmask >> (n - 1 - w)) & 1)
    ham = []
    for letters in itertools.product('xy', repeat=m2):
        p = np.ones((1, 1))
        for ch in letters:
            p = np.kron(p, PAULIS[ch])
        coef = np.vdot(p, k) / (1 << m2)
        if abs(coef) > 1e-12:
            ham.append([float(-coef.imag) * (-1 if negate else 1), ''.join(f'{ch}{w}' for ch, w in zip(letters, listed)) + tail])
    assert len(ham) == 2 ** (m2 - 1)
    return ham


def end_to_end(rows, what, n, build_a, build_b, reps):
    res = {}
    for route, build in (('A pauli_evolution', build_a), ('B excitation', build_b)):
        cir = dq.QubitCircuit(n)
        cir.hlayer()
        build(cir)
        cir.to('cuda')
        with torch.no_grad():
            t = timed_group({'f': lambda: cir()}, reps)['f']
            res[route] = cir().reshape(-1).clone()
        r = {'what': f'{what} route {route}', 'dtype': 'complex64', 'n': n, 'batch': 1, 'ms': round(t[0], 3), 'ms_min': round(t[1], 3),
             'ms_max': round(t[2], 3), 'gates': len(cir.operators)}
        rows.append(r)
        print(f"{r['what']:<48} n={n}  {t[0]:9.3f} ms  [{t[1]:.3f}, {t[2]:.3f}]  operators {len(cir.operators)}", flush=True)
        del cir
    a, b = res.values()
    err = (a - b).abs().max().item()
    rows.append({'what': f'{what} routes differ by', 'max_abs': err, 'largest_amplitude': a.abs().max().item()})
    print(f'  routes differ by {err:.3e} (largest amplitude {a.abs().max().item():.3e})', flush=True)
    ta, tb = rows[-3]['ms'], rows[-2]['ms']
    rows.append({'what': f'{what} excitation over pauli_evolution', 'time_ratio': round(tb / ta, 4)})
    assert tb <= ta, f'{what}: the gate ({tb} ms) is slower than its pauli_evolution route ({ta} ms)'
    del res
    torch.cuda.empty_cache()


def main():
    quick = '--quick' in sys.argv
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'excite', 'bench_excite.json')
    assert torch.cuda.is_available(), 'bench_excite.py measures on the GPU: there is no fallback'
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
    n, theta = (18 if quick else 28), 0.83
    for what, wires in (('single', [3, n - 5]), ('double', [1, 4, n - 9, n - 2])):
        h = len(wires) // 2
        ham = strings_of(n, wires[h:], wires[:h])
        end_to_end(rows, what, n, lambda c: c.pauli_evolution(ham, t=theta),
                   lambda c: c.excitation(wires[h:], wires[:h], inputs=theta), 3 if quick else 7)
    n = 12 if quick else 22
    uc = dq.UCCSD(n, 2, inputs=torch.linspace(-1.0, 1.0, 2 * (n - 2) + (n - 2) * (n - 3) // 2))

    def as_evolutions(cir):
        for g in uc.operators:
            if isinstance(g, dq.ExcitationGate):
                cir.pauli_evolution(strings_of(n, g.create, g.annihilate), t=float(g.theta))
            else:
                cir.add(g)

    def as_excitations(cir):
        for g in uc.operators:
            cir.add(g)

    end_to_end(rows, f'UCCSD({n}, 2) layer', n, as_evolutions, as_excitations, 3)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as fh:
        json.dump({'box': box, 'rows': rows}, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
