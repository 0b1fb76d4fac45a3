"""Pauli-sum kernels on the MI355X (dq_apply_psum_axpby_*, dq_psum_cross_*) against what the package
offered before them -- one ``pauli_cross`` / ``apply_pauli_axpby`` launch per string -- and against one
``dq_apply_pauli_axpby_*`` pass as the traffic yardstick, all timed in the same process on the same buffers.

Three synthetic Hamiltonians, built here:
  (a) a Heisenberg chain sum J (XX + YY + ZZ) at n = 28, batch 4: 81 strings in 28 groups;
  (b) a transverse-field Ising chain at n = 28, batch 4: one group per wire for the X terms, every ZZ term in the group
      without a flip;
  (c) "doubles-like" strings at n = 22: for 200 random quadruples of wires the eight strings of X / Y on them (an even
      number of Ys) with the Z chain of ``gate.excitation_masks`` between them -- 1600 strings in at most 200 groups.

1. Kernels, complex64 and complex128: <H> in one launch against the loop of ``backend.pauli_cross(psi, psi, ...)`` over the
   strings, H|psi> in one launch against the loop of ``apply_pauli_axpby`` plus adds, and the yardstick.  Bytes charged to
   the one-launch kernels: (G + 1) reads of the state, and one write for H|psi>.
2. (c) at the same n with every group cut to 1, 2, 4 and 8 terms: what a term costs beside what a group costs.
3. Forward plus backward of <H> through a UCCSD(22, 2) circuit with (c) as the observable: ``cir.expectation_pauli_sum``
   against the same energy as one ``cir.observable`` per string, at rising string counts while a run stays below
   ``--old-limit`` seconds.

Every point: one warm-up call, then the median of ``reps`` calls between device events; the rows of a group take turns
within every repetition.  The box is recorded first.  The output goes to profiles/psum/.

``--counters NAME``: nothing but a few launches of the two one-launch kernels on Hamiltonian NAME (a, b or c), complex64,
for a counters run of its own under ``rocprofv3 --pmc``.

usage: python tools/bench_psum.py [--quick] [--out FILE] [--old-limit SECONDS] [--counters a|b|c]
"""
import json
import os
import platform
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import deepquantum_amd as dq  # noqa: E402
from deepquantum_amd import backend  # noqa: E402
from deepquantum_amd.gate import excitation_masks  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def string_of(n, xmask, zmask):
    out = ''
    for w in range(n):
        bit = 1 << (n - 1 - w)
        if xmask & bit:
            out += f'y{w}' if zmask & bit else f'x{w}'
        elif zmask & bit:
            out += f'z{w}'
    return out


def heisenberg(n):
    return [[1.0, f'{p}{w}{p}{w + 1}'] for w in range(n - 1) for p in 'xyz']


def ising(n):
    return [[-1.0, f'z{w}z{w + 1}'] for w in range(n - 1)] + [[-0.7, f'x{w}'] for w in range(n)]


def doubles_like(n, quadruples, per_group=8, seed=3):
    rng = np.random.default_rng(seed)
    ham, seen = [], set()
    while len(seen) < quadruples:
        wires = tuple(sorted(int(w) for w in rng.choice(n, 4, replace=False)))
        if wires in seen:
            continue
        seen.add(wires)
        xmask, _, zmask, negate = excitation_masks(n, wires[2:], wires[:2])
        bits = [1 << (n - 1 - w) for w in wires]
        # an even number of Ys: the real strings of E + E^dagger, what a two-body term of a Hamiltonian maps to (the strings
        # with an odd number are imaginary matrices: their expectation in the real state of a UCCSD circuit is 0 identically)
        even = [ys for ys in (3, 5, 6, 9, 10, 12, 0, 15)][:per_group]
        for ys in even:
            ymask = sum(b for k, b in enumerate(bits) if ys >> k & 1)
            ham.append([(-0.125 if negate else 0.125) * (1 if ys in (0, 15, 5, 10) else -1), string_of(n, xmask, zmask | ymask)])
    return ham


def masks_of(H):
    return [(h, x, z) for h, x, z in H.terms]


def kernels(rows, name, ham, n, batch, dtype, reps, loops=True):
    esz = 8 if dtype == torch.complex64 else 16
    H = dq.PauliSum(ham, n)
    terms = masks_of(H)
    psi = torch.randn(batch, 1 << n, dtype=dtype, device='cuda')
    psi /= psi.norm(dim=-1, keepdim=True)
    out = torch.empty_like(psi)
    acc = torch.empty_like(psi)
    sbytes = psi.numel() * esz
    one = torch.ones(batch, dtype=torch.complex128, device='cuda')
    zero = torch.zeros_like(one)
    hs = [h * one for h, _, _ in terms]
    ones = (1 << n) - 1

    def expect_loop():
        e = torch.zeros(batch, dtype=torch.complex128, device='cuda')
        for (h, x, z) in terms:
            e += h * backend.pauli_cross(psi, psi, x, z)
        return e

    def apply_loop():
        acc.zero_()
        for hv, (_, x, z) in zip(hs, terms):
            acc.add_(backend.apply_pauli_axpby(psi, x, z, zero, hv, (), 'map', out=out))
        return acc

    group = {
        '<H> one launch': (lambda: backend.psum_cross(psi, psi, H.table), (H.ngroups + 1) * sbytes),
        'H|psi> one launch': (lambda: backend.apply_psum_axpby(psi, H.table, zero, one, out=out), (H.ngroups + 2) * sbytes),
        'pauli_axpby all ones, in place (yardstick)': (lambda: backend.apply_pauli_axpby(acc, ones, 0, one, zero, out=acc), 2 * sbytes),
    }
    if loops:
        group['<H> loop of pauli_cross'] = (expect_loop, H.nterms * sbytes)
        group['H|psi> loop of pauli_axpby + add'] = (apply_loop, H.nterms * 5 * sbytes + sbytes)
    with torch.no_grad():
        ts = timed_group({k: v[0] for k, v in group.items()}, reps)
        agree = (backend.psum_cross(psi, psi, H.table) - expect_loop()).abs().max().item() if loops else None
    for what, (_, nbytes) in group.items():
        med, lo, hi = ts[what]
        r = {'hamiltonian': name, 'what': what, 'dtype': str(dtype)[6:], 'n': n, 'batch': batch, 'strings': H.nterms,
             'groups': H.ngroups, 'ms': round(med, 4), 'ms_min': round(lo, 4), 'ms_max': round(hi, 4), 'bytes': int(nbytes),
             'TB_per_s': round(nbytes / med / 1e9, 3)}
        rows.append(r)
        print(f"{name:<18} {what:<44} {r['dtype']:<10} n={n} b={batch} T={H.nterms} G={H.ngroups}  {med:10.4f} ms  "
              f"[{lo:.4f}, {hi:.4f}]  {r['TB_per_s']:7.3f} TB/s", flush=True)
    if loops:
        for kind, new, old in (('<H>', '<H> one launch', '<H> loop of pauli_cross'),
                               ('H|psi>', 'H|psi> one launch', 'H|psi> loop of pauli_axpby + add')):
            measured = ts[old][0] / ts[new][0]
            modelled = group[old][1] / group[new][1]
            rows.append({'hamiltonian': name, 'what': f'{kind} loop over one launch', 'dtype': str(dtype)[6:],
                         'time_ratio': round(measured, 3), 'modelled_byte_ratio': round(modelled, 3)})
            print(f'{name:<18} {kind} loop / one launch: measured x{measured:.3f}, bytes modelled x{modelled:.3f}', flush=True)
        rows.append({'hamiltonian': name, 'what': '<H> one launch minus loop', 'dtype': str(dtype)[6:], 'max_abs': agree})
    del psi, out, acc
    torch.cuda.empty_cache()


def uccsd_energy(rows, n, ham_full, old_limit, reps):
    uc_angles = torch.linspace(-0.3, 0.3, 2 * (n - 2) + (n - 2) * (n - 3) // 2)

    def circuit():
        cir = dq.UCCSD(n, 2)
        with torch.no_grad():
            for p, v in zip(cir.parameters(), uc_angles):
                p.copy_(v)
        return cir.to('cuda')

    def step_new(cir, H):
        cir.zero_grad(set_to_none=True)
        cir()
        cir.expectation_pauli_sum(H).backward()

    def step_old(cir, coefs):
        cir.zero_grad(set_to_none=True)
        cir()
        (cir.expectation() * coefs).sum().backward()

    for count in (100, 400, len(ham_full)):
        ham = ham_full[:count]
        H = dq.PauliSum(ham, n)
        cir = circuit()
        t = timed_group({'new': lambda: step_new(cir, H)}, reps)['new']
        g_new = torch.cat([p.grad.reshape(-1) for p in cir.parameters()]).clone()
        rows.append({'what': 'UCCSD forward + backward, expectation_pauli_sum', 'n': n, 'strings': len(ham), 'groups': H.ngroups,
                     'ms': round(t[0], 3), 'ms_min': round(t[1], 3), 'ms_max': round(t[2], 3)})
        print(f'UCCSD({n}, 2) fwd+bwd  expectation_pauli_sum      T={len(ham):5d}  {t[0]:10.3f} ms  [{t[1]:.3f}, {t[2]:.3f}]', flush=True)
        old = circuit()
        import re
        for _, s in ham:
            f = re.findall(r'([xyz])(\d+)', s)
            old.observable([int(w) for _, w in f], ''.join(p for p, _ in f))
        coefs = torch.tensor([h for h, _ in ham], device='cuda')
        torch.cuda.synchronize()
        t0 = time.time()
        step_old(old, coefs)
        torch.cuda.synchronize()
        first = time.time() - t0
        if first > old_limit:
            rows.append({'what': 'UCCSD forward + backward, one observable per string', 'n': n, 'strings': len(ham),
                         'first_call_s': round(first, 2), 'note': f'not repeated: one call took more than {old_limit} s'})
            print(f'UCCSD({n}, 2) fwd+bwd  one observable per string   T={len(ham):5d}  first call {first:.2f} s: not repeated, '
                  'larger counts not tried', flush=True)
            break
        t = timed_group({'old': lambda: step_old(old, coefs)}, max(2, reps // 2))['old']
        g_old = torch.cat([p.grad.reshape(-1) for p in old.parameters()])
        rows.append({'what': 'UCCSD forward + backward, one observable per string', 'n': n, 'strings': len(ham),
                     'ms': round(t[0], 3), 'ms_min': round(t[1], 3), 'ms_max': round(t[2], 3),
                     'peak_GiB': round(torch.cuda.max_memory_allocated() / 2**30, 2),
                     'gradients_differ_by': (g_new - g_old).abs().max().item(), 'largest_gradient': g_old.abs().max().item()})
        print(f'UCCSD({n}, 2) fwd+bwd  one observable per string   T={len(ham):5d}  {t[0]:10.3f} ms  [{t[1]:.3f}, {t[2]:.3f}]  '
              f'gradients differ by {(g_new - g_old).abs().max().item():.2e} (largest {g_old.abs().max().item():.2e})', flush=True)
        del old, cir
        torch.cuda.empty_cache()


def main():
    quick = '--quick' in sys.argv
    arg = lambda flag, default: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default  # noqa: E731
    out = arg('--out', os.path.join(ROOT, 'profiles', 'psum', 'bench_psum.json'))
    old_limit = float(arg('--old-limit', 20))
    assert torch.cuda.is_available(), 'bench_psum.py measures on the GPU: there is no fallback'
    big, small = (20, 14) if quick else (28, 22)
    hams = {'a': ('(a) Heisenberg', heisenberg(big), big, 4), 'b': ('(b) Ising', ising(big), big, 4),
            'c': ('(c) doubles-like', doubles_like(small, 20 if quick else 200), small, 1)}
    if '--counters' in sys.argv:
        name, ham, n, batch = hams[arg('--counters', 'c')]
        H = dq.PauliSum(ham, n)
        psi = torch.randn(batch, 1 << n, dtype=torch.complex64, device='cuda')
        one = torch.ones(batch, dtype=torch.complex128, device='cuda')
        for _ in range(3):
            backend.psum_cross(psi, psi, H.table)
            backend.apply_psum_axpby(psi, H.table, 0 * one, one)
        torch.cuda.synchronize()
        print(f'{name}: n={n} batch={batch} T={H.nterms} G={H.ngroups}: 3 launches of each kernel')
        return
    prop = torch.cuda.get_device_properties(0)
    box = {'device': prop.name, 'cus': prop.multi_processor_count, 'memory_GiB': round(prop.total_memory / 2**30, 1),
           'devices_visible': torch.cuda.device_count(), 'torch': torch.__version__, 'hip': torch.version.hip,
           'host': platform.processor() or platform.machine()}
    print('box:', json.dumps(box), flush=True)
    rows = []
    reps = 3 if quick else 5
    for dtype in (torch.complex64, torch.complex128):
        for key in 'abc':
            name, ham, n, batch = hams[key]
            kernels(rows, name, ham, n, batch, dtype, reps)
    for per_group in (1, 2, 4, 8):
        ham = doubles_like(small, 20 if quick else 200, per_group)
        kernels(rows, f'(c) {per_group} per group', ham, small, 1, torch.complex64, reps, loops=False)
    uccsd_energy(rows, 12 if quick else 22, doubles_like(12 if quick else 22, 20 if quick else 200), old_limit, reps)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as fh:
        json.dump({'box': box, 'rows': rows}, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
