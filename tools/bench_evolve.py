"""What the Pauli-sum evolution costs on the MI355X, on the Hamiltonians of tools/bench_psum.py.

1. One order of the recurrence: the fused step ``dq_pauli_sum_cheb_step_*`` (next written over prev) beside the composition
   it replaces -- ``dq_apply_psum_axpby_*`` into a temporary and two state-sized axpys, on the same buffers in the same run
   -- and beside one ``dq_apply_psum_axpby_*`` launch alone.  (a) and (b) at n = 28, batch 4; (c) at n = 22; both precisions.
2. End to end: ``cir.pauli_sum_evolution`` beside ``cir.pauli_evolution(order=2)`` on (a) at t = 1.  The errors of both against
   the dense exponential are found at n = 12, where that is affordable, and the number of Trotter steps that reaches the
   error of the expansion is CARRIED OVER to n = 24 -- an assumption: the Trotter error of a chain grows with its length.
   A Trotter run of more than ``--trotter-cap`` steps is timed over that many and scaled (the steps are identical).

``--counters NAME``: nothing but a few launches of the fused step and of the composition on Hamiltonian NAME (a, b or c),
complex64, for a counters run of its own under ``rocprofv3 --pmc``.

usage: python tools/bench_evolve.py [--quick] [--out FILE] [--counters a|b|c] [--trotter-cap STEPS]
"""
import json
import os
import platform
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_psum import ROOT, doubles_like, heisenberg, ising, timed_group  # noqa: E402  (puts the repository on sys.path)

import torch  # noqa: E402

import deepquantum_amd as dq  # noqa: E402
from deepquantum_amd import backend  # noqa: E402


def step_rows(rows, name, ham, n, batch, dtype, reps):
    esz = 8 if dtype == torch.complex64 else 16
    H = dq.PauliSum(ham, n)
    cur, prev, acc, tmp = (torch.randn(batch, 1 << n, dtype=dtype, device='cuda') for _ in range(4))
    for v in (cur, prev, acc):
        v /= v.norm(dim=-1, keepdim=True)
    sbytes = cur.numel() * esz
    a = H.norm_bound
    delta = 0.01 - 0.02j
    coef = torch.tensor([[2.0 / a, 0.0, -1.0, delta.real, delta.imag]] * batch, dtype=torch.float64, device='cuda')
    two_over_a = torch.full((batch,), 2.0 / a, dtype=torch.complex128, device='cuda')
    zero = torch.zeros_like(two_over_a)
    ptrs = [backend._ptr(t) for t in H.device_table('cuda')]

    def fused():
        backend._call('dq_pauli_sum_cheb_step', cur, backend._ptr(cur), backend._ptr(prev), backend._ptr(prev), backend._ptr(acc),
                      backend._ptr(coef), *ptrs, H.ngroups, H.nterms, n, batch)

    def composed():
        backend.apply_psum_axpby(cur, H.table, zero, two_over_a, out=tmp)
        torch.sub(tmp, prev, out=prev)
        acc.add_(prev, alpha=delta)

    group = {
        'fused step (next over prev)': (fused, (H.ngroups + 5) * sbytes),
        'psum_axpby into a temporary + two axpys': (composed, (H.ngroups + 9) * sbytes),
        'one psum_axpby launch': (lambda: backend.apply_psum_axpby(cur, H.table, zero, two_over_a, out=tmp), (H.ngroups + 2) * sbytes),
    }
    with torch.no_grad():
        ts = timed_group({k: v[0] for k, v in group.items()}, reps)
    for what, (_, nbytes) in group.items():
        med, lo, hi = ts[what]
        r = {'hamiltonian': name, 'what': what, 'dtype': str(dtype)[6:], 'n': n, 'batch': batch, 'strings': H.nterms,
             'groups': H.ngroups, 'ms': round(med, 4), 'ms_min': round(lo, 4), 'ms_max': round(hi, 4), 'bytes': int(nbytes),
             'TB_per_s': round(nbytes / med / 1e9, 3)}
        rows.append(r)
        print(f"{name:<18} {what:<42} {r['dtype']:<10} n={n} b={batch} T={H.nterms} G={H.ngroups}  {med:10.4f} ms  "
              f"[{lo:.4f}, {hi:.4f}]  {r['TB_per_s']:7.3f} TB/s", flush=True)
    f, c, p = (ts[k][0] for k in group)
    rows.append({'hamiltonian': name, 'what': 'ratios', 'dtype': str(dtype)[6:], 'composition_over_fused': round(c / f, 3),
                 'fused_over_one_psum_launch': round(f / p, 3), 'fused_minus_psum_ms': round(f - p, 4)})
    print(f'{name:<18} composition / fused x{c / f:.3f}; fused / one psum launch x{f / p:.3f} (+{f - p:.4f} ms)', flush=True)
    del cur, prev, acc, tmp
    torch.cuda.empty_cache()


def evolved(kind, ham, n, dtype, t, **kw):
    cir = dq.QubitCircuit(n)
    getattr(cir, kind)(ham, t=torch.tensor(t, dtype=torch.float64 if dtype == torch.complex128 else torch.float32), **kw)
    cir.to('cuda')
    if dtype == torch.complex128:
        cir.to(torch.double)
    return cir


def end_to_end(rows, small, big, t, dtype, cap, reps):
    ham = heisenberg(small)
    H = dq.PauliSum(ham, small)
    eye = torch.eye(1 << small, dtype=torch.complex128, device='cuda')
    dense = backend.apply_psum_axpby(eye, H.table, 0.0, 1.0).T.contiguous()
    exact = torch.linalg.matrix_exp(-1j * t * dense.cpu()).cuda()
    g = torch.Generator().manual_seed(1)
    psi = torch.randn(1 << small, dtype=torch.complex128, generator=g)
    psi = (psi / psi.norm()).to(dtype).cuda()
    want = exact @ psi.to(torch.complex128)

    def err_of(cir):
        with torch.no_grad():
            return (cir(state=psi.reshape(-1, 1)).reshape(-1).to(torch.complex128) - want).norm().item()

    cheb_err = err_of(evolved('pauli_sum_evolution', ham, small, dtype, t))
    order = H.chebyshev_order(t, 1e-6 if dtype == torch.complex64 else 1e-12)
    print(f'n={small} {str(dtype)[6:]}: expansion K={order}, 2-norm error {cheb_err:.3e}', flush=True)
    steps, found, trail = 1, None, []
    while steps <= 4096:
        e = err_of(evolved('pauli_evolution', ham, small, dtype, t, steps=steps, order=2))
        trail.append((steps, e))
        print(f'n={small} {str(dtype)[6:]}: Trotter order 2, {steps} steps, 2-norm error {e:.3e}', flush=True)
        if e <= cheb_err:
            found = steps
            break
        steps *= 2
    best = found if found is not None else min(trail, key=lambda p: p[1])[0]
    rows.append({'what': 'errors at the small size', 'n': small, 'dtype': str(dtype)[6:], 't': t, 'order': order,
                 'expansion_error': cheb_err, 'trotter_errors': trail, 'steps_reaching_it': found, 'steps_carried_over': best})
    # the big size
    ham = heisenberg(big)
    Hb = dq.PauliSum(ham, big)
    new = evolved('pauli_sum_evolution', ham, big, dtype, t)
    timed_steps = min(best, cap)
    old = evolved('pauli_evolution', ham, big, dtype, t * timed_steps / best, steps=timed_steps, order=2)
    with torch.no_grad():
        ts = timed_group({'expansion': lambda: new(), 'trotter': lambda: old()}, reps)
    scale = best / timed_steps
    r = {'what': 'end to end', 'n': big, 'dtype': str(dtype)[6:], 't': t, 'order': Hb.chebyshev_order(t, 1e-6 if dtype == torch.complex64 else 1e-12),
         'expansion_ms': round(ts['expansion'][0], 3), 'trotter_steps': best, 'trotter_steps_timed': timed_steps,
         'trotter_ms_timed': round(ts['trotter'][0], 3), 'trotter_ms_scaled': round(ts['trotter'][0] * scale, 3),
         'trotter_over_expansion': round(ts['trotter'][0] * scale / ts['expansion'][0], 2)}
    rows.append(r)
    print(json.dumps(r), flush=True)


def main():
    quick = '--quick' in sys.argv
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'evolve', 'bench_evolve.json')
    cap = int(sys.argv[sys.argv.index('--trotter-cap') + 1]) if '--trotter-cap' in sys.argv else 16
    big, small = (20, 16) if quick else (28, 22)
    hams = {'a': ('(a) Heisenberg', heisenberg(big), big, 4), 'b': ('(b) Ising', ising(big), big, 4),
            'c': ('(c) doubles-like', doubles_like(small, 20 if quick else 200), small, 1)}
    if '--counters' in sys.argv:
        name, ham, n, batch = hams[sys.argv[sys.argv.index('--counters') + 1]]
        step_rows([], name, ham, n, batch, torch.complex64, 3)
        return
    reps = 3 if quick else 7
    rows = [{'what': 'box', 'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'hip': torch.version.hip,
             'host': platform.platform(), 'time': time.strftime('%Y-%m-%d %H:%M:%S')}]
    print(json.dumps(rows[0]), flush=True)
    for key in 'abc':
        name, ham, n, batch = hams[key]
        for dtype in (torch.complex64, torch.complex128):
            step_rows(rows, name, ham, n, batch, dtype, reps)
    end_to_end(rows, 10 if quick else 12, 18 if quick else 24, 1.0, torch.complex64, cap, 3)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(rows, f, indent=1)
    print(f'wrote {out}')


if __name__ == '__main__':
    main()
