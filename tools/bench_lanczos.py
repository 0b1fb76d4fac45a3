"""What the extremal-eigenpair solver costs on the MI355X, on the Hamiltonians of tools/bench_psum.py.

1. The first launch of a Lanczos step, ``dq_pauli_sum_lanczos_step_*`` (next over prev, two sums), beside the Chebyshev step
   ``dq_pauli_sum_cheb_step_*`` of the same run, which moves one read and one write more and reduces nothing.  (a) and (b) at
   n = 28, batch 4; (c) at n = 22; both precisions.
2. The second launch, ``dq_lanczos_update_*`` with and without the Ritz sum, beside a torch ``add_`` on the same tensors.
3. The whole step -- both launches and the two host reads -- beside the composition the package offered before:
   ``apply_psum_axpby`` into a temporary, two torch axpys, ``torch.vdot`` and ``torch.linalg.vector_norm``, read on the host.
4. End to end: the ground energy of the Heisenberg chain, value only and with the vector, complex64; and the evolution of
   section 4.16's end-to-end case with and without ``bounds=H.spectral_bounds()``, the cost of the bounds beside the saving.

``--counters NAME``: nothing but a few launches of both steps on Hamiltonian NAME (a, b or c), complex64, for a counters
run of its own under ``rocprofv3 --pmc``.

usage: python tools/bench_lanczos.py [--quick] [--out FILE] [--counters a|b|c]
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
from deepquantum_amd import _lib, backend  # noqa: E402


def report(rows, name, H, dtype, n, batch, ts, group):
    for what, (_, nbytes) in group.items():
        med, lo, hi = ts[what]
        r = {'hamiltonian': name, 'what': what, 'dtype': str(dtype)[6:], 'n': n, 'batch': batch, 'strings': H.nterms,
             'groups': H.ngroups, 'ms': round(med, 4), 'ms_min': round(lo, 4), 'ms_max': round(hi, 4), 'bytes': int(nbytes),
             'TB_per_s': round(nbytes / med / 1e9, 3)}
        rows.append(r)
        print(f"{name:<18} {what:<46} {r['dtype']:<10} n={n} b={batch} G={H.ngroups}  {med:10.4f} ms  [{lo:.4f}, {hi:.4f}]  "
              f"{r['TB_per_s']:7.3f} TB/s", flush=True)


def step_rows(rows, name, ham, n, batch, dtype, reps):
    esz = 8 if dtype == torch.complex64 else 16
    H = dq.PauliSum(ham, n)
    cur, prev, acc, tmp = (torch.randn(batch, 1 << n, dtype=dtype, device='cuda') for _ in range(4))
    for v in (cur, prev, acc):
        v /= v.norm(dim=-1, keepdim=True)
    sbytes = cur.numel() * esz
    a = H.norm_bound
    cheb = torch.tensor([[2.0 / a, 0.0, -1.0, 0.01, -0.02]] * batch, dtype=torch.float64, device='cuda')
    lanc = torch.tensor([[1.0 / a, 0.0, -0.5]] * batch, dtype=torch.float64, device='cuda')
    upd = torch.tensor([[-0.25, 0.125]] * batch, dtype=torch.float64, device='cuda')
    out = torch.empty(batch, 2, dtype=torch.float64, device='cuda')
    nbytes = _lib.load().dq_psum_cross_ws_bytes(n, batch, int(dtype == torch.complex128), 0)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device='cuda')
    ptrs = [backend._ptr(t) for t in H.device_table('cuda')]
    tail = (*ptrs, H.ngroups, H.nterms, n, batch)
    sums = (backend._ptr(out), backend._ptr(ws), nbytes)
    one = torch.full((batch,), 1.0 / a, dtype=torch.complex128, device='cuda')
    zero = torch.zeros_like(one)

    def cheb_step():
        backend._call('dq_pauli_sum_cheb_step', cur, backend._ptr(cur), backend._ptr(prev), backend._ptr(prev), backend._ptr(acc),
                      backend._ptr(cheb), *tail)

    def lanczos_step():
        backend._call('dq_pauli_sum_lanczos_step', cur, backend._ptr(cur), backend._ptr(prev), backend._ptr(prev), backend._ptr(lanc),
                      *tail, *sums)

    def update(with_acc):
        backend._call('dq_lanczos_update', cur, backend._ptr(cur), backend._ptr(prev), backend._ptr(acc if with_acc else None),
                      backend._ptr(upd), n, batch, *sums)

    def whole_step():
        lanczos_step()
        got = out.tolist()
        upd[:, 0] = -got[0][0] * 1e-3
        update(False)
        return out.tolist()

    def composed():
        backend.apply_psum_axpby(cur, H.table, zero, one, out=tmp)
        tmp.add_(prev, alpha=-0.5)
        alpha = [torch.vdot(cur[b], tmp[b]).real.item() for b in range(batch)]
        for b in range(batch):
            tmp[b].add_(cur[b], alpha=-alpha[b] * 1e-3)
        return torch.linalg.vector_norm(tmp, dim=-1).tolist()

    group = {
        'lanczos step (next over prev, two sums)': (lanczos_step, (H.ngroups + 3) * sbytes),
        'chebyshev step (next over prev, acc)': (cheb_step, (H.ngroups + 5) * sbytes),
        'lanczos update (w += e v, two sums)': (lambda: update(False), 3 * sbytes),
        'lanczos update with the Ritz sum': (lambda: update(True), 5 * sbytes),
        'torch add_ (w += e v)': (lambda: prev.add_(cur, alpha=-0.25), 3 * sbytes),
        'whole step: two launches, two host reads': (whole_step, (H.ngroups + 6) * sbytes),
        'composition: psum_axpby, 2 axpys, vdot, norm': (composed, (H.ngroups + 12) * sbytes),
    }
    with torch.no_grad():
        ts = timed_group({k: v[0] for k, v in group.items()}, reps)
    report(rows, name, H, dtype, n, batch, ts, group)
    m = {k: ts[k][0] for k in group}
    keys = list(group)
    r = {'hamiltonian': name, 'what': 'ratios', 'dtype': str(dtype)[6:],
         'lanczos_step_over_chebyshev_step': round(m[keys[0]] / m[keys[1]], 3),
         'update_over_torch_add': round(m[keys[2]] / m[keys[4]], 3),
         'update_with_sum_over_torch_add': round(m[keys[3]] / m[keys[4]], 3),
         'composition_over_whole_step': round(m[keys[6]] / m[keys[5]], 3)}
    rows.append(r)
    print(json.dumps(r), flush=True)
    del cur, prev, acc, tmp
    torch.cuda.empty_cache()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = fn()
    torch.cuda.synchronize()
    return got, (time.perf_counter() - t0) * 1e3


def ground_energy(rows, n):
    H = dq.PauliSum(heisenberg(n), n)
    H.ground_state(vector=False, max_steps=2)                                       # (the table's copy, the library's load)
    for vector in (False, True):
        got, ms = wall(lambda: H.ground_state(vector=vector))
        r = {'what': 'ground energy, Heisenberg chain', 'n': n, 'dtype': 'complex64', 'vector': vector, 'steps': int(got.steps),
             'value': float(got.value), 'per_site': float(got.value) / n, 'residual_over_norm_bound': float(got.residual) / H.norm_bound,
             'converged': bool(got.converged), 'ms': round(ms, 2), 'ms_per_step': round(ms / int(got.steps) / (2 if vector else 1), 3)}
        if vector:
            e = dq.expectation_pauli_sum(got.vector, n, H)
            r['energy_of_the_vector'] = float(e)
            r['norm_minus_one'] = float(got.vector.to(torch.complex128).norm()) - 1.0
        rows.append(r)
        print(json.dumps(r), flush=True)
        del got
        torch.cuda.empty_cache()


def evolution_with_bounds(rows, n, t, reps):
    H = dq.PauliSum(heisenberg(n), n)
    g = torch.Generator().manual_seed(1)
    psi = torch.randn(1, 1 << n, dtype=torch.complex64, generator=g).cuda()
    psi /= psi.norm()
    tol = 1e-6
    H.ground_state(vector=False, max_steps=2)
    bounds, bounds_ms = wall(lambda: H.spectral_bounds())
    with torch.no_grad():
        ts = timed_group({'plain': lambda: dq.evolve_pauli_sum(psi, H, t, tol=tol),
                          'bounds': lambda: dq.evolve_pauli_sum(psi, H, t, tol=tol, bounds=bounds)}, reps)
        diff = (dq.evolve_pauli_sum(psi, H, t, tol=tol).to(torch.complex128)
                - dq.evolve_pauli_sum(psi, H, t, tol=tol, bounds=bounds).to(torch.complex128)).norm().item()
    r = {'what': 'evolution with and without bounds', 'n': n, 't': t, 'dtype': 'complex64', 'norm_bound': H.norm_bound,
         'constant': H.constant, 'bounds': bounds, 'order_plain': H.chebyshev_order(t, tol), 'order_bounds': H.chebyshev_order(t, tol, bounds=bounds),
         'plain_ms': round(ts['plain'][0], 3), 'bounds_ms': round(ts['bounds'][0], 3), 'spectral_bounds_ms': round(bounds_ms, 2),
         'difference_2norm': diff}
    rows.append(r)
    print(json.dumps(r), flush=True)


def main():
    quick = '--quick' in sys.argv
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'lanczos', 'bench_lanczos.json')
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
    for n in ((16, 20) if quick else (24, 28)):
        ground_energy(rows, n)
    evolution_with_bounds(rows, 18 if quick else 24, 1.0, 3)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(rows, f, indent=1)
    print(f'wrote {out}')


if __name__ == '__main__':
    main()
