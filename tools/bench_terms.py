"""The per-string kernel on the MI355X (dq_pauli_terms_cross_*), timed in one process on the same
buffers against

  (a) ``backend.psum_cross`` on the same table: its traffic twin, G + 1 reads of the state for G groups, which returns the
      one sum where this returns every string's value;
  (b) the loop the package offered before: one ``psum_cross`` per one-string ``PauliSum``;
  (c) nothing -- ``qmath.pauli_pool_gradients`` for a pool of qubit-excitation strings at n = 22, as an absolute time.

Shapes: the Heisenberg chain of tools/bench_psum.py at n = 28, batch 4 (81 strings, 28 groups) in both dtypes; its 1600-string
"doubles-like" table at n = 22 (at most 200 groups); and a sweep at n = 26, batch 1, of 8 groups of 1, 4, 17 and 200 terms
each, which sets what the transform costs per group beside what a term costs.

Every point: one warm-up call, then the median of ``reps`` calls between device events, the rows of a group taking turns
within every repetition (``bench_psum.timed_group``).  The box is recorded first.  The output goes to profiles/terms/.

usage: python tools/bench_terms.py [--quick] [--out FILE]
"""
import json
import os
import platform
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_psum import ROOT, doubles_like, heisenberg, string_of, timed_group  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import deepquantum_amd as dq  # noqa: E402
from deepquantum_amd import backend, qmath  # noqa: E402


def sweep_table(n, groups, per_group, seed=5):
    """``groups`` random flip masks with ``per_group`` random sign masks each (the Y factors fall where they fall)."""
    rng = np.random.default_rng(seed)
    xs, ham = set(), []
    while len(xs) < groups:
        xs.add(int(rng.integers(1 << n)))
    for x in sorted(xs):
        zs = set()
        while len(zs) < per_group:
            zs.add(int(rng.integers(1 << n)))
        ham += [[1.0, string_of(n, x, z)] for z in sorted(zs)]
    return ham


def compare(rows, name, ham, n, batch, dtype, reps, loop=True):
    H = dq.PauliSum(ham, n)
    psi = torch.randn(batch, 1 << n, dtype=dtype, device='cuda')
    psi /= psi.norm(dim=-1, keepdim=True)
    singles = [dq.PauliSum([[1.0, string_of(n, x, z)]], n) for _, x, z in H.terms] if loop else []
    fns = {'pauli_terms_cross': lambda: backend.pauli_terms_cross(psi, psi, H.table),
           'psum_cross (the sum only)': lambda: backend.psum_cross(psi, psi, H.table)}
    if loop:
        fns['loop of one-string psum_cross'] = lambda: torch.stack([backend.psum_cross(psi, psi, s.table) for s in singles], dim=1)
    with torch.no_grad():
        ts = timed_group(fns, reps)
        got = backend.pauli_terms_cross(psi, psi, H.table)
        h = torch.tensor([t[0] for t in H.terms], dtype=torch.float64, device='cuda')
        differ = ((got * h).sum(-1) - backend.psum_cross(psi, psi, H.table)).abs().max().item()
        if loop:
            differ = max(differ, (got - fns['loop of one-string psum_cross']()).abs().max().item())
    for what, (med, lo, hi) in ts.items():
        rows.append({'table': name, 'what': what, 'dtype': str(dtype)[6:], 'n': n, 'batch': batch, 'strings': H.nterms,
                     'groups': H.ngroups, 'ms': round(med, 4), 'ms_min': round(lo, 4), 'ms_max': round(hi, 4)})
        print(f"{name:<22} {what:<32} {str(dtype)[6:]:<10} n={n} b={batch} T={H.nterms} G={H.ngroups}  {med:10.4f} ms  "
              f'[{lo:.4f}, {hi:.4f}]', flush=True)
    base = ts['pauli_terms_cross'][0]
    ratios = {'over_psum_cross': round(base / ts['psum_cross (the sum only)'][0], 3)}
    if loop:
        ratios['loop_over_it'] = round(ts['loop of one-string psum_cross'][0] / base, 3)
    rows.append({'table': name, 'what': 'ratios', 'dtype': str(dtype)[6:], **ratios, 'values_differ_by': differ})
    print(f'{name:<22} ratios {ratios}  values differ by {differ:.2e}', flush=True)
    del psi
    torch.cuda.empty_cache()


def pool_gradients(rows, n, quadruples, reps):
    H = dq.PauliSum(heisenberg(n), n)
    pool = [s for _, s in doubles_like(n, quadruples)]
    P, _ = dq.PauliSum.from_strings(pool, n)
    psi = torch.randn(1, 1 << n, dtype=torch.complex64, device='cuda')
    psi /= psi.norm(dim=-1, keepdim=True)
    with torch.no_grad():
        med, lo, hi = timed_group({'g': lambda: qmath.pauli_pool_gradients(psi, n, H, P)}, reps)['g']
    rows.append({'what': 'pauli_pool_gradients, Heisenberg H, doubles-like pool', 'dtype': 'complex64', 'n': n, 'pool': P.nterms,
                 'pool_groups': P.ngroups, 'ms': round(med, 4), 'ms_min': round(lo, 4), 'ms_max': round(hi, 4)})
    print(f'pauli_pool_gradients n={n} pool={P.nterms} strings in {P.ngroups} groups  {med:10.4f} ms  [{lo:.4f}, {hi:.4f}]', flush=True)


def main():
    quick = '--quick' in sys.argv
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'terms', 'bench_terms.json')
    assert torch.cuda.is_available(), 'bench_terms.py measures on the GPU: there is no fallback'
    prop = torch.cuda.get_device_properties(0)
    box = {'device': prop.name, 'cus': prop.multi_processor_count, 'memory_GiB': round(prop.total_memory / 2**30, 1),
           'devices_visible': torch.cuda.device_count(), 'torch': torch.__version__, 'hip': torch.version.hip,
           'host': platform.processor() or platform.machine()}
    print('box:', json.dumps(box), flush=True)
    big, small, mid = (20, 14, 16) if quick else (28, 22, 26)
    reps = 3 if quick else 5
    rows = []
    for dtype in (torch.complex64, torch.complex128):
        compare(rows, 'Heisenberg', heisenberg(big), big, 4, dtype, reps)
    compare(rows, 'doubles-like', doubles_like(small, 20 if quick else 200), small, 1, torch.complex64, reps)
    for per_group in (1, 4, 17, 200):
        compare(rows, f'8 groups of {per_group}', sweep_table(mid, 8, per_group), mid, 1, torch.complex64, reps, loop=False)
    pool_gradients(rows, small, 20 if quick else 200, reps)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as fh:
        json.dump({'box': box, 'rows': rows}, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
