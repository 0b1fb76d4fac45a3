"""Cost distributions on the MI355X (dq_cost_hist_*, dq_apply_binned_*), against the kernels that
move the same bytes over the same ``bits``, timed in the same process, taking turns.

1. Kernels, complex64 n = 28 and complex128 n = 27 at batch 4, ``bits`` over all wires (the table streamed beside the
   state) and over 10 scattered wires, V = 2, 200 and max_bins random bins: ``cost_hist`` (bra == ket) against
   ``cost_cross`` (its floor: the same state bytes, a float table where the histogram reads uint16), ``apply_binned``
   against ``apply_diag``, both out of place.
2. End to end, complex64 batch 1 at n = 24 .. 28: ``qmath.cvar_cost`` of the MaxCut table of the complete graph K_n at
   alpha = 0.1 against the torch route -- probabilities, a gather into cost order, a cumulative sum -- with the table
   prepared once on both sides (``qmath.cost_bins`` / ``argsort``); time and peak allocated memory above the state.

Every point: one warm-up call, then the median of ``reps`` calls between device events; the rows of a group take turns
within every repetition.  The box is recorded first.

usage: python tools/bench_costdist.py [--quick] [--out FILE]
"""
import json
import os
import platform
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from deepquantum_amd import backend, qmath  # noqa: E402
from bench_diag import row, timed_group  # noqa: E402


def kernels(rows, dtype, n, batch, reps):
    real = torch.float32 if dtype == torch.complex64 else torch.float64
    esz = 8 if dtype == torch.complex64 else 16
    psi = torch.randn(batch, 1 << n, dtype=dtype, device='cuda')
    out = torch.empty_like(psi)
    sbytes = psi.numel() * esz
    scattered = [n - 1 - (j * (n - 1)) // 9 for j in range(10)]
    for where, bits in (('all wires', list(range(n - 1, -1, -1))), ('10 scattered', scattered)):
        k = len(bits)
        cost = torch.randn(1 << k, dtype=real, device='cuda')
        diag = torch.exp(1j * cost.double()).to(dtype)
        tbytes = (1 << k) * batch if k == n else 0      # table entries streamed beside the state, once per sample
        yard_h, yard_a = f'cost_cross {where} (floor)', f'apply_diag {where} (yardstick)'
        group = {yard_h: (lambda: backend.cost_cross(psi, psi, cost, bits), sbytes + tbytes * cost.element_size()),
                 yard_a: (lambda: backend.apply_diag(psi, diag, bits, out=out), 2 * sbytes + tbytes * esz)}
        for nbins in (2, 200, backend.cost_hist_max_bins()):
            tab = backend.bin_table(torch.randint(0, nbins, (1 << k,), device='cuda'), psi, nbins)
            g = torch.randn(batch, nbins, dtype=torch.complex128, device='cuda')
            group[f'cost_hist {where} V={nbins}'] = (lambda tab=tab, nbins=nbins: backend.cost_hist(psi, psi, tab, nbins, bits),
                                                     sbytes + tbytes * 2)
            group[f'apply_binned {where} V={nbins}'] = (lambda tab=tab, g=g: backend.apply_binned(psi, g, tab, bits, out=out),
                                                        2 * sbytes + tbytes * 2)
        with torch.no_grad():
            ts = timed_group({name: v[0] for name, v in group.items()}, reps)
        base = {'cost_hist': row(rows, yard_h, dtype, n, batch, ts[yard_h], group[yard_h][1]),
                'apply_binned': row(rows, yard_a, dtype, n, batch, ts[yard_a], group[yard_a][1])}
        for name, (_, nbytes) in group.items():
            if name not in (yard_h, yard_a):
                row(rows, name, dtype, n, batch, ts[name], nbytes, base[name.split()[0]])
    del psi, out
    torch.cuda.empty_cache()


def torch_cvar(psi, order, sorted_cost, alpha):
    """The route without the kernels: probabilities, a gather into cost order, a cumulative sum, the split threshold."""
    p = psi.real.double() ** 2 + psi.imag.double() ** 2
    p = (p / p.sum(-1, keepdim=True))[:, order]
    cdf = p.cumsum(-1)
    t = (cdf < alpha).sum(-1, keepdim=True).clamp_(max=p.shape[-1] - 1)
    head = p * (torch.arange(p.shape[-1], device=p.device) < t)
    return ((head * sorted_cost).sum(-1) + sorted_cost[t.squeeze(-1)] * (alpha - head.sum(-1))) / alpha


def end_to_end(rows, sizes, reps, alpha=0.1):
    for n in sizes:
        psi = torch.randn(1, 1 << n, dtype=torch.complex64, device='cuda')
        cost = qmath.ising_cost(n, [(0.5, [i, j]) for i in range(n) for j in range(i + 1, n)], dtype=torch.float32, device='cuda')
        prepared = qmath.cost_bins(cost)
        order = torch.argsort(cost)
        sorted_cost = cost[order].double()
        fns = {'torch (probs, gather, cumsum)': lambda: torch_cvar(psi, order, sorted_cost, alpha),
               'qmath.cvar_cost': lambda: qmath.cvar_cost(psi, n, prepared, alpha)}
        with torch.no_grad():
            a, b = fns['torch (probs, gather, cumsum)'](), fns['qmath.cvar_cost']()
            assert abs(float(a) - float(b)) <= 1e-4 * abs(float(a)), (float(a), float(b))
            peak = {}
            for name, f in fns.items():
                torch.cuda.synchronize()
                floor = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                f()
                torch.cuda.synchronize()
                peak[name] = torch.cuda.max_memory_allocated() - floor
            ts = timed_group(fns, reps)
        base = None
        for name in fns:
            med = row(rows, f'{name} K_{n} V={prepared.values.numel()}', torch.complex64, n, 1, ts[name], psi.numel() * 8, base)
            rows[-1]['peak_bytes_above_inputs'] = peak[name]
            print(f'    peak memory above the inputs: {peak[name] / 2**20:.1f} MiB', flush=True)
            base = med if base is None else base
        del psi, cost, prepared, order, sorted_cost
        torch.cuda.empty_cache()


def main():
    quick = '--quick' in sys.argv
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    assert torch.cuda.is_available(), 'bench_costdist.py measures on the GPU: there is no fallback'
    prop = torch.cuda.get_device_properties(0)
    box = {'device': prop.name, 'cus': prop.multi_processor_count, 'memory_GiB': round(prop.total_memory / 2**30, 1),
           'devices_visible': torch.cuda.device_count(), 'torch': torch.__version__, 'hip': torch.version.hip,
           'host': platform.processor() or platform.machine()}
    print('box:', json.dumps(box), flush=True)
    rows = []
    reps = 5 if quick else 9
    points = ((torch.complex64, 22, 4), (torch.complex128, 21, 4)) if quick else ((torch.complex64, 28, 4), (torch.complex128, 27, 4))
    for dtype, n, batch in points:
        kernels(rows, dtype, n, batch, reps)
    end_to_end(rows, (20, 21) if quick else (24, 25, 26, 27, 28), 3 if quick else 7)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as fh:
            json.dump({'box': box, 'rows': rows}, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
