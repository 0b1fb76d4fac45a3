"""The quantum Fourier transform as FFT stages on the MI355X (dq_apply_qft_*), each case against
what moves the same bytes or does the same work in the same run, taking turns (median of the rounds, min and max kept):

(a) one stage against ``dq_apply_diag_*`` over the same wires (one read, one write of the state, one multiplication per
    amplitude): a group on the top bits (riders on the line), the group on the low bits, a scattered shuffled group;
(b) the whole transform on all wires, on 20 and on 12 wires, ``QuantumFourierTransform(native=True)`` against the gate
    sequence of ``QuantumFourierTransform`` through the fused passes, end to end, with their difference;
(c) the swap form against the swap-free one (the extra ``permute_bits`` pass of a list of more than one stage).

n = 28 (complex64) / 27 (complex128) at batch 4 for the kernels; ``--quick``: n = 22 / 21.

usage: python tools/bench_qft.py [--quick] [--out FILE]
"""
import json
import os
import platform
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deepquantum_amd as dq  # noqa: E402
from deepquantum_amd import backend  # noqa: E402


def timed_group(fns, reps):
    """Median, min and max ms of every function of ``fns``: one warm-up call each, then ``reps`` rounds in which they take
    turns (what drifts over the run then hits all of them alike)."""
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


def row(rows, what, t, **extra):
    r = {'what': what, 'ms': round(t[0], 4), 'ms_min': round(t[1], 4), 'ms_max': round(t[2], 4), **extra}
    rows.append(r)
    print(f"{what:<72} {t[0]:10.4f} ms  [{t[1]:.4f}, {t[2]:.4f}]  " + json.dumps(extra), flush=True)
    return t[0]


def stages(rows, dtype, n, batch, reps):
    esz = 8 if dtype == torch.complex64 else 16
    T = backend.qft_tile_bits(dtype)
    line = 4 if dtype == torch.complex64 else 3
    psi = torch.randn(batch, 1 << n, dtype=dtype, device='cuda')
    out = torch.empty_like(psi)
    nbytes = 2 * psi.numel() * esz
    g = torch.Generator().manual_seed(1)
    scattered = [int(p) for p in (torch.randperm(n - line, generator=g)[:T - line] + line)]
    cases = {
        f'one stage: {T - line} wires on the top bits (riders: the line bits)': list(range(n - 1, n - 1 - (T - line), -1)),
        f'one stage: the {T} lowest bits': list(range(T - 1, -1, -1)),
        f'one stage: {T - line} scattered wires above the line, shuffled': scattered,
    }
    full = list(range(n - 1, -1, -1))
    fns = {}
    for name, bits in cases.items():
        assert backend.qft_passes(n, bits, dtype) == 1
        diag = torch.exp(1j * torch.randn(1 << len(bits), dtype=torch.float64)).to(dtype).cuda()
        fns[name] = lambda b=bits: backend.apply_qft(psi, b, out=out)
        fns[name + ' / diag'] = lambda b=bits, d=diag: backend.apply_diag(psi, d, b, out=out)
    fns['all wires, swap-free'] = lambda: backend.apply_qft(psi, full, out=out)
    fns['all wires, swap form'] = lambda: backend.apply_qft(psi, full, swaps=True, out=out)
    with torch.no_grad():
        ts = timed_group(fns, reps)
    tag = dict(dtype=str(dtype)[6:], n=n, batch=batch)
    for name in cases:
        base = row(rows, name + ' / dq_apply_diag over the same wires', ts[name + ' / diag'], TB_per_s=round(nbytes / ts[name + ' / diag'][0] / 1e9, 3), **tag)
        row(rows, name, ts[name], TB_per_s=round(nbytes / ts[name][0] / 1e9, 3), time_over_diag=round(ts[name][0] / base, 3), **tag)
    k = backend.qft_passes(n, full, dtype)
    base = row(rows, f'all {n} wires, swap-free: {k} stages', ts['all wires, swap-free'], stages=k, **tag)
    row(rows, f'all {n} wires, swap form: {k} stages and a permute_bits pass', ts['all wires, swap form'],
        time_over_swap_free=round(ts['all wires, swap form'][0] / base, 3), **tag)
    del psi, out
    torch.cuda.empty_cache()


def end_to_end(rows, n, m, reps):
    """``QuantumFourierTransform`` on the first m wires of n behind a layer of rotations: one QFTGate against the gate sequence."""
    res = {}
    for native in (True, False):
        cir = dq.QubitCircuit(n)
        cir.hlayer()
        cir.rylayer(inputs=[0.1 * (i + 1) for i in range(n)])
        cir.add(dq.QuantumFourierTransform(n, minmax=[0, m - 1], native=native))
        cir.to('cuda')
        with torch.no_grad():
            t = timed_group({'f': lambda c=cir: c()}, reps)['f']
            res[native] = cir().reshape(-1).clone()
        row(rows, f'QFT on {m} of {n} wires, complex64: ' + ('one QFTGate' if native else 'the gate sequence, fused passes'), t,
            operators=len(cir.operators), passes=dq.executor.LAST_RUN.get('passes'))
        cir.to('cpu')
        torch.cuda.empty_cache()
    err = (res[True] - res[False]).abs().max().item()
    rows.append({'what': f'QFT on {m} of {n} wires: the routes differ by', 'max_abs': err, 'largest_amplitude': res[True].abs().max().item()})
    print(f'  routes differ by {err:.3e} (largest amplitude {res[True].abs().max().item():.3e})', flush=True)


def main():
    quick = '--quick' in sys.argv
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    assert torch.cuda.is_available(), 'bench_qft.py measures on the GPU: there is no fallback'
    prop = torch.cuda.get_device_properties(0)
    box = {'device': prop.name, 'cus': prop.multi_processor_count, 'memory_GiB': round(prop.total_memory / 2**30, 1),
           'torch': torch.__version__, 'hip': torch.version.hip, 'host': platform.processor() or platform.machine()}
    print('box:', json.dumps(box), flush=True)
    rows = []
    reps = 5 if quick else 11
    stages(rows, torch.complex64, 22 if quick else 28, 4, reps)
    stages(rows, torch.complex128, 21 if quick else 27, 4, reps)
    n = 22 if quick else 28
    for m in (n, 20, 12):
        end_to_end(rows, n, m, 3 if quick else 5)
    if out:
        with open(out, 'w') as f:
            json.dump({'box': box, 'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
