"""Mid-circuit measurement on the MI355X (dq_apply_collapse_*, dq_measure_draw), against
``dq_apply_diag_*`` on the same state and the same bits, timed in the same process, taking turns.

1. Kernels, complex64 n = 28 and complex128 n = 27 at batch 4, k = 1, 3, 10 measured bits at the top of the index,
   straddling the 128-byte line and at the bottom: FULL out of place, FULL in place and DROP.  Bytes charged: the output
   written plus 1 / 2^k of the input read (collapse), the state read and written (the diagonal yardstick).
2. End to end through ``QubitCircuit`` without autograd, complex64 n = 28 at batch 4, a circuit of one operation on a
   given state: ``mid_measure(wires, reset=True)`` against ``Reset(postselect=None)`` on the same wires (marginal, draw
   and collapse against marginal, ``multinomial``, the (B, 2^k, 2^k) matrices and ``apply_gate``).

Every point: one warm-up call, then the median of ``reps`` calls between device events; the rows of a group, yardstick
included, take turns within every repetition.  The box is recorded first.

usage: python tools/bench_collapse.py [--quick] [--out FILE]
"""
import json
import os
import platform
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deepquantum_amd as dq  # noqa: E402
from deepquantum_amd import backend  # noqa: E402
from bench_diag import row, timed_group  # noqa: E402


def placements(n, k, dtype):
    line = 4 if dtype == torch.complex64 else 3                       # the first index bit above a 128-byte line
    lo = max(0, line - k // 2)
    return {'top': list(range(n - 1, n - 1 - k, -1)), 'line': list(range(lo + k - 1, lo - 1, -1)), 'bottom': list(range(k - 1, -1, -1))}


def kernels(rows, dtype, n, batch, reps):
    esz = 8 if dtype == torch.complex64 else 16
    psi = torch.randn(batch, 1 << n, dtype=dtype, device='cuda')
    other = psi.clone()
    out = torch.empty_like(psi)
    sbytes = psi.numel() * esz
    for k in (1, 3, 10):
        small = torch.empty(batch, 1 << (n - k), dtype=dtype, device='cuda')
        diag = torch.exp(1j * torch.randn(1 << k, dtype=torch.float64, device='cuda')).to(dtype)
        outcome = torch.arange(batch, device='cuda') % (1 << k)
        rec = backend.collapse_rec(outcome, torch.full((batch,), 1.25, dtype=torch.float64, device='cuda'))
        for where, bits in placements(n, k, dtype).items():
            tag = f'k={k} {where}'
            yard = f'apply_diag {tag} (yardstick)'
            kept = sbytes >> k
            group = {
                yard: (lambda: backend.apply_diag(psi, diag, bits, out=out), 2 * sbytes),
                f'apply_diag {tag} in place': (lambda: backend.apply_diag(other, diag, bits, out=other), 2 * sbytes),
                f'collapse FULL {tag}': (lambda: backend.collapse(psi, bits, rec, 'full', out=out), sbytes + kept),
                f'collapse FULL {tag} in place': (lambda: backend.collapse(other, bits, rec, 'full', out=other), sbytes + kept),
                f'collapse DROP {tag}': (lambda: backend.collapse(psi, bits, rec, 'drop', out=small), 2 * kept),
            }
            with torch.no_grad():
                ts = timed_group({name: v[0] for name, v in group.items()}, reps)
            base = None
            for name, (_, nbytes) in group.items():
                med = row(rows, name, dtype, n, batch, ts[name], nbytes, base)
                base = med if name == yard else base
            other.copy_(psi)                                          # (the in-place rows have emptied it)
        del small
    del psi, other, out
    torch.cuda.empty_cache()


def end_to_end(rows, n, batch, reps):
    dtype = torch.complex64
    psi = torch.randn(batch, 1 << n, dtype=dtype, device='cuda')
    psi /= psi.norm(dim=-1, keepdim=True)
    state = psi.reshape(batch, -1, 1)
    for k in (1, 3, 10):
        for where, wires in (('top', list(range(k))), ('bottom', list(range(n - k, n)))):
            new, old = dq.QubitCircuit(n), dq.QubitCircuit(n)
            new.mid_measure(wires, reset=True)
            old.reset(wires, postselect=None)
            new.to('cuda')
            old.to('cuda')
            with torch.no_grad():
                ts = timed_group({'old': lambda: old(state=state), 'new': lambda: new(state=state)}, reps)
            nbytes = 2 * psi.numel() * 8
            base = row(rows, f'Reset(postselect=None) k={k} {where}', dtype, n, batch, ts['old'], nbytes)
            row(rows, f'mid_measure(reset=True) k={k} {where}', dtype, n, batch, ts['new'], nbytes, base)
    del psi, state
    torch.cuda.empty_cache()


def main():
    quick = '--quick' in sys.argv
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    assert torch.cuda.is_available(), 'bench_collapse.py measures on the GPU: there is no fallback'
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
    end_to_end(rows, 22 if quick else 28, 4, 3 if quick else 7)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as fh:
            json.dump({'box': box, 'rows': rows}, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
