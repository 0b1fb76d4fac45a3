"""Host time per call of the streaming primitives' wrappers, and of the generator nodes of ``ops`` on top of them (a
rotation forward plus backward with a trainable angle), where launches dominate: n = 12, batch 1, complex64.

    python tools/bench_stream_host.py [--package-root DIR] [--calls 4000] [--warmup 500] [--out FILE]

Every call is timed on the host alone (``perf_counter_ns`` around the call, nothing synchronised); the device is
synchronised once, after the last call of a row.  Prints the median and the quartiles in microseconds per call and one
JSON line.  ``--package-root``: import ``deepquantum_amd`` from there (a built checkout of another commit) instead of
from this tree -- profiles/stream_host/ compares two commits that way."""

import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--package-root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--calls', type=int, default=4000)
    ap.add_argument('--warmup', type=int, default=500)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch

    import deepquantum_amd
    from deepquantum_amd import backend, ops

    n, k = 12, 3
    bits, dt = (7, 0, 4), torch.complex64
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 1 << n, dtype=torch.complex128, generator=g).to(dt).cuda()
    out = torch.empty_like(x)
    diag = torch.randn(1 << k, dtype=torch.complex128, generator=g).to(dt).cuda()
    cost = torch.randn(1 << k, generator=g).cuda()
    theta = torch.tensor([0.3], dtype=torch.float64).cuda()
    src = torch.tensor([5, 2, 7, 0, 3, 6, 1, 4]).cuda()
    u = torch.linalg.qr(torch.randn(1 << k, 2, 2, dtype=torch.complex128, generator=g))[0].to(dt).cuda()
    # the generator nodes of `ops` and what they call: a second state, a state rotated in place, an excitation
    # (xmask, amask, zmask, negate, controls) with a string bit and a control, a trainable angle, a cotangent
    y = torch.randn(1, 1 << n, dtype=torch.complex128, generator=g).to(dt).cuda()
    state, gy = x.clone(), y.clone()
    spec = (0b10010000, 0b00010000, 0b00100000, 1, (2,))
    angle = torch.tensor([0.3], dtype=torch.float64, device='cuda', requires_grad=True)
    rows = {
        'apply_diag': lambda: backend.apply_diag(x, diag, bits, (), out=out),
        'apply_pauli_rot': lambda: backend.apply_pauli_rot(x, 0b10010001, 0b00010001, theta, (), out=out),
        'apply_permutation': lambda: backend.apply_permutation(x, src, bits, (), out=out),
        'apply_mux': lambda: backend.apply_mux(x, u, 'u', 2, bits, (), out=out),
        'cost_cross': lambda: backend.cost_cross(x, x, cost, bits, ()),
        'apply_excite_rot': lambda: backend.apply_excite_rot(state, spec, theta, out=state),
        'pauli_cross': lambda: backend.pauli_cross(x, y, 0b10010001, 0b00010001, ()),
        'excite_cross': lambda: backend.excite_cross(x, y, spec),
        'ops.pauli_rot fwd+bwd': lambda: ops.pauli_rot(x, 0b10010001, 0b00010001, angle).backward(gy),
        'ops.excite_rot fwd+bwd': lambda: ops.excite_rot(x, spec, angle).backward(gy),
    }
    result = {'package': os.path.dirname(os.path.abspath(deepquantum_amd.__file__)), 'n': n, 'batch': 1, 'dtype': 'complex64',
              'calls': args.calls, 'warmup': args.warmup, 'us_per_call': {}}
    for name, f in rows.items():
        for _ in range(args.warmup):
            f()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.calls):
            t0 = time.perf_counter_ns()
            f()
            times.append(time.perf_counter_ns() - t0)
        torch.cuda.synchronize()
        q1, med, q3 = (v / 1e3 for v in statistics.quantiles(times, n=4))
        result['us_per_call'][name] = {'median': round(med, 3), 'q1': round(q1, 3), 'q3': round(q3, 3)}
        print(f'{name:24s} median {med:8.3f} us   quartiles {q1:8.3f} .. {q3:8.3f}', flush=True)
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
