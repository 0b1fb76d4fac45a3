"""Gram matrices and linear combinations of state batches on the MI355X (dq_gram_*, dq_combine_*)
against what the package and PyTorch offered before, timed in the same process on the same buffers.

Per shape -- complex64 n = 28 and complex128 n = 27 with M = N in {4, 16} (distinct operands and the self-Gram) and M = N =
32; n = 12 with M = N = 1024, the kernel-methods regime; combine with M = N = 16 -- the rows are
  gram / self-gram          ``backend.gram``
  (a) loop of inner         what the parent commit offers: ``backend.inner`` over all pairs of rows, M * N launches
                            (n = 12: one launch per row of A, the row broadcast over the rows of B -- a million launches
                            would measure nothing else)
  (b) torch.matmul          ``A.conj() @ B.T``: a BLAS, reported, not a target (complex64 accumulates in float32 over the
                            whole row there).  At n = 28 / 27 only with ``--matmul``, one call without a warm-up: the BLAS does not
                            split the long dimension and is slower there by orders of magnitude
  (c) pure read             ``backend.inner(A, B)`` for M = N: dq_inner_* over the same M + N rows (the self-Gram: M rows)
  combine                   ``backend.combine``
  (d) copy                  ``out.copy_(states)``: one read and one write of the same bytes
with the ratios to (c) / (d), TB/s over the bytes charged (every operand row once; combine: one read and one write) and
TFLOP/s (8 flop per complex multiply-add) against the f32 / f64 matrix-core peaks of 157.3 / 78.6.

Every point: one warm-up call, then the median of ``reps`` calls between device events; the rows of a group take turns within
every repetition.  The box is recorded first.

usage: python tools/bench_gram.py [--quick] [--matmul] [--out FILE]
"""
import json
import os
import platform
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from deepquantum_amd import backend  # noqa: E402

PEAK = {torch.complex64: 157.3, torch.complex128: 78.6}


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


def row(rows, what, dtype, n, m, k, t, nbytes, flop=None, base=None, base_name=''):
    med, lo, hi = t
    r = {'what': what, 'dtype': str(dtype)[6:], 'n': n, 'rows': [m, k], 'ms': round(med, 4), 'ms_min': round(lo, 4),
         'ms_max': round(hi, 4), 'bytes': nbytes, 'TB_per_s': round(nbytes / med / 1e9, 3)}
    text = f"{what:<34} {r['dtype']:<10} n={n:<2} {m:>4} x {k:<4} {med:11.4f} ms  [{lo:.4f}, {hi:.4f}]  {r['TB_per_s']:6.3f} TB/s"
    if flop is not None:
        r['TFLOP_per_s'] = round(flop / med / 1e9, 2)
        r['of_matrix_core_peak'] = round(flop / med / 1e9 / PEAK[dtype], 3)
        text += f"  {r['TFLOP_per_s']:7.2f} TFLOP/s ({r['of_matrix_core_peak']:.3f} of peak)"
    if base is not None:
        r['time_over_' + base_name] = round(med / base, 3)
        text += f'  x{med / base:.3f} of {base_name}'
    rows.append(r)
    print(text, flush=True)
    return med


def gram_group(rows, a, b, n, m, reps, loop_reps, matmul='warm', per_row_loop=False):
    """M = N = m rows of the two buffers: distinct operands, then the self-Gram."""
    dtype, esz = a.dtype, a.element_size()
    x, y = a[:m], b[:m]
    row_bytes = (1 << n) * esz
    flop = 8.0 * m * m * (1 << n)

    def loop():
        if per_row_loop:
            for i in range(m):
                backend.inner(x[i:i + 1].expand(m, -1).contiguous(), y)
        else:
            for i in range(m):
                for j in range(m):
                    backend.inner(x[i:i + 1], y[j:j + 1])

    fns = {'gram': lambda: backend.gram(x, y), 'read': lambda: backend.inner(x, y), 'self': lambda: backend.gram(x, x),
           'read_self': lambda: backend.inner(x, x)}
    if matmul == 'warm':
        fns['matmul'] = lambda: torch.matmul(x.conj(), y.T)
    ts = timed_group(fns, reps)
    if matmul == 'once':
        a0, b0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a0.record()
        torch.matmul(x.conj(), y.T)
        b0.record()
        torch.cuda.synchronize()
        ts['matmul'] = (a0.elapsed_time(b0),) * 3
    tl = timed_group({'loop': loop}, loop_reps)['loop']
    base = row(rows, '(c) pure read: inner(A, B)', dtype, n, m, m, ts['read'], 2 * m * row_bytes)
    row(rows, 'gram(A, B)', dtype, n, m, m, ts['gram'], 2 * m * row_bytes, flop, base, 'pure_read')
    row(rows, '(a) loop of inner' + (', one launch per row of A' if per_row_loop else ' over all pairs'), dtype, n, m, m, tl,
        2 * m * m * row_bytes, None, ts['gram'][0], 'gram')
    if matmul:
        row(rows, '(b) torch.matmul(A.conj(), B.T)', dtype, n, m, m, ts['matmul'], 2 * m * row_bytes, flop, ts['gram'][0], 'gram')
    base = row(rows, '(c) pure read: inner(A, A)', dtype, n, m, m, ts['read_self'], m * row_bytes)
    row(rows, 'self-gram(A)', dtype, n, m, m, ts['self'], m * row_bytes, flop / 2, base, 'pure_read')


def combine_group(rows, a, out, n, m, reps):
    dtype, esz = a.dtype, a.element_size()
    s, y = a[:m], out[:m]
    coef = torch.randn(m, m, dtype=torch.complex128, device='cuda')
    nbytes = 2 * m * (1 << n) * esz
    ts = timed_group({'combine': lambda: backend.combine(s, coef, out=y), 'copy': lambda: y.copy_(s)}, reps)
    base = row(rows, '(d) copy: out.copy_(states)', dtype, n, m, m, ts['copy'], nbytes)
    row(rows, 'combine(states, coef)', dtype, n, m, m, ts['combine'], nbytes, 8.0 * m * m * (1 << n), base, 'copy')


def main():
    quick = '--quick' in sys.argv
    big_matmul = '--matmul' in sys.argv
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    assert torch.cuda.is_available(), 'bench_gram.py measures on the GPU: there is no fallback'
    prop = torch.cuda.get_device_properties(0)
    box = {'device': prop.name, 'cus': prop.multi_processor_count, 'memory_GiB': round(prop.total_memory / 2**30, 1),
           'devices_visible': torch.cuda.device_count(), 'torch': torch.__version__, 'hip': torch.version.hip,
           'host': platform.processor() or platform.machine()}
    print('box:', json.dumps(box), flush=True)
    print('geometry:', backend.gram_geometry(torch.complex64), backend.gram_geometry(torch.complex128), flush=True)
    rows = []
    reps = 5 if quick else 9
    with torch.no_grad():
        for dtype, n in ((torch.complex64, 22), (torch.complex128, 21)) if quick else ((torch.complex64, 28), (torch.complex128, 27)):
            a = torch.randn(32, 1 << n, dtype=dtype, device='cuda')
            b = torch.randn(32, 1 << n, dtype=dtype, device='cuda')
            for m in (4, 16, 32):
                gram_group(rows, a, b, n, m, reps, 1 if m == 32 else 3, matmul='once' if big_matmul and m == 16 else '')
            combine_group(rows, a, b, n, 16, reps)
            del a, b
            torch.cuda.empty_cache()
        for dtype in (torch.complex64, torch.complex128):
            m = 256 if quick else 1024
            a = torch.randn(m, 1 << 12, dtype=dtype, device='cuda')
            b = torch.randn(m, 1 << 12, dtype=dtype, device='cuda')
            gram_group(rows, a, b, 12, m, reps, 1, per_row_loop=True)
            del a, b
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as fh:
            json.dump({'box': box, 'rows': rows}, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
