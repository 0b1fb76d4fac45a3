"""k-wire reduced density matrices on the MI355X: the matrix-core reduction (``backend.rdmk_cross``, dq_rdmk_cross_*)
against the GEMM fallback it replaces (``backend._gate_grad_gemm``: two permuted copies of the state, then rocBLAS),
alternated in one process.  n = 28, batch 16, complex64 and n = 28, batch 8, complex128; k in {3, 4, 5, 6, 8, 10}; wire
sets on the lowest index bits, the highest and scattered.  Both routes are timed on x == gy (the Hermitian case: the
reduced density matrix) and the new one also on x != gy (a gate's matrix cotangent).

Bytes and flops come from the shapes: the state is read once (twice for x != gy), 8 4^k K real flops (K = 2^(n-k));
the Hermitian case counts the flops of the tiles it computes (64 x 64 tiles on or above the diagonal: all of them up to
k = 6, 10 of 16 at k = 8, 136 of 256 at k = 10).  The binding peak is the larger of bytes / HBM and flops / MFMA (6 TB/s
and 155 / 78 TFLOP/s for f32 / f64 inputs, the figures of DESIGN §4.6).  Also: the eigensolver time of
``entanglement_entropy`` at k = 10 (one 1024 x 1024 Hermitian matrix per sample), reported separately.

usage: python tools/bench_rdm.py [--quick] [--no-gemm]      (--no-gemm: the new route only, e.g. under a profiler)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from deepquantum_amd import backend, qmath  # noqa: E402

HBM = 6e12
MFMA = {torch.complex64: 155e12, torch.complex128: 78e12}


def timed(f, reps):
    f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def wire_sets(n, k):
    step = max(1, (n - 1) // (k - 1)) if k > 1 else 1
    return {'low': list(range(k)), 'high': list(range(n - k, n)),
            'scattered': sorted({min(n - 1, i * step) for i in range(k)} | {0})[:k]}


def main():
    quick = '--quick' in sys.argv
    n = 22 if quick else 28
    rounds = 2
    with_gemm = '--no-gemm' not in sys.argv
    for dtype, batch in ((torch.complex64, 16), (torch.complex128, 8)):
        psi = torch.randn(batch, 1 << n, dtype=dtype, device='cuda')
        psi /= psi.norm(dim=-1, keepdim=True)
        sbytes = psi.numel() * psi.element_size()
        print(f'# n={n} batch={batch} {str(dtype)[6:]}: state {sbytes / 2**30:.1f} GiB')
        print('k  wires      route      ms       GB/s   TFLOP/s  of-peak  bound')
        for k in (3, 4, 5, 6, 8, 10):
            for name, wires in wire_sets(n, k).items():
                if len(set(wires)) != k:
                    continue
                tg = [n - 1 - w for w in wires]
                K = 1 << (n - k)
                fl_full = 8.0 * (4**k) * K * batch
                # the Hermitian route computes the tiles on or above the diagonal (64 x 64, one tile up to k = 6)
                nt = max(1, (1 << k) // 64)
                fl_herm = fl_full * (nt * (nt + 1) // 2) / (nt * nt)
                reps = 1 if k == 10 else 3
                # the fallback: two permuted copies of the state (skipped when they do not fit beside it)
                gemm_ok = 3 * sbytes < torch.cuda.mem_get_info()[0]
                runs = {'rdmk': [], 'gemm': []}
                for _ in range(rounds):
                    with torch.no_grad():
                        runs['rdmk'].append(timed(lambda: backend.rdmk_cross(psi, psi, tg), reps))
                        if with_gemm and gemm_ok and k <= 8:
                            runs['gemm'].append(timed(lambda: backend._gate_grad_gemm(psi, psi, n, tg, []), 1))
                for route, ts in runs.items():
                    if not ts:
                        continue
                    ms = sorted(ts)[len(ts) // 2]
                    fl = fl_herm if route == 'rdmk' else fl_full
                    gbs = sbytes / (ms * 1e-3) / 1e9
                    tf = fl / (ms * 1e-3) / 1e12
                    t_hbm, t_mma = sbytes / HBM, fl / MFMA[dtype]
                    bound = 'HBM' if t_hbm >= t_mma else 'MFMA'
                    frac = max(t_hbm, t_mma) / (ms * 1e-3)
                    print(f'{k:<2} {name:<10} {route + "-herm":<10} {ms:8.2f} {gbs:8.0f} {tf:8.1f} {frac:8.2f}  {bound}')
                if name == 'scattered':
                    gy = psi.roll(1, 0)
                    with torch.no_grad():
                        ms = sorted(timed(lambda: backend.rdmk_cross(psi, gy, tg), reps) for _ in range(rounds))[rounds // 2]
                    t_hbm, t_mma = 2 * sbytes / HBM, fl_full / MFMA[dtype]
                    print(f'{k:<2} {name:<10} {"rdmk-cross":<10} {ms:8.2f} {2 * sbytes / (ms * 1e-3) / 1e9:8.0f} '
                          f'{fl_full / (ms * 1e-3) / 1e12:8.1f} {max(t_hbm, t_mma) / (ms * 1e-3):8.2f}  '
                          f'{"HBM" if t_hbm >= t_mma else "MFMA"}')
                    del gy
        del psi
        torch.cuda.empty_cache()
    # the eigensolver of entanglement_entropy at k = 10, on its own
    for batch in (1, 16):
        rho = torch.randn(batch, 1024, 1024, dtype=torch.complex128, device='cuda')
        rho = rho @ rho.mH
        ms = timed(lambda: qmath._entropy_of(rho, 1.0, None, 1e-12), 2)
        print(f'entanglement_entropy eigensolver, k = 10, batch {batch}: {ms:.1f} ms')


if __name__ == '__main__':
    main()
