"""Shot sampling on the MI355X: the inverse-CDF sampler (``backend.sample_indices`` / ``qmath.sample``, dq_sample_*)
against ``qmath.measure(sampler='multinomial')`` -- |psi|^2 for the whole batch, then ``torch.multinomial`` per sample --
on the same state in one process.  complex64 n = 28 at batch 1 and 4, complex128 n = 27 at batch 1; shots 1024 and 2^16.

Per point: the tree build (a ``sample_indices`` call with ONE shot: the build, the upper levels and one descent wave --
the kernels cannot be launched apart from Python; the kernel trace of a profiler run has them one by one), the descent
(the call with all the shots minus the call with one, medians of 9 runs each: a small difference of two larger numbers
at 1024 shots), ``qmath.sample`` end to end (uniforms included, outcomes left on the device), ``measure`` of the
multinomial route end to end (it returns host dicts), and ``torch.cuda.max_memory_allocated`` above the state for both
routes (the sampler's tree is dropped first, so it is counted).  The build is one read of the state: its rate is set
against ``dq_expect_pauli_*`` (a Z string: one read as well) on the same state in the same run.

usage: python tools/bench_sample.py [--quick] [--no-measure]   (--no-measure: the new route only, e.g. under a profiler)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from deepquantum_amd import backend, qmath  # noqa: E402


def timed(f, reps):
    f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def peak_above(f):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = f()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def main():
    quick = '--quick' in sys.argv
    with_measure = '--no-measure' not in sys.argv
    points = ((torch.complex64, 28, 1), (torch.complex64, 28, 4), (torch.complex128, 27, 1))
    if quick:
        points = ((torch.complex64, 22, 1), (torch.complex64, 22, 4), (torch.complex128, 21, 1))
    print('dtype  n  batch  shots |  expect_pauli    build + 1 shot        | all - 1 shot  sample()  measure(multinomial) | above the state, MiB')
    print('                       |    ms    GB/s     ms    GB/s  ratio |      ms          ms         ms            |  sample   measure')
    for dtype, n, batch in points:
        psi = torch.randn(batch, 1 << n, dtype=dtype, device='cuda')
        psi /= psi.norm(dim=-1, keepdim=True)
        sbytes = psi.numel() * psi.element_size()
        with torch.no_grad():
            t_exp = timed(lambda: backend.expect_pauli(psi, 0, 1), 9)
            u1 = torch.rand(batch, 1, dtype=torch.float64, device='cuda')
            t_build = timed(lambda: backend.sample_indices(psi, u1), 9)
            for shots in (1024, 1 << 16):
                u = torch.rand(batch, shots, dtype=torch.float64, device='cuda')
                t_all = timed(lambda: backend.sample_indices(psi, u), 9)
                t_sample = timed(lambda: qmath.sample(psi, n, shots=shots), 5)
                backend.clear_sample_workspace()
                m_sample = peak_above(lambda: qmath.sample(psi, n, shots=shots))
                if with_measure:
                    t_meas = timed(lambda: qmath.measure(psi, shots=shots, sampler='multinomial'), 1)
                    m_meas = peak_above(lambda: qmath.measure(psi, shots=shots, sampler='multinomial'))
                else:
                    t_meas = m_meas = float('nan')
                print(f'{str(dtype)[6:]:<10} {n} {batch:>3} {shots:>7} | {t_exp:6.2f} {sbytes / t_exp / 1e6:7.0f} '
                      f'{t_build:6.2f} {sbytes / t_build / 1e6:7.0f} {t_exp / t_build:6.2f} | {t_all - t_build:9.3f}    '
                      f'{t_sample:8.2f} {t_meas:10.1f}           | {m_sample:8.1f} {m_meas:9.1f}')
        del psi
        backend.clear_sample_workspace()
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
