"""Meyer-Wallach measure on the MI355X: the forward and backward at n = 28, batch 16, complex64 (32 GiB per read of
the state; bytes = state transfers x state size, as a fraction of 8 TB/s), and the entangling capability of a 12-qubit
H / Ry / CNOT-ring ansatz over 4096 parameter draws -- circuit plus measure, batched -- against the same number taken
the reference's way (one permute and three inner products per wire, plain torch on the GPU).

usage: python tools/bench_entanglement.py [n] [batch]
"""
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deepquantum_amd as dq  # noqa: E402

PEAK = 8e12


def timed(f, reps=5):
    f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def mw_by_permutes(st):
    """The reference's way: for each wire, the |0> and |1> projections and three inner products of them."""
    b, n = st.shape[0], st.ndim - 1
    acc = 0
    for k in range(n):
        x = st.movedim(k + 1, 1)
        lo, hi = x[:, 0].reshape(b, -1), x[:, 1].reshape(b, -1)
        nlo, nhi = (lo.conj() * lo).sum(-1).real, (hi.conj() * hi).sum(-1).real
        ov = (lo.conj() * hi).sum(-1)
        acc = acc + nlo * nhi - ov.abs() ** 2
    return acc * 4 / n


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 28
    batch = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    psi = torch.randn(batch, 1 << n, dtype=torch.complex64, device='cuda')
    psi /= psi.norm(dim=-1, keepdim=True)
    st = psi.reshape([batch] + [2] * n)
    sbytes = psi.numel() * psi.element_size()
    passes = 1 + max(0, math.ceil((n - 12) / 8))
    with torch.no_grad():
        ms = timed(lambda: dq.meyer_wallach_measure(st))
    print(f'meyer_wallach_measure n={n} batch={batch} c64: {ms:.2f} ms, {passes} reads of {sbytes / 2**30:.0f} GiB, '
          f'{passes * sbytes / (ms * 1e-3) / PEAK:.2f} of 8 TB/s')
    x = st.detach().requires_grad_(True)
    y = dq.meyer_wallach_measure(x).sum()
    ms = timed(lambda: torch.autograd.grad(y, x, retain_graph=True))
    moves = 2 * passes + 2 * (passes - 1)      # the wire sum: psi read per pass, out written per pass, read back after
    print(f'  backward: {ms:.2f} ms, {moves} state transfers, {moves * sbytes / (ms * 1e-3) / PEAK:.2f} of 8 TB/s')
    del psi, st, x, y
    torch.cuda.empty_cache()

    nq, draws = 12, 4096
    cir = dq.QubitCircuit(nq)
    cir.hlayer()
    cir.rylayer(encode=True)
    cir.cnot_ring()
    cir.to('cuda')
    data = torch.rand(draws, nq, device='cuda') * 2 * math.pi
    with torch.no_grad():
        def ours():
            return dq.meyer_wallach_measure(cir(data=data).reshape([draws] + [2] * nq)).mean()

        def theirs():
            return mw_by_permutes(cir(data=data).reshape([draws] + [2] * nq)).mean()

        a, b = ours(), theirs()
        t_ours, t_theirs = timed(ours), timed(theirs)
    print(f'entangling capability, {nq} qubits, {draws} draws: {float(a):.6f} in {t_ours:.2f} ms; '
          f'by permutes and inner products {float(b):.6f} in {t_theirs:.2f} ms ({t_theirs / t_ours:.1f}x)')


if __name__ == '__main__':
    main()
