"""Entanglement fixtures made by running the REAL reference here (same mechanism as make_golden.py): the Meyer-Wallach
measure, Brennen's form, the per-wire ``partial_trace`` of psi psi^dagger, d MW / d data of an entangling circuit and
the Hessian of MW with respect to a few circuit inputs.  Only inputs and outputs are stored; states only up to 12
qubits (the larger cases are rebuilt from their inputs by the tests).

usage: python tests/golden/make_golden_entanglement.py      (about a minute)
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

SIZES = (1, 2, 5, 11, 12, 13, 17, 20)
STATE_MAX = 12          # states stored up to this size
BRENNEN_MAX = 12
PTRACE_MAX = 10
HESS_N = 5
HESS_IDX = (0, 3, 6, 8)  # the circuit inputs the Hessian is taken over


def entangling_circuit(dq, n):
    """H layer, Ry encoder, CNOT ring, Rx encoder, CNOT ring: 2 n inputs.  Builder calls common to both libraries."""
    cir = dq.QubitCircuit(n)
    cir.hlayer()
    cir.rylayer(encode=True)
    if n > 1:
        cir.cnot_ring()
    cir.rxlayer(encode=True)
    if n > 1:
        cir.cnot_ring()
    return cir


def circuit_data(n, batch, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(batch, 2 * n, generator=g, dtype=torch.float64) * 2 * torch.pi


def main():
    from make_golden import import_reference, to_np

    dq = import_reference()
    out = {}
    for n in SIZES:
        for prec in ('c64', 'c128'):
            real = torch.float64 if prec == 'c128' else torch.float32
            for batch in (1, 2):
                key = f'{n}/{prec}/b{batch}'
                data = circuit_data(n, batch, seed=100 * n + batch).to(real)
                cir = entangling_circuit(dq, n)
                if prec == 'c128':
                    cir.to(torch.double)
                x = data.clone().requires_grad_(True)
                state = cir(data=x).reshape([batch] + [2] * n)
                mw = dq.qmath.meyer_wallach_measure(state)
                (g,) = torch.autograd.grad(mw.sum(), x)
                out[f'{key}/data'] = to_np(data)
                out[f'{key}/mw'] = to_np(mw)
                out[f'{key}/grad'] = to_np(g)
                st = state.detach()
                if n <= STATE_MAX:
                    out[f'{key}/state'] = to_np(st)
                if n <= BRENNEN_MAX:
                    out[f'{key}/brennen'] = to_np(dq.qmath.meyer_wallach_measure_brennen(st))
                if n <= PTRACE_MAX:
                    rho = st.reshape(batch, -1, 1) @ st.conj().reshape(batch, 1, -1)
                    rdms = [dq.qmath.partial_trace(rho, n, [i for i in range(n) if i != k]).reshape(batch, 2, 2)
                            for k in range(n)]
                    out[f'{key}/rdms'] = to_np(torch.stack(rdms, dim=1))
                print(key, 'mw', to_np(mw))
    # an un-normalised input
    for prec in ('c64', 'c128'):
        st = torch.from_numpy(out[f'5/{prec}/b2/state']) * 1.7
        out[f'unnorm/{prec}/state'] = to_np(st)
        out[f'unnorm/{prec}/mw'] = to_np(dq.qmath.meyer_wallach_measure(st))
        out[f'unnorm/{prec}/brennen'] = to_np(dq.qmath.meyer_wallach_measure_brennen(st))
    # Hessian of MW over four circuit inputs (the others held), n = 5
    for prec in ('c64', 'c128'):
        real = torch.float64 if prec == 'c128' else torch.float32
        base = circuit_data(HESS_N, 1, seed=7).to(real)

        def f(v):
            d = base.clone()
            d[0, list(HESS_IDX)] = v
            cir = entangling_circuit(dq, HESS_N)
            if prec == 'c128':
                cir.to(torch.double)
            return dq.qmath.meyer_wallach_measure(cir(data=d).reshape([1] + [2] * HESS_N)).sum()

        v0 = base[0, list(HESS_IDX)].clone()
        h = torch.autograd.functional.hessian(f, v0)
        out[f'hessian/{prec}/data'] = to_np(base)
        out[f'hessian/{prec}/hessian'] = to_np(h)
        print('hessian', prec, to_np(h))
    path = os.path.join(HERE, 'golden_entanglement.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
