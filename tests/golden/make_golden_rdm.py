"""k-wire reduced density matrix fixtures made by running the REAL reference here (same mechanism as make_golden.py):
the state of the entangling circuit of make_golden_entanglement.py, the reference's ``partial_trace(psi psi^dagger, n,
complement)`` for several sorted wire sets, and <psi|psi>.  n in {3, 6, 9, 12}, complex64 and complex128.

GPU tests import ``WIRE_SETS`` / ``SIZES`` from here, so the reference is imported inside ``main()`` only.

usage: python tests/golden/make_golden_rdm.py      (a few seconds)
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

SIZES = (3, 6, 9, 12)
WIRE_SETS = {
    3: ([0, 1, 2], [0, 2]),
    6: ([0, 1, 2], [1, 3, 5], [0, 2, 3, 5]),
    9: ([0, 4, 8], [2, 3, 4, 5], [0, 1, 2, 3, 7, 8]),
    12: ([0, 5, 11], [1, 2, 3, 4, 6], [6, 7, 8, 9, 10, 11]),
}


def wires_key(wires):
    return '-'.join(str(w) for w in wires)


def main():
    from make_golden import import_reference, to_np
    from make_golden_entanglement import circuit_data, entangling_circuit

    dq = import_reference()
    out = {}
    for n in SIZES:
        for prec in ('c64', 'c128'):
            real = torch.float64 if prec == 'c128' else torch.float32
            key = f'{n}/{prec}'
            data = circuit_data(n, 1, seed=300 + n).to(real)
            cir = entangling_circuit(dq, n)
            if prec == 'c128':
                cir.to(torch.double)
            with torch.no_grad():
                st = cir(data=data).reshape(1, -1)
            out[f'{key}/data'] = to_np(data)
            out[f'{key}/state'] = to_np(st)
            out[f'{key}/norm'] = to_np((st.conj() * st).sum(-1).real)
            rho = st.reshape(1, -1, 1) @ st.conj().reshape(1, 1, -1)
            for wires in WIRE_SETS[n]:
                traced = [i for i in range(n) if i not in wires]
                red = dq.qmath.partial_trace(rho, n, traced).reshape(1, 1 << len(wires), 1 << len(wires))
                out[f'{key}/rdm/{wires_key(wires)}'] = to_np(red)
            print(key, 'norm', out[f'{key}/norm'])
    path = os.path.join(HERE, 'golden_rdm.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
