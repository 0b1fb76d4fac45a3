"""Pauli-rotation fixtures made by running the REAL reference here (same mechanism as make_golden.py): the entangling
circuit of make_golden_entanglement.py followed by three ``HamiltonianGate([[1.0, s]], t=theta / 2)`` =
``exp(-i theta/2 P)`` -- weights 1 to 5, with Ys and with gaps -- the same with the three gates inverted by the
reference's own ``inverse()``, and one variant per size with a control on the middle gate.  n in {3, 6, 8}, complex64
and complex128; states only.

GPU tests import ``SIZES`` / ``VARIANTS`` / ``gates_of`` from here, so the reference is imported inside ``main()`` only.

usage: python tests/golden/make_golden_pauli.py      (a few seconds)
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

SIZES = (3, 6, 8)
VARIANTS = ('plain', 'inv', 'ctrl')
# (Pauli string with wires, theta, controls): thetas are dyadic, exact in float32
CASES = {
    3: (('x0', 0.75, None), ('y1z2', -1.3125, None), ('y0x1y2', 2.125, None)),
    6: (('y4', 0.75, None), ('x1z3y4', -1.3125, None), ('y0y1x3y4z5', 2.125, None)),
    8: (('z6', 0.75, None), ('y1x6', -1.3125, None), ('x0y2z3y6x7', 2.125, None)),
}
CONTROL = {3: 0, 6: 5, 8: 0}          # the control wire of the middle gate in the 'ctrl' variant (outside the gate's span: the
                                      # reference builds its matrix on the whole range of wires)


def gates_of(n, variant):
    gates = list(CASES[n])
    if variant == 'ctrl':
        s, theta, _ = gates[1]
        gates[1] = (s, theta, [CONTROL[n]])
    return gates


def main():
    from make_golden import import_reference, to_np
    from make_golden_entanglement import circuit_data, entangling_circuit

    dq = import_reference()
    out = {}
    for n in SIZES:
        for prec in ('c64', 'c128'):
            real = torch.float64 if prec == 'c128' else torch.float32
            data = circuit_data(n, 1, seed=500 + n).to(real)
            out[f'{n}/{prec}/data'] = to_np(data)
            for variant in VARIANTS:
                rots = dq.QubitCircuit(n)
                for s, theta, controls in gates_of(n, variant):
                    rots.hamiltonian([[1.0, s]], t=theta / 2, controls=controls)
                cir = entangling_circuit(dq, n)
                cir += rots.inverse() if variant == 'inv' else rots
                if prec == 'c128':
                    cir.to(torch.double)
                with torch.no_grad():
                    st = cir(data=data).reshape(1, -1)
                out[f'{n}/{prec}/{variant}'] = to_np(st)
                print(n, prec, variant, 'norm', float((st.conj() * st).sum().real))
    path = os.path.join(HERE, 'golden_pauli.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
