"""The paths of the single-gate kernels on the MI355X (csrc/dq_gate.hip: apply_small_kernel, copy_uncontrolled_kernel,
apply_big_kernel; csrc/dq_dense.hip: apply_dense56_kernel, apply_dense_mfma_kernel), row by row of `_gate_cases.ROWS` against
complex128 references on the device.  Every row asserts from the mirrors (`_launch_geometry.small_gate` / `.dense`) that
its launch is the path it is the row of, runs a random unitary (|got - ref| <= tau S elementwise, tau derived in
`_gate_cases`) and a signed permutation (bit for bit), holds the uncontrolled amplitudes and, for k <= 4, the in-place result
to bit-for-bit equality, and shows that its criterion rejects the corruptions a broken path would produce.
test_gate_paths_cpu.py proves the mirrors, the table and the references without a GPU.  The worst ratio of every row is
printed (``-s``); DESIGN.md 4.2 holds the table.

With them: the Z-string loop kernels on their default path (n < 8), and the process-wide knobs that choose kernels
(DQ_DENSE_*, DQ_ZMULTI_MFMA, DQ_PERMUTE_LDS), one fresh child process per setting."""

from __future__ import annotations

import os
import subprocess
import sys

import pytest
import torch

import _gate_cases as gc

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('row', gc.ROWS, ids=[r.id for r in gc.ROWS])
def test_gate_path(row):
    res = gc.run_row(row, DEV)
    print(f'\nGATEPATH {row.path} {"c128" if row.c128 else "c64"} {res["route"]} {res["ratio"]:.2e} of its bound ({row.id})')


@pytest.mark.parametrize('c128', [False, True], ids=['c64', 'c128'])
@pytest.mark.parametrize('n', gc.Z_NS)
def test_z_string_loop_kernels_below_eight_qubits(n, c128):
    """expect_zmulti_kernel / scale_zsigns_kernel are the default path for every n < 8: K = 1, 2, 31, 32 (an odd K leaves the
    pair guard of the block sum one string short), 33 (two launches), batch 3, against `_grid_refs`."""
    for k in gc.Z_KS:
        res = gc.check_z_strings(n, k, c128, DEV)
        print(f'\nZSTRINGS n={n} K={k} {"c128" if c128 else "c64"}: sums {res["sums"]:.3e}, amplitudes {res["amps"]:.3e} of their bounds')


def test_the_kernel_choosing_knobs_do_not_change_results():
    """DQ_DENSE_NT, _ROWS_FAST, DQ_DENSE5, DQ_DENSE5_BLOCKS, DQ_DENSE_BIG, DQ_ZMULTI_MFMA and DQ_PERMUTE_LDS are read once per
    process: one fresh child per setting (tests/_gate_knob_child.py), one after the other.  The child judges every knob row
    (`_gate_cases.KNOB_ROWS`) against the reference itself -- the unitary by the bound, the signed permutation bit for bit --
    and the Z-string kernels (n = 1 .. 13: under DQ_ZMULTI_MFMA=0 the loop kernels at n = 8 and 13) and permute_bits at
    nl = 13 (under DQ_PERMUTE_LDS=0 the tiled kernels).  DQ_DENSE_NT, _ROWS_FAST and DQ_DENSE5_BLOCKS only change who does the
    work: there every digest also equals the parent's.  The first child that does not exit 0 ends the test; nothing is
    retried.  What each setting selects among the knob rows is pinned from the mirror in
    test_gate_paths_cpu.py::test_census_every_knob_selected_route_has_a_knob_row."""
    assert not [k for k in gc.KNOB_NAMES if k in os.environ], 'the parent must run with the default environment'
    want = gc.knob_run(DEV, {})
    torch.cuda.empty_cache()
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), '_gate_knob_child.py')
    for knob in gc.KNOBS:
        env = dict(os.environ, **knob)
        done = subprocess.run([sys.executable, child], env=env, timeout=300, capture_output=True, text=True)
        assert done.returncode == 0, (knob, done.returncode, done.stdout[-2000:], done.stderr[-2000:])
        got = [ln.split()[1] for ln in done.stdout.splitlines() if ln.startswith('digest ')]
        assert len(got) == len(want), (knob, len(got), len(want))
        print(f'\nKNOB {knob}:', *[ln[72:] for ln in done.stdout.splitlines() if ln.startswith('digest ') and ' [' in ln], sep='\n  ')
        if next(iter(knob)) in gc.SAME_DIGEST:
            assert got == [d for _, d in want], (knob, [w for (w, d), g in zip(want, got) if d != g])
