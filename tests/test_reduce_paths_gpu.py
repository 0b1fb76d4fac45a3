"""The paths of the reduction kernels on the MI355X (csrc/dq_reduce.hip), row by row of `_reduce_cases.ROWS` and
`_reduce_cases.Z_ROWS` against float64 / complex128 references on the device.  Every row asserts from the mirrors in
`_launch_geometry` that its launch is the path it is the row of, runs an integer-valued input (the result equals the
reference bit for bit, whatever the order of the additions and the atomics) and a seeded normalised state (within the
project's bound for the kernel's accumulation), and shows that the bound rejects what a broken version of the path would
give.  test_reduce_paths_cpu.py proves the mirrors, the table and the references without a GPU.  The worst ratio of every
row is printed (``-s``); DESIGN.md 4.3 holds the table.

More than one tile per workgroup of gate_grad_multi needs n >= 22 and stays with test_grid_paths_gpu.py, like the second
iteration of every grid-stride loop; DQ_ZMULTI_MFMA has its knob test in test_gate_paths_gpu.py."""

from __future__ import annotations

import pytest

import _grid_refs as R
import _reduce_cases as rc
from deepquantum_amd import backend

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('row', rc.ROWS, ids=[r.id for r in rc.ROWS])
def test_reduce_path(row):
    res = rc.run_row(row, DEV)
    print(f'\nREDUCEPATH {row.path} {row.prec} {res["ratio"]:.2e} of its bound ({row.id})')


@pytest.mark.parametrize('n,c128,what', rc.Z_ROWS, ids=rc.Z_IDS)
def test_z_string_path(n, c128, what):
    """expect_zmulti_mfma_kernel (K = 16, 17, 32) and scale_zsigns_mfma_kernel (K = 1, 4, 5, 32; K = 33: two launches) at the sizes
    where slices of a workgroup fall past the end of the state (n = 8 .. 10), where a whole workgroup has no work
    (complex64, n = 11, 12) and where waves of the scaling kernel are idle (n = 8, 9), with masks that isolate one factor
    of the sign decomposition each, among the strings 0 .. 15 and among 16 .. 31.

    K = 33 is two launches of 32 + 1 strings; `backend.scale_z_signs` adds them in complex128 whatever the state's precision,
    so the bound of one rounding, (u_T + (K + 1) 2^-53) |a| sum_k |c_k|, holds for it as for one launch."""
    res = rc.run_z_row(n, c128, what, DEV)
    print(f'\nREDUCEPATH z-{what}-n{n} {"c128" if c128 else "c64"} {res["ratio"]:.2e} of its bound')


@pytest.mark.parametrize('wide_bytes', [16 << 13, 16 << 12, 16 << 9], ids=['two-samples-then-one', 'a-sample-each', 'runs-within-a-sample'])
def test_scale_z_signs_slices_of_the_wide_path(wide_bytes, monkeypatch):
    """A complex64 state with more than 32 strings is widened slice by slice (`backend._scale_z_signs_wide`): whole samples
    (2 + 1 and 1 + 1 + 1 of batch 3 at n = 12), or runs of 2^9 amplitudes of a sample with the sign of the index bits above
    them folded into the run's coefficients.  K = 33 and 70 (two and three launches).  The slicing changes no arithmetic:
    the integer input equals the reference and the random input the unsliced result, both bit for bit."""
    n = 12
    for k in (33, 70):
        masks = rc.z_masks(n, 33, True) + rc.z_masks(n, 33, False) + [0b101, 1 << 11, 0b111000000000, 1]
        masks = masks[:k]
        for kind in rc.KINDS:
            x, coef = rc.z_inputs(n, False, k, kind, DEV)
            whole = backend.scale_z_signs(x, masks, coef)
            with monkeypatch.context() as mp:
                mp.setattr(backend, '_WIDE_BYTES', wide_bytes)
                sliced = backend.scale_z_signs(x, masks, coef)
            assert rc.bits_equal(sliced, whole.to(rc.C128)), (k, kind)
            ref = R.scale_z_signs(x, masks, coef)
            if kind == 'exact':
                assert float(ref.abs().max()) < 2 ** 24 and rc.bits_equal(sliced, ref), (k, kind)
            else:
                assert rc._scale_ratio(sliced, ref, rc.scale_bound(x, coef, False)) <= 1.0, (k, kind)
