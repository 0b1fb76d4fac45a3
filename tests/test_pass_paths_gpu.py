"""The launch paths of the wave-tile pass kernel on the MI355X (csrc/dq_wave.hip: what wave_launch and the kernel's
prologue and epilogue decide from the size of the job), row by row of `_pass_cases.ROWS` against complex128 references on
the device.  Every row asserts from the mirror of wave_launch (`_launch_geometry.wave_pass`) that one of its passes reaches
the path it is the row of; exact rows must equal the reference bit for bit, state and sums, rounding rows stay within the
bounds derived in `_handler_cases`; every row shows that its criterion rejects the corruptions a wrong launch path would
produce.  The criteria, the paths and the negative controls are described in `_pass_cases`; test_pass_paths_cpu.py proves
the mirror, the references and the rows without a GPU.  The worst ratio of every path is printed (``-s``); DESIGN.md 4.0
holds the table."""

from __future__ import annotations

import os
import subprocess
import sys

import pytest
import torch

import _pass_cases as pc

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('row', pc.ROWS, ids=[r.id for r in pc.ROWS])
def test_pass_path(row):
    res = pc.run_row(row, DEV)
    sums = '' if res['sums'] is None else f', sums {res["sums"]:.3f} of their bound'
    drop = '' if res['sums_reject_i'] is not False else '; the sums alone do NOT reject a dropped tile (the exact row of the path does)'
    print(f'\n{row.id}: state {res["state"]:.3f} of its bound{sums}{drop}')
    torch.cuda.empty_cache()


def test_the_measurement_knobs_do_not_change_results():
    """DQ_WAVE_NT, _TILE_ORDER, _XCD, _TPW, _GRAD_TPW, _EXPZ_TPW, _XCD_TPW are read once per process: one fresh child per
    setting (tests/_pass_knob_child.py), one after the other, on an exact reducing row and an exact forward row
    (`_pass_cases.KNOB_ROWS`, sized so that DQ_WAVE_GRAD_TPW = 8 walks eight tiles per wave and DQ_WAVE_TPW = 2 two).  The rows
    are exact, so the digest of state and sums equals the parent's, which is itself held against the reference here.  The
    first child that does not exit 0 ends the test; nothing is retried.  What each setting changes in the launches of the two
    rows is pinned from the mirror in test_pass_paths_cpu.py::test_what_the_knobs_change_in_the_knob_rows."""
    assert not [k for k in os.environ if k.startswith('DQ_WAVE_')], 'the parent must run with the default environment'
    want = []
    for row in pc.KNOB_ROWS:
        assert pc.run_row(row, DEV)['state'] == 0.0
        pl = pc.plan(row)
        want.append(pc.digest(*pc.run_kernel(row, pl, pc.input_state(row, DEV))))
        torch.cuda.empty_cache()
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), '_pass_knob_child.py')
    for knob in pc.KNOBS:
        env = dict(os.environ, **knob)
        done = subprocess.run([sys.executable, child], env=env, timeout=300, capture_output=True, text=True)
        assert done.returncode == 0, (knob, done.returncode, done.stdout[-2000:], done.stderr[-2000:])
        got = [ln.split()[1] for ln in done.stdout.splitlines() if ln.startswith('digest ')]
        assert got == want, (knob, got, want)
