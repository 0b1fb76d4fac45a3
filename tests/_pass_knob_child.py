"""Child process of test_pass_paths_gpu.py::test_the_measurement_knobs_do_not_change_results: runs `_pass_cases.KNOB_ROWS`
on the GPU under whatever DQ_WAVE_* setting its environment holds and prints one digest line per row."""

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import _pass_cases as pc  # noqa: E402


def main():
    for row in pc.KNOB_ROWS:
        pl = pc.plan(row)
        state, acc = pc.run_kernel(row, pl, pc.input_state(row, 'cuda'))
        print('digest', pc.digest(state, acc), row.id, flush=True)
        del state, acc


if __name__ == '__main__':
    main()
