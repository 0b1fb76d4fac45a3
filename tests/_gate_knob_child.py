"""Child process of test_gate_paths_gpu.py::test_the_kernel_choosing_knobs_do_not_change_results: runs `_gate_cases.knob_run`
on the GPU under whatever DQ_DENSE_* / DQ_ZMULTI_MFMA / DQ_PERMUTE_LDS setting its environment holds -- every knob row
against the reference, the signed permutations bit for bit -- and prints one digest line per check."""

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import _gate_cases as gc  # noqa: E402


def main():
    for what, dig in gc.knob_run('cuda', os.environ):
        print('digest', dig, what, flush=True)


if __name__ == '__main__':
    main()
