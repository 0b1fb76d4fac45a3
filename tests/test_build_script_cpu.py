"""The guards of ``csrc/build.sh``, executed: the script is copied into a temporary ``pkg/csrc/`` beside empty sources and
headers and run with ``HIPCC`` pointing at a stub that records its arguments, creates the file after ``-o`` and prints
a chosen remark text for a chosen source.  No compiler, no GPU; the package's own ``build/`` and library are not touched."""

import os
import re
import shutil
import stat
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'deepquantum_amd', 'csrc')
NO_SCRATCH = ['dq_select', 'dq_gram', 'dq_qft', 'dq_terms', 'dq_collapse']
STUB = '''#!/bin/bash
echo "$*" >> "$STUB_LOG"
src=""
while [[ $# -gt 0 ]]; do
  if [[ "$1" == -o ]]; then : > "$2"; fi
  if [[ "$1" == -c ]]; then src="$(basename "$2" .hip)"; fi
  shift
done
if [[ -n "$src" && -f "$STUB_REMARKS/$src" ]]; then cat "$STUB_REMARKS/$src" >&2; fi
exit 0
'''
CLEAN = 'remark: Function Name: some_kernel\nremark:     VGPRs: 64\nremark:     ScratchSize [bytes/lane]: 0\nremark:     VGPRs Spill: 0\n'


def wave_block(vgprs, spill):
    return ('dq_wave.hip:1:1: remark: Function Name: wave_pass_kernel<0> [-Rpass-analysis=kernel-resource-usage]\n'
            'dq_wave.hip:1:1: remark:     SGPRs: 96 [-Rpass-analysis=kernel-resource-usage]\n'
            f'dq_wave.hip:1:1: remark:     VGPRs: {vgprs} [-Rpass-analysis=kernel-resource-usage]\n'
            'dq_wave.hip:1:1: remark:     AGPRs: 0 [-Rpass-analysis=kernel-resource-usage]\n'
            'dq_wave.hip:1:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]\n'
            'dq_wave.hip:1:1: remark:     Occupancy [waves/SIMD]: 3 [-Rpass-analysis=kernel-resource-usage]\n'
            f'dq_wave.hip:1:1: remark:     SGPRs Spill: {spill} [-Rpass-analysis=kernel-resource-usage]\n'
            f'dq_wave.hip:1:1: remark:     VGPRs Spill: {spill} [-Rpass-analysis=kernel-resource-usage]\n')


@pytest.fixture
def run_build(tmp_path):
    """``run(remarks)``: the build script in a fresh tree, ``remarks`` = {object name: what its compile prints to stderr};
    returns (exit status, stderr, the stub's command lines, the sources the script lists)."""
    count = [0]

    def run(remarks):
        count[0] += 1
        root = tmp_path / f'run{count[0]}'
        csrc = root / 'pkg' / 'csrc'
        csrc.mkdir(parents=True)
        (root / 'include').mkdir()
        (root / 'include' / 'dq_hip.h').touch()
        (root / 'remarks').mkdir()
        shutil.copy(os.path.join(CSRC, 'build.sh'), csrc / 'build.sh')
        text = (csrc / 'build.sh').read_text()
        srcs = re.search(r'^srcs=\((.*)\)$', text, re.M).group(1).split()
        for name in srcs + [f for f in os.listdir(CSRC) if f.endswith(('.hpp', '.inc'))]:
            (csrc / name).touch()
        stub = root / 'hipcc_stub.sh'
        stub.write_text(STUB)
        stub.chmod(stub.stat().st_mode | stat.S_IXUSR)
        for name, out in remarks.items():
            (root / 'remarks' / name).write_text(out)
        log = root / 'stub.log'
        env = {**os.environ, 'HIPCC': str(stub), 'STUB_LOG': str(log), 'STUB_REMARKS': str(root / 'remarks')}
        env.pop('DQ_HIPCC_EXTRA', None)
        done = subprocess.run(['bash', str(csrc / 'build.sh')], env=env, capture_output=True, text=True, timeout=60)
        return done.returncode, done.stderr, log.read_text().splitlines(), srcs

    return run


def test_a_clean_run_compiles_every_source_once_and_links(run_build):
    rc, err, lines, srcs = run_build({name: CLEAN for name in NO_SCRATCH + ['dq_wave']})
    assert rc == 0, err
    assert len(srcs) >= 23 and len(lines) == len(srcs) + 1
    compiles = [ln for ln in lines if ' -c ' in ln]
    assert sorted(os.path.basename(ln.split(' -c ')[1].split()[0]) for ln in compiles) == sorted(srcs)
    link = [ln for ln in lines if ' -c ' not in ln]
    assert len(link) == 1 and '-shared' in link[0] and link[0].endswith('libdqhip.so')
    kept = sorted(os.path.basename(ln.split(' -c ')[1].split()[0])[:-4] for ln in compiles if '-Rpass-analysis=kernel-resource-usage' in ln)
    assert kept == sorted(NO_SCRATCH + ['dq_wave'])


@pytest.mark.parametrize('name', NO_SCRATCH)
def test_scratch_in_a_guarded_object_fails_the_build_by_name(run_build, name):
    rc, err, lines, _ = run_build({name: CLEAN.replace('ScratchSize [bytes/lane]: 0', 'ScratchSize [bytes/lane]: 16')})
    assert rc == 1
    assert f'{name}.hip: ' in err and 'spills or uses scratch memory' in err and f'build/{name}.usage' in err
    assert not any('-shared' in ln for ln in lines)


def test_the_wave_guard_is_168_vgprs_and_no_spill(run_build):
    rc, err, lines, _ = run_build({'dq_wave': wave_block(169, 0)})
    assert rc == 1 and 'dq_wave.hip: a wave_pass_kernel instantiation exceeds 168 VGPRs or spills' in err
    assert not any('-shared' in ln for ln in lines)
    rc, err, lines, _ = run_build({'dq_wave': wave_block(168, 0)})
    assert rc == 0, err
    assert any('-shared' in ln for ln in lines)
