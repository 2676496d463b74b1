"""Host check of maggie_amd/csrc/launch_host.h, the HIP-free part of the launch layer: the knob reader parses like atoi / atol and takes the default
only for an unset variable; the per-device once-mask is true exactly once per device index, also under racing threads, and never remembers an index
outside [0, 16). A stand-alone program (tests/csrc/launch_host_check.cpp) built from the very header the launchers include, under the address and
undefined-behaviour sanitizers -- runs without a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not available')
def test_knob_reader_and_once_mask(tmp_path):
    exe = str(tmp_path / 'launch_host_check')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-pthread', '-o', exe,
                           os.path.join(ROOT, 'tests', 'csrc', 'launch_host_check.cpp')])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert 'launch_host: ok' in r.stdout
