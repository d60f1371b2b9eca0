"""csrc/igt_launch.h search64_slots / search64_grid decide how many persistent waves a float64 search launches: every wave slot,
or -- three or more solves in flight (igt_set_concurrency) -- the slots less a reserve that the other lanes' emit and row passes
run in.  They are host functions, so the host side of tests/search_grid.cpp is built against the header (hipcc, no device pass)
under the address and undefined-behaviour sanitizers and run: n_cu in {1, 8, 256, 304}, one and two waves per SIMD, the switch
(DEV_NO_RESERVE) on and off, both kernel families, every reserve of a sweep -- the grid never 0, never above the slots, the slots
themselves below three in flight, and the pools' batch bound (B >= 4 * slots) untouched.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'igt-mpc-int_amd', 'csrc')


def _hipcc():
    return shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)


def test_search_grid_keeps_its_bounds(tmp_path):
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip('no hipcc')
    exe = tmp_path / 'search_grid'
    r = subprocess.run([hipcc, '-x', 'hip', '--offload-host-only', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-Wno-unused-function',
                        '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', CSRC, '-I', os.path.join(ROOT, 'include'),
                        os.path.join(ROOT, 'tests', 'search_grid.cpp'), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'search grid ok', r.stdout + r.stderr


def test_the_switch_is_the_next_free_bit_and_is_documented():
    from igtmpc import _lib as L
    assert L.DEV_NO_RESERVE == 1 << 27 == 2 * L.DEV_NO_REFILL
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert f'| {L.DEV_NO_RESERVE} | `DEV_NO_RESERVE` |' in design
