"""csrc/igt_launch.h decides the shape of the acceleration-row pass (accel_rows_kernel): rows_scenarios_per_block / rows_groups
count its workgroups, plan_search64 names their size (rows_threads: 256 threads, or one wave where solves overlap).  They are
host functions, so the host side of tests/rows_shape.cpp is built against the header (hipcc,
no device pass) under the address and undefined-behaviour sanitizers and run: G in {4, 8, 16, 32, 64}, both workgroup sizes, every
B from 1 to 9000 -- the groups cover B exactly, the one-wave shape is chosen exactly where the row pass runs and solves overlap,
and DEV_WIDE_ROWS brings the 256 threads back without touching another field of the plan.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'igt-mpc-int_amd', 'csrc')


def _hipcc():
    return shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)


def test_rows_shape_covers_the_batch_and_follows_the_rule(tmp_path):
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip('no hipcc')
    exe = tmp_path / 'rows_shape'
    r = subprocess.run([hipcc, '-x', 'hip', '--offload-host-only', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-Wno-unused-function',
                        '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', CSRC, '-I', os.path.join(ROOT, 'include'),
                        os.path.join(ROOT, 'tests', 'rows_shape.cpp'), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith('rows shape ok'), r.stdout + r.stderr


def test_the_switch_is_mirrored_and_documented():
    from igtmpc import _lib as L
    assert L.DEV_WIDE_ROWS == 64
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert f'| {L.DEV_WIDE_ROWS} | `DEV_WIDE_ROWS` |' in design
