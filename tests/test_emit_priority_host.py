"""csrc/igt_launch.h plan_search64 decides whether the one-piece float64 emit raises its wave priority (emit_priority: behind the
pool search, where solves overlap).  It is a host function, so the host side of tests/emit_priority.cpp is built against the
header (hipcc, no device pass) under the address and undefined-behaviour sanitizers and run over the grid of
tests/rows_shape.cpp: the rule holds exactly, never names a family whose emit kernel has no raised build, and DEV_EMIT_PRIO0
brings priority 0 back without touching another field of the plan.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'igt-mpc-int_amd', 'csrc')


def _hipcc():
    return shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)


def test_emit_priority_follows_its_rule(tmp_path):
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip('no hipcc')
    exe = tmp_path / 'emit_priority'
    r = subprocess.run([hipcc, '-x', 'hip', '--offload-host-only', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-Wno-unused-function',
                        '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', CSRC, '-I', os.path.join(ROOT, 'include'),
                        os.path.join(ROOT, 'tests', 'emit_priority.cpp'), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith('emit priority ok'), r.stdout + r.stderr


def test_the_switch_is_mirrored_and_documented():
    from igtmpc import _lib as L
    assert L.DEV_EMIT_PRIO0 == 128
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert f'| {L.DEV_EMIT_PRIO0} | `DEV_EMIT_PRIO0` |' in design
