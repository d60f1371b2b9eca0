"""csrc/igt_value_polish_layout.h is where the scratch of the polish under the value-network cost lies in a solve's workspace
(igt_api.hip solve_impl takes doubles(B, N) in its one carve; value_trials_f64_kernel / value_accept_f64_kernel find the pieces
from the base).  It is plain C++17, so a host compiler builds tests/value_polish_layout.cpp against it alone, under the address and
undefined-behaviour sanitizers: aligned, disjoint pieces inside doubles(B, N) for B in {1, 17, 64, 300, 65 536} x N in {1, 20, 64},
and nothing a launch counts in int overflows at B = 65 536.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'igt-mpc-int_amd', 'csrc')


def test_value_polish_layout_is_disjoint_aligned_and_inside(tmp_path):
    if not shutil.which('g++'):
        pytest.skip('no g++')
    exe = tmp_path / 'value_polish_layout'
    r = subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        '-I', CSRC, os.path.join(ROOT, 'tests', 'value_polish_layout.cpp'), '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'value polish layout ok', r.stdout + r.stderr
    hdr = open(os.path.join(CSRC, 'igt_value_polish_layout.h')).read()
    assert re.findall(r'#include\s*[<"]([^>"]+)', hdr) == ['cstddef']      # no HIP header behind it


def test_the_solve_carves_the_layout_once():
    """solve_impl takes the scratch inside its one carve lambda (no second carve_work in the call), the kernels and the host size
    VnScratch by the layout's constant, and the capture refusal stands ahead of the staging."""
    api = open(os.path.join(CSRC, 'igt_api.hip')).read()
    body = api[api.index('int solve_impl('):api.index('int rollout_impl(')]
    assert body.count('carve_work(') == 1
    assert 'wa.take<double>(igt::ValuePolishLayout::doubles(B, p.N))' in body[body.index('const auto carve'):body.index('carve_work(')]
    assert body.index('capturing(') < body.index('stg.upload()') < body.index('carve_work(')
    assert 'VN_DOUBLES_PER_SCENARIO' in open(os.path.join(CSRC, 'igt_launch.h')).read()
