"""csrc/igt_launch.h plan_search64 decides once, on the host, what a float64 solve runs: the search kernel and its grid, the
prelude (live-row pass, queue builders), the launch-time bits of KP::dev, the emit kernel, the workspace those kernels read and
whether the host zeroes the unit counters.  solve_impl carves from the plan, launch_search64 / launch_emit64 switch on it.  It is
host code over plain numbers, so the host side of tests/search_plan.cpp is built against the header (hipcc, no device pass) under
the address and undefined-behaviour sanitizers and run: it restates the three places that used to decide this -- the workspace
rules of solve_impl, the six predicates and the order of launch_search64's returns, launch_emit64 -- and compares every plan field
with them over the families, costs, batch sizes, shapes, discretisations, chips, concurrency and developer switches listed at its
top, then asserts the invariants that held by convention only.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'igt-mpc-int_amd', 'csrc')


def _hipcc():
    return shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)


def test_the_plan_is_what_the_three_places_decided(tmp_path):
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip('no hipcc')
    exe = tmp_path / 'search_plan'
    r = subprocess.run([hipcc, '-x', 'hip', '--offload-host-only', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror',
                        '-Wno-unused-function', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', CSRC,
                        '-I', os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'search_plan.cpp'), '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith('search plan ok: '), r.stdout + r.stderr
    assert int(r.stdout.split()[3]) > 1_000_000


def test_the_launchers_take_their_grid_from_the_plan():
    """The float64 launchers form no grid of their own: search64_grid is called by plan_search64 and nowhere in igt_kernels_f64.hip
    (search_plan.cpp checks plan.grid == min(items, search64_grid of the plan's family) at every point of its sweep)."""
    src = open(os.path.join(CSRC, 'igt_kernels_f64.hip')).read()
    assert src.count('search64_grid(') + src.count('search64_slots(') + src.replace(' ', '').count('n_cu*4') == 0
