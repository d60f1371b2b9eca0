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


def _build_and_run(tmp_path, name):
    """tests/<name>.cpp, host side only, under the sanitizers, as a program of its own; its standard output"""
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip('no hipcc')
    exe = tmp_path / name
    r = subprocess.run([hipcc, '-x', 'hip', '--offload-host-only', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror',
                        '-Wno-unused-function', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', CSRC,
                        '-I', os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', name + '.cpp'), '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_the_plan_is_what_the_three_places_decided(tmp_path):
    out = _build_and_run(tmp_path, 'search_plan')
    assert out.startswith('search plan ok: '), out
    assert int(out.split()[3]) > 1_000_000


def test_the_float_plan_is_what_the_three_places_decided(tmp_path):
    """plan_search32, the float solve's plan, against tests/search_plan32.cpp's restatement of solve_impl<float>'s rules and carve,
    search_builds_queues, launch_search_fast and launch_emit_fast as they stood before it; then the invariants that held by
    convention only.  The sweep and the one difference that is meant are listed at the top of that file."""
    out = _build_and_run(tmp_path, 'search_plan32')
    assert out.startswith('search plan32 ok: '), out
    assert int(out.split()[3]) > 1_000_000


def test_the_launchers_take_their_grid_from_the_plan():
    """The float64 launchers form no grid of their own: search64_grid is called by plan_search64 and nowhere in igt_kernels_f64.hip
    (search_plan.cpp checks plan.grid == min(items, search64_grid of the plan's family) at every point of its sweep)."""
    src = open(os.path.join(CSRC, 'igt_kernels_f64.hip')).read()
    assert src.count('search64_grid(') + src.count('search64_slots(') + src.replace(' ', '').count('n_cu*4') == 0


def test_the_float_launchers_decide_nothing():
    """launch_search_fast and launch_emit_fast form no grid of their own, apply no batch threshold and test no pointer to choose a
    kernel: between their first line and launch_rollout_all they read the plan (search_plan32.cpp checks its grid, its thresholds
    and its kernels at every point of its sweep)."""
    src = open(os.path.join(CSRC, 'igt_kernels.hip')).read()
    assert 'search_builds_queues' not in src
    lo = src.index('static hipError_t launch_search_fast(')
    search = src[lo:src.index('hipError_t launch_search<float>')]
    lo = src.index('static hipError_t launch_emit_fast(')
    emit = src[lo:src.index('hipError_t launch_emit<float>')]
    for body in (search, emit):
        flat = body.replace(' ', '')
        assert 'n_cu' not in flat and 'waves_per_simd' not in flat and 'B<=' not in flat and 'B<' not in flat
        assert 'if(A.' not in flat and '&&A.' not in flat and 'A.ckpt&&' not in flat
