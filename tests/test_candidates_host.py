"""No GPU: the host side of the per-scenario candidate sets (include/igtmpc.h igt_solve_candidates_f64 /
igt_rollout_candidates_f64; BatchSolver.solve_candidates / rollout_candidates).  The header declares the two entries and says
what they promise, _lib lists them as optional, both libraries export them, a null handle is refused, the methods have the
signatures INTEGRATION.md documents, the three documents name the entries, and the plan of such a solve (csrc/igt_launch.h
plan_candidates64) is checked by a host program of its own, tests/candidates_plan.cpp."""
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'igt-mpc-int_amd', 'csrc')
NAMES = ('igt_solve_candidates_f64', 'igt_rollout_candidates_f64')


def test_header_declares_and_lib_lists_the_entries():
    from igtmpc import _lib as L
    hdr = open(os.path.join(ROOT, 'include', 'igtmpc.h')).read()
    for name in NAMES:
        assert re.search(r'^int ' + name + r'\(igt_handle\* h, int32_t B,', hdr, re.M), name
        assert name in L.SYMBOLS and name in L.OPTIONAL_SYMBOLS
        assert not re.search(name.replace('_f64', '_f32') + r'\s*\(', hdr)
    # the pointer counts: the solve takes U where the _ws solve takes u_ws, the roll-out likewise
    assert L.SYMBOLS[NAMES[0]] == L.SYMBOLS['igt_solve_batch_ws_f64']
    assert L.SYMBOLS[NAMES[1]] == L.SYMBOLS['igt_rollout_batch_ws_f64']
    doc = hdr[hdr.index('Per-scenario candidate sets'):hdr.index('int ' + NAMES[0])]
    for phrase in ('U [B,C,2,N]', 'bit for bit', 'IGT_CAND_TABLE', 'igt_set_candidate_table need not', '16 C N bytes',
                   'There is no _f32 entry', 'IGT_VERSION'):
        assert phrase in doc, phrase
    assert re.search(r'#define IGT_VERSION 201\b', hdr)


def test_both_libraries_export_them_and_refuse_a_null_handle():
    from igtmpc import _lib as L
    for dev in (False, True):
        lib = L.load(dev=dev)
        for name in NAMES:
            fn = getattr(lib, name)
            n_ptr = len(L.SYMBOLS[name][1]) - 4
            rc = fn(None, 1, *([None] * n_ptr), L.IGT_MEM_HOST, None)
            assert rc == -1, (name, rc)                              # IGT_E_INVALID
            assert b'null handle' in lib.igt_last_error()
    hdr = open(os.path.join(ROOT, 'include', 'igtmpc.h')).read()
    assert re.search(r'IGT_E_INVALID\s*=\s*-1\b', hdr)


def test_batchsolver_methods_have_the_signatures():
    from igtmpc.solver import BatchSolver
    sig = inspect.signature(BatchSolver.solve_candidates)
    assert list(sig.parameters) == ['self', 'x0', 'u_prev', 'kparams', 'flags', 'U', 'obs_xy', 'tv_sv', 'enc', 'out', 'stream']
    assert all(sig.parameters[k].default is None for k in ('obs_xy', 'tv_sv', 'enc', 'out', 'stream'))
    sig = inspect.signature(BatchSolver.rollout_candidates)
    assert list(sig.parameters) == ['self', 'x0', 'u_prev', 'kparams', 'flags', 'U', 'obs_xy', 'tv_sv', 'enc', 'want_X', 'want_U',
                                    'stream']
    assert sig.parameters['want_X'].default is True and sig.parameters['want_U'].default is True


def test_documents_name_the_entries():
    for doc in ('README.md', 'INTEGRATION.md', 'DESIGN.md'):
        text = open(os.path.join(ROOT, doc)).read()
        assert 'solve_candidates' in text, doc
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert 'search_cand_staged_f64_kernel' in design and 'profiles/candidates_time.txt' in design


def test_candidates_plan(tmp_path):
    hipcc = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)
    if not hipcc:
        pytest.skip('no hipcc')
    exe = tmp_path / 'candidates_plan'
    r = subprocess.run([hipcc, '-x', 'hip', '--offload-host-only', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror',
                        '-Wno-unused-function', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', CSRC,
                        '-I', os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'candidates_plan.cpp'), '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith('candidates plan ok: '), r.stdout + r.stderr
    assert int(r.stdout.split()[3]) == 10 * 4 * 9 * 2
