"""No GPU: the host side of the closed-loop step on the C ABI (include/igtmpc.h igt_loop_advance_f64 / _f32;
BatchSolver.loop_advance; run_closed_loop(step='fused')).  The numpy restatement the GPU tests compare the kernel with
(tests/loop_advance_restated.py) is held to the statements of igtmpc/evaluate.py's host loop; the launch shape
(csrc/igt_launch.h) is checked by a host program of its own, tests/loop_advance_shape.cpp; the fallback / solved counts that
test_gpu_loop_advance.py's loops rest on are recomputed with the oracle loop."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import loop_advance_restated as LR
import np_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'igt-mpc-int_amd', 'csrc')
NAMES = ('igt_loop_advance_f64', 'igt_loop_advance_f32')


def test_header_declares_and_lib_lists_the_entries():
    from igtmpc import _lib as L
    hdr = open(os.path.join(ROOT, 'include', 'igtmpc.h')).read()
    for name in NAMES:
        m = re.search(r'^int ' + name + r'\(igt_handle\* h, int32_t n,(.*?)\);', hdr, re.M | re.S)
        assert m, name
        assert m[1].count('*') == 16 + 1      # the sixteen buffers and `stream`
        assert 'double a_brake' in m[1] and 'int32_t T_log, int mem, void* stream' in m[1]
        assert name in L.SYMBOLS and name in L.OPTIONAL_SYMBOLS
        assert len(L.SYMBOLS[name][1]) == 2 + 16 + 2 + 2
    doc = hdr[hdr.index('The closed-loop step behind a solve'):hdr.index('int ' + NAMES[0])]
    for phrase in ('evaluate.py:511-545', 'utils.py:354-363', 'igt_frenet_step_f64', 'IGT_FLAG_WARM', 'no workspace', 'capturable',
                   'n = 0 is a no-op', 'IGT_VERSION'):
        assert phrase in doc, phrase
    assert re.search(r'#define IGT_VERSION 201\b', hdr)


def test_both_libraries_export_them_and_refuse_a_null_handle():
    from igtmpc import _lib as L
    for dev in (False, True):
        lib = L.load(dev=dev)
        for name in NAMES:
            rc = getattr(lib, name)(None, 1, *([None] * 6), -4.0, *([None] * 10), 0, L.IGT_MEM_HOST, None)
            assert rc == -1, (name, rc)                              # IGT_E_INVALID
            assert b'null handle' in lib.igt_last_error()


def test_python_face_signatures_and_refusals():
    from igtmpc.evaluate import run_closed_loop
    from igtmpc.solver import BatchSolver
    sig = inspect.signature(BatchSolver.loop_advance)
    assert list(sig.parameters)[:8] == ['self', 'x', 'u_prev', 'kparams', 'status', 'x_sol', 'u_sol', 'a_brake']
    assert all(sig.parameters[k].default is None for k in ('flags', 'infeasible', 'x_log', 'u_log', 'step', 'out', 'stream'))
    assert inspect.signature(run_closed_loop).parameters['step'].default == 'torch'
    with pytest.raises(ValueError, match='device_resident'):            # refused before any GPU call
        run_closed_loop(step='fused')
    with pytest.raises(ValueError, match="'torch' or 'fused'"):
        run_closed_loop(step='both', device_resident=True)


class _ScriptedSolver:
    """Stands in for BatchSolver inside run_closed_loop's HOST loop: the forecast is zeros, the solves answer what the test
    scripted, the model step is the oracle's -- so the statements of evaluate.py between them run on constructed inputs."""
    script, calls = [], []

    def __init__(self, N=20, dt=0.1, n_rk4=4, dtype='f64', n_obs=1, **kw):
        self.N, self.n_obs, self.dtype, self.np_dtype = N, n_obs, dtype, np.float64
        self.P = O.Params(N=N, dt=dt, n_rk4=n_rk4)

    def forecast_scene(self, x, a_prev, route, plan_x, plan_u, has_plan):
        E, M = a_prev.shape
        _ScriptedSolver.calls.append(dict(kind='forecast', x=x.copy(), a_prev=a_prev.copy(), plan_x=plan_x.copy(), plan_u=plan_u.copy(),
                                          has_plan=has_plan.copy()))
        return np.zeros((E * M, M - 1, 2, self.N + 1)), np.zeros((E * M, M - 1, 2))

    def set_value_net(self, **net):
        pass

    def solve(self, x0, u_prev, kparams, flags, obs_xy, tv_sv, enc, u_ws=None):
        t = sum(c['kind'] == 'solve' for c in _ScriptedSolver.calls)
        _ScriptedSolver.calls.append(dict(kind='solve', x0=x0.copy(), u_prev=u_prev.copy(), flags=np.array(flags),
                                          u_ws=None if u_ws is None else u_ws.copy()))
        s = _ScriptedSolver.script[t]
        return dict(status=s['status'].copy(), x=s['x_sol'].copy(), u=s['u_sol'].copy())

    def frenet_step(self, x, u, kparams):
        return O.frenet_rk4_step(x, u[:, 0], u[:, 1], kparams, self.P)

    def close(self):
        pass


def test_restatement_is_the_host_loops_step(monkeypatch):
    """evaluate.py's host loop (run_closed_loop, device_resident=False) and loop_advance_restated on the same constructed
    (x, u_prev, status, xs, us), with np_oracle's exact Frenet step as the model step of both: identical arrays -- the state and
    the applied input of two chained steps as the loop logs them, the counters, and what the loop hands to the next forecast
    (plans, has_plan) and to the next solve (flag words, shifted warm start)."""
    from igtmpc import evaluate as EV, routes as R
    E, M, N, a_brake = 4, 2, 5, -3.5
    n = E * M
    pairs = [R.SCENARIO_ROUTES[0][0], R.SCENARIO_ROUTES[0][3], ('32', '41'), R.SCENARIO_ROUTES[0][1]]
    rid = np.array([[R.ROUTE_ID[r] for r in p] for p in pairs])
    kp = R.kparams(rid).reshape(n, 3)
    flags0 = R.TABLES['abs_heading'][rid].astype(np.uint32).reshape(-1)
    assert flags0.any() and not flags0.all()
    a, b = LR.branch_inputs(n, N, np.float64, seed=1), LR.branch_inputs(n, N, np.float64, seed=2)
    b['status'] = 1 - a['status']                                     # the agents that fell back solve, and the other way round
    rng = np.random.default_rng(3)
    b['x_sol'], b['u_sol'] = rng.normal(0, 5.0, (n, 7, N + 1)), rng.uniform(-1, 1, (n, 2, N))
    b['x_sol'][b['status'] != 0], b['u_sol'][b['status'] != 0] = np.nan, np.nan
    x0 = a['x']
    assert np.isnan(x0[:, 5]).any() and (x0[:, 5] < 0).any() and (x0[:, 5] == 0).any()
    monkeypatch.setattr(EV, 'BatchSolver', _ScriptedSolver)
    _ScriptedSolver.script, _ScriptedSolver.calls = [a, b], []
    got = EV.run_closed_loop(N=N, T_sim=0.2, dtype='f64', cand_mode='track', warm_start=True, init=(x0.reshape(E, M, 7), pairs),
                             terminal_set=False, a_min_policy=a_brake)
    model = lambda x, u, k: O.frenet_rk4_step(x, u[:, 0], u[:, 1], k, O.Params(N=N))
    x_log, u_log = np.zeros((n, 7, 3)), np.zeros((n, 2, 2))
    x_log[:, :, 0] = x0
    r1 = LR.loop_advance_restated(x0, np.tile([0.1, 0.0], (n, 1)), kp, a['status'], a['x_sol'], a['u_sol'], a_brake, model,
                                  flags=flags0, infeasible=np.zeros(n, np.int64), x_log=x_log, u_log=u_log, step=0)
    r2 = LR.loop_advance_restated(r1['x'], r1['u_prev'], kp, b['status'], b['x_sol'], b['u_sol'], a_brake, model,
                                  flags=flags0, infeasible=r1['infeasible'], x_log=r1['x_log'], u_log=r1['u_log'], step=1)
    same = lambda p, q: np.array_equal(p, q, equal_nan=True)
    assert same(got['x_data'], r2['x_log'].reshape(E, 7 * M, 3)) and same(got['u_data'], r2['u_log'].reshape(E, 2 * M, 2))
    assert same(got['infeasible_ratio'] * 2, r2['infeasible'].reshape(E, M))
    assert np.isnan(r2['x_log'][:, :, 1]).any() and not np.isnan(r2['x_log'][:, :, 0][~np.isnan(x0)]).any()
    fc = [c for c in _ScriptedSolver.calls if c['kind'] == 'forecast']
    sv = [c for c in _ScriptedSolver.calls if c['kind'] == 'solve']
    assert len(fc) == 2 and len(sv) == 2
    assert same(fc[1]['x'].reshape(n, 7), r1['x']) and same(sv[1]['x0'], r1['x']) and same(sv[1]['u_prev'], r1['u_prev'])
    assert same(fc[1]['plan_x'].reshape(n, 7, N + 1), r1['plan_x']) and same(fc[1]['plan_u'].reshape(n, 2, N), r1['plan_u'])
    assert same(fc[1]['has_plan'].reshape(n), r1['has_plan']) and not fc[0]['has_plan'].any()
    assert same(sv[1]['flags'], r1['flags']) and same(sv[1]['u_ws'], r1['u_ws']) and sv[0]['u_ws'] is None
    # a step outside the log writes nothing, and the optional groups are optional
    r3 = LR.loop_advance_restated(x0, a['u_prev'], kp, a['status'], a['x_sol'], a['u_sol'], a_brake, model, x_log=x_log,
                                  u_log=u_log, step=2, want_ws=False)
    assert same(r3['x_log'], x_log) and same(r3['u_log'], u_log) and r3['u_ws'] is None and r3['flags'] is None


def _scripted_run(monkeypatch, steps, **kw):
    """run_closed_loop's host loop on E = 2 scenes of M = 2, N = 5, with _ScriptedSolver answering `steps` solves: the agents that
    fall back and the ones that solve swap every step.  -> (result, forecast calls, solve calls, scripted answers, flags0)."""
    from igtmpc import evaluate as EV, routes as R
    E, M, N = 2, 2, 5
    n = E * M
    pairs = [R.SCENARIO_ROUTES[0][0], R.SCENARIO_ROUTES[0][1]]
    rid = np.array([[R.ROUTE_ID[r] for r in p] for p in pairs])
    script = [LR.branch_inputs(n, N, np.float64, seed=10 + t) for t in range(steps)]
    rng = np.random.default_rng(4)
    for t, s in enumerate(script):
        s['status'] = (np.arange(n) % 2 == t % 2).astype(np.int32)
        s['x_sol'], s['u_sol'] = rng.normal(0, 5.0, (n, 7, N + 1)), rng.uniform(-1, 1, (n, 2, N))
        s['x_sol'][s['status'] != 0], s['u_sol'][s['status'] != 0] = np.nan, np.nan
    monkeypatch.setattr(EV, 'BatchSolver', _ScriptedSolver)
    _ScriptedSolver.script, _ScriptedSolver.calls = script, []
    got = EV.run_closed_loop(N=N, T_sim=steps * 0.1, dtype='f64', cand_mode='track', warm_start=True, terminal_set=False,
                             init=(script[0]['x'].reshape(E, M, 7), pairs), **kw)
    fc = [c for c in _ScriptedSolver.calls if c['kind'] == 'forecast']
    sv = [c for c in _ScriptedSolver.calls if c['kind'] == 'solve']
    assert len(fc) == steps and len(sv) == steps
    return got, fc, sv, script, R.TABLES['abs_heading'][rid].astype(np.uint32).reshape(-1)


def test_gt_mpc_first_forecast_and_warm_start_delay(monkeypatch):
    """eval_mode='gt_mpc' (evaluate.py:171, 207-210, 232): the previous inputs start at (0, 0), the first forecast takes
    a = 0.09 (k + 1) for agent k and the later ones the applied acceleration, and the warm start is passed for t > 1 only -- solve 2
    gets the plan of the agents that solved step 1, shifted, with IGT_FLAG_WARM on exactly those."""
    got, fc, sv, script, flags0 = _scripted_run(monkeypatch, 4, eval_mode='gt_mpc', value_net=dict(layers=[]))
    same = lambda p, q: np.array_equal(p, q, equal_nan=True)
    assert same(fc[0]['a_prev'], np.tile([0.09, 0.18], (2, 1)))
    assert same(sv[0]['u_prev'], np.zeros((4, 2)))
    assert same(fc[1]['a_prev'].reshape(-1), sv[1]['u_prev'][:, 0]) and same(sv[1]['u_prev'], got['u_data'][:, :, 0].reshape(4, 2))
    for t in (0, 1):
        assert sv[t]['u_ws'] is None and same(sv[t]['flags'], flags0)
    for t in (2, 3):
        ok = script[t - 1]['status'] == 0
        u = np.nan_to_num(script[t - 1]['u_sol'])
        assert ok.any() and not ok.all()
        assert same(sv[t]['flags'], flags0 | np.where(ok, LR.IGT_FLAG_WARM, 0).astype(np.uint32))
        assert same(sv[t]['u_ws'], np.concatenate([u[:, :, 1:], u[:, :, -1:]], axis=2))
        assert same(fc[t]['has_plan'].reshape(-1), ok) and same(fc[t]['plan_u'].reshape(u.shape), u)


def test_constant_speed_forecast_keeps_the_brake_fallbacks_inputs(monkeypatch):
    """constant_speed=True (mpc): every forecast takes a = 0 (constant_acceleration_model.py:26-29) while the brake fallback goes
    on reading u_prev -- the agents that solved step 0 and fall back in step 1 keep step 0's steering, and the warm start is
    passed from t = 1 (evaluate.py:478)."""
    got, fc, sv, script, flags0 = _scripted_run(monkeypatch, 3, constant_speed=True, a_min_policy=-3.5)
    same = lambda p, q: np.array_equal(p, q, equal_nan=True)
    for c in fc:
        assert c['a_prev'].shape == (2, 2) and not c['a_prev'].any()
    assert same(sv[0]['u_prev'], np.tile([0.1, 0.0], (4, 1))) and sv[0]['u_ws'] is None
    ok0 = script[0]['status'] == 0
    assert same(sv[1]['u_prev'][ok0], script[0]['u_sol'][ok0, :, 0]) and sv[1]['u_prev'][ok0, 0].all()
    assert same(sv[1]['flags'], flags0 | np.where(ok0, LR.IGT_FLAG_WARM, 0).astype(np.uint32)) and sv[1]['u_ws'] is not None
    u1 = got['u_data'][:, :, 1].reshape(4, 2)                         # step 1: the agents that solved step 0 fall back
    assert same(u1[ok0, 1], script[0]['u_sol'][ok0, 1, 0]) and same(sv[2]['u_prev'], u1)
    v = sv[1]['x0'][ok0, 5]
    assert same(u1[ok0, 0], np.where(v > 0, -3.5, 0.0))


def test_launch_shape(tmp_path):
    hipcc = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)
    if not hipcc:
        pytest.skip('no hipcc')
    exe = tmp_path / 'loop_advance_shape'
    r = subprocess.run([hipcc, '-x', 'hip', '--offload-host-only', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror',
                        '-Wno-unused-function', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-pthread', '-I', CSRC,
                        '-I', os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'loop_advance_shape.cpp'), '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == f'loop advance shape ok: {1001 * 64} shapes', r.stdout + r.stderr


def build_c_closed_loop(out):
    """examples/c_closed_loop.c with the system compiler, against include/igtmpc.h and the built library, as c_caller is built."""
    if not shutil.which('gcc') or not os.path.exists('/opt/rocm/lib/libamdhip64.so'):
        pytest.skip('needs gcc and the ROCm runtime library')
    libdir = os.path.join(ROOT, 'igt-mpc-int_amd', 'igtmpc')
    r = subprocess.run(['gcc', '-std=c99', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                        os.path.join(ROOT, 'examples', 'c_closed_loop.c'), '-o', str(out), '-L', libdir, '-ligtmpc',
                        f'-Wl,-rpath,{libdir}', '-L/opt/rocm/lib', '-lamdhip64', '-lm'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def write_c_closed_loop_input(path, x, routes, N, T, cand_mode='lattice', warm=False, dt=0.1, track_env=1.0, a_brake=-4.0):
    """The input file of examples/c_closed_loop.c for run_closed_loop(init=(x, routes), N=N, T_sim=T dt, cand_mode=...)'s
    problem: the route table BatchSolver.set_routes loads, the terminal set run_closed_loop sets, route ids, flags, kparams."""
    from igtmpc import _lib as L, routes as R
    from igtmpc.cinf import cinf_halfplanes
    E, M = x.shape[:2]
    Tb = R.TABLES
    table = np.column_stack([Tb['p0'], Tb['t'], Tb['c'], Tb['b0'], Tb['b1'], Tb['R'], Tb['end'], (Tb['turn'] == 0).astype(np.float64)])
    rid = np.array([[R.ROUTE_ID[r] for r in p] for p in routes], dtype=np.int64)
    p = L.igt_params()
    L.load().igt_params_default(p)
    A, b = cinf_halfplanes(dt=dt, jerk=p.jerk_limit)
    A, b = np.ascontiguousarray(A, dtype=np.float64).reshape(-1, 2), np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    mode = {'lattice': L.IGT_CAND_LATTICE, 'ramp_hold': L.IGT_CAND_RAMP_HOLD, 'track': L.IGT_CAND_TRACK}[cand_mode]
    with open(path, 'wb') as f:
        f.write(np.array([E, M, N, T, len(table), mode, len(b), int(warm)], dtype=np.int32).tobytes())
        f.write(np.array([dt, track_env, a_brake, 0.1, 0.0], dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(table, dtype=np.float64).tobytes())
        f.write(A.tobytes() + b.tobytes())
        f.write(rid.astype(np.int32).tobytes())
        f.write(np.ascontiguousarray(x, dtype=np.float64).tobytes())
        f.write(R.TABLES['abs_heading'][rid].astype(np.uint32).tobytes())
        f.write(np.ascontiguousarray(R.kparams(rid), dtype=np.float64).tobytes())


def test_c_closed_loop_links_against_the_abi(tmp_path):
    """examples/c_closed_loop.c -- C99, include/igtmpc.h alone -- compiles without a warning and links against libigtmpc.so (it is
    run on the GPU box by tests/test_gpu_loop_advance.py); without its two arguments it says how it is called."""
    exe = build_c_closed_loop(tmp_path / 'c_closed_loop')
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and 'usage' in r.stderr


@pytest.mark.parametrize('name', list(LR.LOOP_CASES))
def test_loop_cases_hold_a_fallback_and_a_solved_step(name):
    """The oracle loop alone on every case test_gpu_loop_advance.py runs: the recorded counts are its counts, and every case
    holds fallback steps (one of them the stop below v = 0) beside solved ones."""
    res, ev = LR.oracle_loop(name)
    M = LR.LOOP_CASES[name]['kw']['num_agents']
    want = LR.LOOP_EVENTS[name]
    assert ev['fallback'] == want['fallback'] > 0 and ev['stop'] == want['stop'] > 0 and ev['warm'] == want['warm']
    assert len(res) * M * LR.STEPS - ev['fallback'] == want['solved'] > 0
    assert sum(int(r['infeasible'].sum()) for r in res) == ev['fallback']


def test_documents_and_profiles_name_the_step():
    for doc in ('README.md', 'INTEGRATION.md', 'DESIGN.md'):
        assert 'loop_advance' in open(os.path.join(ROOT, doc)).read(), doc
    ident = open(os.path.join(ROOT, 'profiles', 'loop_advance_identity.txt')).read()
    assert 'loop_advance_kernel' in ident and 'scratch 0' in ident
    src = open(os.path.join(CSRC, 'igt_kernels.hip')).read()
    body = src[src.index('void loop_advance_kernel'):src.index('hipError_t launch_loop_advance')]
    assert 'ExactStepper<double> stp' in body and 'atomic' not in body and '__shared__' not in body
