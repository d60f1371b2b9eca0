"""GPU: the closed-loop step on the C ABI (include/igtmpc.h igt_loop_advance_f64 / _f32, one kernel) -- against its numpy
restatement (tests/loop_advance_restated.py) byte for byte in host and device mode, run_closed_loop(step='fused') against
step='torch' byte for byte, the plain-C closed loop (examples/c_closed_loop.c) against the Python one, and the refusals."""
import subprocess

import numpy as np
import pytest

import loop_advance_restated as LR
from helpers import rel_err

pytestmark = pytest.mark.gpu

T_LOG, A_BRAKE = 4, -4.0
_solvers = {}


@pytest.fixture(scope='module')
def handles():
    """One solver per (N, dtype) and the N = 1 stepper whose igt_frenet_step_f64 is the restatement's model step."""
    import igtmpc

    def get(N, dtype):
        if (N, dtype) not in _solvers:
            _solvers[(N, dtype)] = igtmpc.BatchSolver(N=N, C=64, n_obs=1, dtype=dtype)
        return _solvers[(N, dtype)]
    stepper = igtmpc.BatchSolver(N=1, C=64, n_obs=0, dtype='f64')
    yield get, stepper
    for s in list(_solvers.values()) + [stepper]:
        s.close()
    _solvers.clear()


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


VARIANTS = [('all', 0), ('all', T_LOG - 1), ('all', T_LOG), ('no_ws', 1), ('no_flags', 1), ('no_infeasible', 1), ('no_logs', 1)]


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('N', [1, 13, 20, 64])
@pytest.mark.parametrize('n', [1, 67, 256])
def test_kernel_equals_the_restatement_bytewise(handles, n, N, dtype):
    """Every branch in every case (loop_advance_restated.branch_inputs): status 0 / 1 interleaved, v > 0, = 0, < 0 and NaN among
    the fallback rows, NaN solution rows, turning and straight routes; steps 0, T - 1 and T (which must leave the logs' bytes as
    they were); every optional output given and each optional group absent; host mode and device mode.  Compared in whole:
    x, u_prev, has_plan, plan_x, plan_u, u_ws, flags_out, infeasible and both logs."""
    import torch
    get, stepper = handles
    s = get(N, dtype)
    npdt = np.float64 if dtype == 'f64' else np.float32
    if n == 1:      # one agent takes one branch: five batches of one, rows of the eight-agent inputs -- v > 0, solved, v = 0, v < 0, NaN
        eight = LR.branch_inputs(8, N, npdt)
        batches = [{k: v[i:i + 1].copy() for k, v in eight.items()} for i in (0, 1, 2, 4, 6)]
        v0 = np.array([b['x'][0, 5] for b in batches])
        assert [int(b['status'][0]) for b in batches] == [1, 0, 1, 1, 1] and v0[0] > 0 and v0[2] == 0 and v0[3] < 0 and np.isnan(v0[4])
    else:
        batches = [LR.branch_inputs(n, N, npdt)]
        fb = batches[0]['x'][batches[0]['status'] != 0, 5]
        assert (fb > 0).any() and (fb == 0).any() and (fb < 0).any() and np.isnan(fb).any() and (batches[0]['status'] == 0).any()
    rng = np.random.default_rng(n + N)
    x_log0, u_log0 = rng.normal(size=(n, 7, T_LOG + 1)), rng.normal(size=(n, 2, T_LOG))
    model = lambda x, u, k: stepper.frenet_step(x, u, k)
    for inp, (what, step) in ((b, v) for b in batches for v in VARIANTS):
        logs, fl, inf, ws = what != 'no_logs', what != 'no_flags', what != 'no_infeasible', what != 'no_ws'
        ref = LR.loop_advance_restated(inp['x'], inp['u_prev'], inp['kparams'], inp['status'], inp['x_sol'], inp['u_sol'], A_BRAKE,
                                       model, flags=inp['flags'] if fl else None, infeasible=inp['infeasible'] if inf else None,
                                       x_log=x_log0 if logs else None, u_log=u_log0 if logs else None, step=step, want_ws=ws)
        if step == T_LOG:
            assert _same_bytes(ref['x_log'], x_log0) and _same_bytes(ref['u_log'], u_log0)
        for mode in ('host', 'device'):
            if mode == 'host':
                put = lambda a: None if a is None else np.array(a)
                back = lambda a: a
            else:
                put = lambda a: None if a is None else torch.from_numpy(np.array(a.view(np.int32) if a.dtype == np.uint32 else a)).cuda()
                back = lambda a: a.cpu().numpy()
            x, up = put(inp['x']), put(inp['u_prev'])
            infeasible = put(inp['infeasible']) if inf else None
            xl, ul = (put(x_log0), put(u_log0)) if logs else (None, None)
            st = None if not logs else (step if mode == 'host' else torch.tensor([step], dtype=torch.int64, device='cuda'))
            out = s.loop_advance(x, up, put(inp['kparams']), put(inp['status']), put(inp['x_sol']), put(inp['u_sol']), A_BRAKE,
                                 flags=put(inp['flags']) if fl else None, infeasible=infeasible, x_log=xl, u_log=ul, step=st,
                                 want_ws=ws)
            if mode == 'device':
                torch.cuda.synchronize()
            got = dict(x=back(x), u_prev=back(up), has_plan=back(out['has_plan']), plan_x=back(out['plan_x']),
                       plan_u=back(out['plan_u']))
            if ws:
                got['u_ws'] = back(out['u_ws'])
            else:
                assert out['u_ws'] is None
            if fl:
                got['flags'] = back(out['flags']).view(np.uint32)
            else:
                assert out['flags'] is None
            if inf:
                got['infeasible'] = back(infeasible)
            if logs:
                got['x_log'], got['u_log'] = back(xl), back(ul)
            for k, v in got.items():
                assert _same_bytes(v, ref[k]), (k, what, step, mode)


def _run(name, **extra):
    from igtmpc.evaluate import run_closed_loop
    x, routes, kw = LR.loop_case_init(name)
    return run_closed_loop(device_resident=True, **dict(kw, **extra))


def _run_captured_on_own_stream(name, monkeypatch):
    return _captured_on_own_stream(monkeypatch, lambda: _run(name, step='fused', graph=True))


def _captured_on_own_stream(monkeypatch, run):
    """run(): a run_closed_loop(graph=True).  It captures on `torch.cuda.Stream(dev)`, a stream of torch's pool, which lives -- and keeps its
    hardware queue -- as long as the process: one more of them here and two lanes of tests/test_gpu_overlap.py share a queue
    later in the same process (tests/test_gpu_candidates.py _side_stream has the story).  So for this run
    the driver's request for a new stream is answered with a stream of the test's own, destroyed at the end; every other use
    of the class (torch.cuda.current_stream builds its answer with it) goes through."""
    import torch
    from handle_walk_cases import side_stream
    pool_stream = torch.cuda.Stream
    if torch.cuda.graph.default_capture_stream is None:      # torch makes it at the first capture of a process: not from `own`
        torch.cuda.graph.default_capture_stream = pool_stream()
    with side_stream() as own:
        def stream(*a, **k):
            return pool_stream(*a, **k) if ('stream_id' in k or 'stream_ptr' in k) else own
        monkeypatch.setattr(torch.cuda, 'Stream', stream)
        try:
            return run()
        finally:
            monkeypatch.setattr(torch.cuda, 'Stream', pool_stream)


CROSS_CASES = {
    'gt_mpc_warm': dict(eval_mode='gt_mpc', cand_mode='track', warm_start=True),      # sc 1's shipped network; warm start from t = 2
    'mpc_constant_speed_ramp_hold': dict(eval_mode='mpc', constant_speed=True, cand_mode='ramp_hold'),
}


@pytest.mark.parametrize('name', list(CROSS_CASES))
def test_host_torch_fused_and_captured_loops_agree_bytewise(name, monkeypatch):
    """The one step of run_closed_loop in its four forms -- the host loop, device-resident with step='torch', with step='fused',
    and step='torch' replayed from a captured graph -- on two option sets no other test crosses: x_data, u_data,
    infeasible_ratio and deadlock byte-equal.  Four sampled episodes of scenario 1, N = 20, six steps (t = 0, 1, 2 eagerly or
    captured, three replays), f64."""
    from igtmpc.evaluate import run_closed_loop
    kw = dict(sc=1, num_samples=4, N=20, T_sim=0.6, dtype='f64', **CROSS_CASES[name])
    host = run_closed_loop(**kw)
    runs = {'torch': run_closed_loop(device_resident=True, step='torch', **kw),
            'fused': run_closed_loop(device_resident=True, step='fused', **kw),
            'graph': _captured_on_own_stream(monkeypatch, lambda: run_closed_loop(device_resident=True, step='torch', graph=True, **kw))}
    assert host['x_data'].shape == (4, 14, 7) and np.isfinite(host['x_data']).all() and (host['x_data'][:, :, -1] != host['x_data'][:, :, 0]).any()
    for form, got in runs.items():
        for k in ('x_data', 'u_data', 'infeasible_ratio', 'deadlock'):
            assert _same_bytes(got[k], host[k]), (name, form, k)


@pytest.mark.parametrize('name', list(LR.LOOP_CASES))
def test_fused_loop_equals_the_torch_loop_bytewise(name, monkeypatch):
    """run_closed_loop(device_resident=True, step='fused') against step='torch': x_data, u_data, infeasible_ratio and deadlock
    byte-equal, eager, and for the first case with graph=True as well (one stream, no parallel branches).  Every run holds at
    least one fallback step and one solved step (the oracle's counts: loop_advance_restated.LOOP_EVENTS, recomputed by
    test_loop_advance_host.py); the f64 mpc cases are also held to the oracle loop at 1e-9."""
    torch_run = _run(name, step='torch')
    runs = [_run(name, step='fused')]
    if name == 'mpc_f64_lattice':
        runs.append(_run_captured_on_own_stream(name, monkeypatch))
    kw = LR.LOOP_CASES[name]['kw']
    steps_fb = np.rint(torch_run['infeasible_ratio'] * LR.STEPS).astype(int)
    assert steps_fb.sum() >= 1 and (LR.STEPS - steps_fb).sum() >= 1
    if kw['dtype'] == 'f64':
        assert steps_fb.sum() == LR.LOOP_EVENTS[name]['fallback']
    for got in runs:
        for k in ('x_data', 'u_data', 'infeasible_ratio', 'deadlock'):
            assert _same_bytes(got[k], torch_run[k]), (name, k)
    if kw['dtype'] == 'f64' and kw['eval_mode'] == 'mpc':
        res, _ = LR.oracle_loop(name)
        for e, ref in enumerate(res):
            ex, eu = rel_err(runs[0]['x_data'][e], ref['x_data']).max(), rel_err(runs[0]['u_data'][e], ref['u_data']).max()
            print(f'{name} episode {e}: max rel err x {ex:.2e} u {eu:.2e}')
            assert ex < 1e-9 and eu < 1e-9, (name, e)
            assert np.array_equal(steps_fb[e], ref['infeasible'])


def test_plain_c_closed_loop_equals_the_python_loop(tmp_path):
    """examples/c_closed_loop.c (C99, host buffers, forecast_scene -> solve_ws -> loop_advance through include/igtmpc.h alone) on
    E = 4 scenes of M = 2 vehicles, T = 10 steps, f64: its logs and counters are run_closed_loop(step='fused')'s, byte for byte."""
    import scene_loop_restated as S
    from igtmpc.evaluate import run_closed_loop
    from test_loop_advance_host import build_c_closed_loop, write_c_closed_loop_input
    x2, r2 = S.scenes(2)
    x, routes = np.concatenate([x2, x2 + 0.0]), list(r2) + list(r2)
    x[2:, :, 5] += 0.5
    E, M, N, T = 4, 2, 20, 10
    exe = build_c_closed_loop(tmp_path / 'c_closed_loop')
    write_c_closed_loop_input(tmp_path / 'in.bin', x, routes, N, T, cand_mode='lattice')
    r = subprocess.run([str(exe), str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(tmp_path / 'out.bin', 'rb').read()
    n = E * M
    n_x, n_u = n * 7 * (T + 1), n * 2 * T
    assert len(raw) == 8 * (n_x + n_u + n)
    x_log = np.frombuffer(raw, np.float64, n_x).reshape(E, 7 * M, T + 1)
    u_log = np.frombuffer(raw, np.float64, n_u, 8 * n_x).reshape(E, 2 * M, T)
    infeasible = np.frombuffer(raw, np.int64, n, 8 * (n_x + n_u)).reshape(E, M)
    py = run_closed_loop(N=N, T_sim=T * 0.1, dtype='f64', cand_mode='lattice', init=(x, routes), device_resident=True, step='fused')
    assert _same_bytes(x_log, py['x_data']) and _same_bytes(u_log, py['u_data'])
    assert np.array_equal(infeasible / T, py['infeasible_ratio']) and 0 < infeasible.sum() < n * T
    assert f'{int(infeasible.sum())} fallback steps of {n * T}' in r.stdout


def test_refusals_and_the_empty_batch(handles):
    """IGT_E_INVALID with a message for a null handle, n < 0, a null required buffer, a bad mem and one of a both-or-neither
    pair; n = 0 is a no-op that touches nothing."""
    from igtmpc import _lib as L
    get, _ = handles
    s = get(13, 'f64')
    lib, N, n = s.lib, 13, 3
    inp = LR.branch_inputs(n, N, np.float64)
    keep = dict(x=inp['x'].copy(), u_prev=inp['u_prev'].copy(), kparams=inp['kparams'], status=inp['status'], x_sol=inp['x_sol'],
                u_sol=inp['u_sol'], has_plan=np.zeros(n, np.int32), plan_x=np.zeros((n, 7, N + 1)), plan_u=np.zeros((n, 2, N)),
                u_ws=np.zeros((n, 2, N)), flags_in=inp['flags'], flags_out=np.zeros(n, np.uint32), infeasible=inp['infeasible'].copy(),
                x_log=np.zeros((n, 7, T_LOG + 1)), u_log=np.zeros((n, 2, T_LOG)), step=np.zeros(1, np.int64))
    order = ['x', 'u_prev', 'kparams', 'status', 'x_sol', 'u_sol', 'has_plan', 'plan_x', 'plan_u', 'u_ws', 'flags_in', 'flags_out',
             'infeasible', 'x_log', 'u_log', 'step']

    def call(h=s._h, n_=n, mem=L.IGT_MEM_HOST, **null):
        p = [None if k in null else keep[k].ctypes.data for k in order]
        return lib.igt_loop_advance_f64(h, n_, *p[:6], A_BRAKE, *p[6:], T_LOG, mem, None)

    def refused(rc, word):
        assert rc == -1, rc                                                     # IGT_E_INVALID
        assert word in lib.igt_last_error().decode(), (word, lib.igt_last_error())

    refused(call(h=None), 'null handle')
    refused(call(n_=-1), 'n < 0')
    refused(call(mem=7), 'mem')
    for k in ('x', 'u_prev', 'kparams', 'status', 'x_sol', 'u_sol', 'has_plan', 'plan_x', 'plan_u'):
        refused(call(**{k: True}), 'null')
    refused(call(flags_in=True), 'go together')
    refused(call(flags_out=True), 'go together')
    refused(call(x_log=True), 'go together')
    refused(call(u_log=True), 'go together')
    refused(call(step=True), 'step')
    assert _same_bytes(keep['x'], inp['x']) and _same_bytes(keep['infeasible'], inp['infeasible']) and not keep['plan_x'].any()
    assert lib.igt_loop_advance_f32(None, 1, *([None] * 6), A_BRAKE, *([None] * 10), 0, L.IGT_MEM_HOST, None) == -1
    # n = 0: a no-op, whatever the buffers
    assert call(n_=0) == 0 and lib.igt_loop_advance_f64(s._h, 0, *([None] * 6), A_BRAKE, *([None] * 10), 0, L.IGT_MEM_DEVICE, None) == 0
    assert _same_bytes(keep['x'], inp['x']) and not keep['x_log'].any()
    # the optional groups may all be absent
    assert call(u_ws=True, flags_in=True, flags_out=True, infeasible=True, x_log=True, u_log=True, step=True) == 0
    assert not _same_bytes(keep['x'], inp['x']) and _same_bytes(keep['infeasible'], inp['infeasible'])
