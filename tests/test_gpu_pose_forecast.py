"""GPU: the pose forecast on the C ABI (include/igtmpc.h igt_set_route_headings, igt_forecast_scene_pose_f64,
igt_forecast_batch_pose_f64) and the rectangle closed loop on top of it (run_closed_loop ca_type='obca', pose_forecast='device'):
  1. rows 0-1 and tv_sv byte-equal to igt_forecast_scene_f64, row 2 within 1e-12 of the host code it restates
     (evaluate.obca_headings gathered per ego), not filtered behind an ego;
  2. device tensors and host arrays: the same bytes;
  3. the scene entry byte-equal to the batch entry on the gathered inputs;
  4. the refusals;
  5. the closed loop on device headings against the closed loop on host headings (1e-9);
  6. host loop, device-resident torch step, fused step and fused step under a captured graph: the same bytes;
  7. three vehicles: host loop and fused device loop the same bytes, every solved plan passes the restated verdict;
  8. the default keyword is pose_forecast='host', byte for byte."""
import numpy as np
import pytest

import box_collision_restated as BR
from helpers import rel_err

pytestmark = pytest.mark.gpu

DT = 0.1
SHAPES = [(3, 2, 2), (3, 3, 2), (3, 4, 2), (3, 2, 20), (3, 3, 20), (3, 4, 20), (70, 4, 2)]      # (E, M, N)


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ----------------------------------------------------------------------------- inputs
def _pose_inputs(E, M, N, seed):
    """Scenes for the pose forecast: random agents on the routes' centre lines as in tests/test_gpu_scene.py, and six agents of
    the first three scenes placed by hand so that every shape holds every branch of the heading (see _coverage):
      scene 0   agent 0: '12' (turning), no plan, 1.3 m before its arc at 9 m/s: node 1 before the arc, node 2 inside it, node 20
                         beyond it; agent 1: '32' (|heading| route), no plan, true heading -3.0
      scene 1   agent 0: '13' (straight), shares a plan whose extension takes the a = 0 retry (4.95 + 2.0 dt > 5);
                agent 1: '41' (|heading| route), shares a plan with negative headings whose extension does not (3.0 + 1.0 dt)
      scene 2   agent 0: '23' at s = 40, beyond its arc, eastbound at x = 37.9; agent 1: '31' (straight) at s = 30, westbound at
                         x = 20: back to back, each is behind the other."""
    from igtmpc import routes as R
    rng = np.random.default_rng(seed)
    rid = np.array([[R.ROUTE_ID[R.ROUTES[k]] for k in rng.integers(0, len(R.ROUTES), M)] for _ in range(E)], dtype=np.int32)
    s = rng.uniform(0.0, 45.0, (E, M))
    v = rng.uniform(-0.5, 6.0, (E, M))
    a = rng.uniform(-4.0, 3.0, (E, M))
    has_plan = rng.integers(0, 2, (E, M)).astype(np.int32)
    noise = rng.normal(0, 0.2, (E, M))
    hand = {(0, 0): ('12', 18.0, 9.0, 1.0, 0), (0, 1): ('32', 5.0, 2.0, 0.5, 0), (1, 0): ('13', 12.0, 4.0, 0.2, 1),
            (1, 1): ('41', 8.0, 3.0, 0.1, 1), (2, 0): ('23', 40.0, 2.0, 0.0, 0), (2, 1): ('31', 30.0, 2.0, 0.0, 0)}
    for (e, m), (r, s0, v0, a0, hp) in hand.items():
        rid[e, m], s[e, m], v[e, m], a[e, m], has_plan[e, m], noise[e, m] = R.ROUTE_ID[r], s0, v0, a0, hp, 0.0
    x = np.zeros((E, M, 7))
    x[..., 0:2] = np.stack([R.frenet2global(rid[:, m], s[:, m]) for m in range(M)], axis=1).reshape(E, M, 2)
    x[..., 2], x[..., 5] = s, v
    x[..., 6] = np.stack([R.psi_ref(rid[:, m], s[:, m]) for m in range(M)], axis=1) + noise
    x[0, 1, 6] = -3.0                                        # '32': the lane's heading is pi, the same direction as -3.0
    plan_x = rng.normal(0, 10.0, (E, M, 7, N + 1))
    plan_x[..., 0, :] += x[..., 0, None]
    plan_x[..., 1, :] += x[..., 1, None]
    plan_x[..., 2, :] = s[..., None] + np.linspace(0, 8, N + 1)
    plan_x[..., 5, :] = rng.uniform(4.0, 5.5, (E, M, 1))
    plan_x[..., 6, :] = x[..., 6, None] + rng.normal(0, 0.3, (E, M, N + 1))
    plan_u = rng.uniform(-1.0, 3.0, (E, M, 2, N))
    plan_x[1, 0, 5, N], plan_u[1, 0, 0, N - 1] = 4.95, 2.0
    plan_x[1, 1, 5, N], plan_u[1, 1, 0, N - 1] = 3.0, 1.0
    plan_x[1, 1, 6, :] = -np.abs(plan_x[1, 1, 6, :]) - 0.1
    return x, a, rid, plan_x, plan_u, has_plan


def _coverage(x, a, rid, plan_x, plan_u, has_plan, N):
    """What the inputs hold, computed from the arrays (not from how they were made)."""
    from igtmpc import routes as R
    from igtmpc.predictor import ConstantAccelerationModel
    E, M = a.shape
    T = R.TABLES
    flat = lambda q: np.asarray(q).reshape(E * M)
    turning = flat(T['turn'][rid] != 0)
    hp = flat(has_plan).astype(bool)
    sk = ConstantAccelerationModel(N=N, dt=DT).predict_arrays(flat(x[..., 2]), flat(x[..., 5]), flat(a), flat(rid))['s'][:, 1:]
    b0, b1 = flat(T['b0'][rid])[:, None], flat(T['b1'][rid])[:, None]
    roll = (turning & ~hp)[:, None]                          # nodes whose heading is psi_ref(s_k) on a route with an arc
    before, inside, beyond = roll & (sk < b0), roll & (sk >= b0) & (sk <= b1), roll & (sk > b1)
    vN, aN = flat(plan_x[:, :, 5, N]), flat(plan_u[:, :, 0, N - 1])
    retry = np.clip(vN + aN * DT, -2.0, 20.0) > 5.0
    absh = flat(T['abs_heading'][rid])
    return dict(straight=(~turning).any(), turning=turning.any(),
                arc_in_one_horizon=(before.any(1) & inside.any(1) & beyond.any(1)).any(),
                arc_regimes=before.any() and inside.any() and beyond.any(),
                enters_arc_in_one_horizon=(before.any(1) & inside.any(1)).any(),
                abs_negative_true=(absh & ~hp & (flat(x[..., 6]) < 0)).any(),
                abs_negative_plan=(absh & hp & (plan_x[:, :, 6, 1:].reshape(E * M, N) < 0).any(1)).any(),
                with_plan=hp.any(), without_plan=(~hp).any(), retry=(hp & retry).any(), no_retry=(hp & ~retry).any())


def _host_headings(x, a, rid, plan_x, plan_u, has_plan, N):
    """The parent commit's host code: obca_headings, gathered per ego (what the host loop concatenates behind x, y)."""
    from igtmpc import routes as R
    from igtmpc.evaluate import gather_opponents, obca_headings
    from igtmpc.predictor import ConstantAccelerationModel
    pred = ConstantAccelerationModel(N=N, dt=DT)
    return gather_opponents(obca_headings(pred, x, a, rid, has_plan.astype(bool), plan_x, plan_u, R.TABLES['abs_heading'][rid]))


def _gather(x, a, rid, plan_x, plan_u, has_plan):
    """The inputs of igt_forecast_batch_pose_f64 for the E M problems: ego i, opponents j != i in ascending j."""
    from igtmpc.evaluate import gather_opponents as g
    E, M = a.shape
    ego = x[:, :, [0, 1, 6]].reshape(E * M, 3)
    return ego, g(x[:, :, [0, 1, 2, 5]]), g(a), g(rid), g(x[:, :, 6]), g(plan_x), g(plan_u), g(has_plan)


# ----------------------------------------------------------------------------- 1. the pose against what it restates
@pytest.mark.parametrize('E,M,N', SHAPES)
def test_pose_equals_the_scene_forecast_and_the_host_headings(E, M, N):
    """Rows 0-1 and tv_sv: the bytes of forecast_scene on the same inputs.  Row 2: within 1e-12 absolute of the host headings --
    the project's bar for float64 restatements of closed-form arithmetic; the formula is a subtraction, a division, a clamp
    and one multiply-add on values below 2 pi, and the forecast's dt*dt against numpy's dt**2 moves s by units in the last
    place.  A pair behind the ego: x = y = -20, the heading row still the unfiltered one.
    E = 70, M = 4 has 280 agent rows: a second workgroup of 256 and its tail guard.
    Coverage, asserted: every shape holds a straight and a turning route, an |heading| route with a negative true heading and
    one with negative plan headings, agents with and without a shared plan, a plan whose extension takes the a = 0 retry and
    one that does not, a pair behind its ego, and a forecast that enters its arc within the horizon.  s before, inside AND
    beyond the arc within ONE horizon needs 13.5 m in the horizon: the N = 20 shapes hold it (asserted); two nodes (N = 2) cannot
    lie in three regimes, there the three regimes are held by different agents (asserted)."""
    import igtmpc
    x, a, rid, px, pu, hp = _pose_inputs(E, M, N, seed=1000 * M + 10 * N + E)
    cov = _coverage(x, a, rid, px, pu, hp, N)
    one_horizon = cov.pop('arc_in_one_horizon')
    assert all(cov.values()), cov
    assert one_horizon == (N == 20), (N, one_horizon)
    ref_head = _host_headings(x, a, rid, px, pu, hp, N)
    with igtmpc.BatchSolver(N=N, dt=DT, n_obs=M - 1, dtype='f64') as s:
        for plans in (True, False):
            args = (x, a, rid) + ((px, pu, hp) if plans else ())
            ref = ref_head if plans else _host_headings(x, a, rid, px, pu, np.zeros_like(hp), N)
            xy, tv0 = s.forecast_scene(*args)
            pose, tv = s.forecast_scene_pose(*args)
            assert pose.shape == (E * M, M - 1, 3, N + 1) and tv.shape == (E * M, M - 1, 2)
            assert _same_bytes(pose[:, :, :2], xy) and _same_bytes(tv, tv0), plans
            err = np.abs(pose[:, :, 2] - ref)
            print(f'E={E} M={M} N={N} plans={plans}: max |heading - host heading| = {err.max():.3e}')
            assert np.isfinite(pose).all() and err.max() <= 1e-12, (plans, err.max())
            behind = (xy == -20.0).all(axis=(2, 3))                                  # [E M, M-1]
            assert behind.any() and not behind.all()
            # the filter of the host loop, restated: (p_obs - p_ego) . (cos psi, sin psi) < 0 at the forecast's first point
            assert behind[2 * M + 0, 0] and behind[2 * M + 1, 0]                      # scene 2: agents 0 and 1, back to back
            assert (pose[behind][:, :2] == -20.0).all()
            assert np.abs(pose[behind][:, 2] - ref[behind]).max() <= 1e-12 and not (pose[behind][:, 2] == -20.0).any()
        assert s.forecast_scene_pose(x[:0], a[:0], rid[:0])[0].shape == (0, M - 1, 3, N + 1)      # E = 0: nothing to do


# ----------------------------------------------------------------------------- 2. device tensors and host arrays
@pytest.mark.parametrize('E,M,N', [(3, 2, 20), (70, 4, 2)])
def test_device_tensors_give_the_bytes_of_host_arrays(E, M, N):
    import torch
    import igtmpc
    x, a, rid, px, pu, hp = _pose_inputs(E, M, N, seed=5)
    dev = lambda v: torch.as_tensor(np.ascontiguousarray(v), device='cuda')
    with igtmpc.BatchSolver(N=N, dt=DT, n_obs=M - 1, dtype='f64') as s:
        for plans in (True, False):
            arrs = (x, a, rid) + ((px, pu, hp) if plans else ())
            pose, tv = s.forecast_scene_pose(*arrs)
            d_pose, d_tv = s.forecast_scene_pose(*[dev(v) for v in arrs])
            torch.cuda.synchronize()
            assert _same_bytes(d_pose.cpu().numpy(), pose) and _same_bytes(d_tv.cpu().numpy(), tv), plans


# ----------------------------------------------------------------------------- 3. scene entry against batch entry
@pytest.mark.parametrize('M', [2, 4])
def test_scene_entry_equals_batch_entry_on_gathered_inputs(M):
    import torch
    import igtmpc
    N = 20
    sq = (lambda v: v[:, 0]) if M == 2 else (lambda v: v)       # the two-vehicle entry has no n_obs axis on its inputs
    dev = lambda v: torch.as_tensor(np.ascontiguousarray(v), device='cuda')
    with igtmpc.BatchSolver(N=N, dt=DT, n_obs=M - 1, dtype='f64') as s:
        for E in (3, 70):
            x, a, rid, px, pu, hp = _pose_inputs(E, M, N, seed=40 + E)
            ego, opp, oa, orid, ohead, opx, opu, ohp = _gather(x, a, rid, px, pu, hp)
            for plans in (True, False):
                pose, tv = s.forecast_scene_pose(x, a, rid, *((px, pu, hp) if plans else ()))
                b_pose, b_tv = s.forecast_pose(ego, sq(opp), sq(oa), sq(orid), sq(ohead),
                                               *((sq(opx), sq(opu), sq(ohp)) if plans else ()))
                assert b_pose.shape == (E * M, M - 1, 3, N + 1)
                assert _same_bytes(b_pose, pose) and _same_bytes(b_tv.reshape(tv.shape), tv), (E, plans)
                xy, _ = s.forecast(ego, sq(opp), sq(oa), sq(orid), *((sq(opx), sq(opu), sq(ohp)) if plans else ()))
                assert _same_bytes(b_pose[:, :, :2], xy), (E, plans)                      # the batch entry keeps the batch forecast's bits
            d_pose, d_tv = s.forecast_pose(dev(ego), *[dev(sq(v)) for v in (opp, oa, orid, ohead, opx, opu, ohp)])
            torch.cuda.synchronize()
            pose, tv = s.forecast_scene_pose(x, a, rid, px, pu, hp)
            assert _same_bytes(d_pose.cpu().numpy(), pose) and _same_bytes(d_tv.cpu().numpy().reshape(tv.shape), tv), E


# ----------------------------------------------------------------------------- 4. refusals
def test_refusals():
    import igtmpc
    from igtmpc import _lib as L
    from igtmpc import routes as R
    lib = L.load()
    INVALID = -1
    N, M = 20, 2
    x, a, rid, px, pu, hp = _pose_inputs(3, M, N, seed=9)
    pose, tv = np.zeros((6, 1, 3, N + 1)), np.zeros((6, 1, 2))
    heads = np.ascontiguousarray(np.column_stack([R.TABLES['h0'], R.TABLES['hN'], R.TABLES['abs_heading'].astype(np.float64)]))
    p = lambda v: v.ctypes.data

    def refused(rc, word):
        msg = lib.igt_last_error()
        assert rc == INVALID and msg and word in msg.decode(), (rc, msg)

    def scene(s):
        return lib.igt_forecast_scene_pose_f64(s._h, 3, p(x), p(a), p(rid), None, None, None, p(pose), p(tv), L.IGT_MEM_HOST, None)
    ego, opp, oa, orid, ohead = [np.ascontiguousarray(v) for v in _gather(x, a, rid, px, pu, hp)[:5]]

    with igtmpc.BatchSolver(N=N, dt=DT, n_obs=M - 1, dtype='f64') as s:
        refused(lib.igt_set_route_headings(s._h, len(heads), p(heads)), 'igt_set_routes')      # a handle without routes
        s.set_routes()
        refused(scene(s), 'igt_set_route_headings')                                            # routes, but no headings
        refused(lib.igt_forecast_batch_pose_f64(s._h, 6, p(ego), p(opp), p(oa), p(orid), p(ohead), None, None, None, p(pose), p(tv),
                                                L.IGT_MEM_HOST, None), 'igt_set_route_headings')
        refused(lib.igt_set_route_headings(s._h, len(heads) - 1, p(heads)), 'n_routes')
        refused(lib.igt_set_route_headings(s._h, len(heads), None), 'null')
        refused(lib.igt_set_route_headings(None, len(heads), p(heads)), 'null')
        for col, bad in ((0, np.nan), (0, np.inf), (1, -np.inf)):
            t = heads.copy()
            t[3, col] = bad
            refused(lib.igt_set_route_headings(s._h, len(t), p(t)), 'finite')
        refused(scene(s), 'igt_set_route_headings')                                            # a refused table sets nothing
        assert lib.igt_set_route_headings(s._h, len(heads), p(heads)) == 0
        assert scene(s) == 0
        want = pose.copy()
        got, _ = s.forecast_scene_pose(x, a, rid)                                              # the Python face: the same table
        assert _same_bytes(got, want)
        assert lib.igt_forecast_scene_pose_f64(s._h, 0, None, None, None, None, None, None, None, None, L.IGT_MEM_HOST, None) == 0
        assert lib.igt_forecast_batch_pose_f64(s._h, 0, None, None, None, None, None, None, None, None, None, None, L.IGT_MEM_HOST,
                                               None) == 0                                      # E = 0, B = 0: no-ops
        refused(lib.igt_forecast_scene_pose_f64(s._h, -1, p(x), p(a), p(rid), None, None, None, p(pose), p(tv), L.IGT_MEM_HOST,
                                                None), 'E < 0')
        s.set_routes(np.zeros((5, 12)))                                                        # another n_routes drops the headings
        refused(scene(s), 'igt_set_route_headings')
    with igtmpc.BatchSolver(N=N, dt=DT, n_obs=M - 1, dtype='f32') as s:
        f = lambda v: v.astype(np.float32)
        with pytest.raises(ValueError, match='f64'):
            s.forecast_scene_pose(f(x), f(a), rid)
        with pytest.raises(ValueError, match='f64'):
            s.forecast_pose(f(ego), f(opp[:, 0]), f(oa[:, 0]), orid[:, 0], f(ohead[:, 0]))
        with pytest.raises(ValueError, match='f64'):
            s.set_route_headings()


# ----------------------------------------------------------------------------- 5 .. 8: the closed loop
CASE = dict(ca_type='obca', num_samples=4, N=20, T_sim=2.0, v0=3.0)      # tests/test_gpu_box.py's closed-loop case: from 3 m/s the
_runs = {}                                                               # forecasts do enter the 4.9 m gate
KEYS = ('x_data', 'u_data', 'infeasible_ratio', 'deadlock')


def _loop(name, **kw):
    """One run per configuration for the whole module (the results are read, never written)."""
    from igtmpc.evaluate import run_closed_loop
    if name not in _runs:
        _runs[name] = run_closed_loop(**dict(CASE, **kw))
    return _runs[name]


def _host_loop_device_pose():
    return _loop('host_loop_device_pose', pose_forecast='device', log_plans=True)


def _captured_on_own_stream(monkeypatch, **kw):
    """run_closed_loop(graph=True) captures on `torch.cuda.Stream(dev)`, a stream of torch's pool, which keeps its hardware queue
    as long as the process lives and disturbs tests/test_gpu_overlap.py later (tests/test_gpu_loop_advance.py
    _run_captured_on_own_stream has the story).  The driver's request for a new stream is answered with a stream of the test's
    own, destroyed at the end: one capture, one stream, no parallel branches."""
    import torch
    from handle_walk_cases import side_stream
    from igtmpc.evaluate import run_closed_loop
    pool_stream = torch.cuda.Stream
    if torch.cuda.graph.default_capture_stream is None:      # torch makes it at the first capture of a process: not from `own`
        torch.cuda.graph.default_capture_stream = pool_stream()
    with side_stream() as own:
        def stream(*a, **k):
            return pool_stream(*a, **k) if ('stream_id' in k or 'stream_ptr' in k) else own
        monkeypatch.setattr(torch.cuda, 'Stream', stream)
        try:
            return run_closed_loop(**kw)
        finally:
            monkeypatch.setattr(torch.cuda, 'Stream', pool_stream)


def test_closed_loop_on_device_headings_matches_host_headings():
    """The two runs differ only by the heading's last bits: states and applied inputs within 1e-9 (helpers.rel_err, the project's
    closed-loop bar against its oracle loop), infeasible steps and the deadlock flag equal.  The 'device' run's forecasts enter a
    gate (asserted), so the headings are read."""
    host = _loop('host_loop_host_pose', pose_forecast='host', log_plans=True)
    dev = _host_loop_device_pose()
    n_in = 0
    for step in dev['plans']:
        ok = step['ok'].reshape(-1)
        assert step['obs'].shape == (8, 1, 3, 21)
        n_in += int(BR.margins(step['x'].reshape(8, 1, 7, 21)[ok], step['obs'][ok])[1].sum())
    ex, eu = rel_err(dev['x_data'], host['x_data']).max(), rel_err(dev['u_data'], host['u_data']).max()
    eh = max(np.abs(d['obs'][:, :, 2] - h['obs'][:, :, 2]).max() for d, h in zip(dev['plans'], host['plans']))
    print(f'device against host headings: pairs inside a gate {n_in}, max rel err x {ex:.2e} u {eu:.2e}, step-wise heading {eh:.2e}')
    assert n_in > 0, 'no forecast came inside a gate: the headings were never read'
    assert ex < 1e-9 and eu < 1e-9
    assert np.array_equal(dev['infeasible_ratio'], host['infeasible_ratio']) and np.array_equal(dev['deadlock'], host['deadlock'])


def test_device_resident_rectangle_loops_equal_the_host_loop_bytewise(monkeypatch):
    """pose_forecast='device': the host loop, device_resident with step='torch', with step='fused', and step='fused' under a
    captured graph (T_sim = 2.0: 18 replays) give the same x_data, u_data, infeasible_ratio and deadlock, byte for byte; the
    last column of u_data is non-zero, i.e. the last replay wrote it."""
    host = _host_loop_device_pose()
    runs = dict(torch=_loop('dev_torch', pose_forecast='device', device_resident=True, step='torch'),
                fused=_loop('dev_fused', pose_forecast='device', device_resident=True, step='fused'))
    runs['graph'] = _captured_on_own_stream(monkeypatch, **dict(CASE, pose_forecast='device', device_resident=True, step='fused',
                                                                graph=True))
    assert host['u_data'].shape == (4, 4, 20) and np.rint(host['infeasible_ratio'] * 20).sum() < 4 * 2 * 20      # something solved
    for name, got in runs.items():
        for k in KEYS:
            assert _same_bytes(got[k], host[k]), (name, k)
        assert (got['u_data'][:, :, -1] != 0).any(), name


def test_three_vehicle_rectangle_loop():
    """num_agents = 3 (n_obs = 2: the scene kernel's M = 3 build and two obstacle slots per ego): host loop and fused
    device-resident loop byte-equal, and every solved plan of the host run passes the restated verdict against the pose it was
    solved against."""
    from igtmpc.evaluate import run_closed_loop
    kw = dict(num_agents=3, num_samples=2, N=20, T_sim=1.0, v0=3.0, ca_type='obca', pose_forecast='device')
    host = run_closed_loop(log_plans=True, **kw)
    dev = run_closed_loop(device_resident=True, step='fused', **kw)
    for k in KEYS:
        assert _same_bytes(dev[k], host[k]), k
    n_ok = 0
    for step in host['plans']:
        ok = step['ok'].reshape(-1)
        assert step['obs'].shape == (6, 2, 3, 21)
        g = BR.margins(step['x'].reshape(6, 1, 7, 21)[ok], step['obs'][ok])[0]
        assert (g <= 1e-6 + 1e-9).all()
        n_ok += int(ok.sum())
    print('three vehicles: solved problems', n_ok, 'of', 6 * 10)
    assert n_ok > 0


def test_default_keyword_is_the_host_pose():
    from igtmpc.evaluate import run_closed_loop
    kw = dict(ca_type='obca', num_samples=2, N=20, T_sim=0.5)
    a, b = run_closed_loop(**kw), run_closed_loop(pose_forecast='host', **kw)
    for k in KEYS:
        assert _same_bytes(a[k], b[k]), k
