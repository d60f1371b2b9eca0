"""The rectangle (OBCA) collision model on the device: BatchSolver.solve_box / rollout_all_box (include/igtmpc.h
igt_solve_batch_box_f64 / igt_rollout_batch_box_f64).

  1. parity with the reference answer of every case of tests/box_cases.py (the oracle plus the numpy restatement,
     tests/box_collision_restated.py; tests/test_box_host.py holds the cases' figures to the inputs): no scenario set aside,
     tol = eps = tie = 1e-9; every candidate's roll-out, cost and verdict bits;
  2. reduction: with every obstacle beyond the gate of every candidate the answers are those of solve / rollout_all without
     obstacles, byte for byte -- every family, a refinement pass where the family takes one;
  3. refinement and warm start: every solved winner's own trajectory passes the restated verdict and x is the roll-out of u;
  4. isolation: NaN poses in one scenario leave every other row byte-equal;
  5. device tensors: byte-equal to the host call; captured on one side stream, a replay reads the poses of replay time;
  6. what is refused, and that an empty batch works."""
import contextlib
import ctypes

import numpy as np
import pytest

import box_cases as BC
import box_collision_restated as R
import np_oracle as O
from helpers import compare_solve, host_params, rel_err, verdict_margins
from parity_cases import cinf_default, value_net_case, warm_args

pytestmark = pytest.mark.gpu

SOLVE_KEYS = ('x', 'u', 'cost', 'argmin', 'status')
ROLL_KEYS = ('X', 'U', 'cost', 'viol')
FIRST = ('lattice', 48, 20, 64, 1, 4, False, None)


@pytest.fixture(scope='module')
def igt():
    import igtmpc
    igtmpc.load_library()
    return igtmpc


def _same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@contextlib.contextmanager
def _side_stream(torch):
    """A side stream of this test's own, created on the HIP runtime the process has loaded and destroyed again at the end (not
    one of torch.cuda.Stream()'s pool, which lives as long as the process: tests/test_gpu_candidates.py says why)."""
    path = next(line.split()[-1] for line in open('/proc/self/maps') if 'libamdhip64' in line)
    hip = ctypes.CDLL(path)
    st = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(st), 1) == 0          # hipStreamNonBlocking
    try:
        yield torch.cuda.ExternalStream(st.value)
    finally:
        torch.cuda.synchronize()
        assert hip.hipStreamDestroy(st) == 0


# ----------------------------------------------------------------------------- 1. oracle parity
@pytest.mark.parametrize('key', list(BC.CASES), ids=BC.case_id)
def test_matches_the_reference_answer(igt, key):
    case, want = BC.build(key), BC.CASES[key]
    passes, x0, kp = BC.oracle(case)
    ref, P = passes[0], case['P']
    pos, opt = BC.solve_args(case)
    with BC.open_solver(igt, case) as s:
        got = s.solve_box(*pos, **opt)
        roll = s.rollout_all_box(*pos, **opt)
        xy = np.ascontiguousarray(case['pose'][:, :, :2])
        circle = s.solve(*pos[:4], xy, **opt)
        circle_roll = s.rollout_all(*pos[:4], xy, **opt)
    m = compare_solve(got, passes, P, x0, kp, eps=BC.BAR, tie=BC.BAR, tol=BC.BAR, share=1.0, tie_share=1.0, min_solved=want['solved'],
                      label='box[' + BC.case_id(key) + ']')
    assert m['compared'] == case['B'], 'no scenario is set aside'
    moved = (got['status'] == 0) & (got['argmin'] != case['free']['argmin'])
    assert moved.sum() == want['moved']
    # the same handle still judges circles: stateless entries (its answers differ where the rectangle verdict let a plan pass)
    assert not _same_bytes(circle['argmin'], got['argmin'])
    # every candidate of every scenario.  The controls do not depend on the collision model: with the rectangles near, they are
    # the bytes rollout_all of the same handle gives for the same inputs (the verdicts are what differs)
    assert _same_bytes(roll['U'], circle_roll['U'])
    assert not _same_bytes(roll['viol'], circle_roll['viol'])
    # ... and against the oracle they are held to the bars tests/test_gpu_parity.py holds rollout_all to: exact where they are
    # sums and clamps of the inputs (lattice) or the table itself; 1e-14 for ramp-hold, whose targets go through m(u) = u |u|
    # sqrt|u|, which numpy and the device round an ulp apart; 1e-12 for the tracking family, whose controls are a feedback on the
    # rolled state (v, e_y, e_psi), on every candidate whose RK stages stay clear of the route's curvature break points by 1e-9
    # (np_oracle.breakpoint_distance: at a break point rounding decides which curvature the feedback reads)
    err_u = rel_err(roll['U'], ref['U'])
    if case['family'] == 'track':
        clear_u = O.breakpoint_distance(x0, ref['U'], kp, P) > BC.BAR
        assert clear_u.all(), 'by the oracle alone every candidate of these cases is clear: none is set aside'
        err_u = err_u[clear_u]
    worst_u = err_u.max()
    print('rollout_all_box: worst control error', worst_u)
    assert worst_u <= {'track': 1e-12, 'ramp_hold': 1e-14}.get(case['family'], 0.0)
    assert rel_err(roll['X'], ref['X']).max() < 1e-9
    fin = np.isfinite(ref['J'])
    worst = rel_err(roll['cost'][fin], ref['J'][fin]).max()
    print('rollout_all_box: worst cost error', worst)
    assert worst <= 1e-9
    A, b = case['cinf']
    g = verdict_margins(ref['X'], ref['U'], None, A, b, P)
    g[..., 5] = ref['g_box']
    clear = (np.abs(g - P.feas_tol) > BC.BAR).all(axis=-1)
    print('verdicts clear of feas_tol by 1e-9:', clear.mean(), 'collision bits', int((roll['viol'] & 32 != 0).sum()))
    assert clear.mean() > 0.99
    assert (roll['viol'][clear] == ref['mask'][clear]).all()
    assert ((roll['viol'] == 0) == ref['feas'])[clear].all()
    assert (roll['viol'] & 32 != 0).any() and (ref['mask'][clear] & 32 != 0).any()


# ----------------------------------------------------------------------------- 2. reduction to what exists
def _poses_behind(case, n_obs, back):
    """Stationary rectangles `back` metres behind every ego's start, side by side; -> pose[B,n_obs,3,N+1]."""
    x0 = O.apply_flags(case['x0'], case['flags'])
    psi = x0[:, 6]
    pose = np.zeros((case['B'], n_obs, 3, case['N'] + 1))
    for o in range(n_obs):
        pose[:, o, 0, :] = (x0[:, 0] - back * np.cos(psi) - 3.0 * o * np.sin(psi))[:, None]
        pose[:, o, 1, :] = (x0[:, 1] - back * np.sin(psi) + 3.0 * o * np.cos(psi))[:, None]
        pose[:, o, 2, :] = (psi + 0.3 * o)[:, None]
    return pose


@pytest.mark.parametrize('back', [16.0, 500.0], ids=['in-reach', 'out-of-reach'])
@pytest.mark.parametrize('key', [('lattice', 24, 20, 256, 2, 4, False, None), ('track', 24, 40, 64, 2, 4, False, None),
                                 ('ramp_hold', 48, 20, 64, 1, 4, False, None), ('table', 24, 20, 64, 1, 4, False, 'table')],
                         ids=BC.case_id)
def test_obstacles_beyond_the_gate_reduce_to_the_solve_without_obstacles(igt, key, back):
    case = BC.build(key)
    refine = 1 if case['family'] in ('ramp_hold', 'track') else 0
    pose = _poses_behind(case, case['n_obs'], back)
    # what the test rests on, by the restatement on the oracle's roll-outs: no candidate comes inside any gate; and at 16 m the
    # rectangles are within the reach that decides whether a unit rolls the Cartesian rows at all (csrc/igt_fast64.h
    # box_out_of_reach), at 500 m beyond it
    assert not R.margins(case['free']['X'], pose)[1].any()
    P = case['P']
    reach = (max(abs(P.v_min), abs(P.v_max)) + max(abs(P.a_min), abs(P.a_max)) * P.dt) * P.N * P.dt + 1.0 + R.gate_radius()
    assert (back < reach) == (back == 16.0)
    pos, opt = BC.solve_args(case)
    pos[4] = pose
    with BC.open_solver(igt, case, refine_iters=refine) as s:
        got = s.solve_box(*pos, **opt)
        roll = s.rollout_all_box(*pos, **opt)
    free = dict(case, n_obs=0)
    with BC.open_solver(igt, free, refine_iters=refine) as s0:
        want = s0.solve(*pos[:4], None, **opt)
        roll0 = s0.rollout_all(*pos[:4], None, **opt)
    for k in SOLVE_KEYS:
        assert _same_bytes(got[k], want[k]), k
    for k in ROLL_KEYS:
        assert _same_bytes(roll[k], roll0[k]), k
    assert (got['status'] == 0).sum() >= 4


# ----------------------------------------------------------------------------- 3. refinement and warm start
@pytest.mark.parametrize('key', [('ramp_hold', 48, 20, 64, 1, 4, False, None), ('track', 24, 40, 64, 2, 4, False, None)], ids=BC.case_id)
def test_refined_warm_started_winners_pass_the_restated_verdict(igt, key):
    case = BC.build(key)
    b = dict(u_prev=case['u_prev'], flags=case['flags'])
    u_prev, u_ws, flags = warm_args(b, np.float64, N=case['N'])
    with BC.open_solver(igt, case, refine_iters=2) as s:
        got = s.solve_box(case['x0'], u_prev, case['kparams'], flags, case['pose'], u_ws=u_ws)
        first = s.solve_box(case['x0'], u_prev, case['kparams'], flags, case['pose'])
    sol = got['status'] == 0
    print(BC.case_id(key), 'solved', int(sol.sum()), 'of', case['B'])
    assert sol.sum() >= case['B'] // 3
    assert not _same_bytes(first['u'], got['u']), 'the warm start is read'
    x0 = O.apply_flags(case['x0'], flags)
    X = O.rollout_frenet(x0[sol], got['u'][sol], case['kparams'][sol], case['P'])
    assert rel_err(got['x'][sol], X).max() <= 1e-9, 'x is the roll-out of u'
    g, inside, _ = R.margins(got['x'][sol][:, None], case['pose'][sol])
    print('worst rectangle margin of a winner', g.max(), 'pairs inside the gate', int(inside.sum()))
    assert inside.any()
    assert (g <= case['P'].feas_tol + 1e-9).all()


# ----------------------------------------------------------------------------- 4. isolation
@pytest.mark.parametrize('key', [FIRST, ('track', 24, 40, 64, 2, 4, False, None)], ids=BC.case_id)
def test_nan_poses_stay_in_their_scenario(igt, key):
    case = BC.build(key)
    pos, opt = BC.solve_args(case)
    b0 = int(np.flatnonzero(case['ref']['status'] == 0)[1])
    bad = case['pose'].copy()
    bad[b0] = np.nan
    with BC.open_solver(igt, case) as s:
        clean = s.solve_box(*pos, **opt)
        got = s.solve_box(*pos[:4], bad, **opt)
        roll = s.rollout_all_box(*pos[:4], bad, want_X=False, want_U=False, **opt)
    others = np.arange(case['B']) != b0
    for k in SOLVE_KEYS:
        assert _same_bytes(got[k][others], clean[k][others]), k
    # the poisoned scenario has no rectangle constraint left: the obstacle-free answer
    free = case['free']
    assert got['status'][b0] == free['status'][b0] and got['argmin'][b0] == free['argmin'][b0]
    assert (roll['viol'][b0] & 32 == 0).all()
    # one NaN coordinate of one node removes that node alone
    one = case['pose'].copy()
    one[b0, 0, 1, 1:4] = np.nan
    want = BC.reference_answer(case['free'], one, case['P'])
    with BC.open_solver(igt, case) as s:
        got1 = s.solve_box(*pos[:4], one, **opt)
    assert got1['status'][b0] == want['status'][b0] and got1['argmin'][b0] == want['argmin'][b0]
    for k in SOLVE_KEYS:
        assert _same_bytes(got1[k][others], clean[k][others]), k


# ----------------------------------------------------------------------------- 5. device tensors and capture
def test_device_tensors_and_capture_read_the_poses_at_replay_time(igt):
    import torch
    case = BC.build(FIRST)
    B = 8
    dev = lambda a: torch.from_numpy(np.array(a.view(np.int32) if a.dtype == np.uint32 else a)).cuda()      # (a copy: the case is read-only)
    pos = [dev(case[k][:B]) for k in ('x0', 'u_prev', 'kparams', 'flags')]
    far = _poses_behind(case, 1, 500.0)[:B]
    P1, P2 = dev(case['pose'][:B]), dev(far)
    with BC.open_solver(igt, case) as s:
        eager = []
        for Pi in (P1, P2):
            e = s.solve_box(*pos, Pi)
            torch.cuda.synchronize()
            eager.append({k: v.cpu().numpy() for k, v in e.items()})
        host = s.solve_box(*[case[k][:B] for k in ('x0', 'u_prev', 'kparams', 'flags')], case['pose'][:B])
        for k in SOLVE_KEYS:
            assert _same_bytes(host[k], eager[0][k]), k
        pose = P1.clone()
        out = {k: torch.empty_like(v) for k, v in e.items()}
        replayed = []
        with _side_stream(torch) as side:
            with torch.cuda.stream(side):
                s.solve_box(*pos, pose, out=out)                      # warm-up on the capture stream
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):                    # a single stream, no parallel branches
                s.solve_box(*pos, pose, out=out)
            for Pi in (P1, P2):
                pose.copy_(Pi)
                torch.cuda.synchronize()
                g.replay()
                torch.cuda.synchronize()
                replayed.append({k: v.cpu().numpy() for k, v in out.items()})
            del g
    for i in range(2):
        for k in SOLVE_KEYS:
            assert _same_bytes(replayed[i][k], eager[i][k]), (i, k)
    assert (eager[0]['status'] == 0).sum() >= 2
    assert not _same_bytes(replayed[0]['argmin'], replayed[1]['argmin']), 'the replay did not read the poses on the device'


# ----------------------------------------------------------------------------- 6. refusals
def _raw_box_calls(s, L, B=1):
    """Both box entries called on s's handle through ctypes, past the checks BatchSolver makes itself: -> [(rc, message)].  The
    buffers are never reached by a call that is refused for what the handle is."""
    dummy = np.zeros(8)
    p = dummy.ctypes.data
    out = []
    for name, n_out in (('igt_solve_batch_box_f64', 5), ('igt_rollout_batch_box_f64', 4)):
        rc = getattr(s.lib, name)(s._h, B, *([p] * 8), 4.47, 2.0, 0.0, *([p] * n_out), L.IGT_MEM_HOST, None)
        out.append((rc, s.lib.igt_last_error().decode()))
    return out


def test_refusals_and_edges(igt, monkeypatch):
    case = BC.build(FIRST)
    pos, opt = BC.solve_args(case, slice(0, 4))
    L = igt._lib
    with BC.open_solver(igt, case) as s:
        for fn in (s.solve_box, s.rollout_all_box):
            for kw, word in ((dict(length=0.0), 'length'), (dict(length=np.nan), 'length'), (dict(width=-1.0), 'width'),
                             (dict(width=np.inf), 'width'), (dict(d_box=-0.1), 'd_box'), (dict(d_box=np.nan), 'd_box')):
                with pytest.raises(igt.IgtError, match=word):
                    fn(*pos, **kw)
            with pytest.raises(ValueError, match='shape'):
                fn(*pos[:4], case['pose'][:4, :, :2])              # obs_xy is not a pose array
        e_pos, _ = BC.solve_args(case, slice(0, 0))
        empty = s.solve_box(*e_pos)
        assert empty['x'].shape == (0, 7, 21) and empty['status'].shape == (0,)
        assert s.rollout_all_box(*e_pos)['cost'].shape == (0, 64)
        n_ptr = 8
        dummy = np.zeros(8)
        assert s.lib.igt_solve_batch_box_f64(None, 1, *([dummy.ctypes.data] * n_ptr), 4.47, 2.0, 0.0, *([dummy.ctypes.data] * 5),
                                             L.IGT_MEM_HOST, None) == -1
        assert b'null handle' in s.lib.igt_last_error()
        # a larger d_box refuses more: the distance to keep is read
        a = s.rollout_all_box(*pos, want_X=False, want_U=False)['viol']
        c = s.rollout_all_box(*pos, want_X=False, want_U=False, d_box=1.0)['viol']
        assert ((c & 32) >= (a & 32)).all() and ((c & 32) != (a & 32)).any()
    with BC.open_solver(igt, case, polish_iters=1) as s:
        for fn in (s.solve_box, s.rollout_all_box):
            with pytest.raises(igt.IgtError, match='polish_iters'):
                fn(*pos)
        assert s.solve(*pos[:4], np.ascontiguousarray(case['pose'][:4, :, :2]))['status'].shape == (4,)      # the circle entry is untouched
    net = value_net_case(1, 'f64')['net']
    with igt.BatchSolver(C=64, dtype='f64', cost_mode='value_net', value_polish_iters=1) as s:
        s.set_value_net(**net)
        with pytest.raises(ValueError, match='value_polish'):
            s.solve_box(*pos)
    # ... which pre-empts the library's own refusal of a handle with igt_set_value_polish on (the 'device' driver sets the
    # handle's field): asked directly, both entries return IGT_E_INVALID (-1) and name the cause
    with igt.BatchSolver(C=64, dtype='f64', cost_mode='value_net', value_polish_iters=1, value_polish_driver='device') as s:
        s.set_value_net(**net)
        for rc, msg in _raw_box_calls(s, L):
            assert rc == -1 and 'igt_set_value_polish' in msg, (rc, msg)
    # the developer kernels know the circle alone: a handle created under one of their flags is refused by the library
    monkeypatch.setenv('IGT_DEV_FLAGS', str(L.DEV_LITERAL))
    with BC.open_solver(igt, case) as s:
        assert s.lib is L.load(True)
        for rc, msg in _raw_box_calls(s, L):
            assert rc == -1 and 'developer kernels' in msg, (rc, msg)
        for fn in (s.solve_box, s.rollout_all_box):
            with pytest.raises(igt.IgtError, match='developer kernels'):
                fn(*pos)
    monkeypatch.delenv('IGT_DEV_FLAGS')
    with igt.BatchSolver(C=64, dtype='f32') as s:
        f4 = [p.astype(np.float32) if p.dtype == np.float64 else p for p in pos]
        for fn in (s.solve_box, s.rollout_all_box):
            with pytest.raises(ValueError, match="dtype='f64'"):
                fn(*f4)


# ----------------------------------------------------------------------------- 7. planner
def _scene(routes, s0s, v0s):
    import igtmpc
    from igtmpc import routes as RT
    agents, refs = [], []
    for r, s0, v0 in zip(routes, s0s, v0s):
        rid = RT.ROUTE_ID[r]
        xy = RT.frenet2global(rid, s0)
        K = igtmpc.Curvature.from_route(r)
        agents.append({'type': 'CAV', 'state': igtmpc.VehicleReference(
            {'x': xy[0], 'y': xy[1], 's': s0, 'ey': 0.02, 'epsi': -0.01, 'v': v0, 'heading': float(RT.psi_ref(rid, s0)), 'K': K})})
        kk = np.zeros(151)
        if RT.CONSTANTS[r].get('Kv'):
            kk[40:80] = RT.CONSTANTS[r]['Kv']
        refs.append({'K': kk})
    return agents, refs


@pytest.fixture
def planner_handles(igt, monkeypatch):
    """Planners share solver handles (igtmpc.planner._SHARED) and keep them, and their streams, until the interpreter exits.
    The test gets a table of its own, and what it opened there is closed when it ends: no other test sees a handle of it."""
    own = {}
    monkeypatch.setattr(igt.planner, '_SHARED', own)
    yield own
    while own:
        own.popitem()[1].close()


def test_planner_obca_solves_through_solve_box(igt, planner_handles):
    """MPC_Planner(ca_type='obca'): d_min = 0 (mpc.py:42-43), the predictions marshalled with their heading -- |heading| for
    obstacles on routes '32', '41' (mpc.py:250-253) --, solved through solve_box with the reference's vehicle."""
    N = 20
    routes = ['13', '32']
    agents, refs = _scene(routes, (12.0, 15.0), (3.0, 2.5))
    pred = igt.ConstantAccelerationModel(N=N, dt=0.1)
    inputs = [igt.VehicleAction({'a': 0.1, 'df': 0.0}) for _ in routes]
    preds = pred.predict(agents, inputs, routes, refs)
    for p in preds[1]:      # route '32' runs from heading pi down to pi / 2: the same poses with the sign a wrap-around gives
        p.heading = -p.heading
    with pytest.raises(NotImplementedError):
        igt.MPC_Planner(N=N, dt=0.1, agents=agents, routes=routes, ref=refs, road_dim=(11.4, 50), ds_right=8.6, index=0,
                        num_rk4_steps=4, ca_type='ellipse')
    with pytest.raises(ValueError, match='polish'):
        igt.MPC_Planner(N=N, dt=0.1, agents=agents, routes=routes, ref=refs, road_dim=(11.4, 50), ds_right=8.6, index=0,
                        num_rk4_steps=4, ca_type='obca', polish_iters=1)
    solved = 0
    for i in range(2):
        pl = igt.MPC_Planner(N=N, dt=0.1, ca_radius=2.8, agents=agents, routes=routes, ref=refs, goals=None, road_dim=(11.4, 50),
                             ds_right=8.6, index=i, num_rk4_steps=4, dtype='f64', cand_mode='lattice', ca_type='obca')
        assert pl.d_min == 0.0 and pl.ca_type == 'obca' and (pl.l, pl.width) == (4.47, 2.0)
        pl.update_initial_condition(agents[i], inputs[i])
        pl.update_predictions(preds, raw_preds=preds)
        j = 1 - i
        head = np.array([p.heading for p in preds[j]])
        want = np.array([[[[p.x for p in preds[j]], [p.y for p in preds[j]], np.abs(head) if routes[j] in ('32', '41') else head]]])
        assert pl._obs.shape == (1, 1, 3, N + 1) and np.array_equal(pl._obs, want)
        x, u, ok = pl.solve()
        st = agents[i]['state']
        flags = np.array([1 if routes[i] in ('32', '41') else 0], np.uint32)
        ref = pl._solver.solve_box(np.array([st.state7()]), np.array([[0.1, 0.0]]), np.array([pl.K.kparams]), flags, want)
        assert ok == (ref['status'][0] == 0)
        if ok:
            solved += 1
            assert _same_bytes(x, ref['x'][0]) and _same_bytes(u, ref['u'][0])
            assert (R.margins(x[None, None], want)[0] <= 1e-6 + 1e-9).all()
    assert solved >= 1
    assert len(planner_handles) == 1                                  # both planners share one handle


# ----------------------------------------------------------------------------- 8. closed loop
def test_closed_loop_obca_plans_pass_the_restated_verdict(igt):
    from igtmpc.evaluate import run_closed_loop
    for kw in (dict(device_resident=True), dict(device_resident=True, graph=True)):
        with pytest.raises(ValueError, match='obca'):
            run_closed_loop(ca_type='obca', num_samples=1, N=20, T_sim=0.2, **kw)
    with pytest.raises(ValueError, match='ca_type'):
        run_closed_loop(ca_type='ellipse', num_samples=1, N=20, T_sim=0.2)
    # From rest (the default, fourwayint.yaml:11) the vehicles start up to 10.7 m down a 19.3 m approach and gain about 2.4 m/s
    # in 2 s: run and horizon together end at the mouth of the crossing, and no forecast comes within the 4.9 m gate of any plan
    # (measured: 0 pairs), so that run alone would pass the verdict without asking it.  The same run from 3 m/s covers at least
    # 12 m in run and horizon and meets the other vehicle in the crossing: there the gate must be entered.
    n_in = {}
    for v0 in (0.0, 3.0):
        r = run_closed_loop(ca_type='obca', num_samples=4, N=20, T_sim=2.0, v0=v0, log_plans=True)
        assert r['x_data'].shape == (4, 14, 21) and len(r['plans']) == 20
        n_ok = n_in[v0] = 0
        for step in r['plans']:
            ok = step['ok'].reshape(-1)
            assert step['obs'].shape == (8, 1, 3, 21)
            g, inside, _ = R.margins(step['x'].reshape(8, 1, 7, 21)[ok], step['obs'][ok])
            assert (g <= 1e-6 + 1e-9).all()
            n_ok += int(ok.sum()); n_in[v0] += int(inside.sum())
        print('closed loop obca from', v0, 'm/s: solved problems', n_ok, 'of', 8 * 20, 'pairs inside a gate', n_in[v0])
        assert n_ok >= 8 * 20 // 2
    assert n_in[3.0] > 0, 'no forecast came inside a gate: the verdict above was never asked'
    c = run_closed_loop(ca_type='circle', num_samples=4, N=20, T_sim=2.0)      # the default is untouched
    d = run_closed_loop(num_samples=4, N=20, T_sim=2.0)
    assert _same_bytes(c['x_data'], d['x_data']) and 'plans' not in c
