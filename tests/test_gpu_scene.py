"""Scenes of more than two vehicles on the GPU: the scene-major forecast entry (igt_forecast_scene_*) against the gathered
entry bit for bit and against the oracle, the closed loop for 3 and 4 vehicles against the restated loop
(tests/scene_loop_restated.py), and the two-vehicle loop through the new code path against what the parent commit computed."""
import os

import numpy as np
import pytest

import np_oracle as O
from helpers import rel_err

pytestmark = pytest.mark.gpu


def _scene_inputs(E, M, N, seed, turning=True):
    """Random scenes: states on the routes' centre lines (so that headings are the lanes'), plans with the last speed spread
    round 5 m/s (both sides of the v > 5 retry, utils.py:348), has_plan mixed inside every scene."""
    from igtmpc import routes as R
    rng = np.random.default_rng(seed)
    names = R.ROUTES if turning else R.STRAIGHT
    rid = np.array([[R.ROUTE_ID[names[k]] for k in rng.integers(0, len(names), M)] for _ in range(E)], dtype=np.int32)
    s = rng.uniform(0.0, 45.0, (E, M))
    xy = np.stack([R.frenet2global(rid[:, m], s[:, m]) for m in range(M)], axis=1).reshape(E, M, 2)
    x = np.zeros((E, M, 7))
    x[..., 0:2] = xy + rng.normal(0, 0.1, (E, M, 2))
    x[..., 2] = s
    x[..., 5] = rng.uniform(-0.5, 6.0, (E, M))
    x[..., 6] = np.stack([R.psi_ref(rid[:, m], s[:, m]) for m in range(M)], axis=1) + rng.normal(0, 0.2, (E, M))
    a = rng.uniform(-4.0, 3.0, (E, M))
    plan_x = rng.normal(0, 10.0, (E, M, 7, N + 1))
    plan_x[..., 2, :] = s[..., None] + np.linspace(0, 8, N + 1)
    plan_x[..., 5, :] = rng.uniform(4.0, 5.5, (E, M, 1))
    plan_x[..., 0, :] += x[..., 0, None]
    plan_x[..., 1, :] += x[..., 1, None]
    plan_u = rng.uniform(-1.0, 3.0, (E, M, 2, N))
    has_plan = rng.integers(0, 2, (E, M)).astype(np.int32)
    if M > 1 and E > 0:
        has_plan[:, 0], has_plan[:, 1] = 1, 0            # every scene holds both kinds
    return x, a, rid, plan_x, plan_u, has_plan


def _gather(x, a, rid, plan_x, plan_u, has_plan):
    """The inputs of igt_forecast_batch_* for the E M problems: ego i, opponents j != i in ascending j."""
    E, M = a.shape
    opp_idx = np.array([[j for j in range(M) if j != i] for i in range(M)])          # [M, M-1]
    g = lambda v: v[:, opp_idx].reshape((E * M, M - 1) + v.shape[2:])
    ego = x[:, :, [0, 1, 6]].reshape(E * M, 3)
    return ego, g(x[:, :, [0, 1, 2, 5]]), g(a), g(rid), g(plan_x), g(plan_u), g(has_plan)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('M', [2, 3, 4, 5])
def test_forecast_scene_equals_gathered_forecast_bitwise(dtype, M):
    """igt_forecast_scene_* == igt_forecast_batch_* on the gathered inputs, torch.equal / np.array_equal: host and device
    buffers, with and without shared plans, has_plan mixed inside a scene, turning and straight routes, E from 1 to a few
    thousand (sizes that are no multiple of 64 or 256), on a caller's stream."""
    import torch
    import igtmpc
    npdt = np.float32 if dtype == 'f32' else np.float64
    N = 20
    c = lambda v: np.ascontiguousarray(v.astype(npdt))
    sq = (lambda v: v[:, 0]) if M == 2 else (lambda v: v)       # the two-vehicle entry has no n_obs axis on its inputs
    with igtmpc.BatchSolver(N=N, n_obs=M - 1, dtype=dtype) as s:
        for E, turning in ((1, True), (3, False), (65, True), (1000, True), (4097, True)):
            x, a, rid, px, pu, hp = _scene_inputs(E, M, N, seed=100 * M + E, turning=turning)
            x, a, px, pu = c(x), c(a), c(px), c(pu)
            ego, opp, oa, orid, opx, opu, ohp = _gather(x, a, rid, px, pu, hp)
            for plans in (True, False):
                ref_o, ref_t = s.forecast(ego, sq(opp), sq(oa), sq(orid), *((sq(opx), sq(opu), sq(ohp)) if plans else ()))
                got_o, got_t = s.forecast_scene(x, a, rid, *((px, pu, hp) if plans else ()))
                assert got_o.shape == (E * M, M - 1, 2, N + 1) and got_t.shape == (E * M, M - 1, 2)
                assert np.array_equal(got_o, ref_o) and np.array_equal(got_t.reshape(ref_t.shape), ref_t), (E, plans)
                assert (got_o == -20).any() and (got_o != -20).any() or E < 3          # both filter outcomes
            # device buffers on a caller's stream
            side = torch.cuda.Stream()
            dev = lambda v: torch.as_tensor(np.ascontiguousarray(v), device='cuda')
            with torch.cuda.stream(side):
                d = [dev(v) for v in (x, a, rid, px, pu, hp)]
                dg = [dev(sq(v)) if k else dev(v) for k, v in enumerate((ego, opp, oa, orid, opx, opu, ohp))]
                got_o, got_t = s.forecast_scene(*d, stream=side)
                ref_o, ref_t = s.forecast(*dg, stream=side)
            side.synchronize()
            assert torch.equal(got_o, ref_o) and torch.equal(got_t.reshape(ref_t.shape), ref_t), E
        assert s.forecast_scene(x[:0], a[:0], rid[:0])[0].shape == (0, M - 1, 2, N + 1)      # E = 0: nothing to do


@pytest.mark.parametrize('dtype,tol', [('f64', 1e-9), ('f32', 2e-5)])
def test_forecast_scene_matches_oracle(dtype, tol):
    """Per (ego, opponent) against np_oracle.forecast_for_ego, at the tolerances the two-vehicle entry's test uses
    (test_forecast_matches_oracle: 1e-9 f64, 2e-5 f32 relative with |ref| floored at 1)."""
    import igtmpc
    from igtmpc import routes as R
    import scene_loop_restated as S
    npdt = np.float32 if dtype == 'f32' else np.float64
    N, dt, M, E = 20, 0.1, 4, 40
    C = S.route_constants()
    x, a, rid, px, pu, hp = _scene_inputs(E, M, N, seed=7)
    cast = lambda v: np.ascontiguousarray(v.astype(npdt))
    x, a, px, pu = cast(x), cast(a), cast(px), cast(pu)
    with igtmpc.BatchSolver(N=N, dt=dt, n_obs=M - 1, dtype=dtype) as s:
        obs, tv = s.forecast_scene(x, a, rid, px, pu, hp)
    f = lambda v: np.asarray(v, dtype=np.float64)
    n_filtered = 0
    for e in range(E):
        for i in range(M):
            for o, j in enumerate(k for k in range(M) if k != i):
                r = R.ROUTES[rid[e, j]]
                ref, (sl, vl) = O.forecast_for_ego(r, C[r], f(x[e, i, :2]), float(x[e, i, 6]), f(x[e, j]), float(a[e, j]), N, dt,
                                                   f(px[e, j]) if hp[e, j] else None, f(pu[e, j]) if hp[e, j] else None)
                dot = (ref[0, 0] + 20) == 0
                n_filtered += bool(dot)
                assert rel_err(obs[e * M + i, o], ref).max() < tol, (e, i, j)
                assert rel_err(tv[e * M + i, o], [sl, vl]).max() < tol, (e, i, j)
    assert 0 < n_filtered < E * M * (M - 1)


def test_forecast_scene_refuses_what_it_cannot_do():
    import igtmpc
    from igtmpc import _lib as L
    lib = L.load()
    x = np.zeros((1, 2, 7))
    with igtmpc.BatchSolver(N=20, n_obs=1, dtype='f64') as s:
        z = np.zeros(4)
        assert lib.igt_forecast_scene_f64(s._h, 1, x.ctypes.data, z.ctypes.data, z.ctypes.data, None, None, None, z.ctypes.data,
                                          z.ctypes.data, L.IGT_MEM_HOST, None) == -1        # IGT_E_INVALID: no route table yet
        s.set_routes()
        assert lib.igt_forecast_scene_f64(s._h, -1, x.ctypes.data, z.ctypes.data, z.ctypes.data, None, None, None, z.ctypes.data,
                                          z.ctypes.data, L.IGT_MEM_HOST, None) == -1        # E < 0
    with igtmpc.BatchSolver(N=20, n_obs=0, dtype='f64') as s:
        s.set_routes()
        with pytest.raises(igtmpc.IgtError, match='n_obs'):
            s.forecast_scene(np.zeros((1, 1, 7)), np.zeros((1, 1)), np.zeros((1, 1), np.int32))


@pytest.mark.parametrize('M', [3, 4])
@pytest.mark.parametrize('cand_mode,N,steps', [('track', 20, 30), ('ramp_hold', 20, 30), ('lattice', 20, 30), ('track', 40, 20)])
def test_scene_closed_loop_matches_restated_loop(cand_mode, N, steps, M):
    """run_closed_loop(num_agents = 3, 4), f64, against tests/scene_loop_restated.py at 1e-9 on states and applied inputs,
    identical infeasible counts and deadlock flags; host loop, device-resident eager and device-resident graph bit-identical
    to each other.  Tracking as the drivers run it (no warm start), ramp-hold with its warm start, lattice.  The scenes
    (scene_loop_restated.scenes) contain a fallback step, a stopped vehicle and shared plans -- asserted.
    No episode is left out of the comparison (share left out: 0 %; the cap the issue allows is 10 %)."""
    import scene_loop_restated as S
    from igtmpc.cinf import cinf_halfplanes
    from igtmpc.evaluate import run_closed_loop
    x, routes = S.scenes(M)
    E = len(routes)
    kw = dict(N=N, T_sim=steps * 0.1, dtype='f64', cand_mode=cand_mode, init=(x, routes), num_agents=M)
    got = run_closed_loop(**kw)
    assert got['x_data'].shape == (E, 7 * M, steps + 1) and got['u_data'].shape == (E, 2 * M, steps)
    for g in (False, True):
        dev = run_closed_loop(device_resident=True, graph=g, **kw)
        for k in ('x_data', 'u_data', 'infeasible_ratio', 'deadlock'):
            assert np.array_equal(dev[k], got[k]), (k, g)
    P = O.Params(N=N)
    ev = dict(fallback=0, stop=0, share=0, share_retry=0, warm=0)
    for e in range(E):
        ref = S.run_scene(x[e], routes[e], P, cinf_halfplanes(), M_sim=steps, cand_mode=cand_mode,
                          warm_start=cand_mode == 'ramp_hold', track_env=got['track_env'] if cand_mode == 'track' else 1.0)
        for k in ev:
            ev[k] += ref['events'][k]
        ex, eu = rel_err(got['x_data'][e], ref['x_data']).max(), rel_err(got['u_data'][e], ref['u_data']).max()
        print(f'M={M} {cand_mode} N={N} episode {e}: max rel err x {ex:.2e} u {eu:.2e} infeasible {ref["infeasible"]}')
        assert ex < 1e-9 and eu < 1e-9, (e, routes[e])
        assert np.array_equal(np.rint(got['infeasible_ratio'][e] * steps), ref['infeasible']), (e, routes[e])
        assert bool(got['deadlock'][e]) == ref['deadlock']
    assert ev['fallback'] > 0 and ev['stop'] > 0 and ev['share'] > 0, ev
    assert (ev['warm'] > 0) == (cand_mode == 'ramp_hold')


def test_mpc_planner_takes_a_three_vehicle_scene():
    """MPC_Planner sizes itself by the scene (mpc.py:82-85): with three agents update_predictions fills two obstacle rows in
    ascending agent order and solve() equals the oracle's solve against both forecasts."""
    import igtmpc
    from igtmpc import routes as R
    N = 20
    routes, agents, refs = ['13', '23', '31'], [], []
    for r, s0, v0 in zip(routes, (12.0, 15.0, 10.0), (3.0, 2.5, 2.0)):
        rid = R.ROUTE_ID[r]
        xy = R.frenet2global(rid, s0)
        agents.append({'type': 'CAV', 'state': igtmpc.VehicleReference(
            {'x': xy[0], 'y': xy[1], 's': s0, 'ey': 0.0, 'epsi': 0.0, 'v': v0, 'heading': float(R.psi_ref(rid, s0)),
             'K': igtmpc.Curvature.from_route(r)})})
        kk = np.zeros(151)
        if R.CONSTANTS[r].get('Kv'):
            kk[40:80] = R.CONSTANTS[r]['Kv']
        refs.append({'K': kk})
    inputs = [igtmpc.VehicleAction({'a': 0.1, 'df': 0.0}) for _ in routes]
    preds = igtmpc.ConstantAccelerationModel(N=N, dt=0.1).predict(agents, inputs, routes, refs)
    for i in range(3):
        pl = igtmpc.MPC_Planner(N=N, dt=0.1, ca_radius=2.8, agents=agents, routes=routes, ref=refs, goals=None,
                                road_dim=(11.4, 50), ds_right=8.6, index=i, num_rk4_steps=4)
        assert pl.M == 3 and pl._solver.n_obs == 2
        pl.update_initial_condition(agents[i], inputs[i])
        pl.update_predictions(preds, raw_preds=preds)
        assert pl.pred_ind == [j for j in range(3) if j != i]
        with pytest.raises(AssertionError):
            pl.update_predictions(preds[:2])
        x1, u1, ok = pl.solve()
        obs = np.array([[[[p.x for p in preds[j]], [p.y for p in preds[j]]] for j in pl.pred_ind]])
        ref = O.solve_batch_refined(np.array([agents[i]['state'].state7()]), np.array([[0.1, 0.0]]), np.array([pl.K.kparams]),
                                    np.array([0], np.uint32), obs, *pl.C_inf, O.Params(N=N), cand='track',
                                    track=dict(env=pl.track_env))[-1]
        assert ok == (ref['status'][0] == 0)
        assert ok and rel_err(x1, ref['x'][0]).max() < 1e-9 and rel_err(u1, ref['u'][0]).max() < 1e-9


PARENT = 'closed_loop_m2_parent_d40c6ce.npz'


@pytest.mark.parametrize('cand_mode', ['track', 'ramp_hold'])
def test_two_vehicle_loop_equals_the_parent_commit(cand_mode, golden_dir):
    """num_agents = 2 through the scene-major forecast: host loop, device-resident eager and graph give, bit for bit, what
    the parent commit (d40c6ce, its own library and driver, gathered forecast) gave on an MI355X for 4 episodes of
    scenario 1 started at 2 m/s, N = 20, 80 steps -- tests/golden/closed_loop_m2_parent_d40c6ce.npz."""
    from igtmpc.evaluate import run_closed_loop
    with np.load(os.path.join(golden_dir, PARENT)) as z:
        want = {k[len(cand_mode) + 1:]: z[k] for k in z.files if k.startswith(cand_mode + '_')}
    kw = dict(sc=1, num_samples=4, N=20, T_sim=8.0, v0=2.0, dtype='f64', cand_mode=cand_mode)
    for extra in (dict(), dict(num_agents=2), dict(device_resident=True), dict(device_resident=True, graph=True)):
        got = run_closed_loop(**kw, **extra)
        for k in ('x_data', 'u_data', 'infeasible_ratio', 'deadlock'):
            assert np.array_equal(got[k], want[k]), (k, extra)
    assert (want['x_data'][:, 2::7, -1] - want['x_data'][:, 2::7, 0]).min() > 5              # every vehicle drove
