"""Scenes of more than two vehicles, on the CPU: the restated loop for any M (tests/scene_loop_restated.py) is pinned to the
two-vehicle oracle loop, behaves as a loop over a SCENE should for M = 3 and 4 (permutation, an irrelevant far vehicle), and
the driver's arguments are checked before any GPU call."""
import numpy as np
import pytest

import np_oracle as O
import scene_loop_restated as S


def _two_vehicle_episodes():
    """The episodes of test_closed_loop_matches_oracle_loop's kind: sampled and rolling, and one with agent 0 outside the lane
    bound and slow (brake fallback from step 0, then the v < 0 stop); plans are shared from step 1 on."""
    from igtmpc import routes as R
    from igtmpc.evaluate import initial_states
    pairs = [R.SCENARIO_ROUTES[0][0], ('13', '23')]
    x, _ = initial_states(np.random.default_rng(2026), pairs)
    x[0, :, 5] = 2.0
    x[1, 0, 3], x[1, 0, 5] = 0.25, 0.3
    x[1, 1, 5] = 2.0
    return x, pairs


@pytest.mark.parametrize('cand_mode', ['lattice', 'ramp_hold', 'track'])
def test_restated_loop_equals_the_oracle_loop_for_two_vehicles(cand_mode):
    """M = 2, N = 20: exactly oracle/closed_loop.py (np.array_equal) -- lattice, ramp-hold + warm start, tracking (+ warm start,
    as the oracle loop has it) -- over episodes that go through the fallback, the stop heuristic and plan sharing."""
    import closed_loop as CL
    from igtmpc.cinf import cinf_halfplanes
    x, pairs = _two_vehicle_episodes()
    P, cinf = O.Params(N=20), cinf_halfplanes()
    ev = dict(fallback=0, stop=0, share=0, warm=0)
    for e in range(len(pairs)):
        want = CL.run_episode(x[e], pairs[e], P, cinf, M_sim=25, cand_mode=cand_mode, track_env=0.5)
        got = S.run_scene(x[e], pairs[e], P, cinf, M_sim=25, cand_mode=cand_mode, track_env=0.5)
        for k in ('x_data', 'u_data', 'infeasible'):
            assert np.array_equal(got[k], want[k]), (k, e)
        assert got['deadlock'] == want['deadlock'] and got['events'] == want['events']
        for k in ev:
            ev[k] += got['events'][k]
    assert ev['fallback'] > 0 and ev['stop'] > 0 and ev['share'] > 0 and (ev['warm'] > 0) == (cand_mode != 'lattice'), ev


@pytest.mark.parametrize('M', [3, 4])
def test_permuting_the_agents_permutes_the_rows(M):
    """A scene has no first vehicle: the restated loop on the agents in another order gives the same trajectories, row
    blocks permuted (Jacobi update; the order of the obstacles inside one solve only reorders a max over them)."""
    from igtmpc.cinf import cinf_halfplanes
    x, routes = S.scenes(M)
    P, cinf = O.Params(N=20), cinf_halfplanes()
    perm = [2, 0, 1] if M == 3 else [3, 1, 0, 2]
    for e in range(2):
        a = S.run_scene(x[e], routes[e], P, cinf, M_sim=12, cand_mode='track', warm_start=False, track_env=0.5)
        b = S.run_scene(x[e][perm], [routes[e][p] for p in perm], P, cinf, M_sim=12, cand_mode='track', warm_start=False,
                        track_env=0.5)
        for q, p in enumerate(perm):
            assert np.array_equal(b['x_data'][7 * q:7 * q + 7], a['x_data'][7 * p:7 * p + 7]), (e, q, p)
            assert np.array_equal(b['u_data'][2 * q:2 * q + 2], a['u_data'][2 * p:2 * p + 2]), (e, q, p)
        assert np.array_equal(b['infeasible'], a['infeasible'][perm]) and a['deadlock'] == b['deadlock']


@pytest.mark.parametrize('M', [3, 4])
def test_a_vehicle_far_away_changes_nothing(M):
    """One more vehicle, hundreds of metres down its lane behind everybody's back or merely out of reach (distance far above
    d_min over the whole run): the other vehicles' trajectories equal those of the scene without it."""
    from igtmpc import routes as R
    from igtmpc.cinf import cinf_halfplanes
    x, routes = S.scenes(M - 1)
    P, cinf = O.Params(N=20), cinf_halfplanes()
    for e in range(2):
        lane = next(l for l in '1234' if all(r[0] != l for r in routes[e]))
        r_far = next(r for r in R.STRAIGHT if r[0] == lane)
        s_far = -400.0                                        # far up its approach lane: 400 m from the intersection
        xy = R.frenet2global(R.ROUTE_ID[r_far], s_far)
        far = np.array([xy[0], xy[1], s_far, 0.0, 0.0, 1.0, float(R.psi_ref(R.ROUTE_ID[r_far], s_far))])
        a = S.run_scene(x[e], routes[e], P, cinf, M_sim=12, cand_mode='track', warm_start=False, track_env=0.5)
        b = S.run_scene(np.vstack([x[e], far]), list(routes[e]) + [r_far], P, cinf, M_sim=12, cand_mode='track',
                        warm_start=False, track_env=0.5)
        n = M - 1
        assert np.array_equal(b['x_data'][:7 * n], a['x_data']) and np.array_equal(b['u_data'][:2 * n], a['u_data']), e
        assert np.array_equal(b['infeasible'][:n], a['infeasible'])


def test_initial_states_draw_is_the_parents_for_two_and_does_not_depend_on_m():
    """initial_states at M = 2 for a fixed seed: the numbers the parent commit (d40c6ce) gave; with more agents the same
    offsets (one rng.random((E, 4)) draw, evaluate.py:91-94), so agents 0 and 1 do not move."""
    from igtmpc import routes as R
    from igtmpc.evaluate import initial_states
    pairs = [R.SCENARIO_ROUTES[0][0], R.SCENARIO_ROUTES[5][2], ('12', '34')]
    x, rid = initial_states(np.random.default_rng(7), pairs, v0=0.5)
    want = [6.688521492669937, 2.8, 6.688521492669937, 0.0, 0.0, 0.5, 0.0, 22.1, 21.099812329625543, 9.600187670374456, 0.0, 0.0,
            0.5, -1.5707963267948966, 22.1, 21.35297813426, 9.347021865740002, 0.0, 0.0, 0.5, -1.5707963267948966,
            49.94366124114835, 8.600000000000001, 0.056338758851649545, 0.0, 0.0, 0.5, -3.141592653589793, 8.528642887646894, 2.8,
            8.528642887646894, 0.0, 0.0, 0.5, 0.0, 46.757553033033346, 8.600000000000001, 3.2424469669666545, 0.0, 0.0, 0.5,
            -3.141592653589793]
    assert x.shape == (3, 2, 7) and np.array_equal(x.reshape(-1), np.array(want))
    assert rid.tolist() == [[1, 4], [4, 6], [0, 8]]
    for M in (3, 4):
        tuples = [R.scene_routes(sc, k, M) for sc, k in ((1, 0), (6, 2), (7, 0))]
        assert [t[:2] for t in tuples] == pairs and all(len({r[0] for r in t}) == M for t in tuples)
        xm, ridm = initial_states(np.random.default_rng(7), tuples, v0=0.5)
        assert xm.shape == (3, M, 7) and np.array_equal(xm[:, :2], x) and np.array_equal(ridm[:, :2], rid)
    assert R.scene_routes(1, 0, 4) == ('13', '23', '31', '42') and R.scene_routes(1, 0, 2) == R.SCENARIO_ROUTES[0][0]
    with pytest.raises(ValueError):
        initial_states(np.random.default_rng(7), [('13', '23'), ('13', '23', '31')])


def test_run_closed_loop_refuses_bad_scenes_before_any_gpu_call(monkeypatch):
    from igtmpc import evaluate as EV

    def no_gpu(*a, **k):
        raise AssertionError('a solver was created')
    monkeypatch.setattr(EV, 'BatchSolver', no_gpu)
    x3 = np.zeros((1, 3, 7))
    for kw in (dict(num_agents=1), dict(num_agents=5), dict(num_agents=0),
               dict(num_agents=3, eval_mode='gt_mpc'),
               dict(num_agents=3, eval_mode='gt_mpc', value_net=dict(layers=[])),
               dict(num_agents=2, init=(x3, [('13', '23', '31')])),                  # three routes, two agents asked for
               dict(num_agents=3, init=(x3[:, :2], [('13', '23', '31')])),           # states of two
               dict(num_agents=3, init=(x3, [('13', '23')])),                        # routes of two
               dict(num_agents=3, init=(x3, [('13', '23', '12')])),                  # approach lane 1 twice
               dict(num_agents=2, init=(x3[:, :2], [('13', '12')]))):
        with pytest.raises(ValueError):
            EV.run_closed_loop(N=20, **kw)
    with pytest.raises(ValueError):
        EV.run_closed_loop(N=20, init=(x3, [('13', '23', '31')]))                    # the default is two agents

