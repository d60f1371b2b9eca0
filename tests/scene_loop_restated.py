"""TEST INFRASTRUCTURE ONLY -- the reference's closed-loop time loop (evaluate.py:451-569, --eval_mode mpc) restated for a scene
of ANY number of agents M, one episode at a time, agent by agent, in float64.

oracle/closed_loop.py is the project's yardstick for two vehicles and asserts M == 2; this file is the yardstick beside it for
more.  It is built only from what oracle/np_oracle.py exports (forecast_for_ego, solve_batch / solve_batch_refined,
frenet_rk4_step, shift_controls) and is pinned to the two-vehicle loop: at M = 2 it reproduces oracle/closed_loop.py exactly
(tests/test_scene_host.py, np.array_equal).

    for t in range(M_sim):                                                        evaluate.py:451
        preds      = predictor.predict(cur states, prev inputs)                   :455
        preds4CAV  = share_motion_forecasts(preds, cav_sols of step t-1)          :458-460, utils.py:339-352
        for i in range(M):                                                        :469   (Jacobi: all agents see preds4CAV)
            update_predictions(filter_preds(preds4CAV, i))                        :474-477, utils.py:365-388 -- the agents
                                                                                  j != i in ascending j, each filtered for ego i
            warm start = shifted solution of step t-1 if agent i solved then      :478-481, utils.py:354-363
            solve; ok: next state = x_sol[:,1], applied input = u_sol[:,0]        :482-510
            else: brake a = a_min if v > 0 else 0, keep df, one model step;       :511-545
                  v < 0: applied a = 0, state frozen with v = 0                   :523-526
    deadlock = at least two agents end with s <= 30                               :566-569
"""
import json
import os

import numpy as np

import np_oracle as O

A_MIN_POLICY = -4.0                     # mpc.yaml:8 a_min, used by the brake fallback (evaluate.py:514)
ABS_HEADING_ROUTES = ('32', '41')       # mpc.py:231, 282

_CONST = None


def route_constants():
    global _CONST
    if _CONST is None:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'route_constants.json')) as f:
            _CONST = json.load(f)
    return _CONST


def kparams_of(route):
    """Curvature function of the route as (b0, b1, Kv)  (mpc.py:183-200; straight: K == 0)."""
    k = route_constants()[route]
    return np.array([np.inf, np.inf, 0.0]) if k['straight'] else np.array([k['b0'], k['b1'], k['Kv']])


def run_scene(x_init, routes, P, cinf, M_sim=30, cand_mode='lattice', C=256, refine_iters=0, warm_start=True,
              track_env=1.0, track_vcap=1.0, a_min_policy=A_MIN_POLICY):
    """x_init[M,7] (planner state order), routes = one route per agent.
    -> dict(x_data[7M, M_sim+1], u_data[2M, M_sim], infeasible[M], deadlock, events)."""
    M, N, dt = len(routes), P.N, P.dt
    consts = route_constants()
    A, b = cinf
    kp = [kparams_of(r) for r in routes]
    cur = [np.array(x_init[i], dtype=np.float64) for i in range(M)]
    prev_in = [np.array((0.1, 0.0)) for _ in range(M)]                           # evaluate.py:419
    x_data = np.zeros((7 * M, M_sim + 1))
    u_data = np.zeros((2 * M, M_sim))
    for i in range(M):
        x_data[7 * i:7 * i + 7, 0] = cur[i]
    prev_sol = [None] * M                                                       # evaluate.py:444-445, by agent index
    infeasible = np.zeros(M, dtype=np.int64)
    events = dict(fallback=0, stop=0, share=0, share_retry=0, warm=0)
    for t in range(M_sim):
        nxt_states, cur_in, sols = [None] * M, [None] * M, [None] * M
        for i in range(M):
            obs = []
            for j in range(M):                                                  # filter_preds(preds4CAV, i): ascending j != i
                if j == i:
                    continue
                plan = prev_sol[j] if t > 0 else None                           # evaluate.py:459
                if plan is not None:
                    events['share'] += 1
                    if np.clip(plan[0][5, N] + plan[1][0, N - 1] * dt, -2.0, 20.0) > 5:      # utils.py:348
                        events['share_retry'] += 1
                o, _ = O.forecast_for_ego(routes[j], consts[routes[j]], cur[i][:2], cur[i][6], cur[j], prev_in[j][0], N, dt,
                                          None if plan is None else plan[0], None if plan is None else plan[1])
                obs.append(o)
            flags = np.array([O.FLAG_ABS_HEADING if routes[i] in ABS_HEADING_ROUTES else 0], dtype=np.uint32)
            u_ws = None
            if warm_start and cand_mode in ('ramp_hold', 'track') and prev_sol[i] is not None and t > 0:      # :478
                u_ws = O.shift_controls(prev_sol[i][1])[None]                   # control part of utils.py:354-363
                flags = flags | np.uint32(O.FLAG_WARM)
                events['warm'] += 1
            args = (cur[i][None], prev_in[i][None], kp[i][None], flags, np.stack(obs)[None], A, b, P)
            if cand_mode in ('ramp_hold', 'track'):
                r = O.solve_batch_refined(*args, C=C, refine_iters=refine_iters, u_ws=u_ws, cand=cand_mode,
                                          track=dict(env=track_env, vcap=track_vcap))[-1]
            else:
                r = O.solve_batch(*args, C=C)
            if r['status'][0] == 0:                                             # evaluate.py:484-510
                xs, us = r['x'][0], r['u'][0]
                sols[i] = (xs, us)
                nxt_states[i] = xs[:, 1].copy()
                cur_in[i] = us[:, 0].copy()
            else:                                                               # evaluate.py:511-545
                infeasible[i] += 1
                events['fallback'] += 1
                a_fb = a_min_policy if cur[i][5] > 0 else 0.0
                df_fb = prev_in[i][1]
                ns = O.frenet_rk4_step(cur[i], a_fb, df_fb, kp[i], P)
                if cur[i][5] < 0:                                               # evaluate.py:523-526
                    events['stop'] += 1
                    cur_in[i] = np.array([0.0, df_fb])
                    ns = cur[i].copy()
                    ns[5] = 0.0
                else:
                    cur_in[i] = np.array([a_fb, df_fb])
                nxt_states[i] = ns
            x_data[7 * i:7 * i + 7, t + 1] = nxt_states[i]
            u_data[2 * i:2 * i + 2, t] = cur_in[i]
        cur, prev_in, prev_sol = nxt_states, cur_in, sols                       # evaluate.py:556-561
    deadlock = bool(sum(x_data[7 * i + 2, -1] <= 30 for i in range(M)) >= 2)   # evaluate.py:566-569
    return dict(x_data=x_data, u_data=u_data, infeasible=infeasible, deadlock=deadlock, events=events)



def scenes(M):
    """Initial conditions shared by the CPU and GPU tests of M-vehicle scenes: -> (x[2,M,7], route tuples).
    Episode 0: scenario 1's first route tuple extended to M vehicles, sampled as the driver samples, every vehicle rolling at
    2 m/s (v0 = 0 crawls for 3 s) -- plans are shared from step 1 on.  Episode 1: the same draw of another tuple with agent 0
    outside the lane bound (|ey| = 0.25 > 0.2: infeasible from the first step, mpc.py:296-299) and slow, so the brake fallback
    takes it below v = 0 and the stop heuristic fires (evaluate.py:523-526)."""
    from igtmpc import routes as R
    from igtmpc.evaluate import initial_states
    routes = [R.scene_routes(1, 0, M), R.scene_routes(3, 1, M)]
    x, _ = initial_states(np.random.default_rng(2026), routes)
    x[:, :, 5] = 2.0
    x[1, 0, 3], x[1, 0, 5] = 0.25, 0.3
    return x, routes
