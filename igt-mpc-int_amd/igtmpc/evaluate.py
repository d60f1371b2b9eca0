"""Closed-loop driver: the time loop of the reference's evaluate.py (mpc branch 451-564, gt_mpc
branch 193-330) for E episodes of M = 2..4 agents in lock-step, every (episode, agent) problem of a timestep solved
in ONE batched call on the GPU (the reference's agents of a timestep all read the same
predictions -- a Jacobi update, evaluate.py:469-558 -- so batching changes nothing).

Kept from the reference, with citations:
  * initial states: random offset along the approach lane, v0 = 0, s = offset      (evaluate.py:91-94, 404-418)
  * previous inputs start at (0.1, 0)                                               (evaluate.py:419)
  * gt_mpc: previous inputs start at (0, 0) (:171); the first forecast uses a = 0.09 (k+1) for agent k (:207-210);
    the warm start is passed for t > 1 only (:232; the mpc branch passes it from t = 1, :478)
  * per step: predict -> share motion forecasts (V2V) -> filter_preds -> solve      (evaluate.py:455-482)
  * solved: next state = x*[:,1], applied input = u*[:,0]                           (evaluate.py:491-510)
  * infeasible: brake a = a_min (if v > 0 else 0), keep df, one model step; v < 0 -> stop  (evaluate.py:511-545)
  * deadlock: at least two agents end with s <= 30                                  (evaluate.py:566-569)
Not kept: pickles / CSV / mp4 output, the unseeded route shuffle (routes are sorted pairs here).

    python -m igtmpc.evaluate --sc 1 --num_samples 8 --N 20
"""
import argparse
import json
import os
import time
from functools import partial
from types import SimpleNamespace

import numpy as np

from . import routes as R
from .cinf import cinf_halfplanes
from ._lib import IGT_FLAG_WARM
from .predictor import ConstantAccelerationModel
from .solver import BatchSolver, check_value_polish, check_value_polish_driver
from .value_nets import shipped_value_net

A_MIN_POLICY = -4.0        # mpc.yaml:8, used by the brake fallback (evaluate.py:514)


def initial_states(rng, route_pairs, v0=0.0):
    """evaluate.py:91-94 + 404-418: every episode draws one offset per approach lane (order 1,2,3,4);
    an agent starting at origin o sits `offset_o` metres down its lane with v = 0, ey = epsi = 0.
    route_pairs: one tuple of M = 2..4 routes per episode (the same M for all; the draw does not depend on M)."""
    E = len(route_pairs)
    max_start = (R.ROAD_LENGTH - R.ROAD_WIDTH) / 2 - (R.ROAD_WIDTH - R.CA_RADIUS)      # evaluate.py:48-49
    off = rng.random((E, 4)) * max_start
    M = len(route_pairs[0]) if E else 2
    if any(len(p) != M for p in route_pairs):
        raise ValueError('every episode needs the same number of routes')
    x = np.zeros((E, M, 7))
    rid = np.zeros((E, M), dtype=np.int64)
    for e, pair in enumerate(route_pairs):
        for m, r in enumerate(pair):
            rid[e, m] = R.ROUTE_ID[r]
            s0 = off[e, int(r[0]) - 1]
            xy = R.frenet2global(rid[e, m], s0)
            h0 = {'1': 0.0, '2': -np.pi / 2, '3': -np.pi, '4': np.pi / 2}[r[0]]     # evaluate.py:58-61
            x[e, m] = (xy[0], xy[1], s0, 0.0, 0.0, v0, h0)                          # fourwayint.yaml:11 v0
    return x, rid


def auto_track_env(N, dt):
    """Scale of the tracking family's acceleration envelope (igt_params.track_env) for a CLOSED loop with horizon N dt.
    1 is the derived value -- the stationary acceleration of the NLP's own cost -- and the best setting from a 4 s horizon
    on (mpc.yaml:6 ships N = 40, dt = 0.1); a plan that is optimal over a shorter horizon runs faster into conflicts it
    cannot see yet, so the scale shrinks with the horizon, not below 0.25.  Measured (tools/envelope_sweep.py, 512 episodes):
    N = 20: 0.5 -> 9.2 % infeasible steps / 23 % deadlock flag / 47.6 m against 14.9 % / 29 % / 46.4 m at 1.0;
    N = 40: 1.0 -> 3.3 % / 2.9 % / 60.1 m (0.5: 3.0 % / 2.5 % / 61.1 m) -- round 4, speed cap on, no warm start.
    The library's own default stays 1.0 (one solve knows no closed loop)."""
    return float(min(1.0, max(0.25, N * dt / 4.0)))


def run_closed_loop(sc=1, num_samples=1, N=40, dt=0.1, T_sim=15.0, seed=2026, C=256, n_rk4=4, device=0,
                    dtype='f64', rotation=None, cand_mode='track', refine_iters=0, verbose=False,
                    eval_mode='mpc', value_net=None, device_resident=False, warm_start=None, init=None,
                    terminal_set=True, feas_tol=None, limits=None, graph=False, a_min_policy=None, constant_speed=False,
                    v0=0.0, polish_iters=0, num_agents=2, polish_grad='fd', polish_step='gradient', value_polish_iters=0,
                    value_polish_driver='host', step='torch', ca_type='circle', log_plans=False, pose_forecast='host'):
    """eval_mode 'mpc' (evaluate.py:370-639) or 'gt_mpc' (123-369: terminal value network in the cost;
    value_net = dict(layers=[(W,b),...][, Wn, mu_f, sigma_t, mu_t]), default: the network the reference ships for
    scenario sc -- its normalisation statistics are not shipped, identity unless given).  device_resident=True keeps every per-step array in HBM (torch tensors;
    forecast, solve, fallback step and the state update never leave the GPU) -- for thousands of episodes.
    warm_start (ramp-hold and tracking candidates): an agent that solved the previous step centres its candidates on that
    solution shifted by one step (evaluate.py:478-481, utils.py:354-363 augment_prev_sol) instead of on u_prev held.  Default
    (None): on for ramp-hold, OFF for the tracking family -- with the speed cap of its targets the loop is better without on
    every count at both horizons (N = 40: 3.3 % infeasible steps / 2.9 % deadlock flag / 60.1 m against 5.0 % / 3.9 % /
    57.2 m; N = 20: 9.2 % / 23 % / 47.6 m against 9.7 % / 29 % / 46.2 m).  The reference's warm start
    is IPOPT's initial guess (mpc.py:386-389): it does not move the NLP's optimum, so nothing of its semantics is lost.
    init = (x[E,M,7], route_pairs[E]) overrides the sampled initial states; terminal_set=False drops the C_inf
    constraint (mpc.py:177-180) -- a test switch.  feas_tol: inequality tolerance of the verdicts (default: the
    library's 1e-6; IPOPT's constr_viol_tol is 1e-3, mpc.py:135); limits: further igt_params fields by name
    (e.g. dict(track_env=0.0); without it the tracking family's envelope scale follows the horizon: auto_track_env).
    graph=True (with device_resident): the time loop replays one captured step.
    step (with device_resident): what turns a solve into the next step's inputs -- 'torch' (default): about 40 tensor operations
    and the stepper handle's model step; 'fused': one kernel on the solver's own handle (BatchSolver.loop_advance, igtmpc.h
    igt_loop_advance_*), the same bytes.  'fused' without device_resident raises ValueError.
    a_min_policy: deceleration of the brake fallback (mpc.yaml:8 a_min through evaluate.py:514; default -4);
    constant_speed: the forecast holds the other agent's speed (mpc.yaml:13-14 prediction_type, evaluate.py:76-79);
    v0: initial speed (fourwayint.yaml:11) -- load_reference_configs reads all three from the reference's files.
    polish_iters (f64, eval_mode 'mpc'): projected-gradient steps on every solved problem's winner (igtmpc.h polish_iters);
    polish_grad: their gradient, 'fd' forward differences (default) or 'adjoint' analytic (igtmpc.h igt_set_polish_gradient);
    polish_step: 'gradient' (default) or 'newton', half of the trials along the Gauss-Newton direction (igt_set_polish_step).
    value_polish_iters (0..4; f64, eval_mode 'gt_mpc'; 'mpc' checks its range and does not read it): the solver's polish under
    the value-network cost (BatchSolver(value_polish_iters=)).  value_polish_driver 'host' (default): driven from numpy, so
    device_resident=True (and graph=True) refuse it with a ValueError; 'device': the library takes the steps inside the solve
    (igtmpc.h igt_set_value_polish), device_resident=True runs, graph=True is refused with a ValueError -- the library refuses such
    a solve under stream capture.  polish_iters keeps raising with gt_mpc.
    num_agents = M in 2..4 (evaluate.py:46; four approach lanes): every step solves E M problems with n_obs = M - 1 -- each
    agent against the forecast / shared plan of every other one (Jacobi, evaluate.py:469-558).  Scenario `sc`'s route tuples for
    M > 2: routes.scene_routes; init = (x[E,M,7], route tuples of length M).  eval_mode 'mpc' only beyond two (the value
    network's features are those of a two-vehicle scene, mpc.py:326-338).
    ca_type 'circle' (default; mpc.yaml:16) or 'obca' (mpc.py:42-43, 211-221): every vehicle a 4.47 x 2.0 m rectangle, d_min = 0,
    solved through BatchSolver.solve_box.  With pose_forecast='host' (the default) the host loop only: device_resident=True or
    graph=True with 'obca' raises ValueError.  The obstacles' x, y stay the device forecast's; their headings come from the host
    predictor (igtmpc.predictor predict_arrays), or from the plan an agent shares (utils.py:339-352), |heading| for obstacles on
    routes '32', '41' (mpc.py:250-253), gathered per ego in ascending opponent order.
    pose_forecast (ca_type 'obca'): where the obstacles' headings come from.  'host' (default): the paragraph above, the host loop
    only.  'device': the whole pose [E M, n_obs, 3, N+1] from BatchSolver.forecast_scene_pose (igtmpc.h igt_forecast_scene_pose_f64)
    in one call -- no host predictor, nothing concatenated -- and with it device_resident=True, graph=True and step='fused' run
    with rectangles.  'device' with ca_type 'circle' raises ValueError (nothing reads a pose there).
    log_plans=True: a diagnostic for tests and probes, not part of the loop's interface (host loop only; the device-resident loops
    ignore it) -- the result carries 'plans', one dict(ok[E,M], x[E,M,7,N+1], obs[E M,n_obs,2 or 3,N+1]) per step: what every
    problem was solved against and what it answered.  Copies every step's arrays: leave it off when measuring."""
    obca, pose_dev, gt, vp_iters, M, a_min_policy = _check_options(
        ca_type=ca_type, pose_forecast=pose_forecast, device_resident=device_resident, graph=graph, dtype=dtype,
        polish_iters=polish_iters, value_polish_iters=value_polish_iters, value_polish_driver=value_polish_driver, step=step,
        num_agents=num_agents, eval_mode=eval_mode, a_min_policy=a_min_policy, needs_value_net=value_net is None and init is not None)
    if gt and value_net is None:
        value_net = shipped_value_net(sc)                               # sc{n}_config.yaml:2 model_path
    rng = np.random.default_rng(seed)                                   # evaluate.py:35, 56
    M_sim = int(round(T_sim / dt))                                      # evaluate.py:83-84
    if init is not None:
        x, pairs = np.array(init[0], dtype=np.float64), [tuple(p) for p in init[1]]
        E = num_samples = len(pairs)
        if x.shape != (E, M, 7) or any(len(p) != M for p in pairs):
            raise ValueError(f'init must be (x[E,{M},7], E route tuples of length {M}) for num_agents = {M}; got x{x.shape} and '
                             f'tuples of length {sorted({len(p) for p in pairs})}')
        rid = np.array([[R.ROUTE_ID[r] for r in p] for p in pairs], dtype=np.int64)
    else:
        E = num_samples
        pairs = [R.scene_routes(sc, e if rotation is None else rotation, M) for e in range(E)]
    for p in pairs:
        if len({r[0] for r in p}) != len(p):                            # evaluate.py:96: lanes are drawn without replacement
            raise ValueError(f'routes {p}: two agents of a scene start from the same approach lane')
    if init is None:
        x, rid = initial_states(rng, pairs, v0=v0)                      # x[E,M,7]
    warm = (cand_mode == 'ramp_hold') if warm_start is None else (bool(warm_start) and cand_mode in ('ramp_hold', 'track'))
    limits = dict(limits or {})
    if cand_mode == 'track' and 'track_env' not in limits:
        limits['track_env'] = auto_track_env(N, dt)                     # (not applied with the gt_mpc cost: igtmpc.h)
    kp = R.kparams(rid)                                                 # [E,M,3]
    absh = R.TABLES['abs_heading'][rid]
    u_prev = np.tile(np.array([0.0 if gt else 0.1, 0.0]), (E, M, 1))    # evaluate.py:419 (mpc) / 171 (gt_mpc)
    solver = BatchSolver(N=N, dt=dt, n_rk4=n_rk4, C=C, n_obs=M - 1, device=device, dtype=dtype, cand_mode=cand_mode,
                         refine_iters=refine_iters if cand_mode in ('ramp_hold', 'track') else 0,
                         cost_mode='value_net' if gt else 'progress', polish_iters=polish_iters, polish_grad=polish_grad,
                         polish_step=polish_step, value_polish_iters=vp_iters,
                         value_polish_driver=value_polish_driver if gt else 'host',
                         **dict({} if feas_tol is None else {'feas_tol': feas_tol}, **dict({'d_min': 0.0} if obca else {}, **limits)))
    enc = None
    if gt:
        solver.set_value_net(**value_net)
        # scenario encodings (mpc.py:336-337, utils.py:84-169): (e_ego, e_other) per problem
        enc = np.zeros((E, M, 2))
        for e, pair in enumerate(pairs):
            code = R.scenario_encoding_sign(pair, R.scenario_of(pair))
            enc[e, 0] = (code[0], code[1])
            enc[e, 1] = (code[1], code[0])
        enc = enc.reshape(E * M, 2)
    if terminal_set:
        solver.set_cinf(*cinf_halfplanes(dt=dt, jerk=solver.params.jerk_limit))
    stepper = BatchSolver(N=1, dt=dt, n_rk4=n_rk4, C=64, n_obs=0, device=device, dtype='f64',
                          **{k: v for k, v in limits.items() if k in ('l_r', 'l_f')})      # the same vehicle

    S = _loop_state(x, u_prev, kp, absh.astype(np.uint32).reshape(-1), rid, enc, N, M_sim, solver.np_dtype, warm,
                    a_first=np.tile(0.09 * (np.arange(M) + 1.0), (E, 1)) if gt else None,      # evaluate.py:207-210
                    a_fixed=np.zeros((E, M)) if constant_speed else None,                      # constant_acceleration_model.py:26-29
                    device=device if device_resident else None)
    do = SimpleNamespace(forecast=solver.forecast_scene_pose if pose_dev else solver.forecast_scene,      # pose: x, y, heading in one call
                         solve=partial(solver.solve_box, length=OBCA_LENGTH, width=OBCA_WIDTH, d_box=0.0) if obca else solver.solve,
                         advance=(partial(_advance_fused, solver=solver, a_brake=a_min_policy) if step == 'fused' else
                                  partial(_advance_torch if device_resident else _advance_numpy, stepper=stepper, a_brake=a_min_policy)),
                         headings=None, solve_ms=[], plans=[] if log_plans and not device_resident else None)
    if obca and not pose_dev:      # x, y from the device with the host predictor's (or the shared plan's) headings
        host_pred = ConstantAccelerationModel(N=N, dt=dt, constant_speed=constant_speed)
        do.headings = lambda a_fc: obca_headings(host_pred, S.x, a_fc, S.rid, S.has_plan, S.plan_x, S.plan_u, absh)
    wall = _drive(S, do, M_sim, gt, device=device if device_resident else None, graph=graph, verbose=verbose)
    solver.close()
    stepper.close()

    host = (lambda a: a.cpu().numpy()) if device_resident else (lambda a: a)
    x_data = host(S.x_data)
    res = dict(x_data=x_data, u_data=host(S.u_data), infeasible_ratio=host(S.infeasible) / M_sim,
               deadlock=(x_data[:, 2::7, -1] <= 30).sum(axis=1) >= 2,      # evaluate.py:566-569
               routes=pairs, solve_ms=np.array(do.solve_ms), track_env=limits.get('track_env'))
    if device_resident:
        res.update(solve_ms=np.full(M_sim, wall / M_sim * 1e3), wall_s=wall)
    if do.plans is not None:
        res['plans'] = do.plans
    return res


OBCA_LENGTH, OBCA_WIDTH = 4.47, 2.0      # mpc.py:48-51, 105-106: every vehicle's rectangle


def obca_headings(pred, x, a_fc, rid, have_plan, sol_x, sol_u, absh):
    """heading[E,M,N+1] of every agent's forecast as an 'obca' ego reads it: the host predictor's route heading along the
    constant-acceleration forecast (node 0: the true heading); where the agent shares its plan, the plan's headings shifted by
    one step and the route heading one predicted step behind its end (utils.py:339-352, the retry with a = 0 above v = 5);
    |heading| for agents on routes '32', '41' (mpc.py:250-253)."""
    E, M = x.shape[:2]
    N, dt = pred.N, pred.dt
    flat = lambda q: np.asarray(q, dtype=np.float64).reshape(E * M)
    head = pred.predict_arrays(flat(x[..., 2]), flat(x[..., 5]), flat(a_fc), rid.reshape(E * M))['heading'].reshape(E, M, N + 1).copy()
    head[..., 0] = x[..., 6]
    last, a_last = sol_x[..., N], sol_u[:, :, 0, N - 1]
    a_ext = np.where(np.clip(last[..., 5] + a_last * dt, pred.v_min, pred.v_max) > 5, 0.0, a_last)
    s_ext = last[..., 2] + (last[..., 5] * dt + 0.5 * a_ext * dt ** 2)
    shared = np.concatenate([sol_x[:, :, 6, 1:], R.psi_ref(rid.reshape(E * M), flat(s_ext)).reshape(E, M, 1)], axis=-1)
    head = np.where(np.asarray(have_plan, dtype=bool)[..., None], shared, head)
    return np.where(np.asarray(absh, dtype=bool)[..., None], np.abs(head), head)


def gather_opponents(a):
    """a[E,M,...] per agent -> [E M, M-1, ...]: for every (episode, ego) problem the other agents' rows in ascending order, the
    order of the forecast's obstacle slots."""
    E, M = a.shape[:2]
    idx = np.array([[j for j in range(M) if j != i] for i in range(M)])      # [M, M-1]
    return a[:, idx].reshape((E * M, M - 1) + a.shape[2:])


def shift_controls(u, out=None):
    """Control part of utils.py:354-363 augment_prev_sol: u[...,2,N] -> [u[..., 1:], u[..., -1:]] (numpy or torch; written into
    `out` where one is given)."""
    if isinstance(u, np.ndarray):
        return np.concatenate([u[..., 1:], u[..., -1:]], axis=-1, out=out)
    import torch
    return torch.cat([u[..., 1:], u[..., -1:]], dim=-1, out=out)


def _check_options(ca_type, pose_forecast, device_resident, graph, dtype, polish_iters, value_polish_iters, value_polish_driver,
                   step, num_agents, eval_mode, a_min_policy, needs_value_net):
    """Every refusal run_closed_loop makes of its options, in the order callers rely on, before anything is set up
    -> the derived switches (obca, pose_dev, gt, vp_iters, M, a_min_policy).  needs_value_net: init= without value_net=."""
    if ca_type not in ('circle', 'obca'):
        raise ValueError(f"ca_type must be 'circle' or 'obca', not {ca_type!r}")
    obca = ca_type == 'obca'
    if pose_forecast not in ('host', 'device'):
        raise ValueError(f"pose_forecast must be 'host' or 'device', not {pose_forecast!r}")
    pose_dev = pose_forecast == 'device'
    if pose_dev and not obca:
        raise ValueError("pose_forecast='device' needs ca_type='obca': the circle model reads no pose")
    if obca and not pose_dev and (device_resident or graph):
        raise ValueError("ca_type='obca' runs in the host loop only (no device forecast of headings): not with device_resident=True "
                         'or graph=True')
    if obca and (dtype != 'f64' or polish_iters > 0 or value_polish_iters > 0):
        raise ValueError("ca_type='obca' needs dtype='f64' and takes neither polish_iters nor value_polish_iters (the polish judges "
                         'its trial plans with the circle)')
    if step not in ('torch', 'fused'):
        raise ValueError(f"step must be 'torch' or 'fused', not {step!r}")
    if step == 'fused' and not device_resident:
        raise ValueError("step='fused' is the device-resident loop's step (igt_loop_advance_*): it needs device_resident=True")
    M = int(num_agents)
    if not 2 <= M <= 4:
        raise ValueError(f'num_agents = {num_agents}: a scene has 2, 3 or 4 vehicles (one per approach lane)')
    gt = eval_mode == 'gt_mpc'
    if gt and M > 2:
        raise ValueError("eval_mode='gt_mpc' needs num_agents = 2: the value network's features are those of a two-vehicle "
                         'scene (mpc.py:326-338)')
    check_value_polish(value_polish_iters, dtype if gt else 'f64', 'value_net')      # the range in every mode; the dtype where it is read
    check_value_polish_driver(value_polish_driver)
    vp_iters = value_polish_iters if gt else 0
    if vp_iters and value_polish_driver == 'device' and graph:
        raise ValueError("value_polish_iters > 0 with value_polish_driver='device' is refused under stream capture (igtmpc.h "
                         'igt_set_value_polish): not with graph=True')
    if vp_iters and value_polish_driver == 'host' and device_resident:
        raise ValueError('value_polish_iters > 0 is driven from the host today: not with device_resident=True / graph=True')
    if gt and needs_value_net:
        raise ValueError("eval_mode='gt_mpc' with init= needs value_net (the shipped networks are per scenario)")
    return obca, pose_dev, gt, vp_iters, M, A_MIN_POLICY if a_min_policy is None else float(a_min_policy)


def _loop_state(x, u_prev, kp, flags, rid, enc, N, M_sim, npdt, warm, a_first=None, a_fixed=None, device=None):
    """Everything a step reads and the advance leaves, as one object: numpy arrays (device=None, the host loop) or tensors in HBM.
    State, float64: x[E,M,7], u_prev[E,M,2]; what the next forecast reads: has_plan[E,M] (int32, zeros until a step has run),
    plan_x[E,M,7,N+1], plan_u[E,M,2,N] (solver dtype, nan_to_num of the last answer); what the next solve reads when it is warm-
    started: flags_ws[n] (flags | IGT_FLAG_WARM where solved), u_ws[n,2,N] (plan_u shifted); infeasible[E,M], the logs
    x_data[E,7M,T+1], u_data[E,2M,T] and col, the column the next advance writes.  Constants: kp (float64) / kp_s (solver dtype)
    [n,3], flags[n], rid[E,M], enc[n,2] | None, a_first / a_fixed [E,M] | None (the forecast's acceleration at step 0 / at every
    step), warm.  cast(a): a as the solver's dtype, contiguous.  The device loops update every array in place, so a captured
    step replays on the same buffers."""
    (E, M), n = x.shape[:2], x.shape[0] * x.shape[1]
    as_s = lambda a: None if a is None else np.asarray(a).astype(npdt)
    S = SimpleNamespace(
        x=x.astype(np.float64), u_prev=u_prev.astype(np.float64), has_plan=np.zeros((E, M), np.int32),
        plan_x=np.zeros((E, M, 7, N + 1), npdt), plan_u=np.zeros((E, M, 2, N), npdt), flags_ws=np.zeros(n, np.uint32),
        u_ws=np.zeros((n, 2, N), npdt), infeasible=np.zeros((E, M), np.int64), x_data=np.zeros((E, 7 * M, M_sim + 1)),
        u_data=np.zeros((E, 2 * M, M_sim)), col=np.zeros(1, np.int64), kp=kp.reshape(n, 3).astype(np.float64), kp_s=as_s(kp.reshape(n, 3)),
        flags=flags, rid=rid.astype(np.int32), enc=as_s(enc), a_first=a_first, a_fixed=a_fixed)
    S.x_data[:, :, 0] = x.reshape(E, 7 * M)
    S.warm, S.cast = warm, lambda a: a.astype(npdt)
    if device is not None:
        import torch
        td = torch.float32 if npdt == np.float32 else torch.float64
        for k, a in list(vars(S).items()):
            if isinstance(a, np.ndarray):      # flag words travel as int32: the same bits
                setattr(S, k, torch.as_tensor(np.ascontiguousarray(a.view(np.int32) if a.dtype == np.uint32 else a),
                                              device=torch.device('cuda', device)))
        S.cast = lambda a: a.to(td).contiguous()
    return S


def _step(S, do, first, warm):
    """One time step, host or device: forecast acceleration -> forecast -> warm-start inputs -> solve -> advance.  first: step 0
    (gt_mpc's forecast acceleration); warm: this solve takes the warm start the last advance left."""
    n = S.kp.shape[0]
    # forecast of every other agent for every (episode, ego) problem, from the scene where it lies: predict (evaluate.py:455)
    # -> share motion forecasts (458-460) -> filter_preds (474)
    a_fc = S.a_fixed if S.a_fixed is not None else S.a_first if first and S.a_first is not None else S.u_prev[..., 0]
    obs, tv = do.forecast(S.cast(S.x), S.cast(a_fc), S.rid, S.plan_x, S.plan_u, S.has_plan)
    if do.headings is not None:                                         # pose [E M, n_obs, 3, N+1]
        obs = np.concatenate([obs, gather_opponents(do.headings(a_fc))[:, :, None, :].astype(obs.dtype)], axis=2)
    # solve every (episode, agent) problem at once (evaluate.py:470-482); an agent that solved the previous step passes that
    # solution, shifted by one step, as its warm start (evaluate.py:478-481)
    fl, u_ws = (S.flags_ws, S.u_ws) if warm else (S.flags, None)
    gt = S.enc is not None                                              # (tv is read by the gt_mpc cost only: M = 2, [E M, 2])
    t0 = time.perf_counter()
    out = do.solve(S.cast(S.x.reshape(n, 7)), S.cast(S.u_prev.reshape(n, 2)), S.kp_s, fl, obs, tv.reshape(n, -1) if gt else None,
                   S.enc, u_ws=u_ws)
    do.solve_ms.append((time.perf_counter() - t0) * 1e3)
    if do.plans is not None:
        do.plans.append(dict(ok=(out['status'] == 0).reshape(S.has_plan.shape), x=out['x'].reshape(S.plan_x.shape).astype(np.float64),
                             obs=np.array(obs, dtype=np.float64)))
    do.advance(S, out)


# The advance, three times with one contract: (S, the solve's answer) -> S holds the next step's state, has_plan, plans and -- when
# S.warm -- flags_ws and u_ws, the counters and the two log columns; col moves on.  Solved: next state = x*[:,1], applied input =
# u*[:,0] (evaluate.py:491-510); infeasible: brake fallback, a_brake if v > 0 else 0, one model step, v < 0 -> stop (511-545).
def _advance_numpy(S, out, stepper, a_brake):
    (E, M), N = S.has_plan.shape, S.plan_u.shape[-1]
    x, u_prev = S.x, S.u_prev
    ok = (out['status'] == 0).reshape(E, M)
    xs, us = out['x'].reshape(E, M, 7, N + 1), out['u'].reshape(E, M, 2, N)
    v_now = x[..., 5]
    a_fb = np.where(v_now > 0, a_brake, 0.0)
    u_fb = np.stack([a_fb, u_prev[..., 1]], axis=-1)
    nxt_fb = stepper.frenet_step(x.reshape(E * M, 7), u_fb.reshape(E * M, 2), S.kp).reshape(E, M, 7)
    neg = v_now < 0                                                     # evaluate.py:523-526: instantaneous stop
    stop = x.copy()
    stop[..., 5] = 0.0
    nxt_fb = np.where(neg[..., None], stop, nxt_fb)
    u_fb[..., 0] = np.where(neg, 0.0, u_fb[..., 0])
    S.x = np.where(ok[..., None], xs[:, :, :, 1], nxt_fb)
    S.u_prev = np.where(ok[..., None], us[:, :, :, 0], u_fb)
    S.infeasible += ~ok
    S.has_plan, S.plan_x, S.plan_u = ok.astype(np.int32), np.nan_to_num(xs), np.nan_to_num(us)
    if S.warm:
        S.flags_ws = S.flags | np.where(ok.reshape(-1), IGT_FLAG_WARM, 0).astype(np.uint32)
        S.u_ws = shift_controls(S.plan_u).reshape(E * M, 2, N)
    S.u_data[:, :, S.col[0]] = S.u_prev.reshape(E, 2 * M)
    S.col += 1
    S.x_data[:, :, S.col[0]] = S.x.reshape(E, 7 * M)


def _advance_torch(S, out, stepper, a_brake):
    """About 40 tensor operations and the stepper handle's model step, every one in place on S's buffers."""
    import torch
    (E, M), N = S.has_plan.shape, S.plan_u.shape[-1]
    x, u_prev = S.x, S.u_prev
    ok = (out['status'] == 0).reshape(E, M)
    xs, us = out['x'].reshape(E, M, 7, N + 1), out['u'].reshape(E, M, 2, N)
    v_now = x[..., 5]
    a_fb = torch.where(v_now > 0, torch.full_like(v_now, a_brake), torch.zeros_like(v_now))
    neg = v_now < 0
    u_fb = torch.stack([torch.where(neg, torch.zeros_like(a_fb), a_fb), u_prev[..., 1]], dim=-1)
    u_step = torch.stack([a_fb, u_prev[..., 1]], dim=-1)
    nxt_fb = stepper.frenet_step(x.reshape(E * M, 7).contiguous(), u_step.reshape(E * M, 2).contiguous(), S.kp).reshape(E, M, 7)
    stop = x.clone()
    stop[..., 5] = 0.0
    nxt_fb = torch.where(neg[..., None], stop, nxt_fb)
    x.copy_(torch.where(ok[..., None], xs[:, :, :, 1].to(torch.float64), nxt_fb))
    u_prev.copy_(torch.where(ok[..., None], us[:, :, :, 0].to(torch.float64), u_fb))
    S.infeasible.add_((~ok).to(torch.int64))
    S.has_plan.copy_(ok)
    S.plan_x.copy_(torch.nan_to_num(xs))
    S.plan_u.copy_(torch.nan_to_num(us))
    if S.warm:
        torch.bitwise_or(S.flags, S.has_plan.reshape(-1) * IGT_FLAG_WARM, out=S.flags_ws)
        shift_controls(S.plan_u, out=S.u_ws.view(E, M, 2, N))
    S.u_data.index_copy_(2, S.col, u_prev.reshape(E, 2 * M, 1))
    S.col.add_(1)
    S.x_data.index_copy_(2, S.col, x.reshape(E, 7 * M, 1))


def _advance_fused(S, out, solver, a_brake):
    """step='fused': everything behind the solve is ONE kernel (igtmpc.h igt_loop_advance_*) on the solver's own handle, writing
    into S's buffers ([E,M,...] and [n,...] are the same bytes, the logs agent-major)."""
    n, N, T = S.kp.shape[0], S.plan_u.shape[-1], S.u_data.shape[-1]
    solver.loop_advance(S.x.view(n, 7), S.u_prev.view(n, 2), S.kp, out['status'], out['x'], out['u'], a_brake, flags=S.flags,
                        infeasible=S.infeasible.view(n), x_log=S.x_data.view(n, 7, T + 1), u_log=S.u_data.view(n, 2, T), step=S.col,
                        out=dict(has_plan=S.has_plan.view(n), plan_x=S.plan_x.view(n, 7, N + 1), plan_u=S.plan_u.view(n, 2, N),
                                 u_ws=S.u_ws, flags=S.flags_ws))
    S.col.add_(1)


def _drive(S, do, M_sim, gt, device=None, graph=False, verbose=False):
    """The time loop over _step: owns `first` (step 0), the warm-start delay (evaluate.py:478: mpc passes it from t = 1; :232:
    gt_mpc for t > 1 only) and, with graph=True and M_sim > 3, the graph protocol -- steps 0 and 1 run eagerly, step 1 on the
    capture stream, then ONE step (forecast, solve, advance: every launch between them) is captured in a stream graph and
    replayed for the remaining steps; the loop is launch-bound at a few hundred problems per step, the replay removes the
    launches.  -> wall seconds between the two synchronisations (device) or of the loop (host)."""
    run = lambda t: _step(S, do, first=t == 0, warm=S.warm and t > (1 if gt else 0))
    if device is not None:
        import torch
        dev = torch.device('cuda', device)
        torch.cuda.synchronize(dev)
    t_start = time.perf_counter()
    if device is not None and graph and M_sim > 3:
        run(0)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            run(1)
        torch.cuda.current_stream(dev).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            run(2)
        for _ in range(2, M_sim):
            g.replay()
    else:
        for t in range(M_sim):
            run(t)
            if verbose and device is None and t % 10 == 0:
                print(f't={t:3d} s={S.x[0, :, 2].round(2)} v={S.x[0, :, 5].round(2)} ok={S.has_plan[0] != 0}', flush=True)
    if device is not None:
        torch.cuda.synchronize(dev)
    return time.perf_counter() - t_start


def load_reference_configs(policy_yaml=None, env_yaml=None):
    """The reference driver's two configuration files -- mpc.yaml (evaluate.py:32-33) and common/fourwayint.yaml
    (evaluate.py:28-29) -- as keyword arguments of run_closed_loop: -> (kwargs, policy) where `policy` is the parsed
    mpc.yaml (what save_results writes back, evaluate.py:327-329).  What the driver reads of them is honoured
    (N, dt, a_min of the brake fallback, prediction_type, v0, ca_radius, l_r, l_f); what this package holds as frozen,
    reference-generated tables is CHECKED and refused when it differs (road geometry and fillet radius behind
    igtmpc/data/route_constants.json, the forecast's speed clip, two agents, the circle constraint) -- a silent mismatch
    would be a different intersection."""
    import yaml
    kw, policy = {}, {}
    if policy_yaml is not None:
        with open(policy_yaml) as f:
            policy = yaml.safe_load(f) or {}
        if policy.get('type', 'MPC') != 'MPC':
            raise ValueError(f"{policy_yaml}: type {policy.get('type')!r} -- only 'MPC' is a policy here (evaluate.py:69)")
        if policy.get('collision_avoidance_type', 'circle') != 'circle':
            raise ValueError(f"{policy_yaml}: collision_avoidance_type {policy['collision_avoidance_type']!r} -- only the circle "
                             'constraint (mpc.py:223-226) is implemented')
        pt = str(policy.get('prediction_type', 'constant_acceleration'))
        if 'constant_acceleration' in pt:                                  # evaluate.py:76-81, in the reference's order
            kw['constant_speed'] = False
        elif 'constant_speed' in pt:
            kw['constant_speed'] = True
        else:
            raise ValueError('Invalid prediction type')
        if 'N' in policy:
            kw['N'] = int(policy['N'])
        if 'a_min' in policy:
            kw['a_min_policy'] = float(policy['a_min'])
    if env_yaml is not None:
        with open(env_yaml) as f:
            env = yaml.safe_load(f) or {}
        frozen = {'road_width': R.ROAD_WIDTH, 'road_length': R.ROAD_LENGTH, 'ca_radius': R.CA_RADIUS, 'num_agents': 2,
                  'v_max': 20.0, 'v_min': -2.0}
        for k, want in frozen.items():
            if k in env and abs(float(env[k]) - want) > 1e-12:
                raise ValueError(f'{env_yaml}: {k} = {env[k]} but the route tables / forecast of this package were generated for '
                                 f'{want} (igtmpc/data/route_constants.json, tests/golden/make_golden.py)')
        if 'dt' in env:
            kw['dt'] = float(env['dt'])
        if 'v0' in env:
            kw['v0'] = float(env['v0'])
        lim = {k: float(env[k]) for k in ('l_r', 'l_f') if k in env}
        if lim:
            kw['limits'] = lim
    if 'dt' in policy and 'dt' in kw and abs(float(policy['dt']) - kw['dt']) > 1e-12:
        raise ValueError(f"mpc.yaml dt = {policy['dt']} and fourwayint.yaml dt = {kw['dt']} disagree")
    return kw, policy


def save_results(r, save_dir, eval_mode, sc, seed=2026, policy=None, timenow=None):
    """The run directory the reference's driver leaves behind (evaluate.py:319-369 gt_mpc, 578-640 mpc), from the result of
    run_closed_loop -- so that what reads the reference's runs (generate_video.py:180-191 takes cl_traj.pkl[index] as
    [7 M, T+1] rows x, y, s, ey, epsi, v, heading per agent) reads these:

        <save_dir><eval_mode>_sc<sc>_seed<seed>_<time>/mpc/                  cl_traj.pkl [E, 7M, T+1], u_cl.pkl [E, 2M, T],
                                                                             eval_stats.csv, evaluation_data.pkl, mpc.yaml
        <save_dir><eval_mode>_sc<sc>_seed<seed>_<time>/game_mpc/evaluation/  cl_traj.pkl, u_cl.pkl, stats.csv, mpc.yaml

    `save_dir` is joined the way the reference joins it (plain concatenation: give it a trailing separator).  One csv row per
    episode with the reference's columns; the solve-time columns hold the lock-step batch's step time in seconds for every
    agent (the reference sums IPOPT's t_* statistics per agent, evaluate.py:294-297), its standard deviation over the steps
    (the reference's mpc branch takes the std of the mean, i.e. 0 -- evaluate.py:604).  Not written: the .mp4 (the directory is made) and the `refs`
    entry of evaluation_data.pkl (ReferenceGen's Euler-rolled path arrays, a set-up-time product outside this package).
    -> the run directory."""
    import csv
    import datetime
    import pickle

    import yaml
    gt = eval_mode == 'gt_mpc'
    timenow = timenow or datetime.datetime.now().strftime('%Y%m%d_%H%M%S')                     # evaluate.py:66
    run = save_dir + eval_mode + '_sc' + str(sc) + '_seed' + str(seed) + '_' + timenow
    out = run + ('/game_mpc/evaluation' if gt else '/mpc')
    os.makedirs(out, exist_ok=True)
    os.makedirs(run + ('/game_mpc/evaluation_videos' if gt else '/mpc/evaluation_videos'), exist_ok=True)
    x_cl, u_cl = np.asarray(r['x_data']), np.asarray(r['u_data'])
    E, M = x_cl.shape[0], x_cl.shape[1] // 7
    with open(out + '/mpc.yaml', 'w') as f:
        yaml.safe_dump(dict(policy or {}), f)
    # Runs append (evaluate.py:341-350).  The reference reads its own pickles back for that; this writer NEVER unpickles a
    # file (a run directory may come from anywhere, and unpickling executes what the file says): what it has written so far is
    # kept beside the pickles as plain arrays (.igt_run.npz, read with allow_pickle=False), the pickles are output only, and a
    # directory that holds pickles but not that file -- one this package did not write -- is refused.
    side = out + '/.igt_run.npz'
    new = {'x_cl': x_cl, 'u_cl': u_cl, 'weights': np.ones((E, 2)), 'routes': np.array([list(p) for p in r['routes']]),
           'deadlock': np.asarray(r['deadlock']).reshape(E, 1), 'initial_agents': x_cl[:, :, 0].reshape(E, M, 7)}
    if os.path.isfile(side):
        with np.load(side, allow_pickle=False) as old:
            acc = {k: np.concatenate([old[k], new[k]], axis=0) for k in new}
    elif any(os.path.isfile(out + '/' + n) for n in ('cl_traj.pkl', 'u_cl.pkl', 'evaluation_data.pkl')):
        raise FileExistsError(f'{out} holds pickles this package did not write (no .igt_run.npz beside them): it does not '
                              f'unpickle files to append to them; give another --save_dir')
    else:
        acc = new
    np.savez(side, **acc)
    for name, arr in (('cl_traj.pkl', acc['x_cl']), ('u_cl.pkl', acc['u_cl'])):
        with open(out + '/' + name, 'wb') as f:
            pickle.dump(arr, f)
    step_s = np.asarray(r['solve_ms'], dtype=np.float64) / 1e3
    rows = []
    for e in range(E):
        row = {'avg_sol_times': np.full(M, step_s.mean()), 'std_solve_times': [float(step_s.std())] * M,
               'infeasible_ratio': np.asarray(r['infeasible_ratio'][e]), 'deadlock': bool(r['deadlock'][e])}
        rows.append(dict({'NN_query_time': np.array([-1])}, **row) if gt else row)               # evaluate.py:355, 605
    csv_file = out + ('/stats.csv' if gt else '/eval_stats.csv')
    fresh = not os.path.isfile(csv_file)
    with open(csv_file, mode='w' if fresh else 'a', newline='') as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0].keys()))
        if fresh:
            w.writeheader()
        w.writerows(rows)
    if not gt:                                                                                 # evaluate.py:592-602
        data = dict({'N': (policy or {}).get('N'), 'agent_types': ['CAV'] * M}, **acc)
        with open(out + '/evaluation_data.pkl', 'wb') as f:
            pickle.dump(data, f, protocol=pickle.HIGHEST_PROTOCOL)
    return run


def build_parser():
    ap = argparse.ArgumentParser(description='batched closed-loop evaluation (counterpart of evaluate.py --eval_mode mpc)')
    ap.add_argument('--sc', type=int, default=1)
    ap.add_argument('--num_samples', type=int, default=1)
    ap.add_argument('--num_agents', type=int, default=2, help='vehicles per scene, 2..4 (fourwayint.yaml:7 num_agents; mpc only beyond 2)')
    ap.add_argument('--N', type=int, default=None, help='horizon; default: the policy file\'s, else 40 (mpc.yaml:6; BASELINE.json benchmarks 20)')
    ap.add_argument('--policy_config', default=None, help="the reference's mpc.yaml (evaluate.py:32)")
    ap.add_argument('--env_config', default=None, help="the reference's common/fourwayint.yaml (evaluate.py:28)")
    ap.add_argument('--C', type=int, default=256)
    ap.add_argument('--eval_mode', default='mpc', choices=['mpc', 'gt_mpc'])
    ap.add_argument('--value_net', default=None, help='gt_mpc: .npz with W0,b0,W1,b1,... (optionally prefixed, see --net_prefix); '
                    'default: the network shipped for --sc')
    ap.add_argument('--net_prefix', default='', help="key prefix inside the npz, e.g. 'sc1_'")
    ap.add_argument('--verbose', action='store_true')
    ap.add_argument('--ca_type', default='circle', choices=['circle', 'obca'],
                    help="collision model: 'circle' (mpc.yaml:16) or 'obca', 4.47 x 2.0 m rectangles with d_min = 0 (the host loop "
                         "only, unless --pose_forecast device)")
    ap.add_argument('--pose_forecast', default='host', choices=['host', 'device'],
                    help="with --ca_type obca: the obstacles' headings from the host predictor (default) or the whole pose from the "
                         "device (igt_forecast_scene_pose_f64), which also runs with --device_resident, --graph and --step fused")
    ap.add_argument('--device_resident', action='store_true', help='keep all per-step arrays in HBM (torch tensors)')
    ap.add_argument('--graph', action='store_true', help='with --device_resident: capture one step in a stream graph and replay it')
    ap.add_argument('--step', default='torch', choices=['torch', 'fused'],
                    help="with --device_resident: 'fused' runs everything behind the solve as one kernel (igt_loop_advance_*)")
    ap.add_argument('--cand_mode', default='track', choices=['lattice', 'ramp_hold', 'track'])
    ap.add_argument('--dtype', default='f64', choices=['f64', 'f32'])
    ap.add_argument('--polish_iters', type=int, default=0, help='f64, eval_mode mpc: projected-gradient steps on each winner (0..4)')
    ap.add_argument('--value_polish_iters', type=int, default=0,
                    help='f64, eval_mode gt_mpc: projected-gradient steps on each winner under the value-network cost (0..4); with the '
                         "'host' driver refused with --device_resident and --graph")
    ap.add_argument('--value_polish_driver', choices=('host', 'device'), default='host',
                    help='who takes those steps: numpy on the host (default) or the library inside the solve (runs with '
                         '--device_resident; --graph is refused: stream capture)')
    ap.add_argument('--polish_grad', choices=('fd', 'adjoint'), default='fd', help='gradient of the polish: forward differences or analytic')
    ap.add_argument('--polish_step', choices=('gradient', 'newton'), default='gradient',
                    help='step of the polish: along the gradient, or half of the trials along the Gauss-Newton (LQ) direction')
    ap.add_argument('--save_dir', default=None, help='write the run directory the reference\'s driver writes (cl_traj.pkl, u_cl.pkl, '
                    'stats csv, mpc.yaml; evaluate.py:646) under <save_dir><eval_mode>_sc<sc>_seed2026_<time>/')
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    net = None
    if a.eval_mode == 'gt_mpc':
        if a.value_net:
            z = np.load(a.value_net)
            layers, i = [], 0
            while f'{a.net_prefix}W{i}' in z:
                layers.append((z[f'{a.net_prefix}W{i}'], z[f'{a.net_prefix}b{i}']))
                i += 1
            net = dict(layers=layers)
    kw, policy_file = load_reference_configs(a.policy_config, a.env_config)
    if a.N is not None:
        kw['N'] = a.N
    kw.setdefault('N', 40)
    a.N = kw['N']
    shared = ('sc', 'num_samples', 'C', 'verbose', 'eval_mode', 'device_resident', 'cand_mode', 'dtype', 'graph', 'polish_iters',
              'polish_grad', 'polish_step', 'value_polish_iters', 'value_polish_driver', 'num_agents', 'step', 'ca_type', 'pose_forecast')
    r = run_closed_loop(value_net=net, **{k: getattr(a, k) for k in shared}, **kw)      # the parser's names are the keywords
    if a.save_dir is not None:
        policy = {'type': 'MPC', 'N': a.N, 'dt': kw.get('dt', 0.1), 'a_min': -4, 'a_max': 3, 'v_min': -1.0, 'v_max': 5,      # mpc.yaml's keys
                  'prediction_type': 'constant_acceleration', 'collision_avoidance_type': 'circle', **policy_file,
                  'collision_avoidance_type': a.ca_type, 'N': a.N,
                  'solver': {'library': 'igtmpc', 'cand_mode': a.cand_mode, 'C': a.C, 'dtype': a.dtype, 'track_env': r.get('track_env')}}
        r['run_dir'] = save_results(r, a.save_dir, a.eval_mode, a.sc, policy=policy)
    print(json.dumps({'sc': a.sc, 'episodes': a.num_samples, 'routes': r['routes'][:4],
                      'infeasible_ratio_mean': r['infeasible_ratio'].mean(axis=0).tolist(),
                      'deadlock_rate': float(r['deadlock'].mean()),
                      'final_s_mean': r['x_data'][:, 2::7, -1].mean(axis=0).tolist(),
                      'avg_solve_ms_per_step': float(r['solve_ms'][5:].mean()), 'run_dir': r.get('run_dir')}))


if __name__ == '__main__':
    main()
