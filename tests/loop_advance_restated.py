"""TEST INFRASTRUCTURE ONLY -- the closed-loop step behind a solve (include/igtmpc.h igt_loop_advance_*) restated in numpy,
agent by agent as the header states it, and the cases the CPU and GPU tests of it share.

    ok = status == 0
    ok:      x <- x_sol[:, 1], u_prev <- u_sol[:, 0]                                            evaluate.py:491-510
    not ok:  a_fb = a_brake if v > 0 else 0; x <- model_step(x, (a_fb, u_prev[1]), kparams);     evaluate.py:511-545
             v < 0: x <- x with v = 0, applied a = 0                                             :523-526
    has_plan = ok; plan_* = nan_to_num(solution); u_ws = plan_u shifted, last column repeated    utils.py:339-363
    flags_out = flags_in | (ok ? IGT_FLAG_WARM : 0); infeasible += !ok
    step t in 0..T-1: u_log[:, :, t] = new u_prev, x_log[:, :, t+1] = new x

The model step is a callable (x[n,7], u[n,2], kparams[n,3]) -> x_next[n,7]: np_oracle's exact Frenet step on the CPU
(test_loop_advance_host.py, where the restatement is held to igtmpc/evaluate.py's host loop), igt_frenet_step_f64 on the GPU."""
import numpy as np

IGT_FLAG_WARM = 2


def loop_advance_restated(x, u_prev, kparams, status, x_sol, u_sol, a_brake, model_step, flags=None, infeasible=None,
                          x_log=None, u_log=None, step=None, want_ws=True):
    """Nothing is modified in place: -> dict(x, u_prev, has_plan, plan_x, plan_u, u_ws, flags, infeasible, x_log, u_log), the
    optional ones None where their inputs are."""
    x, u_prev = np.array(x, dtype=np.float64), np.array(u_prev, dtype=np.float64)
    n = len(x)
    ok = np.asarray(status) == 0
    with np.errstate(invalid='ignore'):
        v = x[:, 5]
        a_fb = np.where(v > 0, float(a_brake), 0.0)
        neg = v < 0
    stepped = np.asarray(model_step(x, np.stack([a_fb, u_prev[:, 1]], axis=1), np.asarray(kparams, dtype=np.float64)))
    x_new, u_new = np.empty((n, 7)), np.empty((n, 2))
    for i in range(n):
        if ok[i]:
            x_new[i] = np.asarray(x_sol[i, :, 1], dtype=np.float64)
            u_new[i] = np.asarray(u_sol[i, :, 0], dtype=np.float64)
        elif neg[i]:
            x_new[i] = x[i]
            x_new[i, 5] = 0.0
            u_new[i] = (0.0, u_prev[i, 1])
        else:
            x_new[i] = stepped[i]
            u_new[i] = (a_fb[i], u_prev[i, 1])
    plan_x, plan_u = np.nan_to_num(x_sol), np.nan_to_num(u_sol)
    out = dict(x=x_new, u_prev=u_new, has_plan=ok.astype(np.int32), plan_x=plan_x, plan_u=plan_u,
               u_ws=np.concatenate([plan_u[:, :, 1:], plan_u[:, :, -1:]], axis=2) if want_ws else None,
               flags=None, infeasible=None, x_log=None, u_log=None)
    if flags is not None:
        out['flags'] = (np.asarray(flags, dtype=np.uint32) | np.where(ok, IGT_FLAG_WARM, 0).astype(np.uint32)).astype(np.uint32)
    if infeasible is not None:
        out['infeasible'] = np.asarray(infeasible, dtype=np.int64) + (~ok).astype(np.int64)
    if x_log is not None:
        out['x_log'], out['u_log'] = np.array(x_log, dtype=np.float64), np.array(u_log, dtype=np.float64)
        t, T = int(step), out['u_log'].shape[2]
        if 0 <= t < T:
            out['u_log'][:, :, t] = u_new
            out['x_log'][:, :, t + 1] = x_new
    return out


def branch_inputs(n, N, dtype, seed=0):
    """Inputs that take every branch at any n >= 1: status 0 / 1 interleaved; among the status-1 rows v > 0, = 0, < 0 and NaN
    in turn; their rows of x_sol / u_sol NaN (the solver's contract); turning and straight kparams; non-zero flag words and
    counters.  With n = 1 the one agent is a fallback row with v > 0 -- the other branches need more agents (the GPU test of
    n = 1 runs single rows of the eight-agent inputs, one per branch)."""
    rng = np.random.default_rng(seed + 1000 * n + N)
    status = (np.arange(n) % 2 == 0).astype(np.int32) if n > 1 else np.ones(1, np.int32)      # even rows fall back
    x = np.zeros((n, 7))
    x[:, 2] = rng.uniform(5.0, 40.0, n)
    x[:, 0], x[:, 1] = x[:, 2] + rng.normal(0, 1, n), rng.normal(0, 2, n)
    x[:, 3], x[:, 4] = rng.normal(0, 0.05, n), rng.normal(0, 0.02, n)
    x[:, 5] = rng.uniform(0.5, 5.0, n)
    x[:, 6] = rng.normal(0, 0.5, n)
    fb = np.nonzero(status != 0)[0]
    kind = np.arange(len(fb)) % 4                       # 0: v > 0   1: v = 0   2: v < 0   3: NaN
    x[fb[kind == 1], 5] = 0.0
    x[fb[kind == 2], 5] = -rng.uniform(0.01, 0.5, (kind == 2).sum())
    x[fb[kind == 3], 5] = np.nan
    u_prev = np.column_stack([rng.uniform(-4, 3, n), rng.uniform(-0.4, 0.4, n)])
    kp = np.tile([19.3, 19.3 + 8.6 * np.pi / 2, 1.0 / 8.6], (n, 1))
    kp[np.arange(n) % 3 == 0] = (np.inf, np.inf, 0.0)
    x_sol = rng.normal(0, 5.0, (n, 7, N + 1)).astype(dtype)
    u_sol = rng.uniform(-1, 1, (n, 2, N)).astype(dtype)
    x_sol[status != 0], u_sol[status != 0] = np.nan, np.nan
    flags = rng.integers(0, 2, n).astype(np.uint32)
    infeasible = rng.integers(0, 50, n).astype(np.int64)
    return dict(x=x, u_prev=u_prev, kparams=kp, status=status, x_sol=x_sol, u_sol=u_sol, flags=flags, infeasible=infeasible)


# ---- the closed loops test_gpu_loop_advance.py runs with step='fused' against step='torch' ----
# Every case starts from scene_loop_restated.scenes(M): episode 0 rolls at 2 m/s and solves, episode 1's agent 0 stands outside
# the lane bound and brakes from the first step on.  `events` are the oracle loop's own counts over both episodes (fallback
# steps, of which stopped; solved = 2 M STEPS - fallback), recorded here and recomputed on the CPU by test_loop_advance_host.py.
STEPS = 10
LOOP_CASES = {
    'mpc_f64_lattice': dict(kw=dict(eval_mode='mpc', dtype='f64', cand_mode='lattice', num_agents=2), warm=False),
    'mpc_f32_track_warm': dict(kw=dict(eval_mode='mpc', dtype='f32', cand_mode='track', warm_start=True, num_agents=2), warm=True),
    'gt_mpc_f64': dict(kw=dict(eval_mode='gt_mpc', dtype='f64', cand_mode='track', num_agents=2), warm=False),
    'mpc_f64_three': dict(kw=dict(eval_mode='mpc', dtype='f64', cand_mode='track', num_agents=3), warm=False),
}
LOOP_EVENTS = {       # from oracle_loop() below; test_loop_advance_host.py recomputes them
    'mpc_f64_lattice': dict(fallback=10, stop=1, solved=30, warm=0),
    'mpc_f32_track_warm': dict(fallback=10, stop=1, solved=30, warm=27),
    'gt_mpc_f64': dict(fallback=10, stop=1, solved=30, warm=0),
    'mpc_f64_three': dict(fallback=10, stop=1, solved=50, warm=0),
}


def loop_case_init(name):
    """-> (x[2,M,7], route tuples, run_closed_loop keywords) of a case."""
    import scene_loop_restated as S
    kw = dict(LOOP_CASES[name]['kw'])
    x, routes = S.scenes(kw['num_agents'])
    kw.update(N=20, T_sim=STEPS * 0.1, init=(x, routes))
    if kw['eval_mode'] == 'gt_mpc':
        from igtmpc.value_nets import shipped_value_net
        kw['value_net'] = shipped_value_net(1)
    return x, routes, kw


def oracle_loop(name):
    """The oracle loop alone on a case's episodes: -> (per-episode results, summed events).  Two vehicles: oracle/closed_loop.py;
    three: tests/scene_loop_restated.py.  Float64 whatever the case's dtype: the counts are the oracle's."""
    import closed_loop as CL
    import np_oracle as O
    import scene_loop_restated as S
    from igtmpc.cinf import cinf_halfplanes
    from igtmpc.evaluate import auto_track_env
    x, routes, kw = loop_case_init(name)
    P = O.Params(N=20)
    env = auto_track_env(20, 0.1) if kw['cand_mode'] == 'track' and kw['eval_mode'] == 'mpc' else 1.0
    res, ev = [], dict(fallback=0, stop=0, share=0, share_retry=0, warm=0)
    for e in range(len(routes)):
        if kw['num_agents'] == 2:
            extra = {}
            if kw['eval_mode'] == 'gt_mpc':
                extra = dict(eval_mode='gt_mpc', net=dict(kw['value_net'], Wn=np.eye(6), mu_f=np.zeros(6), sigma_t=1.0, mu_t=0.0))
            r = CL.run_episode(x[e], routes[e], P, cinf_halfplanes(), M_sim=STEPS, cand_mode=kw['cand_mode'],
                               warm_start=LOOP_CASES[name]['warm'], track_env=env, **extra)
        else:
            r = S.run_scene(x[e], routes[e], P, cinf_halfplanes(), M_sim=STEPS, cand_mode=kw['cand_mode'],
                            warm_start=LOOP_CASES[name]['warm'], track_env=env)
        res.append(r)
        for k in ev:
            ev[k] += r['events'][k]
    return res, ev
