"""Per-scenario candidate sets U[B,C,2,N] (BatchSolver.solve_candidates / rollout_candidates): the generator and the cases the
host and the GPU tests share.  The oracle needs nothing new: np_oracle.solve_batch(..., U=) broadcasts U to [B,C,2,N], so a U of
that shape is judged scenario by scenario."""
import numpy as np

import np_oracle as O
from helpers import host_params
from parity_cases import LONG_LIMITS, cinf_default, value_net_case

BAR = 1e-9      # tol = eps = tie of every comparison here (float64: DESIGN.md section 6)


def per_scenario_candidates(u_prev, P, C, N, seed=11):
    """Rate-feasible ramps around each scenario's u_prev, clipped to the input box; the last eighth breaks the rate limit and the
    last sixteenth the input box as well, so both verdicts of a table candidate are raised in every scenario."""
    rng = np.random.default_rng(seed); B = len(u_prev)
    ra, rd = P.dt * P.jerk, P.dt * P.steer_rate
    da = rng.uniform(-1, 1, (B, C, 1)) * ra * rng.uniform(0.2, 1.0, (B, C, N))
    dd = rng.uniform(-1, 1, (B, C, 1)) * rd * 0.3 * rng.uniform(-0.5, 1.0, (B, C, N))
    U = np.empty((B, C, 2, N))
    a = np.broadcast_to(u_prev[:, None, 0], (B, C)).astype(np.float64).copy()
    d = np.broadcast_to(u_prev[:, None, 1], (B, C)).astype(np.float64).copy()
    for k in range(N):
        a = np.clip(a + da[..., k], P.a_min, P.a_max); d = np.clip(d + dd[..., k], -P.df_max, P.df_max)
        U[:, :, 0, k] = a; U[:, :, 1, k] = d
    U[:, C - C // 8:, 0, N // 2] += 3 * ra       # the last eighth breaks the rate limit ...
    U[:, C - C // 16:, 0, 3] = P.a_max + 0.5     # ... and its second half the input box as well
    return U


# (B, N, C, n_obs, n_rk4, long limits, value-network scenario or None) -> what the oracle alone measures (helpers.measure, eps =
# tie = BAR): every scenario is compared; `solved` of them are solved, `crossing` of those cross a curvature break-point; the OR
# of all verdict bits over the case is `bits` (every verdict is raised somewhere; without obstacles there is no collision bit).
CASES = {
    (48, 20, 64, 1, 4, False, None): dict(solved=32, crossing=6, bits=63),
    (24, 20, 256, 1, 4, False, None): dict(solved=17, crossing=0, bits=63),
    (24, 13, 128, 0, 4, False, None): dict(solved=21, crossing=1, bits=31),
    (24, 40, 64, 2, 4, True, None): dict(solved=17, crossing=1, bits=63),
    (16, 64, 64, 1, 3, True, None): dict(solved=10, crossing=2, bits=63),
    (24, 20, 128, 1, 4, False, 1): dict(solved=16, crossing=0, bits=63),
    (24, 20, 64, 1, 4, False, 3): dict(solved=16, crossing=0, bits=63),
}


def case_id(key):
    B, N, C, n_obs, n_rk4, long, sc = key
    return f'{B}-{N}-{C}-{n_obs}-{n_rk4}' + ('-long' if long else '') + (f'-sc{sc}' if sc else '')


_BUILT = {}


def build(key):
    """-> dict(key, B, N, C, n_obs, n_rk4, limits, P, cinf, net, x0, u_prev, kparams, flags, obs, tv_sv, enc, U), float64; built
    once and shared -- nothing may write into it."""
    if key not in _BUILT:
        from igtmpc.scenarios import make_batch
        B, N, C, n_obs, n_rk4, long, sc = key
        limits = dict(LONG_LIMITS) if long else {}
        P = host_params(N=N, n_rk4=n_rk4, **limits)
        b = make_batch(B, dtype=np.float64, N=N)
        obs = np.concatenate([b['obs_xy']] * max(n_obs, 1), axis=1)[:, :n_obs]
        for m in range(1, n_obs):
            obs[:, m, 0] += 3.0 * m
        net = value_net_case(sc, 'f64')['net'] if sc else None
        c = dict(key=key, B=B, N=N, C=C, n_obs=n_obs, n_rk4=n_rk4, limits=limits, P=P, cinf=cinf_default(), net=net,
                 x0=b['x0'], u_prev=b['u_prev'], kparams=b['kparams'], flags=b['flags'], obs=np.ascontiguousarray(obs),
                 tv_sv=b['tv_sv'] if sc else None, enc=b['enc'] if sc else None,
                 U=per_scenario_candidates(b['u_prev'], P, C, N))
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _BUILT[key] = c
    return _BUILT[key]


_ORACLE = {}


def oracle(case):
    """-> (passes, x0[B,1,7] with the flags applied, kp[B,1,3]) as helpers.compare_solve takes them; computed once per case."""
    k = case['key']
    if k not in _ORACLE:
        A, b = case['cinf']
        kw = dict(net=case['net'], tv_sv=case['tv_sv'], enc=case['enc']) if case['net'] else {}
        obs = case['obs'] if case['n_obs'] else None
        r = O.solve_batch(case['x0'], case['u_prev'], case['kparams'], case['flags'], obs, A, b, case['P'], C=case['C'],
                          U=case['U'], return_all=True, **kw)
        _ORACLE[k] = ([r], O.apply_flags(case['x0'], case['flags'])[:, None, :], case['kparams'][:, None, :])
    return _ORACLE[k]


def open_solver(igt, case, **kw):
    """A table solver of the case's shape, limits, terminal set and network; no shared table is set."""
    s = igt.BatchSolver(N=case['N'], n_rk4=case['n_rk4'], C=case['C'], n_obs=case['n_obs'], dtype='f64', cand_mode='table',
                        cost_mode='value_net' if case['net'] else 'progress', **case['limits'], **kw)
    try:
        s.set_cinf(*case['cinf'])
        if case['net']:
            s.set_value_net(**case['net'])
    except BaseException:
        s.close()
        raise
    return s


def solve_args(case, sl=slice(None)):
    """Positional and keyword arguments of solve_candidates / rollout_candidates (without U) for the scenarios `sl`."""
    kw = dict(obs_xy=case['obs'][sl])
    if case['net']:
        kw.update(tv_sv=case['tv_sv'][sl], enc=case['enc'][sl])
    return [case['x0'][sl], case['u_prev'][sl], case['kparams'][sl], case['flags'][sl]], kw
