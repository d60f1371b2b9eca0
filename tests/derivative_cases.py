"""The derivative kernels (igt_cost_gradient_f64, igt_cost_gradient_vn_f64) and the polishes (forward-difference, adjoint, Newton,
value-network) away from the reference's default limits: the stations the host test (tests/test_derivative_cases_host.py) and the
GPU test (tests/test_gpu_derivative_limits.py) share -- tests only, no GPU.

A station is a fixed, named set of limits, not a draw: a failure names its cause.  All stations: B = 24 make_batch scenarios,
N = 20 (turning routes cross a break-point), C = 256 lattice seeds, one obstacle, float64, the terminal set of
cinf_halfplanes(dt=, jerk=) unless the station has none.  Each station carries its own make_batch seed, chosen so that the
conditions of the host test hold (near-ties between trials and stage arguments on a break-point depend on the seed); what the
oracle and the restatements alone measure at that seed is recorded in FACTS and asserted by the host test.

    rear-short      l_r = 1.2, l_f = 3.0: lr_ratio = 0.286, the long-polynomial leaf (hi_order) at n_rk4 = 4
    rear-long       l_r = 3.0, l_f = 1.2: lr_ratio = 0.714 on the (hi_order = 0, NRK = 4) leaf
    rear-short-rk7  rear-short at n_rk4 = 7: the (0, run-time sub-steps) leaf with lr_ratio != 0.5
    dt-fine         dt = 0.05: a terminal set of 143 facets
    dt-coarse       dt = 0.2: hi_order at n_rk4 = 4; 38 facets
    no-steer-rate   steer_rate_limit = 0: the frozen-steering branch of every polish
    tight-box       a in [-1.5, 1], |df| <= 0.35, jerk 4, steering rate 2: the box clamp binds inside the projection
    no-effort       w_u = 0: R = 0 in the LQ model of the Newton step
    heavy-effort    w_u = 0.3
    tol0-vmin       feas_tol = 0, v_min = -1: verdicts without a tolerance band
    fast            v_max = 15, a_max = 6, ey_lim = 1.5, steering rate 0.1, initial speeds in [6, 14], no terminal set: hi_order
                    through the speed bound, a far obstacle reach

no-effort: newton_restated.riccati_direction zeroes the whole direction of a (scenario, iteration) whose Quu has a determinant
<= 0; FACTS records in how many pairs that happens (det_nonpos).  The count is 0: the comment above FACTS says what the station
reaches instead."""
import functools

import numpy as np

import adjoint_restated as A
import newton_restated as NR
import np_oracle as O
import polish_restated as R
from helpers import host_params, oracle_params, params_equal

B, N, C, N_OBS = 24, 20, 256, 1
MODES = ('fd', 'adjoint', 'newton')
ITERS = 2
SOLVER_MODE = dict(fd={}, adjoint=dict(polish_grad='adjoint'), newton=dict(polish_step='newton'))

# name: dict(limits = BatchSolver keywords, seed[, dt, n_rk4, terminal, speeds])
STATIONS = {
    'rear-short': dict(limits=dict(l_r=1.2, l_f=3.0), seed=2026),
    'rear-long': dict(limits=dict(l_r=3.0, l_f=1.2), seed=2026),
    'rear-short-rk7': dict(limits=dict(l_r=1.2, l_f=3.0), n_rk4=7, seed=2026),
    'dt-fine': dict(limits={}, dt=0.05, seed=1),
    'dt-coarse': dict(limits={}, dt=0.2, seed=2026),
    'no-steer-rate': dict(limits=dict(steer_rate_limit=0.0), seed=1),
    'tight-box': dict(limits=dict(a_min=-1.5, a_max=1.0, df_max=0.35, jerk_limit=4.0, steer_rate_limit=2.0), seed=2026),
    'no-effort': dict(limits=dict(w_u=0.0), seed=2026),
    'heavy-effort': dict(limits=dict(w_u=0.3), seed=2026),
    'tol0-vmin': dict(limits=dict(feas_tol=0.0, v_min=-1.0), seed=2026),
    'fast': dict(limits=dict(v_max=15.0, a_max=6.0, ey_lim=1.5, steer_rate_limit=0.1), terminal=False, speeds=(6.0, 14.0), seed=6),
}
GEOMETRY = ('rear-short', 'rear-long', 'rear-short-rk7')          # stations that must see l_r and l_f exchanged
VN_GRADIENT = {'rear-short': 1, 'dt-coarse': 3, 'heavy-effort': 1}      # station -> shipped checkpoint (both depths)
VN_POLISH = {'rear-short': 1, 'dt-coarse': 3, 'no-steer-rate': 3}

# What the oracle and the restatements alone measure at each station's seed (tests/test_derivative_cases_host.py asserts every
# figure): scenarios the lattice solves, those of them on a turning route, KP::hi_order by parity_cases.leaf_hi_order, facets of
# the terminal set.  tight-box: restated plans after ITERS iterations that hold an input exactly on the box, per mode.
# tol0-vmin: solved scenarios whose lattice winner misses the rate limit by one rounding (the solve does not judge the lattice by
# it; at feas_tol = 0 the polish's rate verdict does, and leaves them alone).
# no-effort: det_nonpos = 0 -- the determinant rule of Riccati::step is NOT reached.  With R = 0, Quu = B'PB stays positive
# definite, with determinants from 1.4e-15 to 3.8e-8 over both iterations: the Newton direction is finite and enormous (entries
# up to 1.6e11), every one of its 32 trials clamps to the rate limits all along and loses, and the scaled gradient's trials win:
# the cost drop is the adjoint mode's (0.1767 both).  The station exercises R = 0 in costate_step, Riccati::step and the scale,
# and a Newton half that must lose, not the `det <= 0` branch.
FACTS = {
    'rear-short': dict(solved=19, turning=8, hi_order=1, facets=74),
    'rear-long': dict(solved=18, turning=7, hi_order=0, facets=74),
    'rear-short-rk7': dict(solved=19, turning=8, hi_order=0, facets=74),
    'dt-fine': dict(solved=23, turning=12, hi_order=0, facets=143),
    'dt-coarse': dict(solved=14, turning=5, hi_order=1, facets=38),
    'no-steer-rate': dict(solved=10, turning=5, hi_order=0, facets=74),
    'tight-box': dict(solved=18, turning=9, hi_order=0, facets=22, on_box=dict(fd=6, adjoint=6, newton=16)),
    'no-effort': dict(solved=19, turning=8, hi_order=0, facets=74, det_nonpos=0),
    'heavy-effort': dict(solved=19, turning=8, hi_order=0, facets=74),
    'tol0-vmin': dict(solved=19, turning=8, hi_order=0, facets=74, rate_ulp=6),
    'fast': dict(solved=18, turning=8, hi_order=1, facets=0),
}


def spec(station):
    return dict(dict(dt=0.1, n_rk4=4, terminal=True, speeds=None), **STATIONS[station])


@functools.lru_cache(maxsize=None)
def build(station):
    """-> dict(name, B, N, C, n_obs, dt, n_rk4, limits, P, cinf (A, b) or None, and the batch: x0, u_prev, kparams, flags, obs_xy,
    tv_sv, enc), float64; built once and shared -- nothing may write into it.  The dict itself serves the restatements as `batch`."""
    from igtmpc.cinf import cinf_halfplanes
    from igtmpc.scenarios import make_batch
    s = spec(station)
    b = make_batch(B, N=N, dt=s['dt'], seed=s['seed'], dtype=np.float64)
    if s['speeds']:
        b['x0'][:, O.IV] = np.random.default_rng([s['seed'], 1]).uniform(*s['speeds'], B)
    c = dict(name=station, B=B, N=N, C=C, n_obs=N_OBS, dt=s['dt'], n_rk4=s['n_rk4'], limits=dict(s['limits']),
             P=host_params(N=N, dt=s['dt'], n_rk4=s['n_rk4'], **s['limits']),
             cinf=cinf_halfplanes(dt=s['dt'], jerk=s['limits'].get('jerk_limit', 0.9)) if s['terminal'] else None,
             **{k: b[k] for k in ('x0', 'u_prev', 'kparams', 'flags', 'obs_xy', 'tv_sv', 'enc')})
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def net_of(station):
    """The value network of a value-network station (nonfinite_cases.net_of: non-identity statistics)."""
    import nonfinite_cases as NF
    return NF.net_of({**VN_GRADIENT, **VN_POLISH}[station])


def open_solver(igt, station, cand_mode='lattice', C=C, **kw):
    """A float64 solver of the station's discretisation, limits and terminal set (and, with cost_mode='value_net', its network);
    its parameters must be the ones the oracle runs with."""
    c = build(station)
    s = igt.BatchSolver(N=N, dt=c['dt'], n_rk4=c['n_rk4'], C=C, n_obs=N_OBS, dtype='f64', cand_mode=cand_mode, **c['limits'], **kw)
    try:
        assert params_equal(oracle_params(s), c['P']), (vars(oracle_params(s)), vars(c['P']))
        if c['cinf'] is not None:
            s.set_cinf(*c['cinf'])
        if kw.get('cost_mode') == 'value_net':
            s.set_value_net(**net_of(station))
    except BaseException:
        s.close()
        raise
    return s


def solve_args(c, vn=False):
    return [c[k] for k in ('x0', 'u_prev', 'kparams', 'flags', 'obs_xy') + (('tv_sv', 'enc') if vn else ())]


@functools.lru_cache(maxsize=None)
def grad_inputs(station):
    """-> (x0, kparams, flags, U[B,2,N]): one random lattice candidate per scenario, made from the station's P; every third scenario
    carries the abs-heading flag, every fifth sequence is steered off the lane (the recipe of test_gpu_gradient._grad_inputs)."""
    c = build(station)
    rng = np.random.default_rng(0)
    pick = rng.integers(0, C, size=B)
    U = np.ascontiguousarray(O.candidates_lattice(c['u_prev'], c['P'], C)[np.arange(B), pick])
    U[::5, 1, :5] += 0.2 * np.sign(rng.standard_normal((len(U[::5]), 1)))
    flags = np.asarray(c['flags']).copy()
    flags[::3] |= np.uint32(O.FLAG_ABS_HEADING)
    for a in (U, flags):
        a.setflags(write=False)
    return c['x0'], c['kparams'], flags, U


def swapped(P):
    """P with l_r and l_f exchanged"""
    kw = dict(vars(P))
    kw['l_r'], kw['l_f'] = P.l_f, P.l_r
    return O.Params(**kw)


# ------------------------------------------------------------------------------------------- the oracle and the restatements alone
@functools.lru_cache(maxsize=None)
def oracle_solve(station):
    """np_oracle.solve_batch on the station's lattice (return_all) -- the seeds of the host test's polishes"""
    c = build(station)
    A_, b_ = c['cinf'] if c['cinf'] is not None else (None, None)
    return O.solve_batch(c['x0'], c['u_prev'], c['kparams'], c['flags'], c['obs_xy'], A_, b_, c['P'], C=C, return_all=True)


def restate(station, mode, idx, u, J0, iters=ITERS):
    """(hist, ties) of the mode's restatement from the seeds u [n, 2, N] with cost J0 [n] of the scenarios idx"""
    c = build(station)
    fn = dict(fd=R.polish, adjoint=A.polish_adjoint, newton=NR.polish_newton)[mode]
    return fn(c, idx, u, J0, iters, c['P'], c['cinf'])


@functools.lru_cache(maxsize=None)
def restated(station, mode):
    """-> (idx, hist, ties) of the mode's restatement from the oracle's own winners, ITERS iterations; computed once"""
    r = oracle_solve(station)
    idx = np.flatnonzero(r['status'] == 0)
    hist, ties = restate(station, mode, idx, r['u'][idx], r['cost'][idx])
    return idx, hist, ties


def on_box(u, P):
    """[n] bool: plans u [n, 2, N] that hold an input exactly on a_min, a_max or +-df_max"""
    a, d = u[:, 0], u[:, 1]
    return ((a == P.a_min) | (a == P.a_max)).any(axis=-1) | (np.abs(d) == P.df_max).any(axis=-1)


def frozen_steering(c, idx):
    """[n, N]: the steering row every polished plan of a steer_rate_limit = 0 station must hold, bit for bit"""
    d = np.clip(c['u_prev'][idx, 1], -c['P'].df_max, c['P'].df_max)
    return np.broadcast_to(d[:, None], (len(idx), N))


def det_nonpos(station, iters=ITERS):
    """In how many (scenario, iteration) pairs of the Newton restatement riccati_direction meets a determinant <= 0 (or a
    non-finite one): it then returns a direction of zeros for the whole scenario, which a plan with a non-zero gradient cannot
    have otherwise."""
    c = build(station)
    idx, hist, _ = restated(station, 'newton')
    f = lambda k: c[k][idx]
    n = 0
    for it in range(iters):
        d = NR.newton_direction(f('x0'), f('kparams'), f('flags'), hist[it][0], c['P'])
        n += int((d == 0.0).all(axis=(1, 2)).sum())
    return n
