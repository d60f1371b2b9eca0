"""-m gpu : the solver across the limits igt_params advertises, and its pruning at the edge of its proofs.

test_gpu_fuzz.py draws the discretisation and the families at (mostly) the reference's limits; the limits themselves choose
code paths (df_max < 0.78: the steering trig without range reduction) and feed every hand-derived bound that lets the search
skip work (igt_device.h obstacles_out_of_reach, progress_slack, the incumbent bound, the live acceleration rows).  Here a seeded
generator draws the limits as well -- speed and acceleration boxes, steering box, jerk and steering-rate limits, wheel base
split, feasibility tolerance, the tracking family's speed cap and envelope -- and stretches the inputs to them (previous
controls across the whole box, speeds at its ends, heading errors beyond pi/4).  Every draw must give the oracle's answer,
and the same bits with every pruning switch off (IGT_DEV_FLAGS).  Targeted batches then put obstacles and curvature
break-points exactly at the bounds' edges."""
import numpy as np
import pytest

import np_oracle as O
from igtmpc._lib import DEV_ALL_ROWS, DEV_NO_BOUND, DEV_NO_EARLY_EXIT, DEV_NO_FAR, DEV_NO_PRUNE
from helpers import F32_EPS, F32_TIE, REL_TOL, ambiguous_mask, oracle_params, rel_err, verdict_margins

LIMITS = {
    'v_min': (0.0, -1.0, -2.0),            # mpc.yaml ships -1.0; mpc.py:57 hard-codes 0
    'v_max': (5.0, 8.0, 15.0),
    'a_min': (-4.0, -1.5, -8.0),
    'a_max': (3.0, 6.0, 20.0),
    'df_max': (1.0, 0.6, 0.35),            # either side of the df_small switch (0.78)
    'jerk_limit': (0.9, 0.2, 0.02, 4.0),
    'steer_rate_limit': (0.7, 0.1, 2.0),
    'l_r_l_f': ((2.235, 2.235), (1.2, 3.0)),
    'feas_tol': (1e-6, 0.0, 1e-3),
    'track_vcap': (1.0, 0.0),
    'track_env': (1.0, 0.0, 0.5),
}
# every pruning switch the shipped library honours: no early exit, no Cartesian row skip, all acceleration rows, no incumbent
# bound; under the value-network cost also no value-bound pruning
PRUNE_OFF = DEV_NO_EARLY_EXIT | DEV_NO_FAR | DEV_ALL_ROWS | DEV_NO_BOUND
PRUNE_OFF_NET = PRUNE_OFF | DEV_NO_PRUNE

N_SEEDS = 32
F32_SEEDS = range(0, N_SEEDS, 3)
# Compared share of the draws (scenarios outside the set-asides; 1.0 where not listed), as measured, asserted less one scenario
# (or 0.02).  Every f64 share below 0.95 is the near-tie rule alone, and every such draw is ramp-hold with a refinement pass:
# the re-centred pass spans a narrow interval around a winner pinned at a limit (steering rate 0.1 or 0.7, a clipped target),
# and neighbouring candidates with different controls land within 1e-9 of each other's cost.  No f64 scenario is set aside by
# a threshold or a break-point.  f32: seeds 6 and 21 are near-ties too; seed 12 is one near-tie and five stage arguments within
# F32_EPS of a break-point (lattice, a_max = 20: the fast candidates cross the arc's ends).
SHARE = {('f64', 5): 0.875, ('f64', 6): 0.825, ('f64', 20): 0.95, ('f64', 21): 0.875, ('f64', 25): 0.875,
         ('f32', 6): 0.8, ('f32', 12): 0.914, ('f32', 15): 69 / 70, ('f32', 21): 0.85}


def _floor(share, B):
    return share - max(0.02, 1.0 / B)


def _choice(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def _draw(seed):
    rng = np.random.default_rng([1923, seed])
    cfg = dict(
        N=_choice(rng, (7, 12, 20, 33)),
        n_rk4=_choice(rng, (2, 4, 4)),
        dt=_choice(rng, (0.05, 0.1, 0.1, 0.2)),
        C=_choice(rng, (64, 256, 256)),
        cand=_choice(rng, ('lattice', 'ramp_hold', 'track', 'track')),
        n_obs=_choice(rng, (0, 1, 1, 2)),
        B=_choice(rng, (8, 24, 40, 70)),
        terminal=bool(rng.random() < 0.6),
    )
    lim = {k: _choice(rng, v) for k, v in LIMITS.items() if k not in ('l_r_l_f', 'track_vcap', 'track_env')}
    lim['l_r'], lim['l_f'] = _choice(rng, LIMITS['l_r_l_f'])
    vcap, env = _choice(rng, LIMITS['track_vcap']), _choice(rng, LIMITS['track_env'])
    # the first seeds are pinned to the corners that must be reached whatever the generator draws: the tracking family with
    # the speed cap off and accelerations above the device's old clipped cap (a_max = 20; jerk_limit = 0.02), and with v_min < 0
    if seed in (0, 1, 2):
        cfg['cand'] = 'track'
    if seed == 0:
        lim['a_max'], lim['jerk_limit'], vcap, cfg['dt'] = 20.0, 0.9, 0.0, 0.1
    if seed == 1:
        lim['jerk_limit'], vcap = 0.02, 0.0
    if seed == 2:
        lim['v_min'] = -2.0
    if seed == 3:
        lim['feas_tol'] = 0.0
    if cfg['cand'] == 'track':
        lim['track_vcap'], lim['track_env'] = vcap, env
    cfg['refine'] = _choice(rng, (0, 0, 1)) if cfg['cand'] != 'lattice' else 0
    if seed in (0, 1):          # rollout_all compares every candidate's controls (first pass only)
        cfg['refine'] = 0
    cfg['net'] = _choice(rng, (0, 0, 0, 1, 3)) if cfg['n_obs'] == 1 else 0
    while cfg['B'] * cfg['C'] * cfg['N'] * cfg['n_rk4'] * (1 + cfg['refine']) > 2.5e7:     # the numpy oracle: about a second
        cfg['B'] //= 2
    cfg['limits'] = lim
    return cfg


# (dt, jerk_limit) pairs whose terminal set has more facets than IGT_MAX_CINF = 256: the fixed point converges at every drawn
# pair, but at a slow jerk ramp the polygon keeps one edge per step (dt = 0.05: 982 facets at jerk 0.02, 312 at 0.2;
# dt = 0.1, jerk 0.02: 492) -- and takes minutes to compute.  Those draws run without the terminal set.
CINF_TOO_LARGE = {(0.05, 0.02), (0.1, 0.02), (0.05, 0.2)}


def _cinf(cfg):
    """The terminal set at the drawn (dt, jerk), or (None, None)."""
    from igtmpc.cinf import cinf_halfplanes
    jerk = cfg['limits'].get('jerk_limit', 0.9)
    if not cfg['terminal'] or (cfg['dt'], jerk) in CINF_TOO_LARGE:
        return None, None
    A, b = cinf_halfplanes(dt=cfg['dt'], jerk=jerk, **cfg.get('cinf_kw', {}))
    assert len(b) <= 256
    return A, b


def _inputs(cfg, seed):
    """make_batch's scenes (routes, curvature, opponents) with the ego's state and previous controls stretched to the limits:
    u_prev across [a_min, a_max] x [-df_max, df_max], speeds across [v_min, v_max] with a fifth of them within 0.1 of either end,
    and a sixth of the heading errors beyond pi/4.  float64 arrays."""
    from igtmpc.scenarios import make_batch
    N, dt, B, lim = cfg['N'], cfg['dt'], cfg['B'], cfg['limits']
    b = make_batch(max(B, 8), N=N, dt=dt, seed=300 + seed, dtype=np.float64)
    b = {k: np.ascontiguousarray(v[:B]) for k, v in b.items() if isinstance(v, np.ndarray) and len(v) >= B}
    rng = np.random.default_rng([11, seed])
    v_min, v_max = lim.get('v_min', 0.0), lim.get('v_max', 5.0)
    a_min, a_max, df_max = lim.get('a_min', -4.0), lim.get('a_max', 3.0), lim.get('df_max', 1.0)
    u_prev = np.stack([rng.uniform(a_min, a_max, B), rng.uniform(-df_max, df_max, B)], axis=-1)
    u_prev[0:2, 0] = a_max - 0.02 * (a_max - a_min), a_min + 0.02 * (a_max - a_min)     # the box's ends in rollout_all's scenarios
    x0 = b['x0'].copy()
    v0 = rng.uniform(v_min, v_max, B)
    v0[0::5] = v_min + rng.uniform(0.0, 0.1, len(v0[0::5]))
    v0[1::5] = v_max - rng.uniform(0.0, 0.1, len(v0[1::5]))
    x0[:, 5] = v0
    i = np.arange(2, B, 6)
    dep = np.where(rng.random(len(i)) < 0.5, -1.0, 1.0) * rng.uniform(0.8, 1.3, len(i)) - x0[i, 4]
    x0[i, 4] += dep
    x0[i, 6] += dep
    obs = b['obs_xy']
    if cfg['n_obs'] == 0:
        obs = np.zeros((B, 0, 2, N + 1))
    elif cfg['n_obs'] == 2:                                    # a second vehicle 9 m behind the first along its path
        lag = obs.copy()
        lag[:, 0, 0, :] -= 9.0 * np.cos(0.3 * np.arange(B))[:, None]
        lag[:, 0, 1, :] -= 9.0 * np.sin(0.3 * np.arange(B))[:, None]
        obs = np.concatenate([obs, lag], axis=1)
    return dict(x0=x0, u_prev=u_prev, kparams=b['kparams'], flags=b['flags'], obs=np.ascontiguousarray(obs), u_ws=None,
                tv_sv=b['tv_sv'], enc=b['enc'])


def _net(cfg, golden_dir, seed):
    if not cfg['net']:
        return None
    v = np.load(f'{golden_dir}/value_net_golden.npz')
    layers, i = [], 0
    while f"sc{cfg['net']}_W{i}" in v:
        layers.append((v[f"sc{cfg['net']}_W{i}"], v[f"sc{cfg['net']}_b{i}"]))
        i += 1
    rng = np.random.default_rng([13, seed])
    return dict(layers=layers, Wn=np.eye(6) + 0.05 * rng.normal(size=(6, 6)),
                mu_f=np.array([20.0, 2.5, 0.0, 0.0, 0.0, 0.0]) + 0.1 * rng.normal(size=6), sigma_t=float(_choice(rng, (1.0, -2.0))),
                mu_t=float(rng.normal()))


def _device(cfg, inp, dtype, net, flags_env, monkeypatch, with_all):
    import igtmpc
    npdt = np.float32 if dtype == 'f32' else np.float64
    c = lambda k: None if inp[k] is None else np.ascontiguousarray(inp[k].astype(npdt))
    extra = (c('tv_sv'), c('enc')) if net else ()
    monkeypatch.setenv('IGT_DEV_FLAGS', str(flags_env))
    try:
        with igtmpc.BatchSolver(N=cfg['N'], dt=cfg['dt'], n_rk4=cfg['n_rk4'], C=cfg['C'], n_obs=cfg['n_obs'], dtype=dtype,
                                cand_mode=cfg['cand'], refine_iters=cfg['refine'], cost_mode='value_net' if net else 'progress',
                                **cfg['limits']) as s:
            cinf = _cinf(cfg)
            if cinf[0] is not None:
                s.set_cinf(*cinf)
            if net:
                s.set_value_net(**net)
            got = s.solve(c('x0'), c('u_prev'), c('kparams'), inp['flags'], c('obs'), *extra, u_ws=c('u_ws'))
            allc = None
            if with_all:
                n = min(cfg['B'], 4)
                allc = s.rollout_all(c('x0')[:n], c('u_prev')[:n], c('kparams')[:n], inp['flags'][:n], c('obs')[:n],
                                     *[e[:n] for e in extra], u_ws=None if inp['u_ws'] is None else c('u_ws')[:n])
            P = oracle_params(s)
            tk = dict(ke=s.params.track_ke, span=s.params.track_span, blim=s.params.track_beta_lim, env=s.params.track_env,
                      vcap=s.params.track_vcap)
    finally:
        monkeypatch.delenv('IGT_DEV_FLAGS')
    return got, allc, P, tk, cinf


def _check(cfg, inp, dtype, golden_dir, monkeypatch, seed=0, floor=None, tag='', xtol=None):
    """Solve on the device (pruning on and off: the same bits) and compare with the oracle.  -> the compared share.
    xtol: the trajectories' tolerance where a caller has measured that it must differ from the default (see its comment)."""
    f32 = dtype == 'f32'
    net = _net(cfg, golden_dir, seed)
    B, C = cfg['B'], cfg['C']
    # tracking family in float32: the steering is fed back from the float state (test_gpu_fuzz.py)
    tol, utol = (REL_TOL, 1e-7 if cfg['cand'] != 'track' else REL_TOL) if f32 else (1e-9, 1e-12)
    eps, tie = ((2e-5, 2e-5) if net else (F32_EPS, F32_TIE)) if f32 else (1e-9, 1e-9)
    tol_x = tol if xtol is None else xtol
    with_all = cfg['refine'] == 0
    got, allc, P, tk, cinf = _device(cfg, inp, dtype, net, 0, monkeypatch, with_all)
    off, _, _, _, _ = _device(cfg, inp, dtype, net, PRUNE_OFF_NET if net else PRUNE_OFF, monkeypatch, False)
    for k in ('x', 'u', 'cost', 'argmin', 'status'):
        assert np.array_equal(got[k], off[k], equal_nan=True), (tag, 'pruning off changes', k, cfg)

    npdt = np.float32 if f32 else np.float64
    f = lambda k: None if inp[k] is None else inp[k].astype(npdt).astype(np.float64)     # the device's inputs, exactly
    o = f('obs') if cfg['n_obs'] else None
    kw = dict(net=net, tv_sv=f('tv_sv'), enc=f('enc')) if net else {}
    if cfg['cand'] == 'lattice':
        passes = [O.solve_batch(f('x0'), f('u_prev'), f('kparams'), inp['flags'], o, cinf[0], cinf[1], P, C=C, return_all=True,
                                **kw)]
    else:
        passes = O.solve_batch_refined(f('x0'), f('u_prev'), f('kparams'), inp['flags'], o, cinf[0], cinf[1], P, C=C,
                                       refine_iters=cfg['refine'], cand=cfg['cand'], track=tk, u_ws=f('u_ws'), **kw)
    ref, first = passes[-1], passes[0]
    x0 = O.apply_flags(f('x0'), inp['flags'])[:, None, :]
    kp = f('kparams')[:, None, :]
    if with_all:     # every candidate of the first scenarios: controls, trajectories, verdicts family by family
        n = min(B, 4)
        bp = O.breakpoint_distance(x0[:n], first['U'][:n], kp[:n], P)
        clear = bp > eps
        if f32:      # float32 error grows with the excursion: roll-outs that stay near the lane (every feasible one does)
            clear &= (np.abs(first['X'][:n, :, 3, :]).max(axis=-1) <= 1.0) & (np.abs(first['X'][:n, :, 4, :]).max(axis=-1) <= 0.5)
        if clear.any():
            assert rel_err(allc['U'][clear], first['U'][:n][clear]).max() <= utol, (tag, cfg)
        # ... and clear of the model's pole 1 - K e_y = 0 (test_gpu_fuzz.py)
        pole = np.abs(1.0 - kp[:n, :, 2:3] * first['X'][:n, :, 3, :]).min(axis=-1) > 0.1
        fin = clear & pole & np.isfinite(first['X'][:n]).all(axis=(-1, -2))
        assert (first['feas'][:n] <= pole).all()
        if fin.any():
            assert rel_err(allc['X'][fin], first['X'][:n][fin]).max() <= tol_x, (tag, cfg)
        gm = verdict_margins(first['X'][:n], first['U'][:n], None if o is None else o[:n, None], cinf[0], cinf[1], P)
        vmargin = 1e-6 if f32 else 1e-9
        for fam, bit in ((0, 1), (1, 2), (3, 8), (4, 16), (5, 32)):
            away = fin & (np.abs(gm[..., fam] - P.feas_tol) > vmargin)
            assert (((allc['viol'] & bit) != 0) == (gm[..., fam] > P.feas_tol))[away].all(), (tag, 'verdict bit', bit, cfg)
        thr = fin & (np.abs(first['g'][:n] - P.feas_tol) > vmargin)
        assert ((allc['viol'] == 0) == first['feas'][:n])[thr].all(), (tag, cfg)
    # the solve: set aside a scenario that ANY pass decided inside eps of a threshold, a near-tie or a break-point
    amb = np.zeros(B, dtype=bool)
    for r in passes:
        amb |= ambiguous_mask(r, P, eps, tie, eps, O.breakpoint_distance(x0, r['U'], kp, P))
    ok = ~amb
    assert (got['status'][ok] == ref['status'][ok]).all(), (tag, cfg)
    assert (got['argmin'][ok] == ref['argmin'][ok]).all(), (tag, cfg)
    sol = ok & (ref['status'] == 0)
    if sol.any():
        assert rel_err(got['x'][sol], ref['x'][sol]).max() <= tol_x, (tag, cfg)
        assert rel_err(got['u'][sol], ref['u'][sol]).max() <= max(tol, utol), (tag, cfg)
        assert rel_err(got['cost'][sol], ref['cost'][sol]).max() <= (2e-5 if f32 and net else tol), (tag, cfg)
    bad = got['status'] == 1
    assert np.isnan(got['x'][bad]).all() and np.isinf(got['cost'][bad]).all() and (got['argmin'][bad] == -1).all()
    share = ok.mean()
    print(f'{tag} {dtype}: compared share {share:.3f} ({ok.sum()}/{B}), solved {(got["status"] == 0).mean():.2f}  '
          f'{cfg["cand"]} N={cfg["N"]} C={C} dt={cfg["dt"]} {cfg["limits"]}')
    if floor is not None:
        assert share >= floor, (tag, share, cfg)
    return share


# ----------------------------------------------------------------------------- part 1: the seeded draws
@pytest.mark.gpu
@pytest.mark.parametrize('seed', range(N_SEEDS))
def test_limits_draw_matches_oracle(seed, golden_dir, monkeypatch):
    cfg = _draw(seed)
    _check(cfg, _inputs(cfg, seed), 'f64', golden_dir, monkeypatch, seed, _floor(SHARE.get(('f64', seed), 1.0), cfg['B']),
           f'seed {seed}')


@pytest.mark.gpu
@pytest.mark.parametrize('seed', F32_SEEDS)
def test_limits_draw_matches_oracle_f32(seed, golden_dir, monkeypatch):
    cfg = _draw(seed)
    _check(cfg, _inputs(cfg, seed), 'f32', golden_dir, monkeypatch, seed, _floor(SHARE.get(('f32', seed), 1.0), cfg['B']),
           f'seed {seed}')


def _old_device_cap(cfg):
    """The finite cap the device used to apply with the speed cap off: D clipped at 1000 gives about sqrt(2000 dt jerk)."""
    return np.sqrt(2000.0 * cfg['dt'] * cfg['limits'].get('jerk_limit', 0.9))


def test_the_limit_draws_cover_the_table():
    cfgs = [_draw(s) for s in range(N_SEEDS)]
    for k, vals in LIMITS.items():
        if k == 'l_r_l_f':
            got = {(c['limits']['l_r'], c['limits']['l_f']) for c in cfgs}
        elif k.startswith('track_'):
            got = {c['limits'][k] for c in cfgs if c['cand'] == 'track'}
        else:
            got = {c['limits'][k] for c in cfgs}
        assert got == set(vals), (k, got)
    assert {c['limits']['df_max'] < 0.78 for c in cfgs} == {True, False}                # both df_small builds
    assert {c['limits']['df_max'] < 0.78 for c in cfgs if c['cand'] == 'track'} == {True, False}
    assert {c['cand'] for c in cfgs} == {'lattice', 'ramp_hold', 'track'} and {c['n_obs'] for c in cfgs} == {0, 1, 2}
    assert {c['terminal'] for c in cfgs} == {True, False} and any(c['refine'] for c in cfgs) and any(c['net'] for c in cfgs)
    off = [(s, c) for s, c in enumerate(cfgs) if c['cand'] == 'track' and c['limits']['track_vcap'] == 0.0]
    for pick in (lambda c: c['limits']['a_max'] == 20.0, lambda c: c['limits']['jerk_limit'] == 0.02):
        assert any(pick(c) and (_inputs(c, s)['u_prev'][:4, 0] > _old_device_cap(c)).any() for s, c in off)     # rollout_all's
    assert any(c['cand'] == 'track' and c['limits']['v_min'] < 0 for c in cfgs)
    assert any(c['limits']['feas_tol'] == 0.0 for c in cfgs)
    f32 = [cfgs[s] for s in F32_SEEDS]
    assert {c['cand'] for c in f32} == {'lattice', 'ramp_hold', 'track'} and {c['limits']['df_max'] < 0.78 for c in f32} == {True, False}
    for c in cfgs:
        assert c['B'] * c['C'] * c['N'] * c['n_rk4'] * (1 + c['refine']) <= 2.5e7


# ----------------------------------------------------------------------------- part 2: pruning at the edge of its proofs
def _base_cfg(**kw):
    cfg = dict(N=20, n_rk4=4, dt=0.1, C=256, cand='track', n_obs=1, B=64, terminal=True, refine=0, net=0, limits={})
    cfg.update(kw)
    return cfg


def _reach(lim, N, dt, d_min=5.6):
    """obstacles_out_of_reach (igt_device.h): a speed-feasible candidate moves at most
    (max(|v_min|, |v_max|) + max(|a_min|, |a_max|) dt) N dt, plus a metre to spare; an obstacle further than d_min + that
    from the start at every step cannot collide."""
    vabs = max(abs(lim.get('v_min', 0.0)), abs(lim.get('v_max', 5.0)))
    aabs = max(abs(lim.get('a_min', -4.0)), abs(lim.get('a_max', 3.0)))
    return d_min + (vabs + aabs * dt) * (N * dt) + 1.0


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('cand', ['lattice', 'track'])
@pytest.mark.parametrize('lim', [dict(v_min=-2.0, v_max=5.0), dict(v_min=-1.0, a_min=-8.0, a_max=3.0),
                                 dict(v_min=0.0, v_max=15.0, a_min=-1.5, a_max=20.0, jerk_limit=4.0)])
def test_obstacles_at_the_reach_bound(lim, cand, dtype, golden_dir, monkeypatch):
    """Obstacles parked at obstacles_out_of_reach's bound computed from the limits, +-1e-6 and +-0.5 m, the start speeds
    across the whole box: the row skip (off: 65536) changes nothing, and the solve is the oracle's."""
    cfg = _base_cfg(cand=cand, limits=dict(lim), B=128)
    inp = _inputs(cfg, 7)
    r = _reach(lim, cfg['N'], cfg['dt']) + np.tile(np.array([-0.5, -1e-6, 1e-6, 0.5]), cfg['B'] // 4)
    ang = np.linspace(0, 2 * np.pi, cfg['B'], endpoint=False)
    obs = inp['obs'].copy()
    obs[:, 0, 0, :] = (inp['x0'][:, 0] + r * np.cos(ang))[:, None]
    obs[:, 0, 1, :] = (inp['x0'][:, 1] + r * np.sin(ang))[:, None]
    if dtype == 'f32':        # the device reads float obstacles: put them where the float32 positions sit
        obs = obs.astype(np.float32).astype(np.float64)
    inp['obs'] = obs
    share = 126 / 128 if (dtype, cand, lim.get('a_max')) == ('f32', 'lattice', 20.0) else 1.0      # two break-point set-asides
    # float32 tracking family at v_max = 15, a_max = 20, jerk_limit = 4: the steering is fed back from the float state, and the
    # roll-outs' difference grows with speed times horizon -- measured 2.8e-5 (relative, |ref| floored at 1) on this batch,
    # against the 1e-5 that holds at the reference's limits and in every draw above.  The bar here is 5e-5.
    xtol = 5e-5 if (dtype, cand, lim.get('a_max')) == ('f32', 'track', 20.0) else None
    _check(cfg, inp, dtype, golden_dir, monkeypatch, floor=_floor(share, cfg['B']), tag=f'reach {lim}', xtol=xtol)


def _slack(lim, N, dt, kv):
    """progress_slack (igt_device.h): -> (q = |kv| ey_b, reach of the stage arguments); the bound is off from q >= 0.5."""
    vabs = max(abs(lim.get('v_min', 0.0)), abs(lim.get('v_max', 5.0))) + lim.get('feas_tol', 1e-6) + \
        max(abs(lim.get('a_min', -4.0)), abs(lim.get('a_max', 3.0))) * dt
    eyb = lim.get('ey_lim', 0.2) + lim.get('feas_tol', 1e-6) + 1.5 * dt * vabs
    q = abs(kv) * eyb
    return q, (N + 1) * dt * vabs / (1.0 - q) if q < 0.5 else np.inf


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('lim', [{}, dict(v_min=-1.0, v_max=8.0, a_min=-8.0, feas_tol=1e-3)])
def test_progress_slack_at_its_edges(lim, dtype, golden_dir, monkeypatch):
    """Tracking family, incumbent bound: curvature break-points placed so that s_0 +- reach (progress_slack's) sits just inside
    or just outside [b0, b1) -- the bound's lam is 1 or 1 / (1 - q) --, and curvatures with q = |kv| ey_b either side of 0.5,
    where progress_slack turns the bound off.  No incumbent bound (8388608, with every other switch) gives the same bits, and
    the solve is the oracle's."""
    cfg = _base_cfg(limits=dict(lim), B=96)
    N, dt = cfg['N'], cfg['dt']
    inp = _inputs(cfg, 8)
    eyb = _slack(lim, N, dt, 1.0)[0]
    s0 = inp['x0'][:, 2]
    kp = np.empty((cfg['B'], 3))
    for i in range(cfg['B']):
        case, side = divmod(i, 12)
        if case < 4:        # a modest curvature; the arc begins / ends at s0 +- reach, +- 1e-6 and +- 0.3
            kv = (0.08, -0.15, 0.2, -0.05)[case]
            reach = _slack(lim, N, dt, kv)[1]
            d = (-0.3, -1e-6, 0.0, 1e-6, 0.3, 2.0)[side % 6]
            if side < 6:
                kp[i] = (s0[i] + reach + d, s0[i] + reach + d + 30.0, kv)
            else:
                kp[i] = (s0[i] - reach - 40.0 + d, s0[i] - reach + d, kv)
        else:               # q either side of 0.5, the arc over the start
            q = (0.45, 0.499, 0.4999999, 0.5, 0.5000001, 0.501, 0.55, 0.9)[2 * (case - 4) + side // 6] * (1.0 if side % 2 else -1.0)
            kp[i] = (s0[i] - 5.0 + side, s0[i] + 60.0, q / eyb)
    inp['kparams'] = kp
    inp['x0'][:, 3] *= 0.2          # a lane error this curvature's feasible roll-outs can hold
    # four scenarios set aside by the break-point rule: side 5 of the q cases puts b0 on s_0 itself
    _check(cfg, inp, dtype, golden_dir, monkeypatch, floor=_floor(92 / 96, cfg['B']), tag=f'slack {lim}')


@pytest.mark.gpu
@pytest.mark.parametrize('jerk', [0.9, 4.0])
def test_f32_incumbent_bound_with_braking_to_a_negative_terminal_speed(jerk, golden_dir, monkeypatch):
    """The float32 search sums |v| along the UNCAPPED acceleration recurrence when v_min >= 0 (igt_fast_impl.inc); v_N is not
    box-checked, so with a_min = -8 the last term can fall short by |a_min| dt.  Tracking family, speed cap on, starts near
    v_max so that the top rows ride the cap, a terminal set that admits v < 0 with a = -8, warm starts that brake hard in the
    last steps: the incumbent bound off (8388608) gives the same bits, and the solve is the oracle's."""
    cfg = _base_cfg(dt=0.2, B=96, limits=dict(v_min=0.0, v_max=5.0, a_min=-8.0, a_max=3.0, jerk_limit=jerk), cinf_kw=dict(a_lo=-8.0))
    N, dt = cfg['N'], cfg['dt']
    inp = _inputs(cfg, 9)
    rng = np.random.default_rng(9)
    B = cfg['B']
    inp['x0'][:, 5] = 5.0 - rng.uniform(0.0, 0.3, B)
    inp['x0'][B // 2:, 5] = rng.uniform(0.5, 2.0, B - B // 2)           # slow starts: braking reaches v = 0 inside the horizon
    inp['u_prev'][:, 0] = rng.uniform(-1.0, 3.0, B)
    ws = np.empty((B, 2, N))
    ws[:, 1, :] = inp['u_prev'][:, 1:2]
    ramp = np.clip(np.arange(N, dtype=np.float64) - (N - 1 - rng.integers(2, 8, B))[:, None], 0, None)
    ws[:, 0, :] = np.clip(inp['u_prev'][:, 0:1] - dt * jerk * ramp, -8.0, 3.0)
    inp['u_ws'] = ws
    inp['flags'] = inp['flags'] | np.where(np.arange(B) % 4 != 0, 2, 0).astype(np.uint32)
    for dtype in ('f32', 'f64'):
        _check(cfg, inp, dtype, golden_dir, monkeypatch, floor=_floor(1.0, cfg['B']), tag=f'braking jerk={jerk}')
