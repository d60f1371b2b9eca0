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
from parity_cases import LIMITS, LIMITS_F32_SEEDS as F32_SEEDS, LIMITS_N_SEEDS as N_SEEDS, limits_case, limits_cinf as _cinf, \
    limits_draw as _draw, limits_inputs as _inputs, limits_net as _net
from helpers import F32_EPS, F32_TIE, REL_TOL, compare_solve, floors, oracle_params, params_equal, rel_err, solver_track, verdict_margins

# every pruning switch the shipped library honours: no early exit, no Cartesian row skip, all acceleration rows, no incumbent
# bound; under the value-network cost also no value-bound pruning
PRUNE_OFF = DEV_NO_EARLY_EXIT | DEV_NO_FAR | DEV_ALL_ROWS | DEV_NO_BOUND
PRUNE_OFF_NET = PRUNE_OFF | DEV_NO_PRUNE

# Compared share of the draws (scenarios outside the set-asides; 1.0 where not listed), as measured, asserted less one scenario
# (or 0.02: helpers.share_floor).  Every f64 share below 0.95 is the near-tie rule alone, and every such draw is ramp-hold with a refinement pass:
# the re-centred pass spans a narrow interval around a winner pinned at a limit (steering rate 0.1 or 0.7, a clipped target),
# and neighbouring candidates with different controls land within 1e-9 of each other's cost.  Seed 20 (tracking family,
# feas_tol = 0) is the one f64 draw with threshold set-asides: two winners ride a limit exactly, g = 0.0 = feas_tol.  No f64
# scenario is set aside by a break-point.  f32: seeds 6 and 21 are near-ties too; seed 12 is one near-tie and five stage arguments within
# F32_EPS of a break-point (lattice, a_max = 20: the fast candidates cross the arc's ends).
SHARE = {('f64', 5): 0.875, ('f64', 6): 0.825, ('f64', 20): 0.95, ('f64', 21): 0.875, ('f64', 25): 0.875,
         ('f32', 6): 0.8, ('f32', 12): 0.914, ('f32', 15): 69 / 70, ('f32', 21): 0.85}


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


def _check(cfg, inp, dtype, golden_dir, monkeypatch, seed=0, share=1.0, tag='', xtol=None, min_solved=0, host=None):
    """Solve on the device (pruning on and off: the same bits) and compare with the oracle (helpers.compare_solve; share: the
    measured compared share, asserted less one scenario or 0.02).  -> the compared share.
    xtol: the trajectories' tolerance where a caller has measured that it must differ from the default (see its comment).
    host: the same draw as limits_case built it without a solver -- its oracle parameters must be the handle's."""
    f32 = dtype == 'f32'
    net = _net(cfg, golden_dir, seed)
    B, C = cfg['B'], cfg['C']
    # tracking family in float32: the steering is fed back from the float state (test_gpu_fuzz.py)
    tol, utol = (REL_TOL, 1e-7 if cfg['cand'] != 'track' else REL_TOL) if f32 else (1e-9, 1e-12)
    eps, tie = ((2e-5, 2e-5) if net else (F32_EPS, F32_TIE)) if f32 else (1e-9, 1e-9)
    tol_x = tol if xtol is None else xtol
    with_all = cfg['refine'] == 0
    got, allc, P, tk, cinf = _device(cfg, inp, dtype, net, 0, monkeypatch, with_all)
    if host is not None:
        assert params_equal(P, host['P']) and (cfg['cand'] != 'track' or tk == host['tk']), (vars(P), vars(host['P']), tk, host['tk'])
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
    m = compare_solve(got, passes, P, x0, kp, eps=eps, tie=tie, tol=tol, utol=utol, xtol=tol_x, ctol=2e-5 if f32 and net else tol,
                      share=share, tie_share=0.0, min_solved=min_solved, label=f'{tag} {dtype} {cfg["cand"]} N={cfg["N"]} C={C} '
                      f'dt={cfg["dt"]} {cfg["limits"]}')
    return m['compared'] / B


def _draw_check(seed, dtype, golden_dir, monkeypatch):
    cfg = _draw(seed)
    case = limits_case(seed, dtype)
    _check(cfg, _inputs(cfg, seed), dtype, golden_dir, monkeypatch, seed, SHARE.get((dtype, seed), 1.0), f'seed {seed}',
           min_solved=floors(case['key'])['min_solved'], host=case)


# ----------------------------------------------------------------------------- part 1: the seeded draws
@pytest.mark.gpu
@pytest.mark.parametrize('seed', range(N_SEEDS))
def test_limits_draw_matches_oracle(seed, golden_dir, monkeypatch):
    _draw_check(seed, 'f64', golden_dir, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize('seed', F32_SEEDS)
def test_limits_draw_matches_oracle_f32(seed, golden_dir, monkeypatch):
    _draw_check(seed, 'f32', golden_dir, monkeypatch)


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
    _check(cfg, inp, dtype, golden_dir, monkeypatch, share=share, tag=f'reach {lim}', xtol=xtol)


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
    _check(cfg, inp, dtype, golden_dir, monkeypatch, share=92 / 96, tag=f'slack {lim}')


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
        _check(cfg, inp, dtype, golden_dir, monkeypatch, share=1.0, tag=f'braking jerk={jerk}')
