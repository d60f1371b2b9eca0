"""Inputs of the solve-against-oracle comparisons, built without a solver (tests only).

Every GPU test that compares a solve with the oracle through helpers.compare_solve takes its inputs from a builder here (the seeded draws of
test_gpu_fuzz.py and test_gpu_limits.py included): a `case` dict with the solver's arguments, the device-typed
arrays and the oracle's parameters.  tests/test_parity_floors_host.py and tools/parity_floors.py run the oracle alone on the same
cases (all_cases), so the shares and solved counts recorded in tests/golden/parity_floors.json cannot drift from the inputs."""
import os

import numpy as np

import np_oracle as O
from helpers import F32_EPS, F32_TIE, REL_TOL, compare_solve, floors, host_params, host_track, measure, oracle_params, \
    params_equal, solver_track

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# Limits under which a lattice of constant rates has feasible members over a long horizon.  At the reference's limits
# (ey_lim = 0.2, steering rate 0.7) every column of an even G drifts at least steer_rate dt / 15 per step and has left the lane
# after 64 steps: 99 % of the candidates fail the e_y verdict and 87 % the speed box, and nothing is left to compare.
LONG_LIMITS = dict(ey_lim=1.5, v_max=12.0, steer_rate_limit=0.1)


def nets(sc):
    v = np.load(os.path.join(GOLDEN, 'value_net_golden.npz'))
    layers, i = [], 0
    while f'sc{sc}_W{i}' in v:
        layers.append((v[f'sc{sc}_W{i}'], v[f'sc{sc}_b{i}']))
        i += 1
    return layers


def cinf_default():
    from igtmpc.cinf import cinf_halfplanes
    return cinf_halfplanes()


def _npdt(dtype):
    return np.float64 if dtype == 'f64' else np.float32


def make_case(key, dtype, args, *, N=20, dt=0.1, n_rk4=4, C=256, n_obs=1, cand='lattice', refine=0, limits=None, net=None,
              cinf=None, eps, tie, tol, utol=1e-7, ctol=None, use_bp=True, first=False, crossing=0, need=0, table=None):
    """args: dict(x0, u_prev, kparams, flags, obs[, u_ws, tv_sv, enc]) in the device's dtype.  first: the first pass alone is
    compared as well (key + '/first').  crossing: compared winners that must cross a break-point.  need: the least the recorded
    min_solved may be.  table: the controls [C, 2, N] of cand = 'table'."""
    limits = dict(limits or {})
    return dict(key=key, dtype=dtype, args=args, B=len(args['flags']), N=N, dt=dt, n_rk4=n_rk4, C=C, n_obs=n_obs, cand=cand,
                refine=refine, limits=limits, net=net, cinf=cinf, P=host_params(N=N, dt=dt, n_rk4=n_rk4, **limits),
                tk=host_track(**limits), eps=eps, tie=tie, tol=tol, utol=utol, ctol=ctol, use_bp=use_bp, first=first,
                crossing=crossing, need=need, table=table)


def subcase(case, refine, suffix):
    """The same inputs with another number of refinement passes."""
    return dict(case, refine=refine, key=case['key'] + suffix, first=False)


def oracle_passes(case):
    """-> (passes, x0[B,1,7] with the flags applied, kp[B,1,3]): the float64 oracle on exactly the device's inputs."""
    a = case['args']
    f = lambda k: None if a.get(k) is None else np.asarray(a[k], dtype=np.float64)
    A, b = case['cinf'] if case['cinf'] is not None else (None, None)
    kw = dict(net=case['net'], tv_sv=f('tv_sv'), enc=f('enc')) if case['net'] else {}
    obs = f('obs') if case['n_obs'] else None
    if case['cand'] in ('lattice', 'table'):
        U = None if case['cand'] == 'lattice' else np.broadcast_to(case['table'], (case['B'],) + case['table'].shape)
        passes = [O.solve_batch(f('x0'), f('u_prev'), f('kparams'), a['flags'], obs, A, b, case['P'], C=case['C'], U=U,
                                return_all=True, **kw)]
    else:
        passes = O.solve_batch_refined(f('x0'), f('u_prev'), f('kparams'), a['flags'], obs, A, b, case['P'], C=case['C'],
                                       refine_iters=case['refine'], cand=case['cand'], track=case['tk'], u_ws=f('u_ws'), **kw)
    return passes, O.apply_flags(f('x0'), a['flags'])[:, None, :], f('kparams')[:, None, :]


def oracle_passes_quiet(case):
    """oracle_passes on inputs that hold NaN and inf on purpose (tests/nonfinite_cases.py): numpy's warnings say nothing there."""
    with np.errstate(all='ignore'):
        return oracle_passes(case)


def measure_case(case, oracle=None):
    """The oracle alone -> {key: measured dict} (two entries where the first pass is compared as well)."""
    with np.errstate(all='ignore'):      # (the poisoned inputs of tests/nonfinite_cases.py hold NaN and inf on purpose)
        passes, x0, kp = oracle_passes(case) if oracle is None else oracle
        out = {case['key']: measure(passes, case['P'], x0, kp, case['eps'], case['tie'], case['use_bp'])[0]}
        if case['first']:
            out[case['key'] + '/first'] = measure(passes[:1], case['P'], x0, kp, case['eps'], case['tie'], case['use_bp'])[0]
    return out


def check_case(case, got, oracle, first=False):
    """compare_solve with the case's tolerances and its recorded floors; first: `got` is the first pass's solve."""
    passes, x0, kp = oracle
    key = case['key'] + ('/first' if first else '')
    fl = floors(key)
    return compare_solve(got, passes[:1] if first else passes, case['P'], x0, kp, eps=case['eps'], tie=case['tie'],
                         tol=case['tol'], utol=case['utol'], ctol=case['ctol'], use_bp=case['use_bp'],
                         crossing=0 if first else case['crossing'], label=key, **fl)


def open_solver(igt, case, refine=None, **kw):
    """The case's BatchSolver (terminal set and value network loaded); its parameters must be the ones the oracle runs with."""
    s = igt.BatchSolver(N=case['N'], dt=case['dt'], n_rk4=case['n_rk4'], C=case['C'], n_obs=case['n_obs'], dtype=case['dtype'],
                        cand_mode=case['cand'], refine_iters=case['refine'] if refine is None else refine,
                        cost_mode='value_net' if case['net'] else 'progress', **case['limits'], **kw)
    try:
        assert params_equal(oracle_params(s), case['P']), (vars(oracle_params(s)), vars(case['P']))
        assert case['cand'] != 'track' or solver_track(s) == case['tk'], (solver_track(s), case['tk'])
        if case['cinf'] is not None:
            s.set_cinf(*case['cinf'])
        if case['net']:
            s.set_value_net(**case['net'])
        if case['table'] is not None:
            s.set_candidate_table(case['table'])
    except BaseException:
        s.close()
        raise
    return s


def solve_args(case, n=None):
    a = case['args']
    sl = slice(None) if n is None else slice(0, n)
    pos = [a['x0'][sl], a['u_prev'][sl], a['kparams'][sl], a['flags'][sl], a['obs'][sl]]
    if case['net']:
        pos += [a['tv_sv'][sl], a['enc'][sl]]
    return pos, dict(u_ws=None if a.get('u_ws') is None else a['u_ws'][sl])


def device_solve(s, case):
    pos, kw = solve_args(case)
    return s.solve(*pos, **kw)


def _batch_args(b, obs=None, **more):
    a = dict(x0=b['x0'], u_prev=b['u_prev'], kparams=b['kparams'], flags=b['flags'], obs=b['obs_xy'] if obs is None else obs,
             tv_sv=b['tv_sv'], enc=b['enc'], u_ws=None)
    a.update(more)
    return a


def _bars(dtype, eps32=2e-5, tie32=None):
    """(tol, eps, tie): DESIGN.md section 6."""
    if dtype == 'f64':
        return 1e-9, 1e-9, 1e-9
    return REL_TOL, eps32, eps32 if tie32 is None else tie32


# ----------------------------------------------------------------------------- test_gpu_parity.py
def solve_case(dtype):
    from igtmpc.scenarios import make_batch
    tol, eps, tie = _bars(dtype, F32_EPS, F32_TIE)
    return make_case(f'solve[{dtype}]', dtype, _batch_args(make_batch(512, dtype=_npdt(dtype))), cinf=cinf_default(),
                     eps=eps, tie=tie, tol=tol)


def value_net_case(sc, dtype):
    """The shipped checkpoints with a non-trivial whitening / de-normalisation (synthetic: the reference's statistics are not
    shipped)."""
    from igtmpc.scenarios import make_batch
    rng = np.random.default_rng(5)
    Wn = np.eye(6) + 0.05 * rng.normal(size=(6, 6))
    mu_f = np.array([20.0, 2.5, 0.0, 0.0, 0.0, 0.0]) + 0.1 * rng.normal(size=6)
    net = dict(layers=nets(sc), Wn=Wn, mu_f=mu_f, sigma_t=3.0, mu_t=-1.5)
    tol, eps, tie = _bars(dtype)
    return make_case(f'value_net[{sc}-{dtype}]', dtype, _batch_args(make_batch(160, dtype=_npdt(dtype))), net=net,
                     cinf=cinf_default(), eps=eps, tie=tie, tol=tol)


def ramp_hold_refined_case(dtype):
    from igtmpc.scenarios import make_batch
    tol, eps, tie = _bars(dtype)
    return make_case(f'ramp_hold_refined[{dtype}]', dtype, _batch_args(make_batch(384, dtype=_npdt(dtype))), cand='ramp_hold',
                     refine=2, cinf=cinf_default(), eps=eps, tie=tie, tol=tol, first=True)


SHAPES_F64 = [(10, 4, 256, 1), (40, 4, 64, 1), (20, 7, 64, 1), (20, 4, 1024, 1), (20, 4, 256, 0), (20, 2, 256, 2), (64, 4, 256, 1),
              (64, 4, 64, 3), (64, 3, 1024, 1), (20, 4, 256, 4), (20, 4, 256, 3), (33, 4, 256, 1)]
SHAPES_F32 = [(10, 4, 256, 1), (40, 4, 64, 1), (20, 7, 64, 1), (20, 4, 1024, 1), (20, 4, 256, 0), (20, 2, 256, 2), (20, 1, 256, 1),
              (64, 4, 256, 1), (64, 4, 64, 3), (20, 4, 256, 4), (33, 4, 256, 1)]
LONG_N = 40           # from this horizon on the shape tests and the fuzz run the lattice families at LONG_LIMITS


def shape_case(dtype, N, n_rk4, C, n_obs):
    """24 (f64) / 48 (f32) scenarios at another discretisation; further vehicles are the first one's forecast, displaced.
    N >= LONG_N: at LONG_LIMITS, and at least one compared winner must cross a curvature break-point.  N = 33 is the
    mid-length horizon that is solved at the reference's own limits."""
    from igtmpc.scenarios import make_batch
    # (48 scenarios at the long horizons in f64 as well: of 24, no winner of (64, 4, 64, 3) crosses a break-point)
    b = make_batch(24 if dtype == 'f64' and N < LONG_N else 48, dtype=_npdt(dtype), N=N)
    obs = np.concatenate([b['obs_xy']] * max(n_obs, 1), axis=1)[:, :n_obs]
    for m in range(1, n_obs):
        obs[:, m, 0] += 3.0 * m
        obs[:, m, 1] -= 2.0 * (m - 1)
    tol, eps, tie = _bars(dtype)
    long = N >= LONG_N
    # (the f64 test has never used the break-point set-aside: the f64 kernels take the oracle's side of every switch)
    return make_case(f'other_shapes_{dtype}[{N}-{n_rk4}-{C}-{n_obs}]', dtype, _batch_args(b, np.ascontiguousarray(obs)), N=N,
                     n_rk4=n_rk4, C=C, n_obs=n_obs, limits=LONG_LIMITS if long else None, eps=eps, tie=tie, tol=tol,
                     use_bp=dtype == 'f32', crossing=1 if long else 0, need=12)


def value_net_ramp_hold_case():
    from igtmpc.scenarios import make_batch
    net = dict(layers=nets(1), Wn=np.eye(6), mu_f=np.zeros(6), sigma_t=1.0, mu_t=0.0)
    return make_case('value_net_ramp_hold_refined[f64]', 'f64', _batch_args(make_batch(96, dtype=np.float64)), cand='ramp_hold',
                     refine=1, net=net, cinf=cinf_default(), eps=1e-9, tie=1e-9, tol=1e-9, use_bp=False)


def value_bound_nets(sc):
    rng = np.random.default_rng(9)
    layers = nets(sc)
    return [dict(layers=layers, Wn=np.eye(6), mu_f=np.zeros(6), sigma_t=1.0, mu_t=0.0),
            dict(layers=layers, Wn=np.eye(6) + 0.05 * rng.normal(size=(6, 6)), mu_f=np.array([20.0, 2.5, 0.0, 0.0, 0.0, 0.0]),
                 sigma_t=-2.0, mu_t=0.7)]


def value_bound_case(sc):
    """The first 64 scenarios of test_value_bound_pruning_changes_nothing's batch, sigma_t = 1."""
    from igtmpc.scenarios import make_batch
    b = {k: v[:64] for k, v in make_batch(768, dtype=np.float64).items()}
    return make_case(f'value_bound[{sc}]', 'f64', _batch_args(b), cand='track', net=value_bound_nets(sc)[0], cinf=cinf_default(),
                     eps=1e-9, tie=1e-9, tol=1e-9, use_bp=False)


def warm_args(b, npdt, N=20, dt=0.1, shift=0):
    """A plausible previous solution per scenario (some lattice candidate rolled from u_prev), shifted by one step
    (utils.py:354-363), on two thirds of the scenarios."""
    B = len(b['flags'])
    prev = O.candidates_lattice(np.asarray(b['u_prev'], dtype=np.float64), O.Params(N=N, dt=dt))[np.arange(B), (np.arange(B) * 37 + shift) % 256]
    u_ws = np.ascontiguousarray(O.shift_controls(prev).astype(npdt))
    u_prev = np.ascontiguousarray(prev[:, :, 0].astype(npdt))
    flags = b['flags'] | np.where(np.arange(B) % 3 != 0, 2, 0).astype(np.uint32)
    return u_prev, u_ws, flags


def warm_case(dtype, cand):
    """test_warm_started_ramp_hold_matches_oracle / test_tracking_candidates_match_oracle: one refinement pass on top."""
    from igtmpc.scenarios import make_batch
    b = make_batch(192, dtype=_npdt(dtype))
    u_prev, u_ws, flags = warm_args(b, _npdt(dtype))
    tol, eps, tie = _bars(dtype)
    name = 'warm_ramp_hold' if cand == 'ramp_hold' else 'tracking'
    return make_case(f'{name}[{dtype}]', dtype, _batch_args(b, u_prev=u_prev, u_ws=u_ws, flags=flags), cand=cand, refine=1,
                     cinf=cinf_default(), eps=eps, tie=tie, tol=tol, utol=1e-7 if cand == 'ramp_hold' else 1e-12, first=True)


def speed_cap_case(dtype, vcap):
    from igtmpc.scenarios import make_batch
    B, npdt = 128, _npdt(dtype)
    b = make_batch(B, dtype=npdt)
    rng = np.random.default_rng(77)
    x0 = np.array(b['x0'], dtype=npdt)
    x0[:, 5] = rng.uniform(3.6, 4.9, B).astype(npdt)
    u_prev = np.array(b['u_prev'], dtype=npdt)
    u_prev[:, 0] = rng.uniform(-0.2, 1.2, B).astype(npdt)
    tol, eps, tie = _bars(dtype)
    # float32 tracking: the steering is fed back from the float state, 1e-4 on the trajectories (as the test always had);
    # controls and cost were not compared before and take the same bar
    t = dict(tol=1e-9, utol=1e-12) if dtype == 'f64' else dict(tol=1e-4, utol=1e-4)
    return make_case(f'speed_cap[{dtype}-{vcap:g}]', dtype, _batch_args(b, x0=x0, u_prev=u_prev), cand='track',
                     limits=dict(track_vcap=vcap), cinf=cinf_default(), eps=eps, tie=tie, **t)


def envelope_case(env):
    from igtmpc.scenarios import make_batch
    return make_case(f'envelope[{env:g}]', 'f64', _batch_args(make_batch(96, dtype=np.float64)), cand='track',
                     limits=dict(track_env=env), cinf=cinf_default(), eps=1e-9, tie=1e-9, tol=1e-9, utol=1e-12)


# ----------------------------------------------------------------------------- test_gpu_fullsize.py
FULLSIZE = [('config2', 65536, 0, 'f64', 0, 'lattice'), ('config2', 65536, 0, 'f32', 0, 'lattice'),
            ('config3', 32768, 3 * 32768, 'f64', 0, 'lattice'), ('config3', 32768, 3 * 32768, 'f32', 0, 'lattice'),
            ('config4', 65536, 0, 'f64', 1, 'lattice'), ('config4', 65536, 0, 'f64', 3, 'lattice'),
            ('config4', 65536, 0, 'f32', 1, 'lattice'), ('config4', 65536, 0, 'f32', 3, 'lattice'),
            ('config2_track', 65536, 0, 'f64', 0, 'track'), ('config2_track', 65536, 0, 'f32', 0, 'track')]
_BIG = {}


def big_batch(B, offset, dtype):
    from igtmpc.scenarios import make_batch
    k = (B, offset, dtype)
    if k not in _BIG:
        _BIG.clear()                 # one at a time: 65 536 scenarios of forecasts
        _BIG[k] = make_batch(B, dtype=_npdt(dtype), offset=offset)
    return _BIG[k]


def _subsample_bars(dtype, cand, net):
    """(tol, eps, tie) of a subsample taken from a big batch.  Cost near-ties: 1e-6 for the f32 rollout arithmetic; the f32 value
    network (MFMA, hardware exp/rcp tanh) adds ~1e-6 relative error to V, so with the terminal value in the cost ties are set
    aside at 2e-5.  Tracking in f32: 2e-5 throughout (the steering feedback carries rounding differences forward)."""
    if dtype == 'f64':
        return 1e-9, 1e-9, 1e-9
    if cand == 'track':
        return REL_TOL, 2e-5, 2e-5
    return REL_TOL, F32_EPS, 2e-5 if net else F32_TIE


def _bench_net(gt_sc):
    """bench.py's normalisation of the shipped checkpoint of scenario gt_sc (0: no value network)."""
    return dict(layers=nets(gt_sc), Wn=np.eye(6), mu_f=np.zeros(6), sigma_t=1.0, mu_t=0.0) if gt_sc else None


def fullsize_case(name, B, offset, dtype, gt_sc, cand):
    """A FIXED 512-scenario subsample from inside the big batch -> (case, idx, big batch)."""
    b = big_batch(B, offset, dtype)
    idx = np.sort(np.random.default_rng(7).choice(B, 512, replace=False))
    net = _bench_net(gt_sc)
    tol, eps, tie = _subsample_bars(dtype, cand, net)
    sub = {k: np.ascontiguousarray(v[idx]) for k, v in b.items()}
    case = make_case(f'{name}[{dtype}' + (f'-sc{gt_sc}]' if gt_sc else ']'), dtype, _batch_args(sub), cand=cand, net=net,
                     cinf=cinf_default(), eps=eps, tie=tie, tol=tol)
    return case, idx, b


# ----------------------------------------------------------------------------- test_gpu_overlap.py
OVERLAP_B = 4096
OVERLAP_ROUNDS = 4               # >= 3 rounds of solves in flight per lane, none of them waited for
# (dtype, candidate family, value net of scenario sc or 0); lane q takes OVERLAP_LANES[q % 5]
OVERLAP_LANES = [('f64', 'lattice', 0), ('f64', 'track', 0), ('f32', 'lattice', 0), ('f64', 'lattice', 1), ('f32', 'track', 0)]
OVERLAP_MAX_F = 8                # lanes 0 .. 7: a lane's family, batches and subsample are the same whatever F it runs among


def overlap_lane(q):
    return OVERLAP_LANES[q % len(OVERLAP_LANES)]


def overlap_batch(q, v):
    """Batch v (0, 1: alternating between rounds) of lane q; no two lanes share one (make_batch(offset=...) is the generator's
    per-shard path)."""
    from igtmpc.scenarios import make_batch
    return make_batch(OVERLAP_B, dtype=_npdt(overlap_lane(q)[0]), offset=(2 * q + v + 1) * OVERLAP_B)


def overlap_case(q, b=None):
    """A FIXED 256-scenario subsample of the batch lane q solves in its last round -> (case, idx).  b: that batch
    (overlap_batch(q, (OVERLAP_ROUNDS - 1) % 2)) where the caller has it already."""
    dtype, cand, gt = overlap_lane(q)
    if b is None:
        b = overlap_batch(q, (OVERLAP_ROUNDS - 1) % 2)
    idx = np.sort(np.random.default_rng(5 + q).choice(OVERLAP_B, 256, replace=False))
    net = _bench_net(gt)
    tol, eps, tie = _subsample_bars(dtype, cand, net)
    sub = {k: np.ascontiguousarray(v[idx]) for k, v in b.items()}
    return make_case(overlap_key(q), dtype, _batch_args(sub), cand=cand, net=net, cinf=cinf_default(), eps=eps, tie=tie,
                     tol=tol), idx


def overlap_key(q):
    dtype, cand, gt = overlap_lane(q)
    return f'overlap[lane{q}-{dtype}-{cand}' + (f'-sc{gt}]' if gt else ']')


# ----------------------------------------------------------------------------- test_gpu_fuzz.py: the seeded draws
def _long_horizon(cfg, lim):
    """Lattice and ramp-hold candidates hold constant rates (or ramp to held targets): at the reference's lane and steering-rate
    limits hardly any of them stays feasible from N = 40 on, and a draw would compare status 1 with status 1.  Those draws run at
    LONG_LIMITS (a drawn v_max is kept).  Applied after every draw of the generator, so the draws themselves stay
    what they were.  The tracking family steers by feedback and solves at any horizon."""
    if cfg['N'] >= LONG_N and cfg['cand'] != 'track':
        lim = dict(lim, ey_lim=LONG_LIMITS['ey_lim'], steer_rate_limit=LONG_LIMITS['steer_rate_limit'])
        lim.setdefault('v_max', LONG_LIMITS['v_max'])
    return lim


# Draws whose limits are moved because, as drawn, they leave fewer solved and compared scenarios than a seed must have (8, or
# B // 2 of a batch under 16; tests/test_parity_floors_host.py) -- the limits, not the seeds, so every other draw stays:
#   105 (float32, ramp-hold, N = 7 at dt = 0.05, two refinement passes, value network): the horizon is 0.35 s, the twice
#       re-centred grid is spaced 1e-3 and the control-effort term separates neighbours by w_u N da^2 < 1e-6, under the 2e-5
#       near-tie width of the float32 value-network cost: 36 of 40 scenarios were set aside, none of the rest solved.  Faster
#       rate limits widen the grid and w_u = 20 separates its neighbours: 24 compared, 20 of them solved.
#   218 (ramp-hold, N = 64, C = 64, B = 5): 8 acceleration targets across +-N dt jerk = 5.76 m/s^2 leave one that keeps the
#       speed box and the terminal set over 6.4 s, and one scenario solved; at jerk_limit = 0.2 (and a lane of 3 m) three do.
FUZZ_ADJUSTED = {105: dict(jerk_limit=4.0, steer_rate_limit=2.0, w_u=20.0), 218: dict(jerk_limit=0.2, ey_lim=3.0)}


def fuzz_draw(seed):
    cfg = _fuzz_draw_ext(seed) if seed >= 200 else _fuzz_draw_base(seed)
    cfg['limits'] = dict(cfg['limits'], **FUZZ_ADJUSTED.get(seed, {}))
    return cfg


def _fuzz_draw_base(seed):
    rng = np.random.default_rng([2026, seed])
    cfg = dict(
        N=int(rng.choice([4, 7, 12, 20, 33, 40])),
        n_rk4=int(rng.choice([1, 2, 3, 4, 4, 6])),
        dt=float(rng.choice([0.05, 0.1, 0.1, 0.2])),
        C=int(rng.choice([64, 256, 256, 1024])),
        cand=str(rng.choice(['lattice', 'ramp_hold', 'track', 'track'])),
        n_obs=int(rng.choice([0, 1, 1, 2])),
        B=int(rng.choice([1, 3, 8, 17, 40, 70, 300])),
        terminal=bool(rng.random() < 0.6),
    )
    cfg['refine'] = int(rng.choice([0, 0, 1, 2])) if cfg['cand'] != 'lattice' else 0
    cfg['warm'] = bool(cfg['cand'] != 'lattice' and rng.random() < 0.4)       # igt_solve_batch_ws_*: two thirds of the batch
    cfg['net'] = int(rng.choice([0, 0, 0, 1, 3])) if cfg['n_obs'] == 1 else 0    # terminal value network V_GT_sc1 / sc3 (0: off)
    if cfg['B'] * cfg['C'] * cfg['N'] * cfg['n_rk4'] > 2.5e7:                 # keeps the numpy oracle to about a second
        cfg['B'] = 17
    lim = {}
    if rng.random() < 0.5:
        lim['v_max'] = float(rng.choice([4.0, 6.0]))
    if rng.random() < 0.5:
        lim['a_max'] = float(rng.choice([2.0, 3.5]))
    if rng.random() < 0.3:
        lim['ey_lim'] = 0.35
    if rng.random() < 0.3:
        lim['d_min'] = float(rng.choice([4.0, 7.0]))
    if rng.random() < 0.3:
        lim['w_u'] = 0.3
    if cfg['cand'] == 'track' and rng.random() < 0.5:
        lim['track_env'] = float(rng.choice([0.0, 0.5]))
    if cfg['cand'] == 'track' and rng.random() < 0.3:
        lim['track_vcap'] = 0.0
    cfg['limits'] = _long_horizon(cfg, lim)
    return cfg


def _fuzz_draw_ext(seed):
    """The ranges include/igtmpc.h advertises beyond the reference's configuration: horizons up to IGT_MAX_N = 64 (with C = 256 the
    slice's steering table fits LDS, with C = 64 it does not: both paths), up to IGT_MAX_OBS = 4 obstacles, batches either side
    of the live-row units' bound."""
    rng = np.random.default_rng([4026, seed])
    cfg = dict(
        N=int(rng.choice([48, 64, 64])),
        n_rk4=int(rng.choice([2, 4, 4])),
        dt=float(rng.choice([0.05, 0.1])),
        C=int(rng.choice([64, 256, 256])),
        cand=str(rng.choice(['lattice', 'ramp_hold', 'track'])),
        n_obs=int(rng.choice([2, 3, 4, 4])),
        B=int(rng.choice([5, 40, 130, 1100])),
        terminal=bool(rng.random() < 0.6),
    )
    cfg['refine'] = int(rng.choice([0, 0, 1])) if cfg['cand'] != 'lattice' else 0
    cfg['warm'] = bool(cfg['cand'] != 'lattice' and rng.random() < 0.4)
    cfg['net'] = 0
    if cfg['B'] * cfg['C'] * cfg['N'] * cfg['n_rk4'] * (1 + cfg['refine']) > 9e7:
        cfg['B'] = 130 if cfg['C'] == 256 else 1100
    lim = {}
    if rng.random() < 0.5:
        lim['v_max'] = float(rng.choice([4.0, 6.0]))
    if rng.random() < 0.3:
        lim['d_min'] = float(rng.choice([4.0, 7.0]))
    if cfg['cand'] == 'track' and rng.random() < 0.5:
        lim['track_env'] = float(rng.choice([0.0, 0.5]))
    if cfg['cand'] == 'track' and rng.random() < 0.3:
        lim['track_vcap'] = 0.0
    cfg['limits'] = _long_horizon(cfg, lim)
    return cfg


FUZZ_N_SEEDS = 40
FUZZ_F32_SEEDS = range(100, 118)
FUZZ_EXT_SEEDS = range(200, 214)
FUZZ_EXT_F32_SEEDS = range(214, 220)


def fuzz_case(seed, dtype):
    """The draw's inputs and oracle parameters (parity_cases.make_case); creates no solver."""
    from igtmpc.cinf import cinf_halfplanes
    from igtmpc.scenarios import make_batch
    cfg = fuzz_draw(seed)
    N, dt, B = cfg['N'], cfg['dt'], cfg['B']
    f32 = dtype == 'f32'
    npdt = np.float32 if f32 else np.float64
    # tracking family in float32: the steering is fed back from the float state, the controls carry the trajectories' error
    tol, utol = (REL_TOL, 1e-7 if cfg['cand'] != 'track' else REL_TOL) if f32 else (1e-9, 1e-12)
    eps, tie = ((2e-5, 2e-5) if cfg['net'] else (F32_EPS, F32_TIE)) if f32 else (1e-9, 1e-9)
    b = make_batch(max(B, 8), N=N, dt=dt, seed=100 + seed, dtype=npdt)
    b = {k: np.ascontiguousarray(v[:B]) for k, v in b.items() if isinstance(v, np.ndarray) and len(v) >= B}
    obs = b['obs_xy']                                                  # [B, 1, 2, N+1]
    if cfg['n_obs'] == 0:
        obs = np.zeros((B, 0, 2, N + 1), dtype=npdt)
    elif cfg['n_obs'] >= 2:                                            # further vehicles, 9 m apart behind the first along its path
        more = [obs]
        for m in range(1, cfg['n_obs']):
            lag = obs.copy()
            lag[:, 0, 0, :] -= 9.0 * m * np.cos(0.3 * np.arange(B))[:, None]
            lag[:, 0, 1, :] -= 9.0 * m * np.sin(0.3 * np.arange(B))[:, None]
            more.append(lag)
        obs = np.ascontiguousarray(np.concatenate(more, axis=1))
    rng = np.random.default_rng([7, seed])
    flags, u_prev, u_ws = b['flags'], b['u_prev'], None
    if cfg['warm']:       # previous solution = some lattice candidate of the scenario, shifted by one step (utils.py:354-363)
        u_prev, u_ws, flags = warm_args(b, npdt, N, dt, shift=seed)
    net = None
    if cfg['net']:
        v = np.load(f'{GOLDEN}/value_net_golden.npz')
        layers, i = [], 0
        while f"sc{cfg['net']}_W{i}" in v:
            layers.append((v[f"sc{cfg['net']}_W{i}"], v[f"sc{cfg['net']}_b{i}"]))
            i += 1
        net = dict(layers=layers, Wn=np.eye(6) + 0.05 * rng.normal(size=(6, 6)),
                   mu_f=np.array([20.0, 2.5, 0.0, 0.0, 0.0, 0.0]) + 0.1 * rng.normal(size=6), sigma_t=float(rng.choice([1.0, 3.0, -2.0])),
                   mu_t=float(rng.normal()))
    cinf = cinf_halfplanes(dt=dt, jerk=cfg['limits'].get('jerk_limit', 0.9)) if cfg['terminal'] else None
    args = dict(x0=b['x0'], u_prev=u_prev, kparams=b['kparams'], flags=flags, obs=obs, u_ws=u_ws, tv_sv=b['tv_sv'], enc=b['enc'])
    case = make_case(f'fuzz[{seed}-{dtype}]', dtype, args, N=N, dt=dt, n_rk4=cfg['n_rk4'], C=cfg['C'], n_obs=cfg['n_obs'],
                     cand=cfg['cand'], refine=cfg['refine'], limits=cfg['limits'], net=net, cinf=cinf, eps=eps, tie=tie, tol=tol,
                     utol=utol, ctol=2e-5 if f32 and cfg['net'] else None, need=min(8, B // 2) if B < 16 else 8)
    case['cfg'] = cfg
    return case


# ----------------------------------------------------------------------------- test_gpu_limits.py: the seeded draws
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
LIMITS_N_SEEDS = 32
LIMITS_F32_SEEDS = range(0, LIMITS_N_SEEDS, 3)


def _choice(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def limits_draw(seed):
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
LIMITS_CINF_TOO_LARGE = {(0.05, 0.02), (0.1, 0.02), (0.05, 0.2)}


def limits_cinf(cfg):
    """The terminal set at the drawn (dt, jerk), or (None, None)."""
    from igtmpc.cinf import cinf_halfplanes
    jerk = cfg['limits'].get('jerk_limit', 0.9)
    if not cfg['terminal'] or (cfg['dt'], jerk) in LIMITS_CINF_TOO_LARGE:
        return None, None
    A, b = cinf_halfplanes(dt=cfg['dt'], jerk=jerk, **cfg.get('cinf_kw', {}))
    assert len(b) <= 256
    return A, b


def limits_inputs(cfg, seed):
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


def limits_net(cfg, golden_dir, seed):
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


def limits_case(seed, dtype):
    """A seeded draw as a parity_cases case (inputs and oracle parameters; no solver): what test_limits_draw_matches_oracle
    solves, for the CPU-side measurement of its floors."""
    cfg = limits_draw(seed)
    inp = limits_inputs(cfg, seed)
    f32 = dtype == 'f32'
    net = limits_net(cfg, GOLDEN, seed)
    npdt = np.float32 if f32 else np.float64
    args = {k: (None if v is None else (v if k == 'flags' else np.ascontiguousarray(v.astype(npdt)))) for k, v in inp.items()}
    tol, utol = (REL_TOL, 1e-7 if cfg['cand'] != 'track' else REL_TOL) if f32 else (1e-9, 1e-12)
    eps, tie = ((2e-5, 2e-5) if net else (F32_EPS, F32_TIE)) if f32 else (1e-9, 1e-9)
    cinf = limits_cinf(cfg)
    return make_case(f'limits[{seed}-{dtype}]', dtype, args, N=cfg['N'], dt=cfg['dt'], n_rk4=cfg['n_rk4'], C=cfg['C'],
                     n_obs=cfg['n_obs'], cand=cfg['cand'], refine=cfg['refine'], limits=cfg['limits'], net=net,
                     cinf=None if cinf[0] is None else cinf, eps=eps, tie=tie, tol=tol, utol=utol,
                     ctol=2e-5 if f32 and net else None)


# ----------------------------------------------------------------------------- test_gpu_dispatch_leaves.py
LEAF_FAMILIES = ('lattice', 'table', 'ramp_hold', 'track')
LEAF_N_RK4 = (4, 3, 2, 7)
LEAF_SEED = 0


HI_ORDER_RULE = 'k.hi_order = (k.h * vhi * (0.7 / p.l_r + 0.25) > 0.12) ? 1 : 0;'       # csrc/igt_api.hip, with the line before it:
HI_ORDER_VHI = 'const double vhi = std::fmax(std::fabs(p.v_min), std::fabs(p.v_max)) + 2.0;'


def leaf_hi_order(P):
    """KP::hi_order for the parameters P (np_oracle.Params; the GPU tests hold them equal to the solver's): a restatement of
    the two statements above, which tests/test_host_logic.py holds to the text of csrc/igt_api.hip."""
    vhi = max(abs(P.v_min), abs(P.v_max)) + 2.0
    return (P.dt / P.n_rk4) * vhi * (0.7 / P.l_r + 0.25) > 0.12


def leaf_case(dtype, cand, n_rk4):
    """The smallest solve that selects one leaf of the launchers' dispatch (csrc/igt_dispatch.h): 5 scenarios (no multiple of
    rollout-all's 4 per workgroup), one 64-candidate unit each, 8 steps of dt = 0.1, one obstacle.  n_rk4 = 4 is the build
    of the reference's discretisation; 3 and 2 run the long polynomials (h = dt / n_rk4 > 0.0304 at the default limits: leaf_hi_order); 7 the
    short polynomials with the sub-steps counted at run time.  The table family: scenario 0's lattice as everyone's table,
    and its previous controls as everyone's (a table's controls are held to the rate limits from u_prev)."""
    from igtmpc.scenarios import make_batch
    B, N, C, npdt = 5, 8, 64, _npdt(dtype)
    b = make_batch(8, N=N, dt=0.1, seed=LEAF_SEED, dtype=npdt)
    b = {k: np.ascontiguousarray(v[:B]) for k, v in b.items() if isinstance(v, np.ndarray) and len(v) >= B}
    table = None
    if cand == 'table':
        b['u_prev'] = np.ascontiguousarray(np.broadcast_to(b['u_prev'][:1], b['u_prev'].shape))
        table = np.ascontiguousarray(O.candidates_lattice(b['u_prev'][:1].astype(np.float64), O.Params(N=N, dt=0.1), C)[0])
    tol, eps, tie = _bars(dtype, F32_EPS, F32_TIE)
    return make_case(f'leaf[{dtype}-{cand}-{n_rk4}]', dtype, _batch_args(b), N=N, n_rk4=n_rk4, C=C, cand=cand, table=table,
                     cinf=cinf_default(), eps=eps, tie=tie, tol=tol, utol=1e-7 if cand != 'track' or dtype == 'f64' else REL_TOL,
                     need=B // 2)


# ----------------------------------------------------------------------------- every comparison
def all_cases():
    """Yields (key, builder): every case the GPU tests compare through check_case, built lazily."""
    for dtype in ('f64', 'f32'):
        yield f'solve[{dtype}]', lambda d=dtype: solve_case(d)
        for sc in (1, 3):
            yield f'value_net[{sc}-{dtype}]', lambda d=dtype, s=sc: value_net_case(s, d)
        yield f'ramp_hold_refined[{dtype}]', lambda d=dtype: ramp_hold_refined_case(d)
        for shp in (SHAPES_F64 if dtype == 'f64' else SHAPES_F32):
            yield 'other_shapes_%s[%d-%d-%d-%d]' % ((dtype,) + shp), lambda d=dtype, s=shp: shape_case(d, *s)
        yield f'warm_ramp_hold[{dtype}]', lambda d=dtype: warm_case(d, 'ramp_hold')
        yield f'tracking[{dtype}]', lambda d=dtype: warm_case(d, 'track')
        for vcap in (1.0, 0.0):
            yield f'speed_cap[{dtype}-{vcap:g}]', lambda d=dtype, v=vcap: speed_cap_case(d, v)
    yield 'value_net_ramp_hold_refined[f64]', value_net_ramp_hold_case
    for sc in (1, 3):
        yield f'value_bound[{sc}]', lambda s=sc: value_bound_case(s)
    for env in (0.0, 0.5):
        yield f'envelope[{env:g}]', lambda e=env: envelope_case(e)
    for spec in FULLSIZE:
        yield f'{spec[0]}[{spec[3]}' + (f'-sc{spec[4]}]' if spec[4] else ']'), lambda s=spec: fullsize_case(*s)[0]
    for q in range(OVERLAP_MAX_F):
        yield overlap_key(q), lambda q=q: overlap_case(q)[0]
    for dtype in ('f64', 'f32'):
        for cand in LEAF_FAMILIES:
            for n_rk4 in LEAF_N_RK4:
                yield f'leaf[{dtype}-{cand}-{n_rk4}]', lambda d=dtype, c=cand, n=n_rk4: leaf_case(d, c, n)
    for seeds, dtype in ((range(FUZZ_N_SEEDS), 'f64'), (FUZZ_F32_SEEDS, 'f32'), (FUZZ_EXT_SEEDS, 'f64'), (FUZZ_EXT_F32_SEEDS, 'f32')):
        for seed in seeds:
            yield f'fuzz[{seed}-{dtype}]', lambda s=seed, d=dtype: fuzz_case(s, d)
    for seeds, dtype in ((range(LIMITS_N_SEEDS), 'f64'), (LIMITS_F32_SEEDS, 'f32')):
        for seed in seeds:
            yield f'limits[{seed}-{dtype}]', lambda s=seed, d=dtype: limits_case(s, d)
    import nonfinite_cases as NF                       # test_gpu_nonfinite.py: the poisoned scenarios of every case
    for name in NF.CASES:
        yield f'nonfinite[{name}]', lambda n=name: NF.parity_case(n)


# The numpy oracle takes ten seconds and more on the larger batches: the CPU-side measurement (the host test and the tool) runs the
# first HOST_B scenarios of the cases below, which keeps the host test to minutes.  Listed are only cases whose WHOLE batch the
# oracle compares (share 1.0, as measured in full and as printed by the GPU run: profiles/parity_set_aside_shares.txt).
# Scenarios are independent, so the share of the first HOST_B is then 1.0 as well -- which is what the GPU test asserts of the
# whole batch -- and their solved count is a lower bound of the whole batch's.  The large cases with set-asides (fuzz[32-f64],
# fuzz[219-f32], the float32 refined families, config2_track[f32]) are measured in full: a share of a part is not the batch's.
HOST_B = 130
HOST_SUBSAMPLED = ('fuzz[203-f64]', 'fuzz[204-f64]', 'fuzz[206-f64]', 'fuzz[19-f64]', 'fuzz[21-f64]', 'fuzz[36-f64]', 'fuzz[38-f64]',
                   'fuzz[110-f32]', 'solve[f64]', 'solve[f32]', 'ramp_hold_refined[f64]', 'config2[f64]', 'config2[f32]',
                   'config3[f64]', 'config3[f32]', 'config4[f64-sc1]', 'config4[f64-sc3]', 'config4[f32-sc1]', 'config4[f32-sc3]',
                   'config2_track[f64]')


def host_view(case):
    """The case as the CPU-side measurement runs it."""
    if case['key'] not in HOST_SUBSAMPLED or case['B'] <= HOST_B:
        return case
    args = {k: (None if v is None else v[:HOST_B]) for k, v in case['args'].items()}
    return dict(case, args=args, B=HOST_B)


def min_solved_for(solved):
    """The recorded minimum: what the oracle gives, less a tenth (nothing under ten scenarios: the oracle is deterministic)."""
    return solved - solved // 10


def measure_key(key):
    """Build the case of one key and run the oracle alone on it -> {key: measured} (with key + '/first' where compared)."""
    for k, build in all_cases():
        if k == key:
            case = host_view(build())
            out = measure_case(case)
            for m in out.values():
                m.update(need=case['need'], crossing_needed=case['crossing'], f64=case['dtype'] == 'f64')
            return out
    raise KeyError(key)
