"""The rectangle (OBCA) collision model (BatchSolver.solve_box / rollout_all_box): the cases the host and the GPU tests share,
and their reference answer from the oracle and the numpy restatement (tests/box_collision_restated.py) alone.

A case: make_batch's scenarios; the oracle rolls every candidate without obstacles; then one stationary rectangle per
(scenario, obstacle slot) is placed ahead of the obstacle-free winner's last node so that about half of the otherwise feasible
candidates overlap it.  The reference answer keeps the oracle's trajectories, costs and verdicts and adds the restated
rectangle verdict: g = max(g_oracle, g_box), feasibility from it, the arg-min with ties to the lowest index."""
import numpy as np

import box_collision_restated as R
import np_oracle as O
from helpers import host_params, host_track
from parity_cases import LONG_LIMITS, cinf_default, value_net_case

BAR = 1e-9                                         # tol = eps = tie of every comparison here (float64: DESIGN.md section 6)
HEADINGS = (np.pi / 2, 0.0, 0.4, -2.6)             # obstacle heading relative to the winner's, by (scenario + slot) % 4
OFFSETS = (0.0, 0.0, 2.6, -2.4)                    # lateral offset [m], times 1 for slot 0 and 3 for the others
D_GRID = np.linspace(0.5, 7.0, 27)                 # distances ahead of the winner's last node that a case chooses from
CIRCLE_D_MIN = 5.6                                 # the circle model's centre distance (2 x 2.8 m)

# (family, B, N, C, n_obs, n_rk4, long limits, special) -> figures the oracle and the restatement alone measure (eps = tie =
# BAR; no scenario is set aside in any case): scenarios solved, winners that differ from the obstacle-free winner, winners the
# 5.6 m circle refuses.  special: None, 'table' (one shared table: candidate_cases.per_scenario_candidates(u_prev[:1])[0]) or
# 'net' (the value-network cost, value_net_case(1)).
CASES = {
    ('lattice', 48, 20, 64, 1, 4, False, None): dict(solved=32, moved=31, circle=32),
    ('lattice', 24, 20, 256, 2, 4, False, None): dict(solved=21, moved=21, circle=21),
    ('lattice', 24, 13, 256, 4, 4, False, None): dict(solved=23, moved=19, circle=23),
    ('lattice', 24, 40, 64, 2, 4, True, None): dict(solved=22, moved=18, circle=22),
    ('lattice', 16, 64, 64, 1, 3, True, None): dict(solved=6, moved=4, circle=6),
    ('track', 48, 20, 256, 1, 4, False, None): dict(solved=48, moved=48, circle=48),
    ('track', 24, 40, 64, 2, 4, False, None): dict(solved=24, moved=24, circle=21),
    ('ramp_hold', 48, 20, 64, 1, 4, False, None): dict(solved=28, moved=27, circle=28),
    ('table', 24, 20, 64, 1, 4, False, 'table'): dict(solved=5, moved=4, circle=5),
    ('lattice', 24, 20, 64, 1, 4, False, 'net'): dict(solved=16, moved=16, circle=16),
}


def case_id(key):
    fam, B, N, C, n_obs, n_rk4, long, sp = key
    return f'{fam}-{B}-{N}-{C}-{n_obs}-{n_rk4}' + ('-long' if long else '') + (f'-{sp}' if sp else '')


_BUILT = {}


def _oracle_free(c):
    """The oracle's pass without obstacles (return_all), for the case's family."""
    A, b = c['cinf']
    fam = c['family']
    kw = dict(net=c['net'], tv_sv=c['tv_sv'], enc=c['enc']) if c['net'] else {}
    if fam in ('ramp_hold', 'track'):
        return O.solve_batch_refined(c['x0'], c['u_prev'], c['kparams'], c['flags'], None, A, b, c['P'], C=c['C'], refine_iters=0,
                                     cand=fam, track=host_track(**c['limits']), **kw)[0]
    return O.solve_batch(c['x0'], c['u_prev'], c['kparams'], c['flags'], None, A, b, c['P'], C=c['C'], U=c['table'],
                         return_all=True, **kw)


def place_obstacles(r, n_obs, N, d_grid=D_GRID):
    """pose[B,n_obs,3,N+1] and the chosen D[B] for the obstacle-free pass r."""
    B = len(r['argmin'])
    c0 = np.where(r['argmin'] >= 0, r['argmin'], 0)
    xw = r['X'][np.arange(B), c0]                                        # [B,7,N+1]
    psi = xw[:, O.IPSI, N]
    fwd = np.stack([np.cos(psi), np.sin(psi)], -1)
    lat = np.stack([-np.sin(psi), np.cos(psi)], -1)
    end = xw[:, :2, N]
    feas = r['feas']
    pose = np.zeros((B, n_obs, 3, N + 1))
    D = np.zeros(B)
    for i in range(B):
        kinds = [(i + o) % 4 for o in range(n_obs)]
        head = np.array([psi[i] + HEADINGS[k] for k in kinds])
        off = np.array([OFFSETS[k] * (1.0 if o == 0 else 3.0) for o, k in enumerate(kinds)])
        X = r['X'][i][feas[i]]                                           # the otherwise feasible candidates [F,7,N+1]
        best, pick = None, d_grid[0]
        for d in d_grid:
            q = end[i] + d * fwd[i] + off[:, None] * lat[i]              # [n_obs,2]
            if len(X):
                gap = R.signed_gap(X[:, None, 0, 1:], X[:, None, 1, 1:], X[:, None, 6, 1:], q[None, :, 0, None], q[None, :, 1, None],
                                   head[None, :, None])
                share = (gap.min(axis=(1, 2)) < 0).mean()
            else:
                share = 0.0
            if best is None or abs(share - 0.5) < best:
                best, pick = abs(share - 0.5), d
        D[i] = pick
        q = end[i] + pick * fwd[i] + off[:, None] * lat[i]
        pose[i, :, 0, :] = q[:, 0, None]; pose[i, :, 1, :] = q[:, 1, None]; pose[i, :, 2, :] = head[:, None]
    return pose, D


def reference_answer(r, pose, P, **box):
    """The obstacle-free pass r with the restated rectangle verdict against `pose` added -> a solve_batch(return_all=True)
    result (x, u, cost, argmin, status, X, U, J, g, mask, feas) plus g_box, inside, gap."""
    gb, inside, gap = R.margins(r['X'], pose, **box)
    with np.errstate(invalid='ignore'):
        g_box = np.where(np.isnan(gb), -np.inf, gb).max(axis=(2, 3)) if gb.shape[2] else np.full(r['J'].shape, -np.inf)
    g = np.maximum(r['g'], g_box)
    hit = g_box > P.feas_tol
    mask = r['mask'] | np.where(hit, 32, 0).astype(r['mask'].dtype)
    feas = r['feas'] & ~hit
    B = len(r['argmin'])
    Jm = np.where(feas, r['J'], np.inf)
    arg = np.argmin(Jm, axis=1)
    ok = feas[np.arange(B), arg]
    out = dict(r)
    out.update(g=g, mask=mask, feas=feas, g_box=g_box, inside=inside, gap=gap,
               status=np.where(ok, 0, 1).astype(np.int32), argmin=np.where(ok, arg, -1).astype(np.int32),
               x=np.where(ok[:, None, None], r['X'][np.arange(B), arg], np.nan),
               u=np.where(ok[:, None, None], r['U'][np.arange(B), arg], np.nan),
               cost=np.where(ok, r['J'][np.arange(B), arg], np.inf))
    return out


def build(key):
    """-> dict(key, family, B, N, C, n_obs, n_rk4, limits, P, cinf, net, table, x0, u_prev, kparams, flags, tv_sv, enc, pose, D,
    free, ref), float64; built once and shared -- nothing may write into it.  free: the oracle's obstacle-free pass; ref: the
    reference answer."""
    if key not in _BUILT:
        from igtmpc.scenarios import make_batch
        fam, B, N, C, n_obs, n_rk4, long, sp = key
        limits = dict(LONG_LIMITS) if long else {}
        P = host_params(N=N, n_rk4=n_rk4, **limits)
        b = make_batch(B, dtype=np.float64, N=N)
        net = value_net_case(1, 'f64')['net'] if sp == 'net' else None
        table = None
        if sp == 'table':
            from candidate_cases import per_scenario_candidates
            table = np.ascontiguousarray(per_scenario_candidates(b['u_prev'][:1], P, C, N)[0])
        c = dict(key=key, family=fam, B=B, N=N, C=C, n_obs=n_obs, n_rk4=n_rk4, limits=limits, P=P, cinf=cinf_default(), net=net,
                 table=table, x0=b['x0'], u_prev=b['u_prev'], kparams=b['kparams'], flags=b['flags'],
                 tv_sv=b['tv_sv'] if net else None, enc=b['enc'] if net else None)
        with np.errstate(all='ignore'):
            free = _oracle_free(c)
            pose, D = place_obstacles(free, n_obs, N)
            c.update(pose=pose, D=D, free=free, ref=reference_answer(free, pose, P))
        for v in list(c.values()) + list(c['ref'].values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _BUILT[key] = c
    return _BUILT[key]


def oracle(case):
    """-> (passes, x0[B,1,7] with the flags applied, kp[B,1,3]) as helpers.compare_solve takes them."""
    return [case['ref']], O.apply_flags(case['x0'], case['flags'])[:, None, :], case['kparams'][:, None, :]


def figures(case):
    """What the host test pins: dict(solved, moved, circle, set_aside, overlap_share, gate_share)."""
    from helpers import measure
    passes, x0, kp = oracle(case)
    ref, free, P = case['ref'], case['free'], case['P']
    m, amb, _ = measure(passes, P, x0, kp, BAR, BAR)
    sol = ref['status'] == 0
    B = case['B']
    moved = sol & (ref['argmin'] != free['argmin'])
    xw = ref['x'][sol]
    q = case['pose'][sol]
    d2 = (xw[:, None, 0, 1:] - q[:, :, 0, 1:]) ** 2 + (xw[:, None, 1, 1:] - q[:, :, 1, 1:]) ** 2
    circle = (CIRCLE_D_MIN ** 2 - d2 > P.feas_tol).any(axis=(1, 2))
    of = free['feas']                                                    # the otherwise feasible candidates
    with np.errstate(invalid='ignore'):
        gap_min = np.where(ref['inside'], ref['gap'], np.inf).min(axis=(2, 3))
        overlap = (gap_min < 0) & of
        apart_in = ref['inside'].any(axis=(2, 3)) & ~(gap_min < 0) & of
    n = max(int(of.sum()), 1)
    return dict(solved=int(sol.sum()), moved=int(moved.sum()), circle=int(circle.sum()), set_aside=int(amb.sum()),
                overlap_share=float(overlap.sum() / n), gate_share=float(apart_in.sum() / n), B=B)


def open_solver(igt, case, **kw):
    """A solver of the case's family, shape, limits, terminal set, table and network."""
    s = igt.BatchSolver(N=case['N'], n_rk4=case['n_rk4'], C=case['C'], n_obs=case['n_obs'], dtype='f64', cand_mode=case['family'],
                        cost_mode='value_net' if case['net'] else 'progress', **case['limits'], **kw)
    try:
        s.set_cinf(*case['cinf'])
        if case['table'] is not None:
            s.set_candidate_table(case['table'])
        if case['net']:
            s.set_value_net(**case['net'])
    except BaseException:
        s.close()
        raise
    return s


def solve_args(case, sl=slice(None)):
    """Positional and keyword arguments of solve_box / rollout_all_box for the scenarios `sl`."""
    kw = {}
    if case['net']:
        kw.update(tv_sv=case['tv_sv'][sl], enc=case['enc'][sl])
    return [case['x0'][sl], case['u_prev'][sl], case['kparams'][sl], case['flags'][sl], case['pose'][sl]], kw
