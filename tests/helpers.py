"""Shared parity harness (tests only).  The oracle is the float64 numpy restatement in
oracle/np_oracle.py, fed the SAME inputs as the device (float32 inputs are up-cast
exactly), so differences are the kernel's arithmetic only."""
import json
import os

import numpy as np

import np_oracle as O

REL_TOL = 1e-5       # BASELINE.json north_star: 1e-5 relative, |ref| floored at 1
F32_EPS = 1e-7       # f32 comparisons: width of the threshold / break-point set-aside (tools/f32_margin_probe.py)
F32_TIE = 1e-6       # ... and of the cost near-tie set-aside


def rel_err(got, ref):
    """|got-ref| / max(1,|ref|), elementwise."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return np.abs(got - ref) / np.maximum(1.0, np.abs(ref))


def oracle_params(solver):
    p = solver.params
    return O.Params(N=p.N, dt=p.dt, n_rk4=p.n_rk4, l_r=p.l_r, l_f=p.l_f, v_min=p.v_min, v_max=p.v_max,
                    a_min=p.a_min, a_max=p.a_max, df_max=p.df_max, jerk=p.jerk_limit,
                    steer_rate=p.steer_rate_limit, ey_lim=p.ey_lim, d_min=p.d_min, w_u=p.w_u,
                    feas_tol=p.feas_tol)


# igt_params names that differ from np_oracle.Params's; the tracking family's knobs are no Params fields (host_track)
_RENAMED = {'jerk_limit': 'jerk', 'steer_rate_limit': 'steer_rate'}
TRACK_DEFAULTS = dict(ke=0.3, span=0.1, blim=0.7, env=1.0, vcap=1.0)      # igt_params_default (include/igtmpc.h)


def host_params(N=20, dt=0.1, n_rk4=4, **limits):
    """What oracle_params returns for BatchSolver(N=, dt=, n_rk4=, **limits), without a solver: np_oracle.Params' defaults are
    igt_params_default's (the GPU tests assert the two equal, params_equal).  track_* keys are left to host_track."""
    kw = {_RENAMED.get(k, k): v for k, v in limits.items() if not k.startswith('track_')}
    return O.Params(N=N, dt=dt, n_rk4=n_rk4, **kw)


def host_track(**limits):
    """The tracking family's parameters as the oracle takes them (solve_batch_refined's track=), defaults plus overrides."""
    tk = dict(TRACK_DEFAULTS)
    for k, name in (('track_ke', 'ke'), ('track_span', 'span'), ('track_beta_lim', 'blim'), ('track_env', 'env'),
                    ('track_vcap', 'vcap')):
        if k in limits:
            tk[name] = limits[k]
    return tk


def solver_track(solver):
    p = solver.params
    return dict(ke=p.track_ke, span=p.track_span, blim=p.track_beta_lim, env=p.track_env, vcap=p.track_vcap)


def params_equal(P, Q):
    return vars(P) == vars(Q)


def oracle_solve(batch, P, C=256, cinf=None, U=None):
    f = lambda k: np.asarray(batch[k], dtype=np.float64)
    A, b = (None, None) if cinf is None else cinf
    return O.solve_batch(f('x0'), f('u_prev'), f('kparams'), batch['flags'], f('obs_xy'), A, b, P, C=C, U=U,
                         return_all=True)


def ambiguous_mask(ref, P, eps_margin=2e-5, eps_cost=2e-5, eps_bp=2e-5, bp=None, ties=True):
    """Scenarios whose arg-min is decided inside float32 noise (documented in DESIGN.md):
    some candidate that could win sits within eps of a constraint threshold, or the best
    two feasible costs are closer than eps, or a stage argument of a contender lies
    within eps of a curvature break-point."""
    J, g, feas = ref['J'], ref['g'], ref['feas']
    Jm = np.where(feas, J, np.inf)
    best = Jm.min(axis=1)
    contender = J <= (best[:, None] + eps_cost)             # could win if verdict flipped
    near_thr = np.abs(g - P.feas_tol) < eps_margin
    amb = (contender & near_thr).any(axis=1)
    if ties:
        # the runner-up that matters is the best candidate whose CONTROLS differ from the winner's: candidates with the
        # same control sequence (targets clipped to the same envelope / box) are the same arithmetic on the same numbers,
        # tie exactly on both sides, and the lowest index wins on both sides (test_exact_ties_across_slices_resolve_to_the_lowest_index)
        rival = Jm
        if 'U' in ref:
            Uw = ref['U'][np.arange(J.shape[0]), np.argmin(Jm, axis=1)]
            rival = np.where((ref['U'] == Uw[:, None]).all(axis=(-1, -2)), np.inf, Jm)
        else:
            rival = np.sort(Jm, axis=1)[:, 1:2]
        with np.errstate(invalid='ignore'):
            amb |= (rival.min(axis=1) - best) < eps_cost
    if bp is not None:
        amb |= (contender & (bp < eps_bp)).any(axis=1)
    return amb


def share_floor(share, B):
    """The floor asserted for a measured compared share: less one scenario, or 0.02 (whichever is larger)."""
    return share - max(0.02, 1.0 / B)


def _contender_breakpoints(r, P, x0, kp, tie):
    """O.breakpoint_distance of the candidates ambiguous_mask asks about -- those within `tie` of the best feasible cost --, +inf
    for every other one (re-rolling all of them is half the oracle's time)."""
    best = np.where(r['feas'], r['J'], np.inf).min(axis=1)
    ii, cc = np.nonzero(r['J'] <= best[:, None] + tie)
    bp = np.full(r['J'].shape, np.inf)
    if len(ii):
        bp[ii, cc] = O.breakpoint_distance(x0[ii, 0], r['U'][ii, cc], kp[ii, 0], P)
    return bp


def set_asides(passes, P, x0, kp, eps, tie, use_bp=True):
    """-> (amb, edge): scenarios that ANY pass decided inside eps of a threshold or a break-point or inside `tie` of a near-tie
    (a different winner re-centres the next pass), and the same without the near-ties.  Oracle-side only."""
    B = len(passes[0]['argmin'])
    amb, edge = np.zeros(B, dtype=bool), np.zeros(B, dtype=bool)
    for r in passes:
        bp = _contender_breakpoints(r, P, x0, kp, tie) if use_bp else None
        amb |= ambiguous_mask(r, P, eps, tie, eps, bp)
        edge |= ambiguous_mask(r, P, eps, tie, eps, bp, ties=False)
    return amb, edge


def measure(passes, P, x0, kp, eps, tie, use_bp=True):
    """What the oracle alone says about a comparison: -> (dict(B, compared, tie_compared, solved, winners, crossing), amb, edge).
    solved: compared scenarios the last pass solves; winners: their distinct winning indices; crossing: those on a turning
    route whose winning trajectory crosses a curvature break-point (s_0 < b <= s_N)."""
    amb, edge = set_asides(passes, P, x0, kp, eps, tie, use_bp)
    ref = passes[-1]
    sol = ~amb & (ref['status'] == 0)
    k = kp[:, 0]
    with np.errstate(invalid='ignore'):
        s0, sN = ref['x'][:, O.IS, 0], ref['x'][:, O.IS, -1]
        cross = sol & (k[:, 2] != 0) & (((s0 < k[:, 0]) & (sN >= k[:, 0])) | ((s0 < k[:, 1]) & (sN >= k[:, 1])))
    m = dict(B=len(amb), compared=int((~amb).sum()), tie_compared=int((~edge).sum()), solved=int(sol.sum()),
             winners=len(set(ref['argmin'][sol].tolist())), crossing=int(cross.sum()))
    return m, amb, edge


_FLOORS = None


def floors(key):
    """The recorded, CPU-measured figures of one comparison (tests/golden/parity_floors.json, written by
    tools/parity_floors.py --write and held to the inputs by tests/test_parity_floors_host.py):
    -> dict(share, tie_share, min_solved)."""
    global _FLOORS
    if _FLOORS is None:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'parity_floors.json')) as fh:
            _FLOORS = json.load(fh)['cases']
    e = _FLOORS[key]
    return dict(share=e['compared'] / e['B'], tie_share=e['tie_compared'] / e['B'], min_solved=e['min_solved'])


def compare_solve(got, passes, P, x0, kp, *, eps, tie, tol, utol=1e-7, ctol=None, xtol=None, share=1.0, tie_share=1.0, min_solved=0,
                  use_bp=True, crossing=0, label=''):
    """A device solve `got` (x, u, cost, argmin, status) against the oracle's passes (solve_batch(return_all=True) results; the
    last one is the answer), x0[B,1,7] with the flags applied, kp[B,1,3].

    Compared scenarios (outside the set-asides, set_asides): their share is at least `share` less one scenario (share_floor),
    at least `min_solved` of them are solved (and `crossing` of those cross a curvature break-point), status and arg-min are
    equal, x, u, cost agree within tol (xtol where a caller has measured that the trajectories need another bar) /
    max(tol, utol) / ctol on the solved ones.
    Set-aside scenarios still get a sensible answer: a single-pass pick is near-feasible (feas_tol + 10 tie) and within 10 tie
    of the best feasible cost by the oracle's own g and J, and a status 1 needs the oracle's best feasible candidate within eps
    of a threshold or a break-point; with refinement passes an early pick re-centres the later ones, so there the status is
    equal and the COST agrees within max(10 tol, 1e-7) wherever only near-ties were ambiguous (their share: tie_share);
    everywhere x is the roll-out of u, and status-1 rows carry NaN, +inf, -1.  -> the measured dict."""
    ctol = tol if ctol is None else ctol
    xtol = tol if xtol is None else xtol
    m, amb, edge = measure(passes, P, x0, kp, eps, tie, use_bp)
    ref, B = passes[-1], m['B']
    ok = ~amb
    sol = ok & (ref['status'] == 0)
    print(f'{label}: compared share {ok.mean():.4f} ({m["compared"]}/{B}), not edge-ambiguous {m["tie_compared"]}/{B}, '
          f'solved and compared {m["solved"]}, distinct winners {m["winners"]}, crossing a break-point {m["crossing"]}')
    assert ok.mean() >= share_floor(share, B), (label, 'compared share', ok.mean(), share)
    assert m['solved'] >= min_solved, (label, 'solved and compared', m['solved'], min_solved)
    assert m['crossing'] >= crossing, (label, 'compared winners that cross a break-point', m['crossing'])
    assert (got['status'][ok] == ref['status'][ok]).all(), label
    assert (got['argmin'][ok] == ref['argmin'][ok]).all(), label
    for k, t in (('x', xtol), ('u', max(tol, utol)), ('cost', ctol)):
        worst = rel_err(got[k][sol], ref[k][sol]).max(initial=0.0)
        assert worst <= t, (label, k, worst)
    # ---- the scenarios that were set aside
    single = len(passes) == 1
    if not single:
        t = ~edge
        assert t.mean() >= share_floor(tie_share, B), (label, 'share outside thresholds and break-points', t.mean(), tie_share)
        assert (got['status'][t] == ref['status'][t]).all(), label
        st = t & (ref['status'] == 0)
        worst = rel_err(got['cost'][st], ref['cost'][st]).max(initial=0.0)
        assert worst <= max(10 * tol, 1e-7, ctol), (label, 'cost where only near-ties were ambiguous', worst)
    else:
        for i in np.nonzero(amb)[0]:
            c = int(got['argmin'][i])
            Jm = np.where(ref['feas'][i], ref['J'][i], np.inf)
            best = Jm.min()
            if c >= 0:
                assert ref['g'][i, c] <= P.feas_tol + 10 * tie, (label, i, 'pick is not near-feasible', ref['g'][i, c])
                assert ref['J'][i, c] <= best + 10 * tie or not np.isfinite(best), (label, i, 'pick is not near-optimal')
            elif np.isfinite(best):
                cb = int(np.argmin(Jm))
                near = abs(ref['g'][i, cb] - P.feas_tol) < eps or \
                    O.breakpoint_distance(x0[i, 0], ref['U'][i, cb], kp[i, 0], P) < eps
                assert near, (label, i, 'status 1 although the best feasible candidate is clear of thresholds and break-points')
    rows = amb & (got['status'] == 0)
    u = got['u'][rows].astype(np.float64)
    X = O.rollout_frenet(x0[rows, 0], u, kp[rows, 0], P)
    e = rel_err(got['x'][rows], X).max(axis=(-1, -2))
    clear = O.breakpoint_distance(x0[rows, 0], u, kp[rows, 0], P) >= eps if rows.any() else np.zeros(0, dtype=bool)
    assert e[clear].max(initial=0.0) <= xtol, (label, 'x is not the roll-out of u', e[clear].max(initial=0.0))
    bad = got['status'] == 1
    assert np.isnan(got['x'][bad]).all() and np.isnan(got['u'][bad]).all(), label
    assert np.isposinf(got['cost'][bad]).all() and (got['argmin'][bad] == -1).all(), label
    assert (got['argmin'][~bad] >= 0).all(), label
    return m


def verdict_margins(X, U, obs_xy, cinf_A, cinf_b, P):
    """Worst signed violation PER VERDICT FAMILY (np_oracle.constraint_violation's bits 0, 1, 3, 4, 5; -inf where a family
    does not apply): [..., 7].  Lets a test say that a differing verdict bit sits on its threshold."""
    N = U.shape[-1]
    shape = np.broadcast_shapes(X.shape[:-2], U.shape[:-2])
    g = np.full(shape + (7,), -np.inf)
    v = X[..., O.IV, :N]
    g[..., 0] = np.max(np.maximum(P.v_min - v, v - P.v_max), axis=-1)
    a, d = U[..., 0, :], U[..., 1, :]
    g[..., 1] = np.max(np.maximum(np.maximum(P.a_min - a, a - P.a_max), np.maximum(-P.df_max - d, d - P.df_max)), axis=-1)
    g[..., 3] = np.max(np.abs(X[..., O.IEY, :]) - P.ey_lim, axis=-1)
    if cinf_A is not None and len(cinf_b):
        t = cinf_A[:, 0] * X[..., O.IV, N - 1, None] + cinf_A[:, 1] * U[..., 0, N - 1, None] - cinf_b
        g[..., 4] = np.max(t, axis=-1)
    if obs_xy is not None and obs_xy.shape[-3] > 0:
        dx = X[..., None, O.IX, 1:] - obs_xy[..., :, 0, 1:]
        dy = X[..., None, O.IY, 1:] - obs_xy[..., :, 1, 1:]
        g[..., 5] = np.max(P.d_min ** 2 - (dx * dx + dy * dy), axis=(-1, -2))
    return g
