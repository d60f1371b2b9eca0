"""No GPU: what the oracle and the restatements alone say about the stations of tests/derivative_cases.py, which
tests/test_gpu_derivative_limits.py holds the device to.

  * The restatement is a derivative at every station: adjoint_restated.cost_gradient agrees with central differences (step 1e-6)
    of np_oracle's own cost within 1e-6 max(1, |g|) on every gradient input (truncation measured at 3e-8 to 1.7e-7); the three
    value-network stations the same through value_gradient_restated.cost_gradient_vn.
  * The geometry stations can see l_r and l_f exchanged: the restated gradient moves by more than 1.
  * The conditions that keep the GPU tests from hiding anything, each asserted and, where it is a figure, held equal to
    derivative_cases.FACTS: at least 10 scenarios solved, one unsolved, one solved plan on a turning route; no gradient input
    with an RK stage argument within 1e-5 of a break-point; for the fd, adjoint and Newton restatements and iterations 1 and 2 no
    scenario whose two cheapest feasible trials are closer than 1e-7; no restated polished plan with its worst verdict margin
    within 1e-7 of feas_tol (see below for feas_tol = 0); tight-box: at least 4 polished plans on the input box in every mode;
    no-steer-rate: every polished plan's steering row is clip(u_prev[1], +-df_max); no-effort: the count of determinants <= 0.
  * The n_rk4 = 4 stations reach both hi_order values and rear-short-rk7 the (0, run-time sub-steps) leaf, by
    parity_cases.leaf_hi_order.

The margin condition at feas_tol = 0 (tol0-vmin).  The projection of a trial clamps each step to the rate window around the
step before it and to the input box, so nearly every polished plan holds some rate limit exactly: its rate margin is 0 or one
rounding of a - a_prev away from 0, and at feas_tol = 0 that IS the threshold.  Seeds 1 to 12 and 2026 all show it (a worst
margin of exactly 0 in every mode, and 1 to 6 lattice winners off the rate limit by a rounding): it belongs to the projection,
not to a seed, and it is what the station is there for (verdicts without a tolerance band).  There the condition is asked of what device and restatement compute differently:
the worst margin over the verdicts that read the rolled states (speed box, lane, terminal set, collision) stays 1e-7 away from
feas_tol, and the input verdicts (box, rate), which both sides form with the same two IEEE subtractions from the same clamped
inputs, are either more than 1e-7 inside or within 1e-14 of the limit.  For the same reason the lattice's own winners, which the
solve does not judge by the rate verdict, may miss it by one rounding at feas_tol = 0: FACTS['tol0-vmin']['rate_ulp'] of the
solved scenarios do (measured: their steering steps, by at most 6.9e-17), and no trial of theirs is feasible, so the polish leaves them alone."""
import numpy as np
import pytest

import adjoint_restated as A
import derivative_cases as DC
import np_oracle as O
import parity_cases as PC
import polish_restated as R
import value_gradient_restated as VG
from helpers import verdict_margins

BAND = 1e-7           # near-ties and verdict margins
STATIONS = list(DC.STATIONS)


def _central_differences(cost, U, step=1e-6):
    g = np.empty_like(U)
    for r in range(2):
        for k in range(U.shape[-1]):
            Up, Um = U.copy(), U.copy()
            Up[:, r, k] += step
            Um[:, r, k] -= step
            g[:, r, k] = (cost(Up) - cost(Um)) / (2 * step)
    return g


@pytest.mark.parametrize('station', STATIONS)
def test_restated_gradient_is_the_derivative_of_the_oracles_cost(station):
    c = DC.build(station)
    x0, kp, flags, U = DC.grad_inputs(station)
    P = c['P']
    xf = O.apply_flags(x0, flags)
    bp = O.breakpoint_distance(xf, U, kp, P)
    assert bp.min() >= 1e-5, ('a stage argument on a break-point', bp.min())        # the GPU comparison sets nothing aside
    J, g = A.cost_gradient(x0, kp, flags, U, P)
    assert np.isfinite(J).all() and np.isfinite(g).all()
    X = O.rollout_frenet(xf, U, kp, P)
    assert (kp[:, 2] == 0).any() and (kp[:, 2] != 0).any()                          # straight and turning routes
    assert (np.abs(X[:, O.IEY]).max(axis=-1) > P.ey_lim + 0.1).any()                # some sequences leave the lane
    cd = _central_differences(lambda V: O.stage_cost(O.rollout_frenet(xf, V, kp, P), V, P), U)
    err = (np.abs(g - cd) / np.maximum(1.0, np.abs(g))).max()
    print(f'{station}: max |g| {np.abs(g).max():.1f}, restatement against central differences {err:.2e}, break-points {bp.min():.2e} away')
    assert err <= 1e-6


@pytest.mark.parametrize('station', list(DC.VN_GRADIENT))
def test_restated_value_gradient_is_the_derivative_of_the_oracles_cost(station):
    c = DC.build(station)
    x0, kp, flags, U = DC.grad_inputs(station)
    net = DC.net_of(station)
    J, g = VG.cost_gradient_vn(x0, kp, flags, c['tv_sv'], c['enc'], U, c['P'], net)
    assert np.isfinite(J).all() and np.isfinite(g).all()
    cd = _central_differences(lambda V: VG.cost_vn(x0, kp, flags, c['tv_sv'], c['enc'], V, c['P'], net), U)
    err = (np.abs(g - cd) / np.maximum(1.0, np.abs(g))).max()
    print(f'{station}: max |g| {np.abs(g).max():.1f}, value-network restatement against central differences {err:.2e}')
    assert err <= 1e-6


@pytest.mark.parametrize('station', DC.GEOMETRY)
def test_geometry_stations_see_l_r_and_l_f_exchanged(station):
    c = DC.build(station)
    x0, kp, flags, U = DC.grad_inputs(station)
    J, g = A.cost_gradient(x0, kp, flags, U, c['P'])
    Js, gs = A.cost_gradient(x0, kp, flags, U, DC.swapped(c['P']))
    print(f'{station}: exchanging l_r and l_f moves the gradient by {np.abs(gs - g).max():.2f}, the cost by {np.abs(Js - J).max():.2f}')
    assert np.abs(gs - g).max() > 1.0
    # ... which the default geometry cannot: lr_ratio = 0.5 either way
    P0 = O.Params(N=DC.N)
    assert np.array_equal(A.cost_gradient(x0, kp, flags, U, P0)[1], A.cost_gradient(x0, kp, flags, U, DC.swapped(P0))[1])


def _margins(c, idx, u):
    """-> (worst margin over every verdict, over the verdicts that read the rolled states, box margin, rate margin), each [n]"""
    P = c['P']
    _, feas, g = R.evaluate(c, idx, u[:, None], P, c['cinf'])
    X = O.rollout_frenet(O.apply_flags(c['x0'][idx], c['flags'][idx]), u, c['kparams'][idx], P)
    A_, b_ = c['cinf'] if c['cinf'] is not None else (None, None)
    fam = verdict_margins(X, u, c['obs_xy'][idx], A_, b_, P)
    prev = np.concatenate([c['u_prev'][idx][:, :, None], u[:, :, :-1]], axis=-1)
    rate = np.maximum(np.abs(u[:, 0] - prev[:, 0]) - P.dt * P.jerk, np.abs(u[:, 1] - prev[:, 1]) - P.dt * P.steer_rate).max(axis=-1)
    return g[:, 0], fam[:, [0, 3, 4, 5]].max(axis=-1), fam[:, 1], rate, feas[:, 0]


@pytest.mark.parametrize('station', STATIONS)
def test_conditions_that_keep_the_gpu_tests_from_hiding_anything(station):
    c, want = DC.build(station), DC.FACTS[station]
    P = c['P']
    r = DC.oracle_solve(station)
    idx = np.flatnonzero(r['status'] == 0)
    got = dict(solved=len(idx), turning=int((c['kparams'][idx, 2] != 0).sum()), hi_order=int(PC.leaf_hi_order(P)),
               facets=0 if c['cinf'] is None else len(c['cinf'][1]))
    assert got['solved'] >= 10 and got['solved'] < DC.B and got['turning'] >= 1, got
    _, seed_state, seed_box, seed_rate, seed_feas = _margins(c, idx, r['u'][idx])
    if P.feas_tol >= BAND:
        assert seed_feas.all()                                # the lattice's winners keep the rate limits as well
    else:
        got['rate_ulp'] = int((~seed_feas).sum())             # ... or miss them by a rounding, and nothing else
        assert (seed_state <= P.feas_tol - BAND).all() and (seed_box <= P.feas_tol).all() and (seed_rate <= 1e-14).all()
    plans = {}
    for mode in DC.MODES:
        _, hist, ties = DC.restated(station, mode)
        for k in range(1, DC.ITERS + 1):
            assert ties[k - 1].min() >= BAND, (mode, k, 'a near-tie between the two cheapest trials', ties[k - 1].min())
            u = hist[k][0]
            g, state, box, rate, feas = _margins(c, idx, u)
            moved = hist[k][1] < hist[0][1]
            assert feas[moved].all()
            if P.feas_tol >= BAND:
                assert feas.all()
                assert (np.abs(g - P.feas_tol) >= BAND).all(), (mode, k, 'a verdict margin on feas_tol', np.abs(g - P.feas_tol).min())
            else:
                assert (np.abs(state - P.feas_tol) >= BAND).all(), (mode, k, np.abs(state - P.feas_tol).min())
                for m in (box, rate):
                    assert ((m <= P.feas_tol - BAND) | (np.abs(m - P.feas_tol) <= 1e-14)).all(), (mode, k)
                assert np.array_equal(moved, seed_feas)       # a seed off the rate limit by a rounding has no feasible trial
        plans[mode] = hist[DC.ITERS][0]
        print(f'{station} {mode}: {got["solved"]} solved, {int((hist[DC.ITERS][1] < hist[0][1] - 1e-9).sum())} moved, mean drop '
              f'{(hist[0][1] - hist[DC.ITERS][1]).mean():.4f}, closest trials {min(t.min() for t in ties):.1e}')
    if station == 'tight-box':
        got['on_box'] = {mode: int(DC.on_box(u, P).sum()) for mode, u in plans.items()}
        assert min(got['on_box'].values()) >= 4, got['on_box']
    if P.steer_rate == 0.0:
        for mode, u in plans.items():
            assert np.array_equal(u[:, 1], DC.frozen_steering(c, idx)), mode
    if station == 'no-effort':
        got['det_nonpos'] = DC.det_nonpos(station)
    print(station, got)
    assert got == want, (got, want)


def test_stations_reach_the_leaves_of_the_dispatch():
    hi = {s: int(PC.leaf_hi_order(DC.build(s)['P'])) for s in STATIONS}
    rk4 = [s for s in STATIONS if DC.build(s)['n_rk4'] == 4]
    assert {hi[s] for s in rk4} == {0, 1}
    assert hi['rear-short'] == hi['dt-coarse'] == hi['fast'] == 1 and hi['rear-long'] == 0      # through l_r, dt and v_max
    assert DC.build('rear-short-rk7')['n_rk4'] == 7 and hi['rear-short-rk7'] == 0
    assert all(hi[s] == DC.FACTS[s]['hi_order'] for s in STATIONS)


def test_value_network_stations_are_solved_and_moved():
    """what tests/test_gpu_value_polish*.py ask of a batch before they compare it: at least 8 solved, more than half moved"""
    import value_polish_restated as VP
    for station in DC.VN_POLISH:
        c, net = DC.build(station), DC.net_of(station)
        A_, b_ = c['cinf']
        r = O.solve_batch(c['x0'], c['u_prev'], c['kparams'], c['flags'], c['obs_xy'], A_, b_, c['P'], C=DC.C, net=net,
                          tv_sv=c['tv_sv'], enc=c['enc'])
        idx = np.flatnonzero(r['status'] == 0)
        hist, ties = VP.polish_value(c, idx, r['u'][idx], r['cost'][idx], 1, c['P'], c['cinf'], net)
        assert len(idx) >= 8 and ((hist[0][1] - hist[1][1]) > 1e-9).mean() > 0.5, station
