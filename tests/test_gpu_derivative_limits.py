"""-m gpu : the derivative kernels and the four polishes away from the reference's default limits (igtmpc.h igt_cost_gradient_f64,
igt_cost_gradient_vn_f64, polish_iters with igt_set_polish_gradient / igt_set_polish_step, igt_set_value_polish;
csrc/igt_adjoint64.h, csrc/igt_kernels_f64.hip cost_gradient_f64_kernel, polish_f64_kernel, value_trials_f64_kernel /
value_accept_f64_kernel), float64, eager solves on host arrays.

One test is one station of tests/derivative_cases.py at B = 24, N = 20 (geometry with l_r != l_f, dt = 0.05 and 0.2, a frozen
steering rate, a box that binds inside the projection, w_u = 0 and 0.3, feas_tol = 0, speeds up to 15 m/s).  The bars are the
project's own (tests/test_gpu_gradient.py, tests/test_gpu_polish.py) and nothing is set aside:
tests/test_derivative_cases_host.py shows on the CPU that no gradient input has a stage argument within 1e-5 of a break-point, no
restated iteration a near-tie under 1e-7 and no restated plan a state verdict within 1e-7 of feas_tol, and that the restatements
are derivatives of the oracle's cost at these very stations.
  * cost gradient, every station: gradient and cost against adjoint_restated.cost_gradient within 1e-9 max(1, |ref|) on every
    scenario; cost_out within 1e-9 of rollout_all's cost of the same controls on a table handle of the station's limits;
  * value-network gradient (rear-short, dt-coarse, heavy-effort): the same against value_gradient_restated.cost_gradient_vn;
  * polish, every station x {fd, adjoint, newton}, polish_iters 0, 1, 2: argmin, status and the unsolved rows are those of
    polish_iters = 0 and the cost is monotone; x_out and cost_out are rollout_all's for u_out fed back as a table, bit for bit;
    the oracle's roll-out and cost of u_out within 1e-9 and the plan feasible by every verdict, the rate verdict included (see
    below); after 1 and 2 iterations |cost - restated cost| <= 1e-6 on every solved scenario; every plan inside the input box and
    the rate window as the projection forms them, without a tolerance; no-steer-rate: the steering row is clip(u_prev[1],
    +-df_max) bit for bit; tight-box: as many device plans on the box as the restatement has, less one at most;
  * value-network polish (rear-short, dt-coarse, no-steer-rate), both drivers, 1 and 2 iterations: the self-consistency, oracle and
    restatement assertions of tests/test_gpu_value_polish.py / test_gpu_value_polish_device.py with value_polish_restated and the
    station's parameters, and the two drivers against each other.

The rate verdict of a plan the polish left alone.  Such a plan is the lattice's winner, which the solve does not judge by the rate
verdict (np_oracle.solve_batch: generated families hold the limits by construction) and which keeps them up to one rounding of
a_k - a_k-1.  With feas_tol >= 1e-14 that is feasible as it stands; at feas_tol = 0 (tol0-vmin) the rounding shows, on 6 of 19
winners, and the polish, whose trials are judged by the rate verdict, moves none of them.  So: a plan the polish wrote raises no
verdict; a plan it left alone raises none but, possibly, the rate's, by no more than max(feas_tol, 1e-14); and wherever the device
raises the rate verdict on a fed-back plan, the oracle does on the same numbers, and the reverse.
The measured maxima (profiles/derivative_limits.txt) are printed before they are asserted."""
import numpy as np
import pytest

import adjoint_restated as A
import derivative_cases as DC
import np_oracle as O
import polish_restated as R
import value_gradient_restated as VG
import value_polish_restated as VP
from helpers import oracle_params, rel_err

pytestmark = pytest.mark.gpu

STATIONS = list(DC.STATIONS)
BAR = 1e-9                # DESIGN.md section 6, float64
FOLLOW = 1e-6             # device against restatement, in cost (tests/test_gpu_polish.py)
TIE = 1e-7
RATE_BIT = 4              # np_oracle.constraint_violation bit 2, VIOL_RATE
RATE_ROUNDING = 1e-14     # |a_k - a_k-1| - rate of a lattice plan: roundings of inputs below 16 (ulp 1.8e-15)


@pytest.fixture(scope='module')
def igt():
    import igtmpc
    return igtmpc


def _table_costs(igt, station, flags, U, **kw):
    """rollout_all's cost of U [B, 2, N] as the table of a table handle with the station's limits: scenario b, candidate b"""
    c = DC.build(station)
    n = len(U)
    T = np.zeros((64, 2, DC.N))
    T[:n] = U
    with DC.open_solver(igt, station, cand_mode='table', C=64, **kw) as t:
        t.set_candidate_table(T)
        args = DC.solve_args(c, vn='cost_mode' in kw)
        args[3] = flags
        return t.rollout_all(*args, want_X=False, want_U=False)['cost'][np.arange(n), np.arange(n)]


@pytest.mark.parametrize('station', STATIONS)
def test_cost_gradient(igt, station):
    x0, kp, flags, U = DC.grad_inputs(station)
    with DC.open_solver(igt, station) as s:
        got = s.cost_gradient(x0, kp, flags, U)
        P = oracle_params(s)
    J, g = A.cost_gradient(x0, kp, flags, U, P)
    assert np.isfinite(J).all() and np.isfinite(g).all()
    eg, ej = rel_err(got['grad'], g).max(), rel_err(got['cost'], J).max()
    et = rel_err(got['cost'], _table_costs(igt, station, flags, U)).max()
    print(f'derivative-limits gradient {station}: max |g| {np.abs(g).max():.1f}, max rel err grad {eg:.2e} cost {ej:.2e}, '
          f'cost against the table roll-out {et:.2e}')
    assert eg <= BAR and ej <= BAR
    assert et <= BAR


@pytest.mark.parametrize('station', list(DC.VN_GRADIENT))
def test_value_network_gradient(igt, station):
    c = DC.build(station)
    x0, kp, flags, U = DC.grad_inputs(station)
    with DC.open_solver(igt, station, cost_mode='value_net') as s:
        got = s.cost_gradient(x0, kp, flags, U, tv_sv=c['tv_sv'], enc=c['enc'])
        P = oracle_params(s)
    J, g = VG.cost_gradient_vn(x0, kp, flags, c['tv_sv'], c['enc'], U, P, DC.net_of(station))
    assert np.isfinite(J).all() and np.isfinite(g).all()
    eg, ej = rel_err(got['grad'], g).max(), rel_err(got['cost'], J).max()
    et = rel_err(got['cost'], _table_costs(igt, station, flags, U, cost_mode='value_net')).max()
    print(f'derivative-limits value gradient {station}: max |g| {np.abs(g).max():.1f}, max rel err grad {eg:.2e} cost {ej:.2e}, '
          f'cost against the table roll-out {et:.2e}')
    assert eg <= BAR and ej <= BAR
    assert et <= BAR


def _bookkeeping(out, iters):
    ok = out[0]['status'] == 0
    for k in iters:
        assert np.array_equal(out[k]['argmin'], out[0]['argmin']) and np.array_equal(out[k]['status'], out[0]['status'])
        assert (out[k]['cost'][ok] <= out[k - 1]['cost'][ok]).all() and (out[k]['cost'][ok] <= out[0]['cost'][ok]).all()
        assert np.isnan(out[k]['x'][~ok]).all() and np.isnan(out[k]['u'][~ok]).all()
        assert np.isposinf(out[k]['cost'][~ok]).all() and (out[k]['argmin'][~ok] == -1).all()
        same = out[k]['cost'] == out[k - 1]['cost']           # a scenario whose cost did not move kept its plan
        assert np.array_equal(out[k]['u'][ok & same], out[k - 1]['u'][ok & same])
        assert np.array_equal(out[k]['x'][ok & same], out[k - 1]['x'][ok & same])
    return ok


def _inside_box_and_rate_window(c, idx, u):
    """every input inside the box and inside the window [prev - rate, prev + rate] as the projection forms it: no tolerance"""
    P = c['P']
    prev = np.concatenate([c['u_prev'][idx][:, :, None], u[:, :, :-1]], axis=-1)
    ra, rd = P.dt * P.jerk, P.dt * P.steer_rate
    a, d = u[:, 0], u[:, 1]
    assert ((a >= P.a_min) & (a <= P.a_max) & (d >= -P.df_max) & (d <= P.df_max)).all()
    assert ((a >= prev[:, 0] - ra) & (a <= prev[:, 0] + ra) & (d >= prev[:, 1] - rd) & (d <= prev[:, 1] + rd)).all()


def _rate_margin(c, idx, u):
    P = c['P']
    prev = np.concatenate([c['u_prev'][idx][:, :, None], u[:, :, :-1]], axis=-1)
    return np.maximum(np.abs(u[:, 0] - prev[:, 0]) - P.dt * P.jerk, np.abs(u[:, 1] - prev[:, 1]) - P.dt * P.steer_rate).max(axis=-1)


@pytest.mark.parametrize('mode', DC.MODES)
@pytest.mark.parametrize('station', STATIONS)
def test_polish(igt, station, mode):
    c = DC.build(station)
    args = DC.solve_args(c)
    out = {}
    for k in (0, 1, 2):
        with DC.open_solver(igt, station, polish_iters=k, **DC.SOLVER_MODE[mode]) as s:
            out[k] = s.solve(*args)
            P = oracle_params(s)
    ok = _bookkeeping(out, (1, 2))
    idx = np.flatnonzero(ok)
    assert len(idx) >= 10 and (~ok).any() and (c['kparams'][idx, 2] != 0).any()
    sub = [np.ascontiguousarray(a[idx]) for a in args]
    d = np.arange(len(idx))
    x0f = O.apply_flags(c['x0'][idx], c['flags'][idx])
    A_, b_ = c['cinf'] if c['cinf'] is not None else (None, None)
    worst = dict(x=0.0, cost=0.0)
    with DC.open_solver(igt, station, cand_mode='table', C=64) as t:
        for k in (0, 1, 2):
            u = out[k]['u'][idx]
            wrote = out[k]['cost'][idx] != out[0]['cost'][idx]
            # --- its own table roll-out, bit for bit
            T = np.zeros((64, 2, DC.N))
            T[:len(idx)] = u
            t.set_candidate_table(T)
            r = t.rollout_all(*sub, want_U=False)
            assert np.array_equal(r['X'][d, d], out[k]['x'][idx]), k
            assert np.array_equal(r['cost'][d, d], out[k]['cost'][idx]), k
            viol = r['viol'][d, d].astype(np.int64)
            # --- the oracle's roll-out, cost and verdicts of the same controls
            X = O.rollout_frenet(x0f, u, c['kparams'][idx], P)
            J = O.stage_cost(X, u, P)
            worst['x'] = max(worst['x'], rel_err(out[k]['x'][idx], X).max())
            worst['cost'] = max(worst['cost'], rel_err(out[k]['cost'][idx], J).max())
            g, mask = O.constraint_violation(X, u, c['u_prev'][idx], c['obs_xy'][idx], A_, b_, P, check_rate=True)
            mask = mask.astype(np.int64)
            rate = _rate_margin(c, idx, u)
            print(f'derivative-limits polish {station} {mode} k={k}: {int(wrote.sum())} of {len(idx)} plans written; rate verdict raised on '
                  f'{int((mask & RATE_BIT != 0).sum())} (device: {int((viol & RATE_BIT != 0).sum())}), worst rate margin {rate.max():.2e}')
            assert (viol[wrote] == 0).all() and (mask[wrote] == 0).all(), k
            assert ((viol & ~RATE_BIT) == 0).all() and ((mask & ~RATE_BIT) == 0).all(), k
            assert (rate <= max(P.feas_tol, RATE_ROUNDING)).all(), k
            assert np.array_equal(viol & RATE_BIT, mask & RATE_BIT), k
            _inside_box_and_rate_window(c, idx, u)
            if P.steer_rate == 0.0:
                assert np.array_equal(u[:, 1], DC.frozen_steering(c, idx)), k
    print(f'derivative-limits polish {station} {mode}: max rel err against the oracle x {worst["x"]:.2e} cost {worst["cost"]:.2e}')
    assert worst['x'] <= BAR and worst['cost'] <= BAR
    # --- the restatement from the device's own seeds
    J0, _, _ = R.evaluate(c, idx, out[0]['u'][idx][:, None], P, c['cinf'])
    hist, ties = DC.restate(station, mode, idx, out[0]['u'][idx], J0[:, 0])
    for k in (1, 2):
        diff = np.abs(out[k]['cost'][idx] - hist[k][1])
        moved = (out[0]['cost'][idx] - out[k]['cost'][idx]) > 1e-9
        print(f'derivative-limits polish {station} {mode} k={k}: max |J_device - J_restated| {diff.max():.2e}; closest trials {ties[k - 1].min():.1e}; '
              f'moved {int(moved.sum())} of {len(idx)}; mean drop device {(out[0]["cost"][idx] - out[k]["cost"][idx]).mean():.4f} '
              f'restatement {(J0[:, 0] - hist[k][1]).mean():.4f}')
        assert ties[k - 1].min() >= TIE          # (the host test's condition, on the device's seeds)
        assert diff.max() <= FOLLOW
        if station == 'tight-box':
            dev, ref = int(DC.on_box(out[k]['u'][idx], P).sum()), int(DC.on_box(hist[k][0], P).sum())
            print(f'derivative-limits polish {station} {mode} k={k}: plans on the input box: device {dev}, restatement {ref}')
            assert dev >= ref - 1
            assert k < DC.ITERS or ref >= 4


@pytest.mark.parametrize('driver', ['host', 'device'])
@pytest.mark.parametrize('station', list(DC.VN_POLISH))
def test_value_network_polish(igt, station, driver):
    c, net = DC.build(station), DC.net_of(station)
    args = DC.solve_args(c, vn=True)
    out = {}
    with DC.open_solver(igt, station, cost_mode='value_net') as s:
        for k in (0, 1, 2):
            s.set_value_polish_driver(driver)
            s.set_value_polish(k)
            out[k] = s.solve(*args)
            if driver == 'device' and k > 0:                  # the other driver between the solves of one handle
                s.set_value_polish_driver('host')
                out['host', k] = s.solve(*args)
        P = oracle_params(s)
    ok = _bookkeeping(out, (1, 2))
    idx = np.flatnonzero(ok)
    assert len(idx) >= 8 and (~ok).any()
    drop = out[0]['cost'][ok] - out[1]['cost'][ok]
    assert (drop > 1e-9).mean() > 0.5
    # --- the table roll-out: x bit for bit, no verdict, cost within the bar
    sub = [np.ascontiguousarray(a[idx]) for a in args]
    d = np.arange(len(idx))
    worst = 0.0
    with DC.open_solver(igt, station, cand_mode='table', C=64, cost_mode='value_net') as t:
        for k in (1, 2):
            got = out[k]
            assert (got['cost'][idx] < out[0]['cost'][idx]).mean() > 0.5          # plans the polish wrote, not the emit pass
            T = np.zeros((64, 2, DC.N))
            T[:len(idx)] = got['u'][idx]
            t.set_candidate_table(T)
            r = t.rollout_all(*sub, want_U=False)
            assert np.array_equal(r['X'][d, d], got['x'][idx]), k
            assert (r['viol'][d, d] == 0).all(), k
            worst = max(worst, rel_err(got['cost'][idx], r['cost'][d, d]).max())
    print(f'derivative-limits value polish {station} {driver}: max rel err of cost_out against the table roll-out {worst:.2e}')
    assert worst <= BAR
    # --- the oracle
    x0f = O.apply_flags(c['x0'][idx], c['flags'][idx])
    for k in (1, 2):
        got = out[k]
        U = got['u'][idx]
        X = O.rollout_frenet(x0f, U, c['kparams'][idx], P)
        V = O.terminal_value(net, X[:, None, O.IS, DC.N], X[:, None, O.IV, DC.N], c['tv_sv'][idx], c['enc'][idx])[:, 0]
        J = O.stage_cost(X, U, P, terminal_value=V)
        ex, ej = rel_err(got['x'][idx], X).max(), rel_err(got['cost'][idx], J).max()
        g, mask = O.constraint_violation(X, U, c['u_prev'][idx], c['obs_xy'][idx], c['cinf'][0], c['cinf'][1], P, check_rate=True)
        near = np.abs(g - P.feas_tol) <= 1e-9
        aside = near & (mask != 0)                            # only what needs it: infeasible by the oracle, on the threshold
        print(f'derivative-limits value polish {station} {driver} k={k}: max rel err x {ex:.2e} cost {ej:.2e}; set aside {aside.mean():.4f} '
              f'of {len(idx)} (within 1e-9 of feas_tol: {near.mean():.4f})')
        assert ex <= BAR and ej <= BAR
        assert aside.mean() <= 0.01
        assert (mask[~aside] == 0).all()
        _inside_box_and_rate_window(c, idx, U)
        if P.steer_rate == 0.0:
            assert np.array_equal(U[:, 1], DC.frozen_steering(c, idx)), k
    # --- the restatement
    J0, f0, _ = VP.evaluate(c, idx, out[0]['u'][idx][:, None], P, c['cinf'], net)
    assert f0.all() and rel_err(J0[:, 0], out[0]['cost'][idx]).max() <= BAR
    hist, ties = VP.polish_value(c, idx, out[0]['u'][idx], J0[:, 0], 2, P, c['cinf'], net)
    tied = np.logical_or.accumulate([t < TIE for t in ties], axis=0)
    for k in (1, 2):
        diff = np.abs(out[k]['cost'][idx] - hist[k][1])
        aside = tied[k - 1] & (diff > FOLLOW)                 # only a near-tie that did send the two down different steps
        print(f'derivative-limits value polish {station} {driver} k={k}: max |J_device - J_restated| {diff[~aside].max(initial=0.0):.2e} '
              f'(all: {diff.max():.2e}); set aside {aside.mean():.4f} of {len(idx)} (near-ties: {tied[k - 1].mean():.4f}); mean drop device '
              f'{(out[0]["cost"][idx] - out[k]["cost"][idx]).mean():.4f} restatement {(J0[:, 0] - hist[k][1]).mean():.4f}')
        assert aside.mean() <= 0.02
        assert diff[~aside].max(initial=0.0) <= FOLLOW
        if driver == 'device':                                # the host driver on the same handle and inputs
            dev, host = out[k], out['host', k]
            assert np.array_equal(dev['argmin'], host['argmin']) and np.array_equal(dev['status'], host['status'])
            e = rel_err(dev['cost'][idx], host['cost'][idx])
            off = tied[k - 1] & (e > BAR)
            print(f'derivative-limits value polish {station} k={k}: max rel err of cost, device against host driver '
                  f'{e[~off].max(initial=0.0):.2e} (all: {e.max():.2e}); set aside {off.mean():.4f} of {len(idx)}')
            assert off.mean() <= 0.02
            assert e[~off].max(initial=0.0) <= BAR
