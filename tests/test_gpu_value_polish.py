"""-m gpu : the polish of the winner under the value-network cost (BatchSolver(value_polish_iters=) / set_value_polish, applied by
solve() to host arrays; today driven from the host: the gradient by igt_cost_gradient_vn_f64, the 64 trials rolled, judged and
priced by igt_rollout_batch_f64 on a table handle), float64.

Networks as in tests/test_gpu_value_gradient.py (copied, not imported): V_GT_sc1 (two hidden layers) and V_GT_sc3 (three) with a
non-identity whitening, sigma_t = 1.7, mu_t = -0.4.  Shapes: B = 1, 17, 64, 256, 300 and 1024 at N = 20, N = 40, N = 64 with three
obstacles per scenario, one n_rk4 = 2 case; lattice, ramp-hold and tracking seeds.
  * value_polish_iters = 0, and a handle that never called the setter, give identical bits;
  * for 1..4 iterations argmin and status are the solve's, unsolved rows stay NaN / +inf / -1, cost(k) <= cost(k - 1), a scenario
    whose cost did not move kept x and u bit for bit, and iteration 1 moves more than half of the solved scenarios by more than
    1e-9 (the restatement moves all of them);
  * x is bit for bit the X igt_rollout_batch_f64 of a value-net table handle gives for u fed back as candidates, no verdict
    raised, and cost is that roll-out's within 1e-9 max(1, |ref|) -- for the host-driven steps this only shows that the plan,
    its states and its cost belong together (x comes from such a roll-out); the independent check is the oracle's;
  * it is the oracle's (rollout_frenet, stage_cost with terminal_value, verdicts) at the suite's float64 bar, plans the oracle calls
    infeasible with their worst margin within 1e-9 of feas_tol set aside (at most 1 %);
  * it follows the numpy restatement (tests/value_polish_restated.py) from the same seeds within 1e-6 in cost after 1 and 2
    iterations -- the bar of test_gpu_gradient.test_device_follows_the_adjoint_restatement for the same construction --, a scenario
    set aside only if its two best trials are closer than 1e-7 and it did diverge (at most 2 %);
  * MPC_Planner(value_polish_iters=) returns the batch solve's polished plan, the closed-loop driver in gt_mpc runs with
    value_polish_iters = 1 to other trajectories than without, and the refusals: a progress handle, float32, iters = 5, device
    tensors, the device-resident loop.
Not here, because the steps are not on the device yet: device tensors against host arrays, replay from a stream graph, growth
under capture, four handles in flight, the device-resident closed loop -- each is refused with an error instead."""
import functools

import numpy as np
import pytest

import np_oracle as O
import value_polish_restated as VP
from helpers import oracle_params, rel_err
from igtmpc import _lib as L

pytestmark = pytest.mark.gpu

KEYS = ('x', 'u', 'cost', 'argmin', 'status')
# B, N, n_obs, n_rk4, network, family
CONFIGS = [(1, 20, 1, 4, 1, 'lattice'), (17, 20, 1, 4, 3, 'lattice'), (64, 20, 1, 4, 1, 'lattice'), (256, 20, 1, 4, 3, 'lattice'),
           (300, 20, 1, 4, 1, 'track'), (1024, 20, 1, 4, 1, 'lattice'), (64, 40, 1, 4, 3, 'ramp_hold'), (128, 64, 3, 4, 1, 'lattice'),
           (64, 20, 1, 2, 1, 'lattice')]


def _cinf(dt=0.1):
    from igtmpc.cinf import cinf_halfplanes
    return cinf_halfplanes(dt=dt)


@functools.lru_cache(maxsize=None)
def _net(sc, sigma_t=1.7):
    from igtmpc import shipped_value_net
    rng = np.random.default_rng(100 + sc)
    return dict(shipped_value_net(sc), Wn=np.eye(6) + 0.05 * rng.normal(size=(6, 6)),
                mu_f=np.array([20.0, 2.5, 0.0, 0.0, 0.0, 0.0]) + 0.1 * rng.normal(size=6), sigma_t=sigma_t, mu_t=-0.4)


@functools.lru_cache(maxsize=None)
def _batch(B, N, n_obs, seed=2026):
    """make_batch(max(B, 64)) cut to B rows; B = 1 is row 2 (solved by the lattice at N = 20).  More vehicles: the forecast
    shifted sideways, one more per obstacle (tests/test_gpu_polish.py _batch)."""
    from igtmpc.scenarios import make_batch
    b = make_batch(max(B, 64), N=N, dtype=np.float64, seed=seed)
    b['obs_xy'] = np.concatenate([b['obs_xy'] + 2.5 * m * np.array([1.0, -1.0])[None, None, :, None] for m in range(n_obs)], axis=1)
    lo = 2 if B == 1 else 0
    return {k: np.ascontiguousarray(v[lo:lo + B]) for k, v in b.items() if isinstance(v, np.ndarray) and len(v) == max(B, 64)}


def _args(b):
    return b['x0'], b['u_prev'], b['kparams'], b['flags'], b['obs_xy'], b['tv_sv'], b['enc']


def _solver(N, n_obs, n_rk4, sc, cand, **kw):
    import igtmpc
    s = igtmpc.BatchSolver(dtype='f64', cand_mode=cand, cost_mode='value_net', N=N, n_obs=n_obs, n_rk4=n_rk4, **kw)
    s.set_cinf(*_cinf())
    net = _net(sc)
    s.set_value_net(net['layers'], net['Wn'], net['mu_f'], net['sigma_t'], net['mu_t'])
    return s


@functools.lru_cache(maxsize=None)
def _solved(B, N, n_obs, n_rk4, sc, cand, iters=(0, 1, 2, 3, 4)):
    """{k: outputs of a host-mode solve with value_polish_iters = k} -- one handle, the setter between the solves -- and the
    oracle's parameters"""
    b = _batch(B, N, n_obs)
    out = {}
    with _solver(N, n_obs, n_rk4, sc, cand) as s:
        for k in iters:
            s.set_value_polish(k)
            out[k] = s.solve(*_args(b))
        P = oracle_params(s)
    return out, P


@pytest.mark.parametrize('B,N,n_obs,n_rk4,sc,cand', CONFIGS)
def test_zero_iterations_change_nothing(B, N, n_obs, n_rk4, sc, cand):
    b = _batch(B, N, n_obs)
    with _solver(N, n_obs, n_rk4, sc, cand) as s:             # the setter never called
        assert s.value_polish_iters == 0
        plain = s.solve(*_args(b))
    with _solver(N, n_obs, n_rk4, sc, cand, value_polish_iters=0) as s:      # the keyword, and the setter after a polished solve
        zero = s.solve(*_args(b))
        s.set_value_polish(1)
        s.solve(*_args(b))
        s.set_value_polish(0)
        again = s.solve(*_args(b))
    first = _solved(B, N, n_obs, n_rk4, sc, cand)[0][0]
    assert (plain['status'] == 0).any()
    if B >= 17:
        assert (plain['status'] != 0).any()                   # both kinds of scenario are in the batch
    for k in KEYS:
        for other in (zero, again, first):
            assert np.array_equal(plain[k], other[k], equal_nan=True), k


@pytest.mark.parametrize('B,N,n_obs,n_rk4,sc,cand', CONFIGS)
def test_monotone_and_bookkeeping_untouched(B, N, n_obs, n_rk4, sc, cand):
    out, _ = _solved(B, N, n_obs, n_rk4, sc, cand)
    ok = out[0]['status'] == 0
    for k in range(1, 5):
        assert np.array_equal(out[k]['argmin'], out[0]['argmin']) and np.array_equal(out[k]['status'], out[0]['status'])
        assert (out[k]['cost'][ok] <= out[k - 1]['cost'][ok]).all()
        assert np.isnan(out[k]['x'][~ok]).all() and np.isnan(out[k]['u'][~ok]).all()
        assert np.isposinf(out[k]['cost'][~ok]).all() and (out[k]['argmin'][~ok] == -1).all()
        same = out[k]['cost'] == out[k - 1]['cost']           # a scenario whose cost did not move kept its plan
        assert np.array_equal(out[k]['u'][ok & same], out[k - 1]['u'][ok & same])
        assert np.array_equal(out[k]['x'][ok & same], out[k - 1]['x'][ok & same])
    drop = out[0]['cost'][ok] - out[1]['cost'][ok]
    print(f'{cand} sc{sc} B={B} N={N} n_rk4={n_rk4}: {ok.sum()} solved, mean cost drop after 1 / 2 / 4 iterations',
          ' / '.join(f'{(out[0]["cost"][ok] - out[k]["cost"][ok]).mean():.4f}' for k in (1, 2, 4)),
          f'; moved by iteration 1: {(drop > 1e-9).mean():.3f}')
    assert (drop > 1e-9).mean() > 0.5


@pytest.mark.parametrize('B,N,n_obs,n_rk4,sc,cand', CONFIGS)
def test_polished_plan_is_its_own_table_rollout(B, N, n_obs, n_rk4, sc, cand):
    b = _batch(B, N, n_obs)
    out, _ = _solved(B, N, n_obs, n_rk4, sc, cand)
    worst = 0.0
    with _solver(N, n_obs, n_rk4, sc, 'table', C=64) as t:
        for k in (1, 4):
            got = out[k]
            idx = np.flatnonzero(got['status'] == 0)
            assert (got['cost'][idx] < out[0]['cost'][idx]).mean() > 0.5          # plans the polish wrote, not the emit pass
            for c0 in range(0, len(idx), 64):
                ch = idx[c0:c0 + 64]
                U = np.zeros((64, 2, N))
                U[:len(ch)] = got['u'][ch]
                t.set_candidate_table(U)
                r = t.rollout_all(*(np.ascontiguousarray(a[ch]) for a in _args(b)), want_U=False)
                d = np.arange(len(ch))
                assert np.array_equal(r['X'][d, d], got['x'][ch]), (k, c0)
                assert (r['viol'][d, d] == 0).all(), (k, c0)
                e = rel_err(got['cost'][ch], r['cost'][d, d]).max()
                worst = max(worst, e)
                assert e <= 1e-9, (k, c0, e)
    print(f'{cand} sc{sc} B={B} N={N}: max rel err of cost_out against the table roll-out {worst:.2e}')


@pytest.mark.parametrize('B,N,n_obs,n_rk4,sc,cand', CONFIGS)
def test_polished_plan_against_the_oracle(B, N, n_obs, n_rk4, sc, cand):
    b = _batch(B, N, n_obs)
    out, P = _solved(B, N, n_obs, n_rk4, sc, cand)
    cinf, net = _cinf(), _net(sc)
    for k in (1, 2, 4):
        got = out[k]
        idx = np.flatnonzero(got['status'] == 0)
        U = got['u'][idx]
        x0 = O.apply_flags(b['x0'][idx], b['flags'][idx])
        X = O.rollout_frenet(x0, U, b['kparams'][idx], P)
        V = O.terminal_value(net, X[:, None, O.IS, N], X[:, None, O.IV, N], b['tv_sv'][idx], b['enc'][idx])[:, 0]
        J = O.stage_cost(X, U, P, terminal_value=V)
        ex, ej = rel_err(got['x'][idx], X).max(), rel_err(got['cost'][idx], J).max()
        g, mask = O.constraint_violation(X, U, b['u_prev'][idx], b['obs_xy'][idx], cinf[0], cinf[1], P, check_rate=True)
        near = np.abs(g - P.feas_tol) <= 1e-9
        aside = near & (mask != 0)                            # only what needs it: infeasible by the oracle, on the threshold
        print(f'{cand} sc{sc} B={B} N={N} k={k}: max rel err x {ex:.2e} cost {ej:.2e}; set aside {aside.mean():.4f} of {len(idx)} '
              f'(within 1e-9 of feas_tol: {near.mean():.4f})')
        assert ex <= 1e-9 and ej <= 1e-9
        assert aside.mean() <= 0.01
        assert (mask[~aside] == 0).all()


@pytest.mark.parametrize('B,N,sc,cand', [(256, 20, 1, 'lattice'), (256, 20, 3, 'ramp_hold'), (256, 20, 1, 'track'), (64, 40, 1, 'track')])
def test_device_follows_the_restatement(B, N, sc, cand):
    b = _batch(B, N, 1)
    out, P = _solved(B, N, 1, 4, sc, cand, (0, 1, 2))
    cinf, net = _cinf(), _net(sc)
    idx = np.flatnonzero(out[0]['status'] == 0)
    assert len(idx) >= 8
    J0, f0, _ = VP.evaluate(b, idx, out[0]['u'][idx][:, None], P, cinf, net)
    assert f0.all() and rel_err(J0[:, 0], out[0]['cost'][idx]).max() <= 1e-9
    hist, ties = VP.polish_value(b, idx, out[0]['u'][idx], J0[:, 0], 2, P, cinf, net)
    tied = np.zeros(len(idx), dtype=bool)
    for k in (1, 2):
        tied |= ties[k - 1] < 1e-7
        diff = np.abs(out[k]['cost'][idx] - hist[k][1])
        aside = tied & (diff > 1e-6)                          # only a near-tie that did send the two down different steps
        print(f'{cand} sc{sc} B={B} N={N} k={k}: max |J_device - J_restated| {diff[~aside].max():.2e} (all: {diff.max():.2e}); '
              f'set aside {aside.mean():.4f} of {len(idx)} (near-ties: {tied.mean():.4f}); mean drop device '
              f'{(out[0]["cost"][idx] - out[k]["cost"][idx]).mean():.4f} restatement {(J0[:, 0] - hist[k][1]).mean():.4f}')
        assert aside.mean() <= 0.02
        assert diff[~aside].max() <= 1e-6


def test_planner_solves_with_the_option():
    """MPC_Planner(value_polish_iters=2).solve() on one problem of the batch (its buffers filled from the row): the plan a
    BatchSolver with the option gives for the same problem, cheaper than the plan without it; the option has its own handle."""
    from igtmpc import routes as R
    from igtmpc.planner import MPC_Planner
    b = _batch(64, 20, 1)
    row = int(np.flatnonzero(_solved(64, 20, 1, 4, 1, 'lattice', (0, 2))[0][0]['status'] == 0)[0])
    from igtmpc.scenarios import make_batch
    full = make_batch(64, N=20, dtype=np.float64, seed=2026)
    pair = [R.ROUTES[int(full['ego_rid'][row])], R.ROUTES[int(full['opp_rid'][row])]]
    net = _net(1)
    vn = dict(layers=net['layers'], Wn=net['Wn'], mu_f=net['mu_f'], sigma_t=net['sigma_t'], mu_t=net['mu_t'])
    import igtmpc
    st = lambda x, r: igtmpc.VehicleReference({'x': x[0], 'y': x[1], 's': x[2], 'ey': x[3], 'epsi': x[4], 'v': x[5], 'heading': x[6],
                                               'K': igtmpc.Curvature.from_route(r)})
    agents = [{'type': 'CAV', 'state': st(b['x0'][row], pair[0])}, {'type': 'CAV', 'state': st(b['x0'][row], pair[1])}]
    got = {}
    for k in (0, 2):
        pl = MPC_Planner(N=20, dt=0.1, agents=agents, routes=pair, index=0, num_rk4_steps=4, use_NN_cost2go=True, value_net=vn,
                         cand_mode='lattice', value_polish_iters=k)
        assert pl._solver.value_polish_iters == k
        pl._x0[0], pl._u_prev[0], pl._obs[0] = b['x0'][row], b['u_prev'][row], b['obs_xy'][row]
        pl._tv_sv[0], pl._enc[0] = b['tv_sv'][row], b['enc'][row]
        x, u, ok = pl.solve()
        assert ok
        got[k] = (pl, x, u, pl.sol.stats()['cost'])
        flags = np.array([1 if pl._abs_heading[0] else 0], dtype=np.uint32)
        with _solver(20, 1, 4, 1, 'lattice', value_polish_iters=k, d_min=pl.d_min) as s:
            ref = s.solve(pl._x0, pl._u_prev, np.array([pl.K.kparams]), flags, pl._obs, pl._tv_sv, pl._enc)
        assert np.array_equal(ref['u'][0], u) and np.array_equal(ref['x'][0], x)
    assert got[0][0]._solver is not got[2][0]._solver
    assert got[2][3] < got[0][3] and not np.array_equal(got[0][2], got[2][2])


def test_closed_loop_driver_with_value_polish():
    from igtmpc.evaluate import run_closed_loop
    kw = dict(sc=1, num_samples=16, N=20, eval_mode='gt_mpc')
    plain = run_closed_loop(**kw)
    a = run_closed_loop(value_polish_iters=1, **kw)
    assert np.isfinite(a['x_data']).all()
    assert not np.array_equal(a['u_data'], plain['u_data'])
    for extra in (dict(device_resident=True), dict(device_resident=True, graph=True)):
        with pytest.raises(ValueError, match='host'):
            run_closed_loop(value_polish_iters=1, **extra, **kw)


def test_refusals():
    import igtmpc
    import torch
    b = _batch(64, 20, 1)
    with igtmpc.BatchSolver(dtype='f64', N=20) as p:                      # a progress handle: it has polish_iters
        with pytest.raises(ValueError, match='value_net'):
            p.set_value_polish(1)
        p.set_value_polish(0)
    with _solver(20, 1, 4, 1, 'lattice') as s:
        for k in (5, -1):
            with pytest.raises(ValueError, match=r'\[0, 4\]'):
                s.set_value_polish(k)
        assert s.value_polish_iters == 0
        s.set_value_polish(1)
        dev = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).contiguous().cuda() for a in _args(b)]
        with pytest.raises(TypeError, match='host'):                      # ... and with device tensors, stream capture
            s.solve(*dev)
        s.set_value_polish(0)
        o = s.solve(*dev)
        torch.cuda.synchronize()
        assert (o['status'] == 0).any()
    with igtmpc.BatchSolver(dtype='f64', cost_mode='value_net', N=20, value_polish_iters=1) as v:      # no network loaded
        with pytest.raises(L.IgtError, match='value net not set'):
            v.solve(*_args(b))
    with igtmpc.BatchSolver(dtype='f32', cost_mode='value_net', N=20) as f:
        with pytest.raises(ValueError, match='f64'):
            f.set_value_polish(1)
