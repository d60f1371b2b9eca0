"""CPU: the polish of the winner under the value-network cost (gt_mpc), restated in numpy (tests/value_polish_restated.py) -- the
reference the solver's value_polish_iters option (today driven from the host through igt_cost_gradient_vn_f64 and
igt_rollout_batch_f64) is compared against on the GPU -- and what of that option needs no GPU: its place on the solver, the planner and the driver, and
its refusals.  `polish_iters > 0` stays refused with the value-network cost (tests/test_polish_host.py), repeated here for the
Python face.

The restatement is pinned on make_batch(64, N=20, seed=2026) with the networks of tests/test_gpu_value_gradient.py (V_GT_sc1, two
hidden layers; V_GT_sc3, three; a non-identity whitening, sigma_t = 1.7, mu_t = -0.4), seeded with the oracle's own lattice
winners under that cost: 49 solved each, every polished plan feasible by constraint_violation(check_rate=True), the cost
monotone, and the first iteration lowers every seed.  Mean cost drop after 1 / 2 / 4 iterations when this was written:
sc1 0.0972 / 0.1192 / 0.1424, sc3 0.0928 / 0.1148 / 0.1351."""
import functools
import inspect

import numpy as np
import pytest

import np_oracle as O
import value_polish_restated as VP
from igtmpc import _lib as L


@functools.lru_cache(maxsize=None)
def _net(sc, sigma_t=1.7):
    from igtmpc import shipped_value_net
    rng = np.random.default_rng(100 + sc)
    return dict(shipped_value_net(sc), Wn=np.eye(6) + 0.05 * rng.normal(size=(6, 6)),
                mu_f=np.array([20.0, 2.5, 0.0, 0.0, 0.0, 0.0]) + 0.1 * rng.normal(size=6), sigma_t=sigma_t, mu_t=-0.4)


@functools.lru_cache(maxsize=None)
def _seeds(sc):
    from igtmpc.cinf import cinf_halfplanes
    from igtmpc.scenarios import make_batch
    P, cinf, net = O.Params(), cinf_halfplanes(), _net(sc)
    b = make_batch(64, N=20, dtype=np.float64, seed=2026)
    sol = O.solve_batch(b['x0'], b['u_prev'], b['kparams'], b['flags'], b['obs_xy'], *cinf, P, net=net, tv_sv=b['tv_sv'],
                        enc=b['enc'])
    idx = np.flatnonzero(sol['status'] == 0)
    return b, idx, sol['u'][idx], sol['cost'][idx], P, cinf, net


@pytest.mark.parametrize('sc', [1, 3])
def test_restatement_is_feasible_monotone_and_moves_every_seed(sc):
    b, idx, u, J, P, cinf, net = _seeds(sc)
    assert len(idx) == 49
    Js, fs, _ = VP.evaluate(b, idx, u[:, None], P, cinf, net)
    # the seeds are the oracle's own winners under the value cost (the network is a matrix product whose summation order depends on
    # how many rows it is given, so a plan evaluated alone and among 256 candidates agrees to rounding, not bit for bit)
    assert fs.all() and (np.abs(Js[:, 0] - J) <= 1e-12 * np.maximum(1.0, np.abs(J))).all()
    hist, ties = VP.polish_value(b, idx, u, J, 4, P, cinf, net)
    assert len(hist) == 5 and len(ties) == 4
    for it in range(1, 5):
        uk, Jk = hist[it]
        Je, fe, _ = VP.evaluate(b, idx, uk[:, None], P, cinf, net)
        assert fe.all(), f'sc{sc}: infeasible plan after {it} iterations'
        assert (np.abs(Je[:, 0] - Jk) <= 1e-12 * np.maximum(1.0, np.abs(Jk))).all()
        assert (Jk <= hist[it - 1][1]).all() and (Jk <= J).all()
    drop1 = J - hist[1][1]
    print(f'sc{sc}: mean drop after 1 / 2 / 4 iterations',
          ' / '.join(f'{(J - hist[k][1]).mean():.4f}' for k in (1, 2, 4)), f'-- lowered by iteration 1: {(drop1 > 0).sum()} of {len(idx)}')
    assert (drop1 > 0).all()


def test_restated_gradient_step_is_a_descent_direction():
    """one iteration's direction against the restated cost: a short step along d lowers J for every seed (no projection, no verdicts)"""
    import value_gradient_restated as VG
    b, idx, u, J, P, cinf, net = _seeds(1)
    f = lambda k: np.asarray(b[k], dtype=np.float64)[idx]
    _, g = VG.cost_gradient_vn(f('x0'), f('kparams'), np.asarray(b['flags'])[idx], f('tv_sv'), f('enc'), u, P, net)
    assert np.isfinite(g).all()
    step = 1e-4 / np.abs(g).max(axis=(1, 2), keepdims=True)
    J1 = VG.cost_vn(f('x0'), f('kparams'), np.asarray(b['flags'])[idx], f('tv_sv'), f('enc'), u - step * g, P, net)
    assert (J1 < J + 1e-12).all() and (J1 < J).mean() > 0.9


def test_polish_iters_keeps_raising_with_the_value_cost(monkeypatch):
    import igtmpc
    lib = L.load()

    def no_create(*a):
        raise AssertionError('igt_create reached')
    monkeypatch.setattr(igtmpc.solver.L, 'load', lambda: type('NoCreate', (), {
        'igt_params_default': lib.igt_params_default, 'igt_create': no_create, 'igt_destroy': lambda *a: 0})())
    with pytest.raises(ValueError, match='progress'):
        igtmpc.BatchSolver(dtype='f64', cost_mode='value_net', polish_iters=1)


def test_solver_planner_and_driver_take_the_option():
    import igtmpc
    from igtmpc.evaluate import run_closed_loop
    from igtmpc.planner import MPC_Planner
    assert inspect.signature(igtmpc.BatchSolver.__init__).parameters['value_polish_iters'].default == 0
    assert list(inspect.signature(igtmpc.BatchSolver.set_value_polish).parameters) == ['self', 'k']
    assert inspect.signature(MPC_Planner.__init__).parameters['value_polish_iters'].default == 0
    assert inspect.signature(run_closed_loop).parameters['value_polish_iters'].default == 0
    assert not hasattr(L.igt_params, 'value_polish_iters')                   # an explicit keyword: the struct is not versioned
    src = inspect.getsource(MPC_Planner.__init__)
    assert 'value_polish_iters)' in src[src.index('key = ('):src.index('if key not in _SHARED')]      # part of the cache key ...
    assert 'value_polish_iters=value_polish_iters' in src                     # ... because the handle is built with it


@pytest.mark.parametrize('kw, word', [
    (dict(dtype='f64', cost_mode='value_net', value_polish_iters=5), '[0, 4]'),
    (dict(dtype='f64', cost_mode='value_net', value_polish_iters=-1), '[0, 4]'),
    (dict(dtype='f32', cost_mode='value_net', value_polish_iters=1), 'f64'),
    (dict(dtype='f64', cost_mode='progress', value_polish_iters=1), 'value_net'),
])
def test_python_refuses_before_igt_create(kw, word, monkeypatch):
    import igtmpc
    lib = L.load()

    def no_create(*a):
        raise AssertionError('igt_create reached')
    monkeypatch.setattr(igtmpc.solver.L, 'load', lambda: type('NoCreate', (), {
        'igt_params_default': lib.igt_params_default, 'igt_create': no_create, 'igt_destroy': lambda *a: 0})())
    with pytest.raises(ValueError, match=word.replace('[', r'\[').replace(']', r'\]')):
        igtmpc.BatchSolver(**kw)


@pytest.mark.parametrize('kw, word', [
    (dict(eval_mode='gt_mpc', value_polish_iters=5), '[0, 4]'),
    (dict(eval_mode='mpc', value_polish_iters=5), '[0, 4]'),
    (dict(eval_mode='gt_mpc', value_polish_iters=1, dtype='f32'), 'f64'),
    (dict(eval_mode='gt_mpc', value_polish_iters=1, device_resident=True), 'host'),
    (dict(eval_mode='gt_mpc', value_polish_iters=1, device_resident=True, graph=True), 'host'),
])
def test_driver_refuses_before_any_gpu_call(kw, word, monkeypatch):
    import igtmpc.evaluate as E

    def no_solver(*a, **k):
        raise AssertionError('BatchSolver reached')
    monkeypatch.setattr(E, 'BatchSolver', no_solver)
    with pytest.raises(ValueError, match=word.replace('[', r'\[').replace(']', r'\]')):
        E.run_closed_loop(sc=1, num_samples=2, N=20, **kw)
