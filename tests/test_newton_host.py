"""CPU: the Newton (LQ) mode of the polish as restated in numpy (tests/newton_restated.py) -- what the GPU tests compare the
device against (tests/test_gpu_newton.py) --, and the parts of its public interface that need no GPU (igtmpc.h igt_set_polish_step).

The LQ direction: the Riccati recursion's dN against the dense solution of the same model, which shares nothing with the
recursion (S = d z / d u by propagating A_k, B_k; H = R (x) I + sum S'QS; H d = -g_LQ), relative 1e-8 of the scenario's largest
entry and entry by entry at 1e-8 max(1, |dN|), on the 256 make_batch scenarios of test_adjoint_host._inputs at N = 20 and 40 (measured 4e-14 and 4e-13); the model's
linear term g_LQ against adjoint_restated.cost_gradient at 1e-10 max(1, |g|) (measured 1.6e-15 and 4.5e-14, |g| up to 78 and 312).

The restated polish on the seeds of test_adjoint_host._seeds (64 make_batch scenarios seeded with the oracle's winners), mean
cost drop after 1 / 2 / 4 iterations, measured when this was written (the adjoint mode of tests/adjoint_restated.py in brackets):
    lattice   0.575447 / 0.640000 / 0.658865   (0.14273 / 0.20407 / 0.26472)
    tracking  0.0028727 / 0.0039534 / 0.0051044   (0.002112 / 0.003195 / 0.004340)
pinned to half a unit of the last digit given.  Independent of the pins: on the lattice seeds one Newton iteration drops at
least 3 x what one adjoint iteration does (measured 4.0 x) and more than four adjoint iterations do; on the tracking seeds the
Newton drop is at least the adjoint mode's after 1, 2 and 4 iterations (measured 1.36 x / 1.24 x / 1.18 x)."""
import functools
import inspect
import os

import numpy as np
import pytest

import adjoint_restated as A
import newton_restated as NR
import polish_restated as R
import test_adjoint_host as TA
from igtmpc import _lib as L


@pytest.mark.parametrize('N', [20, 40])
def test_riccati_direction_is_the_dense_solution_of_the_same_model(N):
    P, b, flags, U = TA._inputs(N)
    M = NR.lq_model(b['x0'], b['kparams'], flags, U, P)
    d = NR.riccati_direction(M)
    dense, g_lq = NR.dense_direction(M)
    assert d.shape == dense.shape == U.shape and np.isfinite(dense).all()
    assert (np.abs(d).max(axis=(1, 2)) > 0).all()                       # no scenario fell back to the zero direction
    top = np.abs(dense).max(axis=(1, 2))
    err = np.abs(d - dense).max(axis=(1, 2)) / top
    _, g = A.cost_gradient(b['x0'], b['kparams'], flags, U, P)
    gerr = (np.abs(g_lq - g) / np.maximum(1.0, np.abs(g))).max()
    print(f'N={N}: worst relative error of dN {err.max():.2e} (max |dN| {top.max():.2f}); linear term against cost_gradient {gerr:.2e}')
    assert err.max() <= 1e-8
    assert (np.abs(d - dense) / np.maximum(1.0, np.abs(dense))).max() <= 1e-8      # entry by entry, the project's max(1, |.|)
    assert gerr <= 1e-10


def test_degenerate_models_give_the_zero_direction_and_no_steering_rate_a_zero_row():
    P, b, flags, U = TA._inputs(20)
    M = NR.lq_model(b['x0'][:8], b['kparams'][:8], flags[:8], U[:8], P)
    M['R'] = np.diag([-1e3, 1e3])                                       # Quu indefinite at the last step already: det < 0
    assert (NR.riccati_direction(M) == 0.0).all()
    M = NR.lq_model(b['x0'][:8], b['kparams'][:8], flags[:8], U[:8], P)
    M['q'][3, 5, 0] = np.nan                                            # reaches p, then kappa: entries from step 4 back to 0
    d = NR.riccati_direction(M)
    assert np.isfinite(d).all() and (d[3] == 0.0).all() and (np.abs(d[[0, 1, 2, 4, 5, 6, 7]]).max(axis=(1, 2)) > 0).all()
    d = NR.riccati_direction(NR.lq_model(b['x0'][:8], b['kparams'][:8], flags[:8], U[:8], P), steer=False)
    assert (d[:, 1] == 0.0).all() and (np.abs(d[:, 0]).max(axis=-1) > 0).all()


@functools.lru_cache(maxsize=None)
def _polished(cand):
    b, idx, u, J, P, cinf = TA._seeds(cand)
    hist, ties = NR.polish_newton(b, idx, u, J, 4, P, cinf)
    adj, _ = A.polish_adjoint(b, idx, u, J, 4, P, cinf)
    return (b, idx, u, J, P, cinf), hist, ties, adj


# the restatement's drops after 1 / 2 / 4 iterations and half a unit of the last digit they are given in (module docstring)
@pytest.mark.parametrize('cand, solved, pinned, pin_tol', [('lattice', 49, (0.575447, 0.640000, 0.658865), 5e-7),
                                                          ('track', 58, (0.0028727, 0.0039534, 0.0051044), 5e-8)])
def test_restated_newton_polish_is_feasible_exact_monotone_and_drops_as_pinned(cand, solved, pinned, pin_tol):
    (b, idx, u, J, P, cinf), hist, ties, _ = _polished(cand)
    assert len(idx) == solved
    for it in range(1, 5):
        uk, Jk = hist[it]
        Je, fe, _ = R.evaluate(b, idx, uk[:, None], P, cinf)
        assert fe.all(), f'{cand}: infeasible plan after {it} iterations'
        assert np.array_equal(Je[:, 0], Jk)
        assert (Jk <= hist[it - 1][1]).all() and (Jk <= J).all()
    drops = [(J - hist[k][1]).mean() for k in (1, 2, 4)]
    exact_ties = sum(int((t == 0.0).sum()) for t in ties)
    print(f'{cand}: mean drop after 1 / 2 / 4 iterations, newton', ' / '.join(f'{d:.6f}' for d in drops),
          f'; exact ties of the two cheapest trials: {exact_ties}')
    for d, pin in zip(drops, pinned):
        assert abs(d - pin) <= pin_tol


def test_newton_against_the_adjoint_mode_on_the_lattice_seeds():
    (_, _, _, J, _, _), hist, _, adj = _polished('lattice')
    n1, a1, a4 = (J - hist[1][1]).mean(), (J - adj[1][1]).mean(), (J - adj[4][1]).mean()
    print(f'lattice: newton after one iteration {n1:.5f} = {n1 / a1:.2f} x the adjoint mode\'s {a1:.5f}; adjoint after four {a4:.5f}')
    assert n1 >= 3.0 * a1
    assert n1 > a4
    assert (hist[1][1] <= adj[1][1]).all()            # the gradient trials 0 .. 31 are among the Newton mode's trials


def test_newton_against_the_adjoint_mode_on_the_tracking_seeds():
    (_, _, _, J, _, _), hist, _, adj = _polished('track')
    for k in (1, 2, 4):
        n, a = (J - hist[k][1]).mean(), (J - adj[k][1]).mean()
        print(f'tracking k={k}: newton {n:.6f} = {n / a:.2f} x adjoint {a:.6f}')
        assert n >= a


def test_header_declares_the_setter_and_both_constants():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'igtmpc.h')).read()
    assert 'enum { IGT_POLISH_STEP_GRADIENT = 0, IGT_POLISH_STEP_NEWTON = 1 };' in hdr
    assert 'int igt_set_polish_step(igt_handle* h, int mode);' in hdr
    assert (L.IGT_POLISH_STEP_GRADIENT, L.IGT_POLISH_STEP_NEWTON) == (0, 1)
    assert 'igt_set_polish_step' in L.SYMBOLS and 'igt_set_polish_step' in L.OPTIONAL_SYMBOLS
    for lib in (L.load(), L.load(dev=True)):
        assert hasattr(lib, 'igt_set_polish_step')


def test_refusals_that_need_no_gpu():
    lib = L.load()
    for mode in (0, 1):
        assert lib.igt_set_polish_step(None, mode) == -1
        assert b'null handle' in lib.igt_last_error() and b'IGT_POLISH_STEP_' in lib.igt_last_error()
    for mode in (-1, 2, 7):                     # the mode is judged first, so this needs no handle
        assert lib.igt_set_polish_step(None, mode) == -1
        assert b'mode must be IGT_POLISH_STEP_' in lib.igt_last_error()


def test_python_takes_the_option_and_refuses_other_words(monkeypatch):
    import igtmpc
    from igtmpc.evaluate import run_closed_loop
    from igtmpc.planner import MPC_Planner
    assert inspect.signature(igtmpc.BatchSolver.__init__).parameters['polish_step'].default == 'gradient'
    assert inspect.signature(MPC_Planner.__init__).parameters['polish_step'].default == 'gradient'
    assert inspect.signature(run_closed_loop).parameters['polish_step'].default == 'gradient'
    lib = L.load()

    def no_create(*a):
        raise AssertionError('igt_create reached')
    monkeypatch.setattr(igtmpc.solver.L, 'load', lambda: type('NoCreate', (), {
        'igt_params_default': lib.igt_params_default, 'igt_create': no_create, 'igt_destroy': lambda *a: 0})())
    for word in ('gauss', 'Newton', None, 1):
        with pytest.raises(ValueError, match='polish_step'):
            igtmpc.BatchSolver(dtype='f64', polish_iters=1, polish_step=word)
