"""CPU: the analytic cost gradient and the adjoint polish as restated in numpy (tests/adjoint_restated.py) -- what the GPU tests
compare the device against (tests/test_gpu_gradient.py) --, and the parts of the public interface that need no GPU.

The yardstick of the gradient is the central difference of stage_cost o rollout_frenet with h = 1e-5 (agrees with h = 1e-4 and
1e-6 to <= 1e-6 on these inputs), the tolerance the project's REL_TOL, 1e-5 max(1, |g|); sequences with a RK stage argument within
1e-3 of a curvature break-point are set aside (the difference quotient straddles the jump of K there; at most 5 % of a batch).

Polish, measured when this was written (64 make_batch scenarios seeded with the oracle's winners, mean cost drop after 1 / 2 / 4
iterations; the forward-difference restatement of tests/polish_restated.py in brackets):
    lattice   0.14273 / 0.20407 / 0.26472   (0.14274 / 0.20384 / 0.26548)
    tracking  0.00211 / 0.00319 / 0.00434   (0.00211 / 0.00319 / 0.00431)
The two gradients differ by the forward difference's truncation only, but the plans drift apart over the iterations (which of two
nearly tied trials wins changes with the gradient's fourth digit): the means differ by 1e-5 / 2.3e-4 / 7.6e-4 (lattice) and
< 1e-5 / < 1e-5 / 3e-5 (tracking).  The assertion allows 1e-3 and 1e-4 -- the largest difference of the run rounded up to the next
power of ten --, and holds the forward-difference drops to the pinned figures within half a unit of their last digit."""
import inspect

import numpy as np
import pytest

import adjoint_restated as A
import np_oracle as O
import polish_restated as R
from igtmpc import _lib as L

REL_TOL = 1e-5
FD_H = 1e-5


def _inputs(N, n_rk4=4, abs_heading=False):
    from igtmpc.scenarios import make_batch
    P = O.Params(N=N, n_rk4=n_rk4)
    b = make_batch(256, N, dtype=np.float64)
    rng = np.random.default_rng(0)
    U = O.candidates_lattice(b['u_prev'], P)                       # [B, C, 2, N]
    pick = rng.integers(0, U.shape[1], size=U.shape[0])
    U = U[np.arange(U.shape[0]), pick]
    flags = np.asarray(b['flags']).copy()
    if abs_heading:
        flags = flags | np.uint32(O.FLAG_ABS_HEADING)
    return P, b, flags, U


def _central(x0, kp, flags, U, P):
    x0 = O.apply_flags(x0, flags)
    J = lambda V: O.stage_cost(O.rollout_frenet(x0, V, kp, P), V, P)
    g = np.empty_like(U)
    for r in range(2):
        for k in range(U.shape[-1]):
            Up, Um = U.copy(), U.copy()
            Up[:, r, k] += FD_H
            Um[:, r, k] -= FD_H
            g[:, r, k] = (J(Up) - J(Um)) / (2 * FD_H)
    return g


@pytest.mark.parametrize('N, n_rk4, absh, cap', [(20, 4, False, 0.05), (40, 4, False, 0.05), (20, 7, False, 0.05), (20, 4, True, 0.05)])
def test_restated_gradient_against_central_differences(N, n_rk4, absh, cap):
    P, b, flags, U = _inputs(N, n_rk4, absh)
    J, g = A.cost_gradient(b['x0'], b['kparams'], flags, U, P)
    x0 = O.apply_flags(b['x0'], flags)
    assert np.array_equal(J, O.stage_cost(O.rollout_frenet(x0, U, b['kparams'], P), U, P))
    ref = _central(b['x0'], b['kparams'], flags, U, P)
    aside = O.breakpoint_distance(x0, U, b['kparams'], P) < 1e-3
    err = np.abs(g - ref) / np.maximum(1.0, np.abs(ref))
    worst = err[~aside].max()
    print(f'N={N} n_rk4={n_rk4} abs={absh}: set aside {aside.mean():.3%}, max |g| {np.abs(ref).max():.1f}, worst error {worst:.2e}')
    assert aside.mean() <= cap
    assert worst <= REL_TOL


def test_nonfinite_cost_gives_a_nan_row():
    P, b, flags, U = _inputs(20)
    x0 = b['x0'].copy()
    x0[3, O.IEY] = np.inf
    U[5, 0, 2] = np.nan
    J, g = A.cost_gradient(x0, b['kparams'], flags, U, P)
    assert not np.isfinite(J[3]) and not np.isfinite(J[5])
    assert np.isnan(g[3]).all() and np.isnan(g[5]).all()
    ok = np.ones(len(J), bool)
    ok[[3, 5]] = False
    assert np.isfinite(g[ok]).all()


def _seeds(cand):
    from igtmpc.cinf import cinf_halfplanes
    from igtmpc.scenarios import make_batch
    P, cinf = O.Params(), cinf_halfplanes()
    b = make_batch(64, dtype=np.float64)
    args = (b['x0'], b['u_prev'], b['kparams'], b['flags'], b['obs_xy'], *cinf, P)
    sol = O.solve_batch(*args) if cand == 'lattice' else O.solve_batch_refined(*args, refine_iters=0, cand='track')[0]
    idx = np.flatnonzero(sol['status'] == 0)
    return b, idx, sol['u'][idx], sol['cost'][idx], P, cinf


# the forward-difference restatement's drops after 1 / 2 / 4 iterations (tests/test_polish_host.py prints them), and the margin
# (half a unit of the last digit they are given in), and the margin between the two gradients' drops (module docstring)
@pytest.mark.parametrize('cand, solved, pinned, pin_tol, margin', [('lattice', 49, (0.143, 0.204, 0.265), 5e-4, 1e-3),
                                                                   ('track', 58, (0.0021, 0.0032, 0.0043), 5e-5, 1e-4)])
def test_polish_adjoint_is_feasible_monotone_and_drops_like_forward_differences(cand, solved, pinned, pin_tol, margin):
    b, idx, u, J, P, cinf = _seeds(cand)
    assert len(idx) == solved
    hist, _ = A.polish_adjoint(b, idx, u, J, 4, P, cinf)
    for it in range(1, 5):
        uk, Jk = hist[it]
        Je, fe, _ = R.evaluate(b, idx, uk[:, None], P, cinf)
        assert fe.all(), f'{cand}: infeasible plan after {it} iterations'
        assert np.array_equal(Je[:, 0], Jk)
        assert (Jk <= hist[it - 1][1]).all() and (Jk <= J).all()
    assert (J - hist[1][1] > 0).all()
    fd, _ = R.polish(b, idx, u, J, 4, P, cinf)
    drops = [(J - hist[k][1]).mean() for k in (1, 2, 4)]
    drops_fd = [(J - fd[k][1]).mean() for k in (1, 2, 4)]
    print(f'{cand}: mean drop after 1 / 2 / 4 iterations, adjoint', ' / '.join(f'{d:.5f}' for d in drops),
          '-- forward differences', ' / '.join(f'{d:.5f}' for d in drops_fd))
    for d, dfd, pin in zip(drops, drops_fd, pinned):
        assert abs(dfd - pin) <= pin_tol
        assert abs(d - dfd) <= margin


def test_header_declares_the_entry_and_the_setter():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'igtmpc.h')).read()
    assert 'enum { IGT_GRAD_FORWARD_DIFF = 0, IGT_GRAD_ADJOINT = 1 };' in hdr
    assert 'int igt_set_polish_gradient(igt_handle* h, int mode);' in hdr
    assert 'int igt_cost_gradient_f64(igt_handle* h, int32_t B, const double* x0, const double* kparams, const uint32_t* flags,' in hdr
    assert '#define IGT_VERSION 201' in hdr
    assert (L.IGT_GRAD_FORWARD_DIFF, L.IGT_GRAD_ADJOINT) == (0, 1)
    for lib in (L.load(), L.load(dev=True)):
        assert hasattr(lib, 'igt_cost_gradient_f64') and hasattr(lib, 'igt_set_polish_gradient')


def test_refusals_that_need_no_gpu():
    lib = L.load()
    assert lib.igt_set_polish_gradient(None, 1) == -1 and b'null handle' in lib.igt_last_error()
    assert lib.igt_cost_gradient_f64(None, 1, None, None, None, None, None, None, L.IGT_MEM_HOST, None) == -1
    assert b'null handle' in lib.igt_last_error()


def test_python_takes_the_option_and_refuses_other_words(monkeypatch):
    import igtmpc
    from igtmpc.evaluate import run_closed_loop
    from igtmpc.planner import MPC_Planner
    assert inspect.signature(igtmpc.BatchSolver.__init__).parameters['polish_grad'].default == 'fd'
    assert inspect.signature(MPC_Planner.__init__).parameters['polish_grad'].default == 'fd'
    assert inspect.signature(run_closed_loop).parameters['polish_grad'].default == 'fd'
    assert 'cost_gradient' in dir(igtmpc.BatchSolver)
    lib = L.load()

    def no_create(*a):
        raise AssertionError('igt_create reached')
    monkeypatch.setattr(igtmpc.solver.L, 'load', lambda: type('NoCreate', (), {
        'igt_params_default': lib.igt_params_default, 'igt_create': no_create, 'igt_destroy': lambda *a: 0})())
    with pytest.raises(ValueError, match='polish_grad'):
        igtmpc.BatchSolver(dtype='f64', polish_iters=1, polish_grad='central')
