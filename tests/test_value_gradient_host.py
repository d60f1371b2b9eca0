"""CPU: the terminal value's partials and the gradient of the value-network cost as restated in numpy
(tests/value_gradient_restated.py) -- what tests/test_gpu_value_gradient.py compares the device against --, and the parts of the
public interface that need no GPU.

Networks: V_GT_sc1 (two hidden layers) and V_GT_sc3 (three), each with a non-identity whitening Wn = I + 0.05 normal, a random
mu_f around the feature means, sigma_t = 1.7 and mu_t = -0.4 (the shipped Wn is the identity and would hide a transposed or
mis-indexed column 3 / 4).  Terminal states: those of the gradient inputs' own roll-outs (200 make_batch scenarios, N = 20); on them
neither network saturates -- measured when this was written, max |dV_out/ds_N| = 2.49 / 0.39 and max |dV_out/dv_N| = 0.31 / 0.092
(sc1 / sc3) -- so no other states had to be picked.

Yardsticks: torch.autograd in float64 through a tensor restatement written independently of the numpy one (<= 1e-9), central
differences of the restated value with step 1e-6 (<= 1e-6) and of the restated cost with step 1e-5 (<= 1e-6 max(1, |g|)); sequences
with a RK stage argument within 1e-5 of a curvature break-point are set aside, at most 1 % of a batch."""
import functools
import os

import numpy as np
import pytest

import np_oracle as O
import value_gradient_restated as VG
from igtmpc import _lib as L

CONFIGS = [(1, 20, 4), (64, 20, 4), (192, 20, 2), (200, 64, 4), (1000, 40, 2)]      # (B, N, n_rk4)


@functools.lru_cache(maxsize=None)
def _net(sc):
    from igtmpc import shipped_value_net
    rng = np.random.default_rng(100 + sc)
    return dict(shipped_value_net(sc), Wn=np.eye(6) + 0.05 * rng.normal(size=(6, 6)),
                mu_f=np.array([20.0, 2.5, 0.0, 0.0, 0.0, 0.0]) + 0.1 * rng.normal(size=6), sigma_t=1.7, mu_t=-0.4)


@functools.lru_cache(maxsize=None)
def _grad_inputs(B, N, n_rk4):
    """the recipe of tests/test_gpu_gradient.py: one random lattice candidate per make_batch scenario, every third scenario with
    the abs-heading flag, every fifth sequence steered off the lane; plus the batch's own tv_sv and enc"""
    from igtmpc.scenarios import make_batch
    b = make_batch(max(B, 64), N=N, dtype=np.float64, seed=2026)
    P = O.Params(N=N, n_rk4=n_rk4)
    rng = np.random.default_rng(0)
    n = len(b['x0'])
    pick = rng.integers(0, 256, size=n)
    U = np.concatenate([O.candidates_lattice(b['u_prev'][i:i + 256], P)[np.arange(len(pick[i:i + 256])), pick[i:i + 256]]
                        for i in range(0, n, 256)])
    U[::5, 1, :5] += 0.2 * np.sign(rng.standard_normal((len(U[::5]), 1)))
    flags = np.asarray(b['flags']).copy()
    flags[::3] |= np.uint32(O.FLAG_ABS_HEADING)
    c = lambda a: np.ascontiguousarray(a[:B], dtype=None)
    return c(b['x0']), c(b['kparams']), c(flags), c(b['tv_sv']), c(b['enc']), c(U), P


@functools.lru_cache(maxsize=None)
def _terminal_states(B=200, N=20):
    x0, kp, flags, tv, enc, U, P = _grad_inputs(B, N, 4)
    X = O.rollout_frenet(O.apply_flags(x0, flags), U, kp, P)
    return np.ascontiguousarray(np.stack([X[:, O.IS, N], X[:, O.IV, N]], axis=-1)), tv, enc


def _torch_value(net, sv, tv_sv, enc):
    """V_out[n] as a float64 tensor of sv (requires_grad) -- written from mpc.py:326-338, 367-369 and model.py, not from numpy"""
    import torch
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    tv, en = t(tv_sv), t(enc)
    x = torch.stack([tv[:, 0], tv[:, 1], en[:, 1], sv[:, 0] - tv[:, 0], sv[:, 1] - tv[:, 1], en[:, 0] - en[:, 1]], dim=1)
    h = torch.matmul(x - t(net['mu_f']), t(net['Wn']).T)
    n_l = len(net['layers'])
    for i, (W, b) in enumerate(net['layers']):
        h = torch.matmul(h, t(W).T) + t(b)
        if i + 1 < n_l:
            h = torch.tanh(h)
    return h[:, 0] * net['sigma_t'] + net['mu_t']


@pytest.mark.parametrize('sc', [1, 3])
def test_restated_partials_against_autograd_and_central_differences(sc):
    import torch
    net = _net(sc)
    assert len(net['layers']) == (3 if sc == 1 else 4)
    sv, tv, enc = _terminal_states()
    V, dV = VG.terminal_value_and_partials(net, sv, tv, enc)
    assert np.allclose(V, O.terminal_value(net, sv[:, 0:1], sv[:, 1:2], tv, enc)[:, 0], rtol=0, atol=1e-13)
    svt = torch.tensor(sv, dtype=torch.float64, requires_grad=True)
    Vt = _torch_value(net, svt, tv, enc)
    Vt.sum().backward()
    e_auto = np.abs(dV - svt.grad.numpy()).max()
    e_val = np.abs(V - Vt.detach().numpy()).max()
    h = 1e-6
    fd = np.empty_like(dV)
    for c in range(2):
        d = np.zeros(2)
        d[c] = h
        fd[:, c] = (VG.terminal_value_and_partials(net, sv + d, tv, enc)[0] -
                    VG.terminal_value_and_partials(net, sv - d, tv, enc)[0]) / (2 * h)
    e_fd = np.abs(dV - fd).max()
    print(f'sc{sc}: max |dV/ds_N| {np.abs(dV[:, 0]).max():.3f} |dV/dv_N| {np.abs(dV[:, 1]).max():.3f}; against autograd {e_auto:.2e} '
          f'(values {e_val:.2e}), against central differences {e_fd:.2e}')
    assert e_val <= 1e-9 and e_auto <= 1e-9
    assert e_fd <= 1e-6
    # not trivially small on the test inputs: a zero derivative would pass every comparison of two zero derivatives
    assert np.abs(dV[:, 0]).max() > 1e-3 and np.abs(dV[:, 1]).max() > 1e-3


def test_break_point_set_aside_of_the_gradient_inputs_stays_under_one_percent():
    for B, N, n_rk4 in CONFIGS:
        x0, kp, flags, tv, enc, U, P = _grad_inputs(B, N, n_rk4)
        aside = O.breakpoint_distance(O.apply_flags(x0, flags), U, kp, P) < 1e-5
        print(f'B={B} N={N} n_rk4={n_rk4}: set aside at 1e-5 {aside.mean():.4f}')
        assert aside.mean() <= 0.01


@pytest.mark.parametrize('sc', [1, 3])
@pytest.mark.parametrize('B, N, n_rk4', [(64, 20, 4), (200, 64, 2)])
def test_restated_cost_gradient_against_central_differences(sc, B, N, n_rk4):
    net = _net(sc)
    x0, kp, flags, tv, enc, U, P = (a[:16] if isinstance(a, np.ndarray) else a for a in _grad_inputs(B, N, n_rk4))
    J, g = VG.cost_gradient_vn(x0, kp, flags, tv, enc, U, P, net)
    assert np.isfinite(J).all() and np.isfinite(g).all()
    assert np.abs(J - VG.cost_vn(x0, kp, flags, tv, enc, U, P, net)).max() <= 1e-12      # the terminal value by np_oracle itself
    h = 1e-5
    ref = np.empty_like(U)
    for r in range(2):
        for k in range(N):
            Up, Um = U.copy(), U.copy()
            Up[:, r, k] += h
            Um[:, r, k] -= h
            ref[:, r, k] = (VG.cost_vn(x0, kp, flags, tv, enc, Up, P, net) - VG.cost_vn(x0, kp, flags, tv, enc, Um, P, net)) / (2 * h)
    aside = O.breakpoint_distance(O.apply_flags(x0, flags), U, kp, P) < 1e-5
    err = (np.abs(g - ref) / np.maximum(1.0, np.abs(ref))).max(axis=(1, 2))
    # the network's part of the gradient is there: without the terminal seed the a rows would miss dt dV/dv_N
    _, dV = VG.terminal_value_and_partials(net, *_sv_of(x0, kp, flags, U, P), tv, enc)
    print(f'sc{sc} B=16 of {B} N={N} n_rk4={n_rk4}: max |g| {np.abs(ref).max():.1f}, worst error {err[~aside].max():.2e}, set aside '
          f'{aside.sum()} of 16; max |dt dV/dv_N| {P.dt * np.abs(dV[:, 1]).max():.3f}')
    assert (~aside).sum() >= 15
    assert err[~aside].max() <= 1e-6


def _sv_of(x0, kp, flags, U, P):
    X = O.rollout_frenet(O.apply_flags(x0, flags), U, kp, P)
    return (np.stack([X[:, O.IS, -1], X[:, O.IV, -1]], axis=-1),)


def test_sigma_zero_leaves_the_stage_terms_and_nonfinite_cost_gives_a_nan_row():
    import adjoint_restated as A
    x0, kp, flags, tv, enc, U, P = _grad_inputs(64, 20, 4)
    net0 = dict(_net(1), sigma_t=0.0, mu_t=0.0)
    J0, g0 = VG.cost_gradient_vn(x0, kp, flags, tv, enc, U, P, net0)
    Jp, gp = A.cost_gradient(x0, kp, flags, U, P)
    # the progress cost's gradient plus the derivative of its progress term: -(s_N - s_0) seeds the s costate with -1
    X = O.rollout_frenet(O.apply_flags(x0, flags), U, kp, P)
    assert np.abs(J0 - (Jp + (X[:, O.IS, -1] - X[:, O.IS, 0]))).max() <= 1e-12
    assert not np.allclose(g0, gp)
    x0, U = x0.copy(), U.copy()
    x0[3, O.IS] = np.nan
    U[5, 0, 2] = np.inf
    J, g = VG.cost_gradient_vn(x0, kp, flags, tv, enc, U, P, _net(3))
    assert not np.isfinite(J[[3, 5]]).any() and np.isnan(g[[3, 5]]).all()
    ok = np.ones(64, bool)
    ok[[3, 5]] = False
    assert np.isfinite(g[ok]).all() and np.isfinite(J[ok]).all()


def test_header_declares_the_entries_and_both_libraries_export_them():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'igtmpc.h')).read()
    assert 'int igt_terminal_value_f64(igt_handle* h, int32_t n, const double* sv, const double* tv_sv, const double* enc,' in hdr
    assert 'int igt_cost_gradient_vn_f64(igt_handle* h, int32_t B, const double* x0, const double* kparams, const uint32_t* flags,' in hdr
    assert '#define IGT_VERSION 201' in hdr
    assert 'igt_terminal_value_f32' not in hdr and 'igt_cost_gradient_vn_f32' not in hdr
    for name in ('igt_terminal_value_f64', 'igt_cost_gradient_vn_f64'):
        assert name in L.SYMBOLS and name in L.OPTIONAL_SYMBOLS
        for lib in (L.load(), L.load(dev=True)):
            assert hasattr(lib, name)
            assert not hasattr(lib, name.replace('f64', 'f32'))


def test_refusals_that_need_no_gpu():
    lib = L.load()
    assert lib.igt_terminal_value_f64(None, 1, None, None, None, None, None, L.IGT_MEM_HOST, None) == -1
    assert b'null handle' in lib.igt_last_error()
    assert lib.igt_cost_gradient_vn_f64(None, 1, None, None, None, None, None, None, None, None, L.IGT_MEM_HOST, None) == -1
    assert b'null handle' in lib.igt_last_error()


class _OlderLibrary:
    """libigtmpc.so as it was before the two entries: every other symbol answers, igt_create hands out a handle without a GPU"""
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        if name in ('igt_terminal_value_f64', 'igt_cost_gradient_vn_f64'):
            raise AttributeError(name)
        if name == 'igt_params_default':
            return self._lib.igt_params_default
        if not name.startswith('igt_'):
            raise AttributeError(name)

        def stub(*a):
            self.calls.append(name)
            return 0
        return stub


def test_a_library_without_the_entries_says_so_and_serves_everything_else(monkeypatch):
    import igtmpc
    old = _OlderLibrary(L.load())
    monkeypatch.setattr(igtmpc.solver.L, 'load', lambda: old)
    x0, kp, flags, tv, enc, U, _ = _grad_inputs(64, 20, 4)
    sv = np.zeros((64, 2))
    with igtmpc.BatchSolver(dtype='f64', cost_mode='value_net', N=20) as s:
        with pytest.raises(L.IgtError, match='does not export igt_terminal_value_f64'):
            s.terminal_value(sv, tv, enc)
        with pytest.raises(L.IgtError, match='does not export igt_cost_gradient_vn_f64'):
            s.cost_gradient(x0, kp, flags, U, tv_sv=tv, enc=enc)
        s.cost_gradient(x0, kp, flags, U)                       # the entry from before: reached as ever
        assert old.calls[-1] == 'igt_cost_gradient_f64'
    assert old.calls[-1] == 'igt_destroy'
    with igtmpc.BatchSolver(dtype='f32', cost_mode='value_net', N=20) as f:
        with pytest.raises(ValueError, match='f64'):
            f.cost_gradient(x0, kp, flags, U, tv_sv=tv, enc=enc)
        with pytest.raises(ValueError, match='f64'):
            f.terminal_value(sv, tv, enc)
