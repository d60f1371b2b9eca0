"""-m gpu : the Newton (LQ) mode of the polish on the device (igtmpc.h igt_set_polish_step; csrc/igt_kernels_f64.hip
polish_f64_kernel NEWTON, csrc/igt_adjoint64.h Riccati), float64.  The structure of tests/test_gpu_gradient.py's polish half.

Shapes (B, N, n_obs): (64, 20, 1), (256, 40, 1), (128, 64, 3), (64, 7, 1) -- N <= 32, N > 32, the LDS above 64 KB with all 64
lanes forming Jacobians, a short odd horizon.
  * IGT_POLISH_STEP_GRADIENT set explicitly, or NEWTON set and taken back, is a handle that never called the setter, bit for bit
    on every output, under both gradient modes; NEWTON gives other plans;
  * the polished plan is its own table roll-out bit for bit (x_out, cost_out; no verdict raised), k = 1 and 4; the cost is
    monotone, argmin / status / unsolved scenarios are those of polish_iters = 0, more than half of the solved move at k = 1;
  * the device follows newton_restated.polish_newton scenario by scenario within 1e-6 in cost after 1 and 2 iterations (lattice,
    ramp-hold, tracking; (64, 20) and (256, 40)); a scenario is set aside only if the restatement's two cheapest feasible trials
    lie within 1e-7 of each other AND it differs by more than 1e-6, at most 2 % (the share is printed);
  * at (256, 20, lattice) the device's mean drop after one Newton iteration is above the adjoint mode's after four;
  * it replays from a graph, runs with four handles in flight, and through run_closed_loop(polish_step='newton') eager and
    device-resident from a graph with equal trajectories, which are not the gradient mode's;
  * n_rk4 = 3, 2, 7 (the builds for a general n_rk4 and for the high-order sub-step) at (64, 20): the restatement within 1e-6
    and the table roll-out bit for bit."""
import functools

import numpy as np
import pytest

import newton_restated as NR
import polish_restated as R
from helpers import oracle_params, rel_err
from igtmpc import _lib as L

pytestmark = pytest.mark.gpu

KEYS = ('x', 'u', 'cost', 'argmin', 'status')
SHAPES = [(64, 20, 1), (256, 40, 1), (128, 64, 3), (64, 7, 1)]


def _cinf(dt=0.1):
    from igtmpc.cinf import cinf_halfplanes
    return cinf_halfplanes(dt=dt)


@functools.lru_cache(maxsize=None)
def _batch(B, N, n_obs=1, seed=2026):
    from igtmpc.scenarios import make_batch
    b = make_batch(B, N=N, dtype=np.float64, seed=seed)
    b['obs_xy'] = np.ascontiguousarray(np.concatenate(
        [b['obs_xy'] + 2.5 * m * np.array([1.0, -1.0])[None, None, :, None] for m in range(n_obs)], axis=1))
    return b


def _args(b):
    return b['x0'], b['u_prev'], b['kparams'], b['flags'], b['obs_xy']


def _dev(torch, b):
    return [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).contiguous().cuda() for a in _args(b)]


def _solver(N, n_obs=1, cand='lattice', **kw):
    import igtmpc
    s = igtmpc.BatchSolver(dtype='f64', cand_mode=cand, N=N, n_obs=n_obs, **kw)
    s.set_cinf(*_cinf())
    return s


@functools.lru_cache(maxsize=None)
def _solved(B, N, n_obs, cand='lattice', iters=(0, 1, 2, 4), **mode):
    """{polish_iters: outputs} of the Newton mode (or of `mode`), and the oracle's parameters; computed once, left unchanged"""
    b = _batch(B, N, n_obs)
    out = {}
    for k in iters:
        with _solver(N, n_obs, cand, polish_iters=k, **(mode or dict(polish_step='newton'))) as s:
            out[k] = s.solve(*_args(b))
            P = oracle_params(s)
    return out, P


@pytest.mark.parametrize('grad', ['fd', 'adjoint'])
@pytest.mark.parametrize('B,N,n_obs', SHAPES)
def test_gradient_step_set_explicitly_or_set_back_changes_nothing(B, N, n_obs, grad):
    b = _batch(B, N, n_obs)
    with _solver(N, n_obs, polish_iters=2, polish_grad=grad) as s:        # never called the setter
        plain = s.solve(*_args(b))
    with _solver(N, n_obs, polish_iters=2, polish_grad=grad) as s:
        s._check(s.lib.igt_set_polish_step(s._h, L.IGT_POLISH_STEP_GRADIENT))
        explicit = s.solve(*_args(b))
        s._check(s.lib.igt_set_polish_step(s._h, L.IGT_POLISH_STEP_NEWTON))
        other = s.solve(*_args(b))
        s._check(s.lib.igt_set_polish_step(s._h, L.IGT_POLISH_STEP_GRADIENT))
        back = s.solve(*_args(b))
        assert s.lib.igt_set_polish_step(s._h, 2) == -1 and b'IGT_POLISH_STEP_' in s.lib.igt_last_error()
        assert s.lib.igt_set_polish_step(s._h, -1) == -1
        still = s.solve(*_args(b))                                        # a refused call changes nothing
    newton, _ = _solved(B, N, n_obs)
    for k in KEYS:
        assert np.array_equal(plain[k], explicit[k], equal_nan=True), k
        assert np.array_equal(plain[k], back[k], equal_nan=True), k
        assert np.array_equal(plain[k], still[k], equal_nan=True), k
        assert np.array_equal(other[k], newton[2][k], equal_nan=True), k    # the Newton step takes the analytic gradient either way
    assert not np.array_equal(plain['u'], other['u'], equal_nan=True)


@pytest.mark.parametrize('B,N,n_obs', SHAPES)
def test_newton_monotone_and_bookkeeping_untouched(B, N, n_obs):
    out, _ = _solved(B, N, n_obs)
    ok = out[0]['status'] == 0
    assert 0.0 < ok.mean() < 1.0             # (128, 64, 3): three scenarios are solved at this horizon with three obstacles
    prev = 0
    for k in (1, 2, 4):
        assert np.array_equal(out[k]['argmin'], out[0]['argmin']) and np.array_equal(out[k]['status'], out[0]['status'])
        assert (out[k]['cost'][ok] <= out[prev]['cost'][ok]).all() and (out[k]['cost'][ok] <= out[0]['cost'][ok]).all()
        assert np.isnan(out[k]['x'][~ok]).all() and np.isnan(out[k]['u'][~ok]).all()
        assert np.isposinf(out[k]['cost'][~ok]).all() and (out[k]['argmin'][~ok] == -1).all()
        same = out[k]['cost'] == out[prev]['cost']
        assert np.array_equal(out[k]['u'][ok & same], out[prev]['u'][ok & same])
        assert np.array_equal(out[k]['x'][ok & same], out[prev]['x'][ok & same])
        prev = k
    drop = out[0]['cost'][ok] - out[1]['cost'][ok]
    print(f'B={B} N={N}: {ok.sum()} solved, mean cost drop after 1 / 2 / 4 iterations',
          ' / '.join(f'{(out[0]["cost"][ok] - out[k]["cost"][ok]).mean():.4f}' for k in (1, 2, 4)), f'; moved by iteration 1: {(drop > 1e-9).mean():.3f}')
    assert (drop > 1e-9).mean() > 0.5


@pytest.mark.parametrize('B,N,n_obs', SHAPES)
def test_newton_polished_plan_is_its_own_table_rollout_bit_for_bit(B, N, n_obs):
    b = _batch(B, N, n_obs)
    out, _ = _solved(B, N, n_obs)
    with _solver(N, n_obs, 'table', C=64) as t:
        for k in (1, 4):
            got = out[k]
            idx = np.flatnonzero(got['status'] == 0)
            for c0 in range(0, len(idx), 64):
                ch = idx[c0:c0 + 64]
                U = np.zeros((64, 2, N))
                U[:len(ch)] = got['u'][ch]
                t.set_candidate_table(U)
                sub = [np.ascontiguousarray(a[ch]) for a in _args(b)]
                r = t.rollout_all(*sub, want_U=False)
                d = np.arange(len(ch))
                assert np.array_equal(r['X'][d, d], got['x'][ch]), (k, c0)
                assert np.array_equal(r['cost'][d, d], got['cost'][ch]), (k, c0)
                assert (r['viol'][d, d] == 0).all(), (k, c0)


@pytest.mark.parametrize('cand', ['lattice', 'ramp_hold', 'track'])
@pytest.mark.parametrize('B,N', [(64, 20), (256, 40)])
def test_device_follows_the_newton_restatement(B, N, cand):
    b = _batch(B, N, 1)
    out, P = _solved(B, N, 1, cand, (0, 1, 2))
    cinf = _cinf()
    idx = np.flatnonzero(out[0]['status'] == 0)
    assert len(idx) >= 8
    J0, f0, _ = R.evaluate(b, idx, out[0]['u'][idx][:, None], P, cinf)
    assert f0.all() and rel_err(J0[:, 0], out[0]['cost'][idx]).max() <= 1e-9
    hist, ties = NR.polish_newton(b, idx, out[0]['u'][idx], J0[:, 0], 2, P, cinf)
    tied = np.zeros(len(idx), dtype=bool)
    for k in (1, 2):
        tied |= ties[k - 1] < 1e-7
        diff = np.abs(out[k]['cost'][idx] - hist[k][1])
        aside = tied & (diff > 1e-6)
        print(f'{cand} B={B} N={N} k={k}: max |J_device - J_restated| {diff[~aside].max():.2e} (all: {diff.max():.2e}); '
              f'set aside {aside.mean():.4f} of {len(idx)} (near-ties: {tied.mean():.4f}); mean drop {(J0[:, 0] - hist[k][1]).mean():.4f}')
        assert aside.mean() <= 0.02
        assert diff[~aside].max() <= 1e-6


@pytest.mark.parametrize('n_rk4', [3, 2, 7])
def test_other_discretisations_follow_the_restatement_and_their_table_rollout(n_rk4):
    """the kernel's builds for a general n_rk4 and for the high-order sub-step (n_rk4 = 4 is every other test's)"""
    B, N = 64, 20
    b = _batch(B, N, 1)
    out, P = _solved(B, N, 1, 'lattice', (0, 1, 2), polish_step='newton', n_rk4=n_rk4)
    assert P.n_rk4 == n_rk4
    cinf = _cinf()
    idx = np.flatnonzero(out[0]['status'] == 0)
    assert len(idx) >= 8
    J0, f0, _ = R.evaluate(b, idx, out[0]['u'][idx][:, None], P, cinf)
    assert f0.all() and rel_err(J0[:, 0], out[0]['cost'][idx]).max() <= 1e-9
    hist, ties = NR.polish_newton(b, idx, out[0]['u'][idx], J0[:, 0], 2, P, cinf)
    tied = np.zeros(len(idx), dtype=bool)
    for k in (1, 2):
        tied |= ties[k - 1] < 1e-7
        diff = np.abs(out[k]['cost'][idx] - hist[k][1])
        aside = tied & (diff > 1e-6)
        print(f'n_rk4={n_rk4} k={k}: max |J_device - J_restated| {diff[~aside].max():.2e}; set aside {aside.mean():.4f} of {len(idx)}; '
              f'mean drop {(J0[:, 0] - hist[k][1]).mean():.4f}')
        assert aside.mean() <= 0.02
        assert diff[~aside].max() <= 1e-6
    with _solver(N, 1, 'table', C=64, n_rk4=n_rk4) as t:
        U = np.zeros((64, 2, N))
        U[:len(idx)] = out[2]['u'][idx]
        t.set_candidate_table(U)
        r = t.rollout_all(*[np.ascontiguousarray(a[idx]) for a in _args(b)], want_U=False)
        d = np.arange(len(idx))
        assert np.array_equal(r['X'][d, d], out[2]['x'][idx]) and np.array_equal(r['cost'][d, d], out[2]['cost'][idx])
        assert (r['viol'][d, d] == 0).all()


def test_one_newton_iteration_drops_more_than_four_adjoint_iterations_on_the_lattice():
    newton, _ = _solved(256, 20, 1, 'lattice', (0, 1))
    adjoint, _ = _solved(256, 20, 1, 'lattice', (4,), polish_grad='adjoint')
    ok = newton[0]['status'] == 0
    assert ok.sum() >= 64 and np.array_equal(adjoint[4]['status'], newton[0]['status'])
    n1 = (newton[0]['cost'][ok] - newton[1]['cost'][ok]).mean()
    a4 = (newton[0]['cost'][ok] - adjoint[4]['cost'][ok]).mean()
    print(f'(256, 20, lattice), {ok.sum()} solved: mean drop after one Newton iteration {n1:.4f}, after four adjoint iterations {a4:.4f}')
    assert n1 > a4


def test_newton_polished_solve_replays_from_a_graph():
    import torch
    B, cand = 1024, 'lattice'
    b1, b2 = _batch(B, 20, 1, seed=1), _batch(B, 20, 1, seed=2)
    with _solver(20, 1, cand, polish_iters=2, polish_step='newton') as s:
        bufs = _dev(torch, b1)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            out = s.solve(*bufs)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            s.solve(*bufs, out=out)
        for rnd, src_batch in enumerate((b2, b1, b2)):
            for dst, src in zip(bufs, _dev(torch, src_batch)):
                dst.copy_(src)
            g.replay()
            torch.cuda.synchronize()
            replayed = {k: v.clone() for k, v in out.items()}
            eager = s.solve(*_dev(torch, src_batch))
            torch.cuda.synchronize()
            for k in KEYS:
                assert torch.equal(replayed[k].nan_to_num(), eager[k].nan_to_num()), (rnd, k)
        host = s.solve(*_args(b2))
        for k in KEYS:
            assert np.array_equal(eager[k].cpu().numpy(), host[k], equal_nan=True), k
    with _solver(20, 1, cand) as s0:
        plain = s0.solve(*_dev(torch, b2))
        torch.cuda.synchronize()
    ok = plain['status'] == 0
    assert (eager['cost'][ok] < plain['cost'][ok]).float().mean() > 0.5


def test_newton_four_handles_in_flight_give_each_batch_solved_alone():
    import torch
    B, N, F, ROUNDS = 1024, 20, 4, 3
    from igtmpc.scenarios import make_batch
    host = [make_batch(B, dtype=np.float64, offset=(q + 1) * B) for q in range(F)]
    dargs = [_dev(torch, h) for h in host]
    fam = lambda q: 'lattice' if q % 2 == 0 else 'track'
    solvers = [_solver(N, 1, fam(q), polish_iters=2, polish_step='newton') for q in range(F)]
    for s in solvers:
        s.set_concurrency(F)
    streams = [torch.cuda.Stream() for _ in range(F)]
    outs = [[None] * ROUNDS for _ in range(F)]
    for q in range(F):
        solvers[q].solve(*dargs[q])
    torch.cuda.synchronize()
    for r in range(ROUNDS):
        for q in range(F):
            with torch.cuda.stream(streams[q]):
                outs[q][r] = solvers[q].solve(*dargs[q])
    torch.cuda.synchronize()
    got = [[{k: outs[q][r][k].cpu().numpy() for k in KEYS} for r in range(ROUNDS)] for q in range(F)]
    for s in solvers:
        s.close()
    for q in range(F):
        with _solver(N, 1, fam(q), polish_iters=2, polish_step='newton') as solo:
            alone = solo.solve(*_args(host[q]))
        with _solver(N, 1, fam(q)) as solo:
            plain = solo.solve(*_args(host[q]))
        ok = plain['status'] == 0
        assert (alone['cost'][ok] < plain['cost'][ok]).mean() > 0.5
        for r in range(ROUNDS):
            for k in KEYS:
                assert np.array_equal(got[q][r][k], alone[k], equal_nan=True), (q, r, k)


def test_closed_loop_driver_with_the_newton_polish_eager_and_from_a_graph():
    from igtmpc.evaluate import run_closed_loop
    kw = dict(sc=1, num_samples=16, N=20)
    grad = run_closed_loop(polish_iters=1, polish_grad='adjoint', **kw)
    a = run_closed_loop(polish_iters=1, polish_step='newton', **kw)
    g = run_closed_loop(polish_iters=1, polish_step='newton', device_resident=True, graph=True, **kw)
    assert np.isfinite(a['x_data']).all()
    assert np.array_equal(a['x_data'], g['x_data']) and np.array_equal(a['u_data'], g['u_data'])
    assert np.array_equal(a['infeasible_ratio'], g['infeasible_ratio']) and np.array_equal(a['deadlock'], g['deadlock'])
    assert not np.array_equal(a['u_data'], grad['u_data'])
