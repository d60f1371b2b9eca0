"""-m gpu : the analytic cost gradient on the device (igtmpc.h igt_cost_gradient_f64, igt_set_polish_gradient; csrc/igt_adjoint64.h,
csrc/igt_kernels_f64.hip cost_gradient_f64_kernel and polish_f64_kernel's adjoint mode), float64.

The gradient entry
  * against the numpy restatement (tests/adjoint_restated.py) within 1e-9 max(1, |g|), B in {1, 64, 1000, 4096}, N in {20, 40, 64},
    n_rk4 in {4, 2}; make_batch scenarios (straight and turning routes) with one random lattice candidate each, every third
    scenario with the abs-heading flag, every fifth sequence steered off the lane (infeasible); sequences with a RK stage argument
    within 1e-7 of a curvature break-point set aside (at most 1 %);
  * cost_out within 1e-9 of igt_rollout_batch_f64's cost of the same controls as a table candidate;
  * host arrays and device tensors give the same bits; the call replays from a captured graph to the eager result;
  * the refusals return IGT_E_INVALID with a message; B = 0 is a no-op.
The polish with polish_grad='adjoint' (the structure of tests/test_gpu_polish.py)
  * polish_grad='fd' after igt_set_polish_gradient(h, 0) is a handle that never called it, bit for bit on every output;
  * the polished plan is its own table roll-out bit for bit; the cost is monotone, argmin / status / unsolved scenarios untouched;
  * the device follows polish_adjoint scenario by scenario within 1e-6 in cost after 1 and 2 iterations, a near-tie (< 1e-7 between
    the two best trials) set aside only where it excuses something (at most 2 %);
  * it runs from a graph, with four handles in flight, and through run_closed_loop(polish_grad='adjoint') eager and from a graph
    with equal results."""
import functools

import numpy as np
import pytest

import adjoint_restated as A
import np_oracle as O
import polish_restated as R
from helpers import oracle_params, rel_err
from igtmpc import _lib as L

pytestmark = pytest.mark.gpu

KEYS = ('x', 'u', 'cost', 'argmin', 'status')


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


def _solver(N, n_obs=1, cand='lattice', **kw):
    import igtmpc
    s = igtmpc.BatchSolver(dtype='f64', cand_mode=cand, N=N, n_obs=n_obs, **kw)
    s.set_cinf(*_cinf())
    return s


@functools.lru_cache(maxsize=None)
def _grad_inputs(B, N, n_rk4):
    """x0, kparams, flags, U[B,2,N]: one random lattice candidate per scenario; every third scenario carries the abs-heading
    flag, every fifth sequence is steered off the lane"""
    b = _batch(max(B, 64), N)
    P = O.Params(N=N, n_rk4=n_rk4)
    rng = np.random.default_rng(0)
    n = len(b['x0'])
    pick = rng.integers(0, 256, size=n)
    U = np.concatenate([O.candidates_lattice(b['u_prev'][i:i + 256], P)[np.arange(len(pick[i:i + 256])), pick[i:i + 256]]
                        for i in range(0, n, 256)])
    U[::5, 1, :5] += 0.2 * np.sign(rng.standard_normal((len(U[::5]), 1)))         # a turn of the wheel: off the lane within the horizon
    flags = np.asarray(b['flags']).copy()
    flags[::3] |= np.uint32(O.FLAG_ABS_HEADING)
    return (np.ascontiguousarray(b['x0'][:B]), np.ascontiguousarray(b['kparams'][:B]), np.ascontiguousarray(flags[:B]),
            np.ascontiguousarray(U[:B]), P)


@pytest.mark.parametrize('n_rk4', [4, 2])
@pytest.mark.parametrize('N', [20, 40, 64])
@pytest.mark.parametrize('B', [1, 64, 1000, 4096])
def test_gradient_against_the_restatement(B, N, n_rk4):
    x0, kp, flags, U, P = _grad_inputs(B, N, n_rk4)
    with _solver(N, n_rk4=n_rk4) as s:
        got = s.cost_gradient(x0, kp, flags, U)
        P = oracle_params(s)
    J, g = A.cost_gradient(x0, kp, flags, U, P)
    assert np.isfinite(J).all() and np.isfinite(g).all()
    xf = O.apply_flags(x0, flags)
    if B >= 64:
        assert (kp[:, 2] == 0).any() and (kp[:, 2] != 0).any()            # straight and turning routes
        X = O.rollout_frenet(xf, U, kp, P)
        assert (np.abs(X[:, O.IEY]).max(axis=-1) > P.ey_lim + 0.1).any()  # some sequences leave the lane
    aside = O.breakpoint_distance(xf, U, kp, P) < 1e-7
    eg = rel_err(got['grad'], g).max(axis=(1, 2))
    ej = rel_err(got['cost'], J)
    print(f'B={B} N={N} n_rk4={n_rk4}: max |g| {np.abs(g).max():.1f}, max rel err grad {eg[~aside].max() if (~aside).any() else 0:.2e} '
          f'cost {ej.max():.2e}; set aside {aside.mean():.4f}')
    assert aside.mean() <= 0.01
    assert ej.max() <= 1e-9
    if (~aside).any():
        assert eg[~aside].max() <= 1e-9


@pytest.mark.parametrize('B,N', [(256, 20), (128, 64)])
def test_cost_is_the_table_rollouts(B, N):
    x0, kp, flags, U, _ = _grad_inputs(B, N, 4)
    U = np.ascontiguousarray(U[np.arange(B) % 64])                        # scenario b takes table candidate b % 64
    b = _batch(max(B, 64), N)
    with _solver(N, cand='table', C=64) as t:
        t.set_candidate_table(U[:64])
        r = t.rollout_all(x0, np.ascontiguousarray(b['u_prev'][:B]), kp, flags, np.ascontiguousarray(b['obs_xy'][:B]),
                          want_X=False, want_U=False)
        got = t.cost_gradient(x0, kp, flags, U)
    ref = r['cost'][np.arange(B), np.arange(B) % 64]
    err = rel_err(got['cost'], ref).max()
    print(f'B={B} N={N}: max rel err of cost_out against the table roll-out {err:.2e}')
    assert err <= 1e-9


def test_nonfinite_cost_gives_a_nan_row():
    x0, kp, flags, U, _ = _grad_inputs(64, 20, 4)
    x0, U = x0.copy(), U.copy()
    x0[3, O.IEY] = np.inf
    U[5, 0, 2] = np.nan
    with _solver(20) as s:
        got = s.cost_gradient(x0, kp, flags, U)
    assert not np.isfinite(got['cost'][[3, 5]]).any()
    assert np.isnan(got['grad'][[3, 5]]).all()
    ok = np.ones(64, bool)
    ok[[3, 5]] = False
    assert np.isfinite(got['grad'][ok]).all() and np.isfinite(got['cost'][ok]).all()


def _dev(torch, arrs):
    return [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).contiguous().cuda() for a in arrs]


@pytest.mark.parametrize('B,N', [(1000, 20), (4096, 40), (200, 64)])
def test_device_tensors_give_the_host_bits_and_replay_from_a_graph(B, N):
    import torch
    x0, kp, flags, U, _ = _grad_inputs(B, N, 4)
    Ub = np.ascontiguousarray(U[::-1])                                    # other controls for the same scenarios
    with _solver(N) as s:
        host = s.cost_gradient(x0, kp, flags, U)
        host_b = s.cost_gradient(x0, kp, flags, Ub)
        bufs = _dev(torch, (x0, kp, flags, U))
        out = s.cost_gradient(*bufs)
        torch.cuda.synchronize()
        for k in ('cost', 'grad'):
            assert np.array_equal(out[k].cpu().numpy(), host[k], equal_nan=True), k
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            s.cost_gradient(*bufs, out=out)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            s.cost_gradient(*bufs, out=out)
        for rnd, (src, ref) in enumerate(((Ub, host_b), (U, host), (Ub, host_b))):
            bufs[3].copy_(torch.from_numpy(src))
            out['grad'].zero_()
            out['cost'].zero_()
            g.replay()
            torch.cuda.synchronize()
            for k in ('cost', 'grad'):
                assert np.array_equal(out[k].cpu().numpy(), ref[k], equal_nan=True), (rnd, k)


def test_refusals_and_the_empty_batch():
    lib = L.load()
    x0, kp, flags, U, _ = _grad_inputs(64, 20, 4)
    cost, grad = np.empty(64), np.empty((64, 2, 20))
    ptr = lambda a: a.ctypes.data
    with _solver(20) as s:
        call = lambda B, c, g: lib.igt_cost_gradient_f64(s._h, B, ptr(x0), ptr(kp), ptr(flags), ptr(U), c, g, L.IGT_MEM_HOST, None)
        assert call(-1, ptr(cost), ptr(grad)) == -1 and b'B < 0' in lib.igt_last_error()
        assert call(64, None, ptr(grad)) == -1 and b'null output' in lib.igt_last_error()
        assert call(64, ptr(cost), None) == -1 and b'null output' in lib.igt_last_error()
        cost[:] = 7.0
        assert call(0, ptr(cost), ptr(grad)) == 0 and (cost == 7.0).all()
        assert lib.igt_cost_gradient_f64(s._h, 64, ptr(x0), ptr(kp), ptr(flags), ptr(U), ptr(cost), ptr(grad), 5, None) == -1
        assert b'mem must be' in lib.igt_last_error()
        assert lib.igt_set_polish_gradient(s._h, 2) == -1 and b'IGT_GRAD_' in lib.igt_last_error()
        assert lib.igt_set_polish_gradient(s._h, -1) == -1
        assert lib.igt_set_polish_gradient(s._h, 1) == 0 and lib.igt_set_polish_gradient(s._h, 0) == 0
    import igtmpc
    with igtmpc.BatchSolver(dtype='f64', cost_mode='value_net', N=20) as v:
        rc = lib.igt_cost_gradient_f64(v._h, 64, ptr(x0), ptr(kp), ptr(flags), ptr(U), ptr(cost), ptr(grad), L.IGT_MEM_HOST, None)
        assert rc == -1 and b'IGT_COST_PROGRESS' in lib.igt_last_error()
    with igtmpc.BatchSolver(dtype='f32', N=20) as f:
        with pytest.raises(ValueError, match='f64'):
            f.cost_gradient(x0, kp, flags, U)


# ---------------------------------------------------------------------------------------------------------------- the polish
CONFIGS = [(256, 20, 1), (4096, 20, 1), (1024, 40, 1), (128, 64, 3)]


@functools.lru_cache(maxsize=None)
def _solved(B, N, n_obs, cand='lattice', iters=(0, 1, 2, 4)):
    b = _batch(B, N, n_obs)
    out = {}
    for k in iters:
        with _solver(N, n_obs, cand, polish_iters=k, polish_grad='adjoint') as s:
            out[k] = s.solve(*_args(b))
            P = oracle_params(s)
    return out, P


@pytest.mark.parametrize('B,N,n_obs', [(256, 20, 1), (4096, 20, 1), (128, 64, 3)])
def test_forward_difference_mode_set_explicitly_changes_nothing(B, N, n_obs):
    b = _batch(B, N, n_obs)
    with _solver(N, n_obs, polish_iters=2) as s:                          # never called the setter
        plain = s.solve(*_args(b))
    with _solver(N, n_obs, polish_iters=2) as s:
        s._check(s.lib.igt_set_polish_gradient(s._h, L.IGT_GRAD_ADJOINT))
        other = s.solve(*_args(b))
        s._check(s.lib.igt_set_polish_gradient(s._h, L.IGT_GRAD_FORWARD_DIFF))
        back = s.solve(*_args(b))
    for k in KEYS:
        assert np.array_equal(plain[k], back[k], equal_nan=True), k
    assert not np.array_equal(plain['u'], other['u'], equal_nan=True)     # ... and the other mode is another computation


@pytest.mark.parametrize('B,N,n_obs', CONFIGS)
def test_adjoint_monotone_and_bookkeeping_untouched(B, N, n_obs):
    out, _ = _solved(B, N, n_obs)
    ok = out[0]['status'] == 0
    assert 0.0 < ok.mean() < 1.0
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


@pytest.mark.parametrize('B,N,n_obs', CONFIGS)
def test_adjoint_polished_plan_is_its_own_table_rollout_bit_for_bit(B, N, n_obs):
    b = _batch(B, N, n_obs)
    out, _ = _solved(B, N, n_obs)
    with _solver(N, n_obs, 'table', C=64) as t:
        for k in (1, 4):
            got = out[k]
            idx = np.flatnonzero(got['status'] == 0)
            assert (got['cost'][idx] < out[0]['cost'][idx]).mean() > 0.5
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
@pytest.mark.parametrize('B,N', [(256, 20), (64, 40)])
def test_device_follows_the_adjoint_restatement(B, N, cand):
    b = _batch(B, N, 1)
    out, P = _solved(B, N, 1, cand, (0, 1, 2))
    cinf = _cinf()
    idx = np.flatnonzero(out[0]['status'] == 0)
    assert len(idx) >= 8
    J0, f0, _ = R.evaluate(b, idx, out[0]['u'][idx][:, None], P, cinf)
    assert f0.all() and rel_err(J0[:, 0], out[0]['cost'][idx]).max() <= 1e-9
    hist, ties = A.polish_adjoint(b, idx, out[0]['u'][idx], J0[:, 0], 2, P, cinf)
    tied = np.zeros(len(idx), dtype=bool)
    for k in (1, 2):
        tied |= ties[k - 1] < 1e-7
        diff = np.abs(out[k]['cost'][idx] - hist[k][1])
        aside = tied & (diff > 1e-6)
        print(f'{cand} B={B} N={N} k={k}: max |J_device - J_restated| {diff[~aside].max():.2e} (all: {diff.max():.2e}); '
              f'set aside {aside.mean():.4f} of {len(idx)} (near-ties: {tied.mean():.4f}); mean drop {(J0[:, 0] - hist[k][1]).mean():.4f}')
        assert aside.mean() <= 0.02
        assert diff[~aside].max() <= 1e-6


def _dev_batch(torch, b):
    return _dev(torch, _args(b))


@pytest.mark.parametrize('B,cand', [(4096, 'lattice'), (2048, 'track')])
def test_adjoint_polished_solve_replays_from_a_graph(B, cand):
    import torch
    b1, b2 = _batch(B, 20, 1, seed=1), _batch(B, 20, 1, seed=2)
    with _solver(20, 1, cand, polish_iters=2, polish_grad='adjoint') as s:
        bufs = _dev_batch(torch, b1)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            out = s.solve(*bufs)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            s.solve(*bufs, out=out)
        for rnd, src_batch in enumerate((b2, b1, b2)):
            for dst, src in zip(bufs, _dev_batch(torch, src_batch)):
                dst.copy_(src)
            g.replay()
            torch.cuda.synchronize()
            replayed = {k: v.clone() for k, v in out.items()}
            eager = s.solve(*_dev_batch(torch, src_batch))
            torch.cuda.synchronize()
            for k in KEYS:
                assert torch.equal(replayed[k].nan_to_num(), eager[k].nan_to_num()), (rnd, k)
        host = s.solve(*_args(b2))
        for k in KEYS:
            assert np.array_equal(eager[k].cpu().numpy(), host[k], equal_nan=True), k
    with _solver(20, 1, cand) as s0:
        plain = s0.solve(*_dev_batch(torch, b2))
        torch.cuda.synchronize()
    ok = plain['status'] == 0
    assert (eager['cost'][ok] < plain['cost'][ok]).float().mean() > 0.5


def test_adjoint_four_handles_in_flight_give_each_batch_solved_alone():
    import torch
    B, N, F, ROUNDS = 4096, 20, 4, 3
    from igtmpc.scenarios import make_batch
    host = [make_batch(B, dtype=np.float64, offset=(q + 1) * B) for q in range(F)]
    dargs = [_dev_batch(torch, h) for h in host]
    fam = lambda q: 'lattice' if q % 2 == 0 else 'track'
    solvers = [_solver(N, 1, fam(q), polish_iters=2, polish_grad='adjoint') for q in range(F)]
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
        with _solver(N, 1, fam(q), polish_iters=2, polish_grad='adjoint') as solo:
            alone = solo.solve(*_args(host[q]))
        with _solver(N, 1, fam(q)) as solo:
            plain = solo.solve(*_args(host[q]))
        ok = plain['status'] == 0
        assert (alone['cost'][ok] < plain['cost'][ok]).mean() > 0.5
        for r in range(ROUNDS):
            for k in KEYS:
                assert np.array_equal(got[q][r][k], alone[k], equal_nan=True), (q, r, k)


def test_closed_loop_driver_with_the_adjoint_polish_eager_and_from_a_graph():
    from igtmpc.evaluate import run_closed_loop
    kw = dict(sc=1, num_samples=16, N=20)
    plain = run_closed_loop(**kw)
    a = run_closed_loop(polish_iters=1, polish_grad='adjoint', **kw)
    g = run_closed_loop(polish_iters=1, polish_grad='adjoint', device_resident=True, graph=True, **kw)
    assert np.isfinite(a['x_data']).all()
    assert np.array_equal(a['x_data'], g['x_data']) and np.array_equal(a['u_data'], g['u_data'])
    assert np.array_equal(a['infeasible_ratio'], g['infeasible_ratio']) and np.array_equal(a['deadlock'], g['deadlock'])
    assert not np.array_equal(a['u_data'], plain['u_data'])
