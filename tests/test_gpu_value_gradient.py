"""-m gpu : the terminal value with its partials and the gradient of the value-network cost on the device (igtmpc.h
igt_terminal_value_f64, igt_cost_gradient_vn_f64; csrc/igt_value_net.h terminal_value_f64_kernel, csrc/igt_kernels_f64.hip
cost_gradient_f64_kernel<TERM_LEAVE / TERM_VALUE>), float64.

Networks as in tests/test_value_gradient_host.py: V_GT_sc1 (two hidden layers) and V_GT_sc3 (three) with a non-identity whitening,
sigma_t = 1.7, mu_t = -0.4.  Inputs: the recipe of tests/test_gpu_gradient.py (copied, not imported) with the batch's own tv_sv and
enc.  The bar is the project's float64 one, 1e-9 max(1, |ref|), against tests/value_gradient_restated.py.

  * terminal_value: n in {1, 15, 16, 17, 64, 1000} (partly filled tile, one tile, tile + 1, several waves, more groups than one
    pass of a small grid), V and dV against the restatement, want_grad=False the same V bits, nothing stored past n;
    V against the value inside igt_rollout_batch_f64's cost on a value-net table handle, 4096 states;
  * cost_gradient(tv_sv=, enc=): B in {1, 64, 200, 1000}, N in {20, 64}, n_rk4 in {4, 2}, both depths; break-point set-aside
    (< 1e-7) at most 1 %; cost_out against the table roll-out; sigma_t = 0 leaves the stage terms;
  * NaN rows, host arrays == device tensors bit for bit, replay from a captured graph, growth under capture -> IGT_E_STATE,
    every refusal, and a gt_mpc solve on the same handle unchanged by calls to the two entries."""
import functools

import numpy as np
import pytest

import adjoint_restated as A
import np_oracle as O
import value_gradient_restated as VG
from helpers import oracle_params, rel_err
from igtmpc import _lib as L

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _net(sc, sigma_t=1.7):
    from igtmpc import shipped_value_net
    rng = np.random.default_rng(100 + sc)
    return dict(shipped_value_net(sc), Wn=np.eye(6) + 0.05 * rng.normal(size=(6, 6)),
                mu_f=np.array([20.0, 2.5, 0.0, 0.0, 0.0, 0.0]) + 0.1 * rng.normal(size=6), sigma_t=sigma_t, mu_t=-0.4)


@functools.lru_cache(maxsize=None)
def _batch(B, N):
    from igtmpc.scenarios import make_batch
    return make_batch(B, N=N, dtype=np.float64, seed=2026)


@functools.lru_cache(maxsize=None)
def _grad_inputs(B, N, n_rk4):
    """x0, kparams, flags, tv_sv, enc, U[B,2,N], P: one random lattice candidate per scenario; every third scenario carries the
    abs-heading flag, every fifth sequence is steered off the lane"""
    b = _batch(max(B, 64), N)
    P = O.Params(N=N, n_rk4=n_rk4)
    rng = np.random.default_rng(0)
    n = len(b['x0'])
    pick = rng.integers(0, 256, size=n)
    U = np.concatenate([O.candidates_lattice(b['u_prev'][i:i + 256], P)[np.arange(len(pick[i:i + 256])), pick[i:i + 256]]
                        for i in range(0, n, 256)])
    U[::5, 1, :5] += 0.2 * np.sign(rng.standard_normal((len(U[::5]), 1)))
    flags = np.asarray(b['flags']).copy()
    flags[::3] |= np.uint32(O.FLAG_ABS_HEADING)
    c = lambda a: np.ascontiguousarray(a[:B])
    return c(b['x0']), c(b['kparams']), c(flags), c(b['tv_sv']), c(b['enc']), c(U), P


def _solver(N, sc=1, n_rk4=4, cand='lattice', net=None, **kw):
    import igtmpc
    from igtmpc.cinf import cinf_halfplanes
    s = igtmpc.BatchSolver(dtype='f64', cand_mode=cand, cost_mode='value_net', N=N, n_rk4=n_rk4, **kw)
    s.set_cinf(*cinf_halfplanes())
    net = net or _net(sc)
    s.set_value_net(net['layers'], net['Wn'], net['mu_f'], net['sigma_t'], net['mu_t'])
    return s


@functools.lru_cache(maxsize=None)
def _table_rollout(sc, N=20, B=64):
    """A value-net table handle's roll-out of 64 candidates for B scenarios: (sv[B 64, 2], tv[B 64, 2], enc[B 64, 2], the value
    inside its cost [B 64], the cost [B, 64], the table [64, 2, N])."""
    x0, kp, flags, tv, enc, U, _ = _grad_inputs(max(B, 64), N, 4)
    b = _batch(max(B, 64), N)
    table = np.ascontiguousarray(U[:64])
    with _solver(N, sc, cand='table', C=64) as t:
        t.set_candidate_table(table)
        r = t.rollout_all(x0[:B], np.ascontiguousarray(b['u_prev'][:B]), kp[:B], flags[:B], np.ascontiguousarray(b['obs_xy'][:B]),
                          tv[:B], enc[:B], want_U=False)
        P = oracle_params(t)
    X = r['X']
    stage = O.stage_cost(X, table[None], P, terminal_value=0.0)           # cost = stage terms - V (mpc.py:369)
    sv = np.ascontiguousarray(np.stack([X[:, :, O.IS, N], X[:, :, O.IV, N]], axis=-1).reshape(-1, 2))
    rep = lambda a: np.ascontiguousarray(np.repeat(a[:B], 64, axis=0))
    return sv, rep(tv), rep(enc), (stage - r['cost']).reshape(-1), r['cost'], table


@functools.lru_cache(maxsize=None)
def _restated_values(sc):
    sv, tv, enc, _, _, _ = _table_rollout(sc)
    return VG.terminal_value_and_partials(_net(sc), sv, tv, enc)


@pytest.mark.parametrize('sc', [1, 3])
@pytest.mark.parametrize('n', [1, 15, 16, 17, 64, 1000])
def test_terminal_value_against_the_restatement(n, sc):
    import torch
    sv, tv, enc, _, _, _ = (a[:n] for a in _table_rollout(sc))
    V, dV = (a[:n] for a in _restated_values(sc))
    with _solver(20, sc) as s:
        got = s.terminal_value(sv, tv, enc)
        only = s.terminal_value(sv, tv, enc, want_grad=False)
        # device buffers 16 states longer than n: nothing behind n is stored
        bV = torch.full((n + 16,), 7.0, dtype=torch.float64, device='cuda')
        bG = torch.full((n + 16, 2), 7.0, dtype=torch.float64, device='cuda')
        dev = s.terminal_value(*(torch.from_numpy(a).cuda() for a in (sv, tv, enc)), out=dict(V=bV[:n], dV=bG[:n]))
        torch.cuda.synchronize()
    eV, eG = rel_err(got['V'], V).max(), rel_err(got['dV'], dV).max()
    print(f'sc{sc} n={n}: max rel err V {eV:.2e} dV {eG:.2e}; max |dV| {np.abs(dV).max(axis=0)}')
    assert eV <= 1e-9 and eG <= 1e-9
    assert only['dV'] is None and np.array_equal(only['V'], got['V'])
    assert np.array_equal(bV[:n].cpu().numpy(), got['V']) and np.array_equal(bG[:n].cpu().numpy(), got['dV'])
    assert (bV[n:] == 7.0).all() and (bG[n:] == 7.0).all()


@pytest.mark.parametrize('sc', [1, 3])
def test_terminal_value_is_the_value_inside_the_table_rollouts_cost(sc):
    sv, tv, enc, V_roll, _, _ = _table_rollout(sc)
    V, dV = _restated_values(sc)
    with _solver(20, sc) as s:
        got = s.terminal_value(sv, tv, enc)
    e_roll, eV, eG = rel_err(got['V'], V_roll).max(), rel_err(got['V'], V).max(), rel_err(got['dV'], dV).max()
    print(f'sc{sc} n={len(sv)}: max rel err of V against the roll-out {e_roll:.2e}, against the restatement V {eV:.2e} dV {eG:.2e}; '
          f'max |dV| {np.abs(dV).max(axis=0)}')
    assert np.abs(dV[:, 0]).max() > 1e-3 and np.abs(dV[:, 1]).max() > 1e-3
    assert e_roll <= 1e-9 and eV <= 1e-9 and eG <= 1e-9


@pytest.mark.parametrize('B, N, n_rk4, sc', [(1, 20, 4, 1), (64, 20, 4, 3), (200, 20, 2, 1), (1000, 20, 4, 3), (1000, 20, 2, 1),
                                            (64, 64, 4, 1), (200, 64, 2, 3), (1, 64, 2, 3)])
def test_gradient_against_the_restatement(B, N, n_rk4, sc):
    x0, kp, flags, tv, enc, U, _ = _grad_inputs(B, N, n_rk4)
    with _solver(N, sc, n_rk4) as s:
        got = s.cost_gradient(x0, kp, flags, U, tv_sv=tv, enc=enc)
        P = oracle_params(s)
    J, g = VG.cost_gradient_vn(x0, kp, flags, tv, enc, U, P, _net(sc))
    assert np.isfinite(J).all() and np.isfinite(g).all()
    aside = O.breakpoint_distance(O.apply_flags(x0, flags), U, kp, P) < 1e-7
    eg = rel_err(got['grad'], g).max(axis=(1, 2))
    ej = rel_err(got['cost'], J)
    print(f'sc{sc} B={B} N={N} n_rk4={n_rk4}: max |g| {np.abs(g).max():.1f}, max rel err grad '
          f'{eg[~aside].max() if (~aside).any() else 0:.2e} cost {ej.max():.2e}; set aside {aside.mean():.4f}')
    assert aside.mean() <= 0.01
    assert ej.max() <= 1e-9
    if (~aside).any():
        assert eg[~aside].max() <= 1e-9


@pytest.mark.parametrize('sc, N', [(1, 20), (3, 64)])
def test_cost_is_the_value_net_table_rollouts(sc, N):
    B = 128
    x0, kp, flags, tv, enc, _, _ = _grad_inputs(B, N, 4)
    _, _, _, _, cost, table = _table_rollout(sc, N, B)
    U = np.ascontiguousarray(table[np.arange(B) % 64])                    # scenario b takes table candidate b % 64
    with _solver(N, sc) as s:
        got = s.cost_gradient(x0, kp, flags, U, tv_sv=tv, enc=enc)
    err = rel_err(got['cost'], cost[np.arange(B), np.arange(B) % 64]).max()
    print(f'sc{sc} B={B} N={N}: max rel err of cost_out against the value-net table roll-out {err:.2e}')
    assert err <= 1e-9


def test_sigma_zero_gives_the_stage_terms_only():
    import igtmpc
    x0, kp, flags, tv, enc, U, _ = _grad_inputs(200, 20, 4)
    net0 = _net(1, 0.0)
    with _solver(20, net=net0) as s:
        got = s.cost_gradient(x0, kp, flags, U, tv_sv=tv, enc=enc)
        P = oracle_params(s)
    with igtmpc.BatchSolver(dtype='f64', N=20) as p:
        prog = p.cost_gradient(x0, kp, flags, U)
    J0, g0 = VG.cost_gradient_vn(x0, kp, flags, tv, enc, U, P, net0)
    _, gp = A.cost_gradient(x0, kp, flags, U, P)
    assert rel_err(got['grad'], g0).max() <= 1e-9 and rel_err(got['cost'], J0).max() <= 1e-9
    # ... which is the progress gradient plus the derivative of its progress term, d (s_N - s_0) / du
    ds = g0 - gp
    assert np.abs(ds).max() > 0.1
    # (two device gradients, each held to 1e-9 of its own restatement: their difference to the sum of the two bars)
    assert (np.abs((got['grad'] - prog['grad']) - ds) / np.maximum(1.0, np.abs(g0))).max() <= 2e-9


def test_nonfinite_cost_gives_a_nan_row():
    x0, kp, flags, tv, enc, U, _ = _grad_inputs(64, 20, 4)
    x0, U = x0.copy(), U.copy()
    x0[3, O.IS] = np.nan                                                  # reaches the cost through the network alone
    x0[7, O.IEY] = np.inf
    U[5, 0, 2] = np.nan
    bad = [3, 5, 7]
    with _solver(20, 3) as s:
        got = s.cost_gradient(x0, kp, flags, U, tv_sv=tv, enc=enc)
        sv = np.array([[np.nan, 3.0], [20.0, 3.0], [20.0, np.inf]])
        tvl = s.terminal_value(sv, tv[:3], enc[:3])
    assert not np.isfinite(got['cost'][bad]).any()
    assert np.isnan(got['grad'][bad]).all()
    ok = np.ones(64, bool)
    ok[bad] = False
    assert np.isfinite(got['grad'][ok]).all() and np.isfinite(got['cost'][ok]).all()
    assert np.isnan(tvl['V'][[0, 2]]).all() and np.isnan(tvl['dV'][[0, 2]]).all()
    assert np.isfinite(tvl['V'][1]) and np.isfinite(tvl['dV'][1]).all()


def _dev(torch, arrs):
    return [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).contiguous().cuda() for a in arrs]


@pytest.mark.parametrize('B, N, sc', [(1000, 20, 1), (200, 64, 3)])
def test_device_tensors_give_the_host_bits_and_replay_from_a_graph(B, N, sc):
    import torch
    x0, kp, flags, tv, enc, U, _ = _grad_inputs(B, N, 4)
    Ub = np.ascontiguousarray(U[::-1])                                    # other controls for the same scenarios
    sv = np.ascontiguousarray(np.stack([x0[:, O.IS] + 20.0, x0[:, O.IV]], axis=-1))
    svb = np.ascontiguousarray(sv[::-1])
    with _solver(N, sc) as s:
        host, host_b = (s.cost_gradient(x0, kp, flags, u, tv_sv=tv, enc=enc) for u in (U, Ub))
        thost, thost_b = (s.terminal_value(q, tv, enc) for q in (sv, svb))
        dx0, dkp, dfl, dtv, den, dU, dsv = _dev(torch, (x0, kp, flags, tv, enc, U, sv))
        out = s.cost_gradient(dx0, dkp, dfl, dU, tv_sv=dtv, enc=den)
        tout = s.terminal_value(dsv, dtv, den)
        torch.cuda.synchronize()
        for k in ('cost', 'grad'):
            assert np.array_equal(out[k].cpu().numpy(), host[k], equal_nan=True), k
        for k in ('V', 'dV'):
            assert np.array_equal(tout[k].cpu().numpy(), thost[k]), k
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            s.cost_gradient(dx0, dkp, dfl, dU, out=out, tv_sv=dtv, enc=den)
            s.terminal_value(dsv, dtv, den, out=tout)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            s.cost_gradient(dx0, dkp, dfl, dU, out=out, tv_sv=dtv, enc=den)
            s.terminal_value(dsv, dtv, den, out=tout)
        for rnd, (src, ssrc, ref, tref) in enumerate(((Ub, svb, host_b, thost_b), (U, sv, host, thost), (Ub, svb, host_b, thost_b))):
            dU.copy_(torch.from_numpy(src))
            dsv.copy_(torch.from_numpy(ssrc))
            for v in (*out.values(), *tout.values()):
                v.zero_()
            g.replay()
            torch.cuda.synchronize()
            for k in ('cost', 'grad'):
                assert np.array_equal(out[k].cpu().numpy(), ref[k], equal_nan=True), (rnd, k)
            for k in ('V', 'dV'):
                assert np.array_equal(tout[k].cpu().numpy(), tref[k]), (rnd, k)


def test_workspace_growth_under_capture_is_refused():
    import torch
    x0, kp, flags, tv, enc, U, _ = _grad_inputs(256, 20, 4)
    with _solver(20) as s:
        bufs = _dev(torch, (x0, kp, flags, tv, enc, U))
        out = dict(cost=torch.empty(256, dtype=torch.float64, device='cuda'),
                   grad=torch.empty((256, 2, 20), dtype=torch.float64, device='cuda'))
        ptrs = [t.data_ptr() for t in (*bufs, out['cost'], out['grad'])]
        side = torch.cuda.Stream()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):                            # the handle has no workspace yet
            rc = s.lib.igt_cost_gradient_vn_f64(s._h, 256, *ptrs, L.IGT_MEM_DEVICE, side.cuda_stream)
            msg = s.lib.igt_last_error()
        assert rc == -4 and b'workspace too small for stream capture' in msg
        warm = s.cost_gradient(bufs[0], bufs[1], bufs[2], bufs[5], tv_sv=bufs[3], enc=bufs[4])      # eager: grows it
        torch.cuda.synchronize()
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2, stream=side):
            rc = s.lib.igt_cost_gradient_vn_f64(s._h, 256, *ptrs, L.IGT_MEM_DEVICE, side.cuda_stream)
        assert rc == 0
        g2.replay()
        torch.cuda.synchronize()
        assert torch.equal(out['grad'], warm['grad']) and torch.equal(out['cost'], warm['cost'])


def test_refusals_and_the_empty_batch():
    import igtmpc
    lib = L.load()
    x0, kp, flags, tv, enc, U, _ = _grad_inputs(64, 20, 4)
    sv = np.ascontiguousarray(np.stack([x0[:, O.IS] + 20.0, x0[:, O.IV]], axis=-1))
    cost, grad, V, dV = np.empty(64), np.empty((64, 2, 20)), np.empty(64), np.empty((64, 2))
    ptr = lambda a: None if a is None else a.ctypes.data
    H = L.IGT_MEM_HOST

    def grad_call(h, B=64, a=(x0, kp, flags, tv, enc, U), c=cost, g=grad, mem=H):
        rc = lib.igt_cost_gradient_vn_f64(h, B, *(ptr(q) for q in a), ptr(c), ptr(g), mem, None)
        return rc, lib.igt_last_error()

    def tv_call(h, n=64, a=(sv, tv, enc), v=V, d=dV, mem=H):
        rc = lib.igt_terminal_value_f64(h, n, *(ptr(q) for q in a), ptr(v), ptr(d), mem, None)
        return rc, lib.igt_last_error()

    with _solver(20) as s:
        for call in (grad_call, tv_call):
            rc, msg = call(s._h, -1)
            assert rc == -1 and b'< 0' in msg
            rc, msg = call(s._h, mem=5)
            assert rc == -1 and b'mem must be' in msg
        rc, msg = grad_call(s._h, c=None)
        assert rc == -1 and b'null output' in msg
        rc, msg = grad_call(s._h, g=None)
        assert rc == -1 and b'null output' in msg
        rc, msg = tv_call(s._h, v=None)
        assert rc == -1 and b'null output' in msg
        for i in range(6):
            a = [x0, kp, flags, tv, enc, U]
            a[i] = None
            rc, msg = grad_call(s._h, a=a)
            assert rc == -1 and (b'null buffer' in msg or b'tv_sv / enc required' in msg), i
        for i in range(3):
            a = [sv, tv, enc]
            a[i] = None
            rc, msg = tv_call(s._h, a=a)
            assert rc == -1 and b'null buffer' in msg, i
        cost[:], V[:] = 7.0, 7.0
        assert grad_call(s._h, 0)[0] == 0 and (cost == 7.0).all()
        assert tv_call(s._h, 0)[0] == 0 and (V == 7.0).all()
        assert tv_call(s._h, d=None)[0] == 0                              # dV_out may be null
        # the progress entry keeps refusing value-network handles
        rc = lib.igt_cost_gradient_f64(s._h, 64, ptr(x0), ptr(kp), ptr(flags), ptr(U), ptr(cost), ptr(grad), H, None)
        assert rc == -1 and b'IGT_COST_PROGRESS' in lib.igt_last_error()
        # Python: without tv_sv / enc the call goes where it always went
        with pytest.raises(L.IgtError, match='IGT_COST_PROGRESS'):
            s.cost_gradient(x0, kp, flags, U)
    with igtmpc.BatchSolver(dtype='f64', N=20) as p:                      # a progress handle
        for call in (grad_call, tv_call):
            rc, msg = call(p._h)
            assert rc == -1 and b'IGT_COST_VALUE_NET' in msg
        got = p.cost_gradient(x0, kp, flags, U, tv_sv=tv, enc=enc)        # ... and its Python path is the progress entry's
        assert np.array_equal(got['grad'], p.cost_gradient(x0, kp, flags, U)['grad'])
    with igtmpc.BatchSolver(dtype='f64', cost_mode='value_net', N=20) as v:      # no network loaded
        for call in (grad_call, tv_call):
            rc, msg = call(v._h)
            assert rc == -4 and b'value net not set' in msg
    with igtmpc.BatchSolver(dtype='f32', cost_mode='value_net', N=20) as f:
        with pytest.raises(ValueError, match='f64'):
            f.cost_gradient(x0, kp, flags, U, tv_sv=tv, enc=enc)
        with pytest.raises(ValueError, match='f64'):
            f.terminal_value(sv, tv, enc)


def test_a_gt_mpc_solve_is_unchanged_by_calls_to_the_two_entries():
    B = 256
    b = _batch(B, 20)
    x0, kp, flags, tv, enc, U, _ = _grad_inputs(1000, 20, 4)
    sv = np.ascontiguousarray(np.stack([x0[:, O.IS] + 20.0, x0[:, O.IV]], axis=-1))
    args = (b['x0'], b['u_prev'], b['kparams'], b['flags'], b['obs_xy'], b['tv_sv'], b['enc'])
    with _solver(20) as s:
        before = s.solve(*args)
        assert (before['status'] == 0).any()
        s.cost_gradient(x0, kp, flags, U, tv_sv=tv, enc=enc)
        s.terminal_value(sv, tv, enc)
        after = s.solve(*args)
        s.cost_gradient(x0[:B], kp[:B], flags[:B], U[:B], tv_sv=tv[:B], enc=enc[:B])
        again = s.solve(*args)
    for k in ('x', 'u', 'cost', 'argmin', 'status'):
        assert np.array_equal(before[k], after[k], equal_nan=True), k
        assert np.array_equal(before[k], again[k], equal_nan=True), k
