"""-m gpu : the polish of the winner under the value-network cost taken by the library inside the solve (igtmpc.h
igt_set_value_polish; BatchSolver(value_polish_driver='device') / set_value_polish_driver('device'); csrc/igt_kernels_f64.hip
value_trials_f64_kernel / value_accept_f64_kernel around the gradient's and the network's kernels), float64.

Batches and networks are those of tests/test_gpu_value_polish.py (_batch, _net, _cinf, _solver copied, not imported): make_batch
seed 2026, the whitened V_GT_sc1 / V_GT_sc3.  Configurations (B, N, n_obs, n_rk4, network, family): a single problem; a ragged
batch with three hidden layers; one full 64-scenario block of the gradient kernel (tracking seeds); B = 300, past the
256-scenario kept-trajectory path with a ragged tail; N = 40 (ramp-hold seeds); N = 64 with three obstacles, where the kernels'
LDS passes 64 KB; n_rk4 = 2, the generic discretisation.  Every driver here is 'device' unless named.
(The driver of a live solver is switched by set_value_polish_driver: set_value_polish keeps the signature (k) that
tests/test_value_polish_host.py pins.)
The N = 64 batch of 32 has no solved scenario (make_batch(64, N = 64) cut to its first 32 rows, three obstacles each: status 1
throughout, measured): there the two kernels run their skipping paths only, with the dynamic LDS above 64 KB, and every statement
about solved scenarios is empty -- _rows lets that one configuration through and no other.  So that the full path runs above
64 KB as well, the file adds (128, 64, 3, 4, 1, lattice), the batch of tests/test_gpu_value_polish.py, with three solved scenarios.
  * the library exports the setter and a solve on device tensors returns with it on (the parent raises TypeError);
  * k = 0 through the setter, and again after a k = 1 solve, is a handle that never called it, bit for bit on all five outputs;
  * for k = 1..4 argmin and status are the k = 0 solve's, unsolved rows stay NaN / +inf / -1, cost(k) <= cost(k - 1), a scenario
    whose cost did not move kept x and u bit for bit, iteration 1 moves more than half of the solved scenarios by more than 1e-9;
  * x is bit for bit the X igt_rollout_batch_f64 of a 64-candidate value-net table handle gives for u, no verdict raised, cost within
    1e-9 max(1, |ref|) of that roll-out's;
  * the oracle (rollout_frenet, stage_cost with terminal_value, verdicts): x and cost within 1e-9, plans whose worst margin lies
    within 1e-9 of feas_tol set aside, at most 1 %;
  * the restatement (value_polish_restated.polish_value from the k = 0 seeds, k = 1 and 2): cost within 1e-6, a scenario set aside
    only if its two best trials are closer than 1e-7 and it diverged, at most 2 %;
  * the 'host' driver on the same handle and inputs: argmin, status equal, cost within 1e-9 max(1, |ref|) outside those near-ties;
  * device tensors on a side stream, and the warm-start entry, give the bits of the host-array solve;
  * four handles on four streams, two rounds in flight, k = 2: every lane bit-equal to the same batch solved alone;
  * the C entry's refusals, and a solve under stream capture refused with IGT_E_STATE ('stream capture') -- the graph is deleted
    without a replay (nothing in this file is replayed) and the handle solves eagerly to the warm-up's bits afterwards;
  * run_closed_loop with the driver, host arrays and device-resident: finite, other controls than without, equal to each other.
The measured values (profiles/value_polish_device_tests.txt) are printed before they are asserted."""
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
CONFIGS = [(1, 20, 1, 4, 1, 'lattice'), (17, 20, 1, 4, 3, 'lattice'), (64, 20, 1, 4, 1, 'track'), (300, 20, 1, 4, 1, 'lattice'),
           (64, 40, 1, 4, 3, 'ramp_hold'), (32, 64, 3, 4, 1, 'lattice'), (64, 20, 1, 2, 1, 'lattice'), (128, 64, 3, 4, 1, 'lattice')]
NONE_SOLVED = (32, 64, 3, 4, 1, 'lattice')
IGT_E_INVALID = -1                                    # igtmpc.h
cases = pytest.mark.parametrize('B,N,n_obs,n_rk4,sc,cand', CONFIGS)


def _rows(status, *cfg):
    """indices of the solved scenarios; none only in the one configuration known for it"""
    idx = np.flatnonzero(status == 0)
    assert len(idx) > 0 or cfg == NONE_SOLVED, cfg
    return idx


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


def _dev(arrs):
    import torch
    return [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).contiguous().cuda() for a in arrs]


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in KEYS)


def _solver(N, n_obs, n_rk4, sc, cand, **kw):
    import igtmpc
    s = igtmpc.BatchSolver(dtype='f64', cand_mode=cand, cost_mode='value_net', N=N, n_obs=n_obs, n_rk4=n_rk4, **kw)
    s.set_cinf(*_cinf())
    net = _net(sc)
    s.set_value_net(net['layers'], net['Wn'], net['mu_f'], net['sigma_t'], net['mu_t'])
    return s


@functools.lru_cache(maxsize=None)
def _solved(B, N, n_obs, n_rk4, sc, cand):
    """{k: outputs of a host-array solve with k iterations on the device} -- one handle, the setter between the solves --, the
    same for the 'host' driver at k = 1, 2 on that handle (key ('host', k)), and the oracle's parameters.  Computed once, shared."""
    b = _batch(B, N, n_obs)
    out = {}
    with _solver(N, n_obs, n_rk4, sc, cand) as s:
        for k in (0, 1, 2, 3, 4):
            s.set_value_polish_driver('device')
            s.set_value_polish(k)
            out[k] = s.solve(*_args(b))
            if k in (1, 2):                                   # the drivers switched between solves of one handle
                s.set_value_polish_driver('host')
                s.set_value_polish(k)
                out['host', k] = s.solve(*_args(b))
        P = oracle_params(s)
    return out, P


def test_the_library_exports_the_setter_and_takes_device_tensors():
    import torch
    b = _batch(64, 20, 1)
    with _solver(20, 1, 4, 1, 'lattice') as s:
        assert hasattr(s.lib, 'igt_set_value_polish')
        s.set_value_polish_driver('device')
        s.set_value_polish(1)
        assert (s.value_polish_iters, s.value_polish_driver) == (1, 'device')
        o = s.solve(*_dev(_args(b)))
        torch.cuda.synchronize()
        assert (o['status'] == 0).any()
        assert _same(_host(o), _solved(64, 20, 1, 4, 1, 'lattice')[0][1])
    with _solver(20, 1, 4, 1, 'lattice', value_polish_iters=1, value_polish_driver='device') as s:      # the keywords
        assert _same(s.solve(*_args(b)), _solved(64, 20, 1, 4, 1, 'lattice')[0][1])


@cases
def test_zero_iterations_change_nothing(B, N, n_obs, n_rk4, sc, cand):
    b = _batch(B, N, n_obs)
    with _solver(N, n_obs, n_rk4, sc, cand) as s:             # the setter never called
        plain = s.solve(*_args(b))
    with _solver(N, n_obs, n_rk4, sc, cand) as s:
        s.set_value_polish_driver('device')
        s.set_value_polish(0)
        assert s.lib.igt_set_value_polish(s._h, 0) == 0       # (Python makes no call while the field stays 0: the raw entry)
        zero = s.solve(*_args(b))
        s.set_value_polish(1)
        assert s.value_polish_driver == 'device'
        one = s.solve(*_args(b))
        s.set_value_polish(0)
        again = s.solve(*_args(b))
    first = _solved(B, N, n_obs, n_rk4, sc, cand)[0]
    idx = _rows(plain['status'], B, N, n_obs, n_rk4, sc, cand)
    if B >= 17:
        assert (plain['status'] != 0).any()                   # both kinds of scenario are in the batch
    for other in (zero, again, first[0]):
        assert _same(plain, other)
    assert _same(one, first[1]) and (len(idx) == 0 or not np.array_equal(one['u'], plain['u'], equal_nan=True))


@cases
def test_monotone_and_bookkeeping_untouched(B, N, n_obs, n_rk4, sc, cand):
    out, _ = _solved(B, N, n_obs, n_rk4, sc, cand)
    ok = out[0]['status'] == 0
    n_ok = len(_rows(out[0]['status'], B, N, n_obs, n_rk4, sc, cand))
    for k in range(1, 5):
        assert np.array_equal(out[k]['argmin'], out[0]['argmin']) and np.array_equal(out[k]['status'], out[0]['status'])
        assert (out[k]['cost'][ok] <= out[k - 1]['cost'][ok]).all()
        assert np.isnan(out[k]['x'][~ok]).all() and np.isnan(out[k]['u'][~ok]).all()
        assert np.isposinf(out[k]['cost'][~ok]).all() and (out[k]['argmin'][~ok] == -1).all()
        same = out[k]['cost'] == out[k - 1]['cost']           # a scenario whose cost did not move kept its plan
        assert np.array_equal(out[k]['u'][ok & same], out[k - 1]['u'][ok & same])
        assert np.array_equal(out[k]['x'][ok & same], out[k - 1]['x'][ok & same])
    if n_ok == 0:
        return
    drop = out[0]['cost'][ok] - out[1]['cost'][ok]
    print(f'{cand} sc{sc} B={B} N={N} n_rk4={n_rk4}: {ok.sum()} solved, mean cost drop after 1 / 2 / 4 iterations',
          ' / '.join(f'{(out[0]["cost"][ok] - out[k]["cost"][ok]).mean():.4f}' for k in (1, 2, 4)),
          f'; moved by iteration 1: {(drop > 1e-9).mean():.3f}')
    assert (drop > 1e-9).mean() > 0.5


@cases
def test_polished_plan_is_its_own_table_rollout(B, N, n_obs, n_rk4, sc, cand):
    b = _batch(B, N, n_obs)
    out, _ = _solved(B, N, n_obs, n_rk4, sc, cand)
    worst = 0.0
    with _solver(N, n_obs, n_rk4, sc, 'table', C=64) as t:
        for k in (1, 4):
            got = out[k]
            idx = _rows(got['status'], B, N, n_obs, n_rk4, sc, cand)
            assert len(idx) == 0 or (got['cost'][idx] < out[0]['cost'][idx]).mean() > 0.5      # plans the polish wrote, not the emit pass
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
                print(f'{cand} sc{sc} B={B} N={N} k={k} rows {c0}..: rel err of cost_out against the table roll-out {e:.2e}')
                assert e <= 1e-9, (k, c0, e)
    print(f'{cand} sc{sc} B={B} N={N}: max rel err of cost_out against the table roll-out {worst:.2e}')


@cases
def test_polished_plan_against_the_oracle(B, N, n_obs, n_rk4, sc, cand):
    b = _batch(B, N, n_obs)
    out, P = _solved(B, N, n_obs, n_rk4, sc, cand)
    cinf, net = _cinf(), _net(sc)
    for k in (1, 2, 4):
        got = out[k]
        idx = _rows(got['status'], B, N, n_obs, n_rk4, sc, cand)
        if len(idx) == 0:
            return
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


@functools.lru_cache(maxsize=None)
def _restated(B, N, n_obs, n_rk4, sc, cand):
    """the restatement's history from the k = 0 seeds (two iterations) and, per scenario, whether an iteration so far had its two
    best trials closer than 1e-7 -- shared by the restatement test and the comparison of the drivers"""
    b = _batch(B, N, n_obs)
    out, P = _solved(B, N, n_obs, n_rk4, sc, cand)
    cinf, net = _cinf(), _net(sc)
    idx = _rows(out[0]['status'], B, N, n_obs, n_rk4, sc, cand)
    if len(idx) == 0:
        return idx, None, None, None, None
    J0, f0, _ = VP.evaluate(b, idx, out[0]['u'][idx][:, None], P, cinf, net)
    hist, ties = VP.polish_value(b, idx, out[0]['u'][idx], J0[:, 0], 2, P, cinf, net)
    tied = np.logical_or.accumulate([t < 1e-7 for t in ties], axis=0)
    return idx, J0[:, 0], f0[:, 0], hist, tied


@cases
def test_device_follows_the_restatement(B, N, n_obs, n_rk4, sc, cand):
    out, _ = _solved(B, N, n_obs, n_rk4, sc, cand)
    idx, J0, f0, hist, tied = _restated(B, N, n_obs, n_rk4, sc, cand)
    if len(idx) == 0:
        return
    assert f0.all() and rel_err(J0, out[0]['cost'][idx]).max() <= 1e-9
    for k in (1, 2):
        diff = np.abs(out[k]['cost'][idx] - hist[k][1])
        aside = tied[k - 1] & (diff > 1e-6)                   # only a near-tie that did send the two down different steps
        print(f'{cand} sc{sc} B={B} N={N} k={k}: max |J_device - J_restated| {diff[~aside].max(initial=0.0):.2e} (all: {diff.max():.2e}); '
              f'set aside {aside.mean():.4f} of {len(idx)} (near-ties: {tied[k - 1].mean():.4f}); mean drop device '
              f'{(out[0]["cost"][idx] - out[k]["cost"][idx]).mean():.4f} restatement {(J0 - hist[k][1]).mean():.4f}')
        assert aside.mean() <= 0.02
        assert diff[~aside].max(initial=0.0) <= 1e-6


@cases
def test_host_driver_on_the_same_handle(B, N, n_obs, n_rk4, sc, cand):
    out, _ = _solved(B, N, n_obs, n_rk4, sc, cand)
    idx, _, _, _, tied = _restated(B, N, n_obs, n_rk4, sc, cand)
    for k in (1, 2):
        dev, host = out[k], out['host', k]
        assert np.array_equal(dev['argmin'], host['argmin']) and np.array_equal(dev['status'], host['status'])
        if len(idx) == 0:
            assert _same(dev, host)
            continue
        e = rel_err(dev['cost'][idx], host['cost'][idx])
        aside = tied[k - 1] & (e > 1e-9)
        print(f'{cand} sc{sc} B={B} N={N} k={k}: max rel err of cost, device against host driver {e[~aside].max(initial=0.0):.2e} '
              f'(all: {e.max():.2e}); set aside {aside.mean():.4f} of {len(idx)}; bit-equal u: '
              f'{np.mean([np.array_equal(dev["u"][i], host["u"][i]) for i in idx]):.3f}')
        assert aside.mean() <= 0.02
        assert e[~aside].max(initial=0.0) <= 1e-9


@pytest.mark.parametrize('B,N,n_obs,n_rk4,sc,cand', [CONFIGS[1], CONFIGS[3], CONFIGS[5], CONFIGS[7]])
def test_device_tensors_on_a_side_stream(B, N, n_obs, n_rk4, sc, cand):
    import torch
    b = _batch(B, N, n_obs)
    ref = _solved(B, N, n_obs, n_rk4, sc, cand)[0][2]
    with _solver(N, n_obs, n_rk4, sc, cand) as s:
        s.set_value_polish_driver('device')
        s.set_value_polish(2)
        bufs = _dev(_args(b))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            o = s.solve(*bufs)
        side.synchronize()
        assert _same(_host(o), ref)


def test_warm_start_entry_on_device_tensors():
    import torch
    B, N = 64, 20
    b = _batch(B, N, 1)
    seed = _solved(B, N, 1, 4, 1, 'track')[0][0]
    u_ws = np.concatenate([seed['u'][:, :, 1:], seed['u'][:, :, -1:]], axis=2)          # the k = 0 plan shifted by one step
    ok = seed['status'] == 0
    u_ws[~ok] = 0.0
    flags = (b['flags'] | np.where(ok, L.IGT_FLAG_WARM, 0).astype(np.uint32)).astype(np.uint32)
    args = (b['x0'], b['u_prev'], b['kparams'], flags, b['obs_xy'], b['tv_sv'], b['enc'])
    with _solver(N, 1, 4, 1, 'track') as s:
        s.set_value_polish_driver('device')
        s.set_value_polish(2)
        host = s.solve(*args, u_ws=u_ws)
        side = torch.cuda.Stream()
        bufs, ws = _dev(args), torch.from_numpy(u_ws).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            o = s.solve(*bufs, u_ws=ws)
        side.synchronize()
        s.set_value_polish(0)
        plain = s.solve(*args, u_ws=u_ws)
    assert _same(_host(o), host)
    assert (host['status'] == 0).any() and (host['cost'][ok] <= plain['cost'][ok]).all()
    assert not np.array_equal(host['u'], plain['u'], equal_nan=True)


def test_four_handles_on_four_streams():
    import torch
    B, N, F = 64, 20, 4
    batches = [_batch(B, N, 1, seed=2026 + f) for f in range(F)]
    alone = []
    with _solver(N, 1, 4, 1, 'lattice') as s:
        s.set_value_polish_driver('device')
        s.set_value_polish(2)
        alone = [s.solve(*_args(b)) for b in batches]
    solvers = [_solver(N, 1, 4, 1, 'lattice', value_polish_iters=2, value_polish_driver='device') for _ in range(F)]
    try:
        streams = [torch.cuda.Stream() for _ in range(F)]
        bufs = [_dev(_args(b)) for b in batches]
        torch.cuda.synchronize()
        outs = [[None] * F for _ in range(2)]
        for rnd in range(2):                                  # two rounds in flight: nothing waits between them
            for f in range(F):
                with torch.cuda.stream(streams[f]):
                    outs[rnd][f] = solvers[f].solve(*bufs[f])
        torch.cuda.synchronize()
        for rnd in range(2):
            for f in range(F):
                assert _same(_host(outs[rnd][f]), alone[f]), (rnd, f)
        assert all((a['status'] == 0).any() for a in alone)
    finally:
        for s in solvers:
            s.close()


def test_c_refusals():
    import igtmpc
    b = _batch(64, 20, 1)
    with _solver(20, 1, 4, 1, 'lattice') as s:
        fn = s.lib.igt_set_value_polish
        for k in (5, -1):
            assert fn(s._h, k) == IGT_E_INVALID and b'igt_set_value_polish' in s.lib.igt_last_error()
        assert fn(None, 1) == IGT_E_INVALID and b'igt_set_value_polish' in s.lib.igt_last_error()
        assert fn(s._h, 0) == 0 and fn(s._h, 4) == 0 and fn(s._h, 0) == 0
    with igtmpc.BatchSolver(dtype='f64', N=20) as p:                      # a progress handle: it has polish_iters
        assert p.lib.igt_set_value_polish(p._h, 1) == IGT_E_INVALID
        assert b'igt_set_value_polish' in p.lib.igt_last_error() and b'IGT_COST_VALUE_NET' in p.lib.igt_last_error()
        p.set_value_polish_driver('device')
        with pytest.raises(ValueError, match='value_net'):
            p.set_value_polish(1)
            p.set_value_polish(1)
    with igtmpc.BatchSolver(dtype='f32', cost_mode='value_net', N=20) as f:      # the field set on the raw entry, then an _f32 solve
        f.set_cinf(*_cinf())
        net = _net(1)
        f.set_value_net(net['layers'], net['Wn'], net['mu_f'], net['sigma_t'], net['mu_t'])
        f32 = [a.astype(np.float32) if a.dtype == np.float64 else a for a in _args(b)]
        plain = f.solve(*f32)
        assert f.lib.igt_set_value_polish(f._h, 1) == 0
        with pytest.raises(igtmpc.IgtError, match='_f64'):
            f.solve(*f32)
        assert f.lib.igt_set_value_polish(f._h, 0) == 0
        assert _same(f.solve(*f32), plain)
        f.set_value_polish_driver('device')
        with pytest.raises(ValueError, match='f64'):
            f.set_value_polish(1)
            f.set_value_polish(1)


def test_stream_capture_is_refused():
    """Shaped like test_gpu_api.py's workspace-growth case: the refusal is an error return ahead of every stream operation, so the
    capture ends empty and is dropped; nothing is replayed."""
    import igtmpc
    import torch
    B, N = 64, 20
    b = _batch(B, N, 1)
    with _solver(N, 1, 4, 1, 'lattice') as s:
        s.set_value_polish_driver('device')
        s.set_value_polish(1)
        bufs = _dev(_args(b))
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            out = s.solve(*bufs)                         # eager warm-up: the workspace exists
        side.synchronize()
        warm = _host(out)
        g = torch.cuda.CUDAGraph()
        with pytest.raises(igtmpc.IgtError, match='stream capture'):
            with torch.cuda.graph(g, stream=side):
                s.solve(*bufs, out=out)
        del g
        with torch.cuda.stream(side):
            again = s.solve(*bufs)
        side.synchronize()
        assert _same(_host(again), warm)
    assert _same(warm, _solved(B, N, 1, 4, 1, 'lattice')[0][1])


def test_closed_loop_driver_with_the_device_driver():
    from igtmpc.evaluate import run_closed_loop
    kw = dict(sc=1, num_samples=16, N=20, eval_mode='gt_mpc')
    plain = run_closed_loop(**kw)
    a = run_closed_loop(value_polish_iters=1, value_polish_driver='device', **kw)
    r = run_closed_loop(value_polish_iters=1, value_polish_driver='device', device_resident=True, **kw)
    for got in (a, r):
        assert np.isfinite(got['x_data']).all() and np.isfinite(got['u_data']).all()
        assert not np.array_equal(got['u_data'], plain['u_data'])
    assert np.array_equal(a['u_data'], r['u_data'])
