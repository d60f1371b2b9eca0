"""-m gpu : host staging of the C ABI (csrc/igt_api.hip Staging over csrc/igt_stage.h StagePlan).  Every entry that takes
mem = IGT_MEM_HOST | IGT_MEM_DEVICE gives, from host arrays, the bits it gives from device tensors -- the kernels are the same
launches on the same numbers, so any difference is a buffer staged at the wrong place or with the wrong size.

  entry                      host == device asserted by
  solve f64 / f32            here: B = 8 (one packed copy each way) and B = 192 / 384 (past 256 KiB: one copy per buffer);
                             tracking family with a warm start and IGT_FLAG_WARM; value-network cost (tv_sv, enc); n_obs = 0
  rollout-all                here, through ctypes (the Python wrapper is host only): with and without X_all / U_all, both costs
  frenet_step                here, n = 5
  cartesian_euler            here, n = 5: steps = 3, and steps = 0 with u null
  forecast_batch / _scene    here: n_obs = 1 and 2, with and without the three plan arrays
  terminal_value             with dV_out: test_gpu_value_gradient.py::test_device_tensors_give_the_host_bits_and_replay_from_a_graph;
                             without dV_out: here, n = 5
  cost_gradient              test_gpu_gradient.py::test_device_tensors_give_the_host_bits_and_replay_from_a_graph
  cost_gradient_vn           test_gpu_value_gradient.py::test_device_tensors_give_the_host_bits_and_replay_from_a_graph
  solve with polish          test_gpu_polish.py::test_device_tensors_give_the_host_bits

The tests named for the two cost gradients and for terminal_value with dV_out use their own shapes (B = 1000 at N = 20, B = 200 at
N = 64, B = 4096 at N = 40), not B = 4 and n = 5: the entries stage three to five inputs and two outputs whatever B is.

Then one handle through a packed solve, a forecast that grows the staging arena, the packed solve again and a direct one, each
against a fresh handle; and what every entry answers to a `mem` that is neither."""
import ctypes as ct
import functools

import numpy as np
import pytest

from igtmpc import _lib as L
from test_gpu_scene import _gather, _scene_inputs

pytestmark = pytest.mark.gpu

N, C = 20, 64
_NP = {'f32': np.float32, 'f64': np.float64}


@functools.lru_cache(maxsize=None)
def _batch(B, dtype):
    from igtmpc.scenarios import make_batch
    b = make_batch(B, N=N, dtype=_NP[dtype], seed=2026)
    return {k: np.ascontiguousarray(b[k]) for k in ('x0', 'u_prev', 'kparams', 'flags', 'obs_xy', 'tv_sv', 'enc')}


def _solver(dtype='f64', cand='lattice', value=False, **kw):
    import igtmpc
    s = igtmpc.BatchSolver(dtype=dtype, cand_mode=cand, cost_mode='value_net' if value else 'progress', N=N, C=C, **kw)
    if value:
        s.set_value_net(igtmpc.shipped_value_net(1)['layers'])
    return s


def _dev(a):
    import torch
    if a is None:
        return None
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).contiguous().cuda()


def _bits(a):
    return None if a is None else (a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)).tobytes()


def _same(host, dev):
    """bit for bit (NaN rows of unsolved scenarios included), key by key or item by item"""
    items = [(k, host[k], dev[k]) for k in host] if isinstance(host, dict) else list(zip(range(len(host)), host, dev))
    assert items
    for k, a, b in items:
        assert _bits(a) == _bits(b), k


def _solve_args(B, dtype, warm=False, value=False, n_obs=1):
    b = _batch(B, dtype)
    flags, u_ws = b['flags'], None
    if warm:
        flags = flags.copy()
        flags[::2] |= np.uint32(L.IGT_FLAG_WARM)
        u_ws = np.ascontiguousarray(np.repeat(b['u_prev'][:, :, None], N, axis=2) * _NP[dtype](0.9))
    return dict(x0=b['x0'], u_prev=b['u_prev'], kparams=b['kparams'], flags=flags, obs_xy=b['obs_xy'] if n_obs else None,
                tv_sv=b['tv_sv'] if value else None, enc=b['enc'] if value else None, u_ws=u_ws)


@pytest.mark.parametrize('dtype,B,kw', [
    ('f64', 8, {}), ('f64', 192, {}), ('f32', 8, {}), ('f32', 384, {}),
    ('f64', 8, dict(cand='track', warm=True)), ('f64', 8, dict(value=True)), ('f64', 8, dict(n_obs=0))])
def test_solve_from_host_arrays_equals_solve_from_device_tensors(dtype, B, kw):
    import torch
    kw = dict(kw)
    a = _solve_args(B, dtype, warm=kw.pop('warm', False), value=kw.get('value', False), n_obs=kw.get('n_obs', 1))
    with _solver(dtype, **kw) as s:
        host = s.solve(**a)
        dev = s.solve(**{k: _dev(v) for k, v in a.items()})
        torch.cuda.synchronize()
        _same(host, dev)
        assert (host['status'] == 0).any()                            # something was solved: the outputs are not all markers


def _rollout(s, a, want, device):
    """igt_rollout_batch_ws_f64 through ctypes, host arrays or device tensors -> (X, U, cost, viol), X = U = None unless want"""
    import torch
    B = len(a['x0'])
    shapes = [((B, C, 7, N + 1), np.float64), ((B, C, 2, N), np.float64), ((B, C), np.float64), ((B, C), np.int32)]
    if device:
        out = [torch.empty(sh, dtype=torch.float64 if dt is np.float64 else torch.int32, device='cuda') for sh, dt in shapes]
        ins = [_dev(v) for v in a.values()]
        ptr = lambda t: None if t is None else t.data_ptr()
    else:
        out = [np.empty(sh, dt) for sh, dt in shapes]
        ins = list(a.values())
        ptr = lambda t: None if t is None else t.ctypes.data
    if not want:
        out[0] = out[1] = None
    rc = s.lib.igt_rollout_batch_ws_f64(s._h, B, *(ptr(t) for t in ins), *(ptr(t) for t in out),
                                        L.IGT_MEM_DEVICE if device else L.IGT_MEM_HOST, ct.c_void_p(1) if device else None)
    assert rc == 0, s.lib.igt_last_error()
    torch.cuda.synchronize()
    return out, ins


@pytest.mark.parametrize('value', [False, True])
@pytest.mark.parametrize('want', [True, False])
def test_rollout_all_from_host_arrays_equals_rollout_all_from_device_tensors(want, value):
    a = _solve_args(4, 'f64', value=value)
    with _solver('f64', value=value) as s:
        host, _ = _rollout(s, a, want, device=False)
        dev, keep = _rollout(s, a, want, device=True)
        _same(host, dev)
        assert np.isfinite(host[2]).any()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_model_steps_from_host_arrays_equal_those_from_device_tensors(dtype):
    import torch
    b = _batch(8, dtype)
    x, u, kp = (np.ascontiguousarray(b[k][:5]) for k in ('x0', 'u_prev', 'kparams'))
    z0 = np.ascontiguousarray(x[:, [0, 1, 6, 5]])
    uu = np.ascontiguousarray(np.repeat(u[:, :, None], 3, axis=2))
    with _solver(dtype) as s:
        _same([s.frenet_step(x, u, kp)], [s.frenet_step(_dev(x), _dev(u), _dev(kp))])
        _same([s.cartesian_euler(z0, uu)], [s.cartesian_euler(_dev(z0), _dev(uu))])
        # steps = 0 with u null: z_out[n,4,1] is z0
        cart = getattr(s.lib, f'igt_cartesian_euler_{dtype}')
        h0, d0, dz = np.empty((5, 4, 1), _NP[dtype]), torch.empty((5, 4, 1), dtype=_dev(z0).dtype, device='cuda'), _dev(z0)
        assert cart(s._h, 5, 0, z0.ctypes.data, None, h0.ctypes.data, L.IGT_MEM_HOST, None) == 0
        assert cart(s._h, 5, 0, dz.data_ptr(), None, d0.data_ptr(), L.IGT_MEM_DEVICE, ct.c_void_p(1)) == 0
        torch.cuda.synchronize()
        _same([h0], [d0])
        assert np.array_equal(h0[:, :, 0], z0)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('M', [2, 3])
def test_forecasts_from_host_arrays_equal_those_from_device_tensors(M, dtype):
    import torch
    import igtmpc
    c = lambda v: np.ascontiguousarray(v.astype(_NP[dtype]) if v.dtype == np.float64 else v)
    sq = (lambda v: np.ascontiguousarray(v[:, 0])) if M == 2 else (lambda v: v)      # two vehicles: no n_obs axis on the inputs
    scene = [c(v) for v in _scene_inputs(5, M, N, seed=31 + M)]
    gathered = [c(v) if k == 0 else c(sq(v)) for k, v in enumerate(_gather(*scene))]
    with igtmpc.BatchSolver(N=N, n_obs=M - 1, dtype=dtype) as s:
        for plans in (True, False):
            sc, ga = (scene, gathered) if plans else (scene[:3], gathered[:4])
            host = s.forecast_scene(*sc)
            _same(host, s.forecast_scene(*(_dev(v) for v in sc)))
            torch.cuda.synchronize()
            _same(s.forecast(*ga), s.forecast(*(_dev(v) for v in ga)))
            assert np.isfinite(host[0]).all() and np.isfinite(host[1]).all()


def test_terminal_value_without_partials_from_host_arrays_equals_that_from_device_tensors():
    b = _batch(8, 'f64')
    tv, enc = b['tv_sv'][:5].copy(), b['enc'][:5].copy()
    sv = np.ascontiguousarray(np.stack([b['x0'][:5, 2] + 20.0, b['x0'][:5, 5]], axis=-1))
    with _solver('f64', value=True) as s:
        host = s.terminal_value(sv, tv, enc, want_grad=False)
        dev = s.terminal_value(_dev(sv), _dev(tv), _dev(enc), want_grad=False)
        assert host['dV'] is None and dev['dV'] is None and np.isfinite(host['V']).all()
        _same([host['V']], [dev['V']])
        _same([host['V']], [s.terminal_value(sv, tv, enc)['V']])           # ... and asking for the partials leaves V alone


def test_one_handle_through_packed_grown_and_direct_calls_equals_fresh_handles():
    """Packed solve, a forecast_scene that grows the staging arena (d_stage is reallocated, the pinned mirror is not), the packed
    solve again, a direct solve: each result is a fresh handle's."""
    small, big = _solve_args(8, 'f64'), _solve_args(192, 'f64')
    scene = [np.ascontiguousarray(v) for v in _scene_inputs(200, 2, N, seed=5)]      # 134 KB of obs_xy against a 24 KB arena
    steps = [('solve', small), ('scene', scene), ('solve', small), ('solve', big)]
    run = lambda s, what, a: s.solve(**a) if what == 'solve' else s.forecast_scene(*a)
    fresh = []
    for what, a in steps:
        with _solver('f64') as s:
            fresh.append(run(s, what, a))
    with _solver('f64') as s:
        for (what, a), ref in zip(steps, fresh):
            _same(ref, run(s, what, a))


def test_every_entry_refuses_a_mem_that_is_neither_host_nor_device():
    """mem = 7: IGT_E_INVALID 'mem must be ...' from each of the nine staged entries for a non-empty batch; for an empty one the two
    value-gradient entries refuse it as well (they look at mem first), the other seven return IGT_OK."""
    b = _batch(8, 'f64')
    p = lambda a: a.ctypes.data
    x0, up, kp, fl, obs, tv, enc = (p(b[k]) for k in ('x0', 'u_prev', 'kparams', 'flags', 'obs_xy', 'tv_sv', 'enc'))
    big = np.zeros(8 * C * 7 * (N + 1))                                     # an output of any entry fits (none is written)
    o = p(big)
    route = p(np.zeros(16, np.int32))
    with _solver('f64') as s, _solver('f64', value=True) as v:
        s.set_routes()
        lib = s.lib
        calls = {
            'solve': lambda n: lib.igt_solve_batch_f64(s._h, n, x0, up, kp, fl, obs, None, None, o, o, o, o, o, 7, None),
            'rollout': lambda n: lib.igt_rollout_batch_f64(s._h, n, x0, up, kp, fl, obs, None, None, o, o, o, o, 7, None),
            'frenet_step': lambda n: lib.igt_frenet_step_f64(s._h, n, x0, up, kp, o, 7, None),
            'cartesian': lambda n: lib.igt_cartesian_euler_f64(s._h, n, 3, x0, o, o, 7, None),
            'forecast': lambda n: lib.igt_forecast_batch_f64(s._h, n, x0, x0, x0, route, None, None, None, o, o, 7, None),
            'forecast_scene': lambda n: lib.igt_forecast_scene_f64(s._h, n, x0, x0, route, None, None, None, o, o, 7, None),
            'cost_gradient': lambda n: lib.igt_cost_gradient_f64(s._h, n, x0, kp, fl, o, o, o, 7, None),
            'terminal_value': lambda n: lib.igt_terminal_value_f64(v._h, n, x0, tv, enc, o, o, 7, None),
            'cost_gradient_vn': lambda n: lib.igt_cost_gradient_vn_f64(v._h, n, x0, kp, fl, tv, enc, o, o, o, 7, None),
        }
        for name, call in calls.items():
            assert call(2) == -1 and b'mem must be IGT_MEM_DEVICE or IGT_MEM_HOST' in lib.igt_last_error(), name
            want = -1 if name in ('terminal_value', 'cost_gradient_vn') else 0
            assert call(0) == want, name
            if want:
                assert b'mem must be' in lib.igt_last_error(), name
        assert not big.any()
