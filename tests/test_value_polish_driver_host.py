"""The public face of the device-driven polish under the value-network cost (BatchSolver(value_polish_driver=) /
set_value_polish_driver, MPC_Planner, run_closed_loop; igtmpc.h igt_set_value_polish), as far as it needs no GPU: what is
refused and when, what reaches the C entry, and that the default -- the 'host' driver -- never asks for it."""
import os

import numpy as np
import pytest

from igtmpc import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Recording:
    """libigtmpc.so with every entry but igt_params_default answered by a stub that records the call: igt_create hands out a
    handle without a GPU.  without: entries this library does not export (one from before they were added)."""
    def __init__(self, lib, without=()):
        self._lib, self.calls, self._without = lib, [], without

    def __getattr__(self, name):
        if name in self._without:
            raise AttributeError(name)
        if name == 'igt_params_default':
            return self._lib.igt_params_default
        if not name.startswith('igt_'):
            raise AttributeError(name)

        def stub(*a):
            self.calls.append((name,) + tuple(a[1:]) if name == 'igt_set_value_polish' else name)
            return 0
        return stub


def test_header_symbols_and_null_handle():
    hdr = open(os.path.join(ROOT, 'include', 'igtmpc.h')).read()
    assert 'int igt_set_value_polish(igt_handle* h, int iters);' in hdr and 'stream capture' in hdr
    assert 'igt_set_value_polish' in L.SYMBOLS and 'igt_set_value_polish' in L.OPTIONAL_SYMBOLS
    for lib in (L.load(), L.load(dev=True)):
        assert hasattr(lib, 'igt_set_value_polish')
        assert lib.igt_set_value_polish(None, 1) == -1 and b'igt_set_value_polish' in lib.igt_last_error()


def test_unknown_driver_is_refused_before_igt_create(monkeypatch):
    import igtmpc
    rec = _Recording(L.load())
    monkeypatch.setattr(igtmpc.solver.L, 'load', lambda: rec)
    for word in ('gpu', '', None, 'Device'):
        with pytest.raises(ValueError, match='value_polish_driver'):
            igtmpc.BatchSolver(dtype='f64', cost_mode='value_net', N=20, value_polish_driver=word)
    assert 'igt_create' not in rec.calls
    with igtmpc.BatchSolver(dtype='f64', cost_mode='value_net', N=20) as s:
        with pytest.raises(ValueError, match='value_polish_driver'):
            s.set_value_polish_driver('gpu')
        assert (s.value_polish_iters, s.value_polish_driver) == (0, 'host')


def test_device_driver_keeps_the_existing_refusals(monkeypatch):
    import igtmpc
    rec = _Recording(L.load())
    monkeypatch.setattr(igtmpc.solver.L, 'load', lambda: rec)
    with pytest.raises(ValueError, match='f64'):
        igtmpc.BatchSolver(dtype='f32', cost_mode='value_net', N=20, value_polish_iters=1, value_polish_driver='device')
    with pytest.raises(ValueError, match='value_net'):
        igtmpc.BatchSolver(dtype='f64', N=20, value_polish_iters=1, value_polish_driver='device')
    with pytest.raises(ValueError, match=r'\[0, 4\]'):
        igtmpc.BatchSolver(dtype='f64', cost_mode='value_net', N=20, value_polish_iters=5, value_polish_driver='device')
    assert 'igt_create' not in rec.calls
    with igtmpc.BatchSolver(dtype='f32', cost_mode='value_net', N=20) as f:
        f.set_value_polish_driver('device')
        with pytest.raises(ValueError, match='f64'):
            f.set_value_polish(1)
    with igtmpc.BatchSolver(dtype='f64', N=20) as p:
        p.set_value_polish_driver('device')
        with pytest.raises(ValueError, match='value_net'):
            p.set_value_polish(1)
        p.set_value_polish(0)
    assert not [c for c in rec.calls if isinstance(c, tuple)]          # nothing refused reached the C entry


def test_what_reaches_the_c_entry(monkeypatch):
    import igtmpc
    rec = _Recording(L.load())
    monkeypatch.setattr(igtmpc.solver.L, 'load', lambda: rec)
    sets = lambda: [c[1] for c in rec.calls if isinstance(c, tuple)]
    with igtmpc.BatchSolver(dtype='f64', cost_mode='value_net', N=20, value_polish_iters=2) as s:      # the default driver
        s.set_value_polish(1)
        s.set_value_polish(0)
        assert sets() == [] and s.value_polish_driver == 'host'
        s.set_value_polish_driver('device')                   # k = 0: the field stays 0, no call
        assert sets() == []
        s.set_value_polish(3)
        s.set_value_polish(1)                                 # the driver stays
        assert (s.value_polish_iters, s.value_polish_driver) == (1, 'device')
        s.set_value_polish_driver('host')                     # the handle's field goes back to 0, the iterations stay
        assert (s.value_polish_iters, s.value_polish_driver) == (1, 'host')
        s.set_value_polish(2)
        s.set_value_polish_driver('device')
        assert sets() == [3, 1, 0, 2]
    del rec.calls[:]
    with igtmpc.BatchSolver(dtype='f64', cost_mode='value_net', N=20, value_polish_iters=4, value_polish_driver='device') as s:
        assert sets() == [4] and rec.calls.index('igt_create') < rec.calls.index(('igt_set_value_polish', 4))


def test_a_library_without_the_entry_says_so_and_serves_the_host_driver(monkeypatch):
    import igtmpc
    old = _Recording(L.load(), without=('igt_set_value_polish',))
    monkeypatch.setattr(igtmpc.solver.L, 'load', lambda: old)
    with igtmpc.BatchSolver(dtype='f64', cost_mode='value_net', N=20, value_polish_iters=1) as s:
        s.set_value_polish(2)
        with pytest.raises(L.IgtError, match='does not export igt_set_value_polish'):
            s.set_value_polish_driver('device')
        assert (s.value_polish_iters, s.value_polish_driver) == (2, 'host')
    with pytest.raises(L.IgtError, match='rebuild it'):
        igtmpc.BatchSolver(dtype='f64', cost_mode='value_net', N=20, value_polish_iters=1, value_polish_driver='device')


def test_closed_loop_refuses_the_graph_before_a_solver_is_created(monkeypatch):
    import igtmpc
    from igtmpc import evaluate as E
    made = []
    monkeypatch.setattr(E, 'BatchSolver', lambda *a, **k: made.append(k) or (_ for _ in ()).throw(AssertionError('a solver was created')))
    kw = dict(sc=1, num_samples=2, N=20, eval_mode='gt_mpc', value_polish_iters=1)
    for extra in (dict(graph=True), dict(graph=True, device_resident=True)):
        with pytest.raises(ValueError, match='stream capture'):
            E.run_closed_loop(value_polish_driver='device', **extra, **kw)
    with pytest.raises(ValueError, match='value_polish_driver'):
        E.run_closed_loop(value_polish_driver='gpu', **kw)
    with pytest.raises(ValueError, match='host'):             # the default driver's refusal, as it was
        E.run_closed_loop(device_resident=True, **kw)
    assert made == []


def test_planner_solver_key_differs_between_drivers(monkeypatch):
    """planners share a handle by its settings; the driver is one of them (a handle's igt_set_value_polish field is the driver's)"""
    import igtmpc
    from igtmpc import planner as PL
    from igtmpc import routes as R
    made = []

    class Fake:
        np_dtype = np.float64

        def __init__(self, **kw):
            self.kw = kw
            made.append(self)

        def set_cinf(self, *a):
            pass

        def set_value_net(self, **kw):
            pass

        def close(self):
            pass

    monkeypatch.setattr(PL, 'BatchSolver', Fake)
    monkeypatch.setattr(PL, '_SHARED', {})
    pair = list(R.scene_routes(1, 0, 2))
    st = lambda r: igtmpc.VehicleReference({'x': 0.0, 'y': 0.0, 's': 0.0, 'ey': 0.0, 'epsi': 0.0, 'v': 1.0, 'heading': 0.0,
                                            'K': igtmpc.Curvature.from_route(r)})
    agents = [{'type': 'CAV', 'state': st(pair[0])}, {'type': 'CAV', 'state': st(pair[1])}]
    vn = dict(layers=[(np.zeros((128, 6)), np.zeros(128)), (np.zeros((128, 128)), np.zeros(128)), (np.zeros((1, 128)), np.zeros(1))])
    mk = lambda **kw: PL.MPC_Planner(N=20, dt=0.1, agents=agents, routes=pair, index=0, num_rk4_steps=4, use_NN_cost2go=True,
                                     value_net=vn, cand_mode='lattice', value_polish_iters=1, **kw)
    a, b, c, d = mk(), mk(value_polish_driver='device'), mk(value_polish_driver='device'), mk(value_polish_driver='host')
    assert a._solver is d._solver and b._solver is c._solver and a._solver is not b._solver
    assert [m.kw['value_polish_driver'] for m in made] == ['host', 'device']
    assert len(PL._SHARED) == 2
    with pytest.raises(ValueError, match='value_polish_driver'):
        mk(value_polish_driver='gpu')
