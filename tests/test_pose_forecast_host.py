"""No GPU: what run_closed_loop(pose_forecast=) refuses before any solver exists, the keyword's default, the CLI switch and the
binding's declaration of the three pose entries (include/igtmpc.h igt_set_route_headings, igt_forecast_scene_pose_f64,
igt_forecast_batch_pose_f64)."""
import inspect
import os
import re

import pytest


@pytest.mark.parametrize('kw, word', [
    (dict(pose_forecast='bogus'), 'pose_forecast'),
    (dict(pose_forecast='bogus', ca_type='obca'), 'pose_forecast'),
    (dict(pose_forecast='device', ca_type='circle'), 'obca'),
    (dict(pose_forecast='device'), 'obca'),                                             # 'circle' is the default
    (dict(ca_type='obca', pose_forecast='host', device_resident=True), 'obca'),
    (dict(ca_type='obca', pose_forecast='host', device_resident=True, graph=True), 'obca'),
    (dict(ca_type='obca', device_resident=True), 'host loop only'),                     # the default keeps today's message
    (dict(ca_type='obca', pose_forecast='device', dtype='f32'), 'f64'),
    (dict(ca_type='obca', pose_forecast='device', device_resident=True, dtype='f32'), 'f64'),
    (dict(ca_type='obca', pose_forecast='device', polish_iters=1), 'polish'),
    (dict(ca_type='obca', pose_forecast='device', device_resident=True, value_polish_iters=1), 'polish'),
])
def test_driver_refuses_before_any_gpu_call(kw, word, monkeypatch):
    import igtmpc.evaluate as E

    def no_solver(*a, **k):
        raise AssertionError('BatchSolver reached')
    monkeypatch.setattr(E, 'BatchSolver', no_solver)
    with pytest.raises(ValueError, match=word):
        E.run_closed_loop(sc=1, num_samples=2, N=20, **kw)


def test_device_pose_reaches_the_solver_where_the_host_pose_is_refused(monkeypatch):
    """'obca' + 'device' + device_resident / graph / step='fused' passes every refusal: the first thing it fails on is the solver
    this test withholds."""
    import igtmpc.evaluate as E

    class Reached(Exception):
        pass

    def no_solver(*a, **k):
        raise Reached
    monkeypatch.setattr(E, 'BatchSolver', no_solver)
    for kw in (dict(), dict(device_resident=True), dict(device_resident=True, graph=True),
               dict(device_resident=True, step='fused'), dict(device_resident=True, step='fused', graph=True)):
        with pytest.raises(Reached):
            E.run_closed_loop(sc=1, num_samples=2, N=20, ca_type='obca', pose_forecast='device', **kw)


def test_keyword_default_and_cli():
    import igtmpc.evaluate as E
    assert inspect.signature(E.run_closed_loop).parameters['pose_forecast'].default == 'host'
    ap = E.build_parser()
    assert ap.parse_args([]).pose_forecast == 'host'
    assert ap.parse_args(['--pose_forecast', 'host']).pose_forecast == 'host'
    a = ap.parse_args(['--ca_type', 'obca', '--pose_forecast', 'device', '--device_resident', '--graph', '--step', 'fused'])
    assert (a.ca_type, a.pose_forecast, a.device_resident, a.graph, a.step) == ('obca', 'device', True, True, 'fused')
    with pytest.raises(SystemExit):
        ap.parse_args(['--pose_forecast', 'bogus'])


def test_binding_declares_the_pose_entries_as_the_header_does():
    """The three entries are optional symbols of the binding, and each prototype has as many arguments as the header's."""
    from igtmpc import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'igtmpc.h')).read()
    for name in ('igt_set_route_headings', 'igt_forecast_scene_pose_f64', 'igt_forecast_batch_pose_f64'):
        assert name in L.OPTIONAL_SYMBOLS and name in L.SYMBOLS
        decl = re.search(r'\bint ' + name + r'\(([^;]*)\);', header)
        assert decl, name
        assert len(L.SYMBOLS[name][1]) == decl.group(1).count(',') + 1, name
    assert 'IGT_VERSION' in header and L.SYMBOLS['igt_forecast_scene_pose_f64'][1] == L.SYMBOLS['igt_forecast_scene_f64'][1]


def test_f32_handle_refuses_the_pose_methods_before_any_library_call():
    """dtype='f32' handles refuse with a ValueError; nothing of the library is reached (the object has no handle at all)."""
    import numpy as np
    import igtmpc
    s = object.__new__(igtmpc.BatchSolver)
    s.dtype, s._h = 'f32', None

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError(f'library reached: {name}')
    s.lib = NoLib()
    z = np.zeros((1, 2, 7), np.float32)
    with pytest.raises(ValueError, match='f64'):
        s.set_route_headings()
    with pytest.raises(ValueError, match='f64'):
        s.forecast_scene_pose(z, z[..., 0], z[..., 0].astype(np.int32))
    with pytest.raises(ValueError, match='f64'):
        s.forecast_pose(z[:, 0, :3], z[:, 0, :4], z[:, 0, 0], z[:, 0, 0].astype(np.int32), z[:, 0, 0])
