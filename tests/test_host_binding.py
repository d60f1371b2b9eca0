"""What BatchSolver hands to the C entries of the solves, the roll-outs of every candidate and the forecasts, without a GPU and
without the library: the entries are recorders, and what reaches them is held against the prototypes of include/igtmpc.h,
restated below by hand -- argument count and order, which positions are pointers and which scalars, every pointer the address
of an array of the prototype's shape and type, and the three rectangle scalars behind u_ws."""
import numpy as np
import pytest

from igtmpc import _lib as L
from igtmpc.solver import BatchSolver

B, N, C = 3, 4, 64
F8, F4, U4, I4 = np.float64, np.float32, np.uint32, np.int32
HANDLE = 0x5eed


class RecorderLib:
    """Every igt_* symbol: a function that keeps its arguments and answers 0 (no error)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith('igt_'):
            raise AttributeError(name)

        def entry(*args):
            if name == 'igt_create':
                args[2]._obj.value = HANDLE      # ct.byref(h): the handle the later calls must bring back
            self.calls.append((name, args))
            return 0
        return entry

    def last(self, name):
        got = [a for n, a in self.calls if n == name]
        assert got, f'{name} was not called'
        return got[-1]


@pytest.fixture
def lib(monkeypatch):
    rec = RecorderLib()
    monkeypatch.setattr(L, 'load', lambda dev=None: rec)
    return rec


def solver(n_obs, dtype='f64'):
    return BatchSolver(N=N, n_rk4=4, C=C, n_obs=n_obs, dtype=dtype, cand_mode='table')


# ---- the prototypes (include/igtmpc.h), restated: (name, shape, dtype) per pointer, ('name', float) per double by value ----
def common_inputs(fp, no, rows, last):
    """x0 .. enc and the eighth pointer (u_ws, or U of the per-scenario entries); rows = 2 (obs_xy) or 3 (obs_pose)."""
    return [('x0', (B, 7), fp), ('u_prev', (B, 2), fp), ('kparams', (B, 3), fp), ('flags', (B,), U4),
            ('obs', (B, no, rows, N + 1), fp), ('tv_sv', (B, 2), fp), ('enc', (B, 2), fp), last]


def solve_outputs(fp):
    return [('x', (B, 7, N + 1), fp), ('u', (B, 2, N), fp), ('cost', (B,), fp), ('argmin', (B,), I4), ('status', (B,), I4)]


def rollout_outputs(fp):
    return [('X', (B, C, 7, N + 1), fp), ('U', (B, C, 2, N), fp), ('cost', (B, C), fp), ('viol', (B, C), U4)]


BOX = [('length', 4.25), ('width', 1.75), ('d_box', 0.125)]


def u_ws(fp):
    return ('u_ws', (B, 2, N), fp)


def u_cand(fp):
    return ('U_in', (B, C, 2, N), fp)


def make(spec, rng):
    """Arrays for the pointer entries of a spec, C-contiguous and of the prototype's type: what _prep hands on without a copy."""
    out = {}
    for name, shape, dt in spec:
        a = rng.standard_normal(shape) if dt in (F8, F4) else rng.integers(0, 3, shape)
        out[name] = np.ascontiguousarray(a, dtype=dt)
    return out


def check_call(args, count, inputs, arrays, scalars, outputs, result):
    """args: what reached the entry.  h, B | inputs | scalars | outputs | mem, stream."""
    assert len(args) == 2 + len(inputs) + len(scalars) + len(outputs) + 2
    assert getattr(args[0], 'value', args[0]) == HANDLE and args[1] == count
    pos = 2
    for name, shape, dt in inputs:
        a = arrays[name]
        assert isinstance(args[pos], int) and args[pos] == a.ctypes.data, f'{name} at {pos}'
        assert a.shape == shape and a.dtype == dt
        pos += 1
    for name, value in scalars:
        assert isinstance(args[pos], float) and args[pos] == value, f'{name} at {pos}'
        pos += 1
    for name, shape, dt in outputs:
        a = result[name]
        assert isinstance(a, np.ndarray) and a.shape == shape and a.dtype == dt and a.flags.c_contiguous, name
        assert isinstance(args[pos], int) and args[pos] == a.ctypes.data, f'{name} at {pos}'
        pos += 1
    assert args[pos] == L.IGT_MEM_HOST and args[pos + 1] is None      # numpy buffers: host mode, the handle's own stream


# ------------------------------------------------------------------------------------------------ solves and roll-outs
SOLVES = {       # method -> (entry, rows of the obstacle array, eighth pointer, scalars by value, outputs)
    'solve': ('igt_solve_batch_ws_{}', 2, u_ws, [], solve_outputs),
    'solve_candidates': ('igt_solve_candidates_f64', 2, u_cand, [], solve_outputs),
    'solve_box': ('igt_solve_batch_box_f64', 3, u_ws, BOX, solve_outputs),
    'rollout_all': ('igt_rollout_batch_ws_{}', 2, u_ws, [], rollout_outputs),
    'rollout_candidates': ('igt_rollout_candidates_f64', 2, u_cand, [], rollout_outputs),
    'rollout_all_box': ('igt_rollout_batch_box_f64', 3, u_ws, BOX, rollout_outputs),
}


def call_solve(s, method, a, **kw):
    lead = (a['x0'], a['u_prev'], a['kparams'], a['flags'])
    if 'candidates' in method:
        return getattr(s, method)(*lead, a['U_in'], a['obs'], a['tv_sv'], a['enc'], **kw)
    if 'box' in method:
        return getattr(s, method)(*lead, a['obs'], a['tv_sv'], a['enc'], u_ws=a['u_ws'], **dict(BOX), **kw)
    return getattr(s, method)(*lead, a['obs'], a['tv_sv'], a['enc'], u_ws=a['u_ws'], **kw)


@pytest.mark.parametrize('n_obs', [1, 2])
@pytest.mark.parametrize('method,dtype', [(m, 'f64') for m in SOLVES] + [('solve', 'f32'), ('rollout_all', 'f32')])
def test_solves_and_rollouts_reach_their_entry_as_the_header_declares(lib, method, dtype, n_obs):
    entry, rows, last, scalars, outputs = SOLVES[method]
    fp = F8 if dtype == 'f64' else F4
    inputs = common_inputs(fp, n_obs, rows, last(fp))
    a = make(inputs, np.random.default_rng(1))
    s = solver(n_obs, dtype)
    res = call_solve(s, method, a)
    args = lib.last(entry.format(dtype))
    check_call(args, B, inputs, a, scalars, outputs(fp), res)
    if scalars:      # the three doubles sit behind u_ws (position 2 + 7), ahead of the first output
        assert [type(v) for v in args[10:13]] == [float] * 3 and args[9] == a['u_ws'].ctypes.data
        assert args[13] == res['x' if method == 'solve_box' else 'X'].ctypes.data


@pytest.mark.parametrize('method', ['solve', 'solve_candidates', 'solve_box'])
def test_optional_inputs_left_out_reach_the_entry_as_null(lib, method):
    entry, rows, last, scalars, outputs = SOLVES[method]
    inputs = common_inputs(F8, 1, rows, last(F8))
    a = make(inputs, np.random.default_rng(2))
    a['tv_sv'] = a['enc'] = a['u_ws'] = None
    call_solve(solver(1), method, a)
    args = lib.last(entry.format('f64'))
    assert args[7] is None and args[8] is None
    assert (args[9] is None) == (method != 'solve_candidates')


@pytest.mark.parametrize('method', ['rollout_all', 'rollout_candidates', 'rollout_all_box'])
def test_rollouts_without_X_or_U_pass_null_for_them(lib, method):
    entry, rows, last, scalars, outputs = SOLVES[method]
    inputs = common_inputs(F8, 1, rows, last(F8))
    a = make(inputs, np.random.default_rng(3))
    res = call_solve(solver(1), method, a, want_X=False, want_U=False)
    args = lib.last(entry.format('f64'))
    first = 2 + 8 + len(scalars)
    assert res['X'] is None and res['U'] is None and args[first] is None and args[first + 1] is None
    assert args[first + 2] == res['cost'].ctypes.data and args[first + 3] == res['viol'].ctypes.data


@pytest.mark.parametrize('method', ['solve', 'solve_candidates', 'solve_box'])
def test_a_non_contiguous_out_u_is_refused(lib, method):
    entry, rows, last, scalars, outputs = SOLVES[method]
    inputs = common_inputs(F8, 1, rows, last(F8))
    a = make(inputs, np.random.default_rng(4))
    out = {k: np.empty(shape, dt) for k, shape, dt in solve_outputs(F8)}
    out['u'] = np.empty((B, 2, 2 * N), F8)[:, :, ::2]
    with pytest.raises(ValueError, match=r"out\['u'\] must be a contiguous array of the solver dtype"):
        call_solve(solver(1), method, a, out=out)
    assert not [n for n, _ in lib.calls if n == entry.format('f64')]      # refused before the entry


@pytest.mark.parametrize('method', ['solve', 'solve_candidates', 'solve_box'])
def test_the_callers_out_buffers_are_the_ones_written(lib, method):
    entry, rows, last, scalars, outputs = SOLVES[method]
    inputs = common_inputs(F8, 1, rows, last(F8))
    a = make(inputs, np.random.default_rng(5))
    out = {k: np.empty(shape, dt) for k, shape, dt in solve_outputs(F8)}
    res = call_solve(solver(1), method, a, out=out)
    assert res is out
    check_call(lib.last(entry.format('f64')), B, inputs, a, scalars, solve_outputs(F8), out)


# ------------------------------------------------------------------------------------------------ forecasts
def batch_forecast_spec(fp, no, rows, heading):
    ax = () if no == 1 else (no,)
    inputs = [('ego_xyh', (B, 3), fp), ('opp', (B, *ax, 4), fp), ('opp_a', (B, *ax), fp), ('opp_route', (B, *ax), I4)]
    if heading:
        inputs.append(('opp_heading', (B, *ax), fp))
    inputs += [('plan_x', (B, *ax, 7, N + 1), fp), ('plan_u', (B, *ax, 2, N), fp), ('has_plan', (B, *ax), I4)]
    return inputs, [('obs', (B, no, rows, N + 1), fp), ('tv', (B, 2) if no == 1 else (B, no, 2), fp)]


def scene_forecast_spec(fp, no, rows):
    M = no + 1
    inputs = [('x', (B, M, 7), fp), ('a_prev', (B, M), fp), ('route', (B, M), I4), ('plan_x', (B, M, 7, N + 1), fp),
              ('plan_u', (B, M, 2, N), fp), ('has_plan', (B, M), I4)]
    return inputs, [('obs', (B * M, no, rows, N + 1), fp), ('tv', (B * M, no, 2), fp)]


FORECASTS = {       # method -> (entry, spec)
    'forecast': ('igt_forecast_batch_{}', lambda fp, no: batch_forecast_spec(fp, no, 2, False)),
    'forecast_pose': ('igt_forecast_batch_pose_f64', lambda fp, no: batch_forecast_spec(fp, no, 3, True)),
    'forecast_scene': ('igt_forecast_scene_{}', lambda fp, no: scene_forecast_spec(fp, no, 2)),
    'forecast_scene_pose': ('igt_forecast_scene_pose_f64', lambda fp, no: scene_forecast_spec(fp, no, 3)),
}


@pytest.mark.parametrize('n_obs', [1, 2])
@pytest.mark.parametrize('method,dtype', [(m, 'f64') for m in FORECASTS] + [('forecast', 'f32'), ('forecast_scene', 'f32')])
def test_forecasts_reach_their_entry_as_the_header_declares(lib, method, dtype, n_obs):
    entry, spec = FORECASTS[method]
    fp = F8 if dtype == 'f64' else F4
    inputs, outputs = spec(fp, n_obs)
    a = make(inputs, np.random.default_rng(6))
    s = solver(n_obs, dtype)
    obs, tv = getattr(s, method)(*(a[name] for name, _, _ in inputs))
    check_call(lib.last(entry.format(dtype)), B, inputs, a, [], outputs, dict(obs=obs, tv=tv))
    names = [n for n, _ in lib.calls]
    assert 'igt_set_routes' in names      # the default route table is set on the way
    assert ('igt_set_route_headings' in names) == ('pose' in method)


def test_forecasts_without_a_plan_pass_null_for_it(lib):
    for method in FORECASTS:
        entry, spec = FORECASTS[method]
        inputs, outputs = spec(F8, 1)
        a = make(inputs, np.random.default_rng(7))
        given = [a[name] for name, _, _ in inputs if name not in ('plan_x', 'plan_u', 'has_plan')]
        getattr(solver(1), method)(*given)
        args = lib.last(entry.format('f64'))
        assert len(args) == 2 + len(inputs) + 2 + 2
        assert list(args[2 + len(given):2 + len(inputs)]) == [None] * 3
