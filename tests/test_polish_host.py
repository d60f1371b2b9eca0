"""CPU: the `polish_iters` option (igtmpc.h) -- the parameter struct, the refusals that need no GPU, and the numpy restatement
of the polish (tests/polish_restated.py) that the GPU tests compare the device against.

The restatement is pinned on 64 make_batch scenarios, seeded with the oracle's own lattice and tracking winners: every polished
plan is feasible by constraint_violation(check_rate=True), none is dearer than its seed, and the first iteration lowers the cost
of every solved scenario (49 of 49 lattice seeds, 58 of 58 tracking seeds when this was written)."""
import ctypes as ct

import numpy as np
import pytest

import np_oracle as O
import polish_restated as R
from igtmpc import _lib as L


def test_params_field_replaces_reserved_in_place():
    assert L.igt_params.polish_iters.offset == L.igt_params.refine_iters.offset + 4
    assert L.igt_params.polish_iters.offset == 24 + 14 * 8 + 4 and L.igt_params.polish_iters.size == 4
    assert L.igt_params.track_ke.offset == 24 + 14 * 8 + 8
    assert ct.sizeof(L.igt_params) == 24 + 14 * 8 + 8 + 5 * 8
    assert not hasattr(L.igt_params, 'reserved')
    lib = L.load()
    p = L.igt_params()
    p.polish_iters = 3
    assert lib.igt_params_default(ct.byref(p)) == 0
    assert p.polish_iters == 0 and p.refine_iters == 0


def test_header_names_the_field_where_the_struct_has_it():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'igtmpc.h')).read()
    body = hdr[hdr.index('typedef struct igt_params'):hdr.index('} igt_params;')]
    assert 'reserved' not in body
    assert body.index('int32_t refine_iters;') < body.index('int32_t polish_iters;') < body.index('double track_ke;')


@pytest.mark.parametrize('kw, word', [
    (dict(dtype='f32', polish_iters=1), 'f64'),
    (dict(dtype='f64', polish_iters=1, cost_mode='value_net'), 'progress'),
    (dict(dtype='f64', polish_iters=5), '[0, 4]'),
    (dict(dtype='f64', polish_iters=-1), '[0, 4]'),
])
def test_python_refuses_before_any_gpu_call(kw, word, monkeypatch):
    import igtmpc
    lib = L.load()

    def no_create(*a):
        raise AssertionError('igt_create reached')
    monkeypatch.setattr(igtmpc.solver.L, 'load', lambda: type('NoCreate', (), {
        'igt_params_default': lib.igt_params_default, 'igt_create': no_create, 'igt_destroy': lambda *a: 0})())
    with pytest.raises(ValueError, match=word.replace('[', r'\[').replace(']', r'\]')):
        igtmpc.BatchSolver(**kw)


@pytest.mark.parametrize('field, value, cost, word', [
    ('polish_iters', 5, L.IGT_COST_PROGRESS, 'polish_iters must be in [0, 4]'),
    ('polish_iters', -1, L.IGT_COST_PROGRESS, 'polish_iters must be in [0, 4]'),
    ('polish_iters', 1, L.IGT_COST_VALUE_NET, 'polish_iters needs IGT_COST_PROGRESS'),
])
def test_create_refuses_in_the_checker(field, value, cost, word):
    lib = L.load()
    p = L.igt_params()
    assert lib.igt_params_default(ct.byref(p)) == 0
    setattr(p, field, value)
    p.cost_mode = cost
    h = ct.c_void_p()
    assert lib.igt_create(ct.byref(p), 0, ct.byref(h)) == -1      # IGT_E_INVALID: the checker runs before any device call
    assert word in lib.igt_last_error().decode()


def test_planner_and_driver_take_the_option():
    import inspect
    from igtmpc.evaluate import run_closed_loop
    from igtmpc.planner import MPC_Planner
    assert inspect.signature(MPC_Planner.__init__).parameters['polish_iters'].default == 0
    assert inspect.signature(run_closed_loop).parameters['polish_iters'].default == 0


def _seeds(cand):
    from igtmpc.cinf import cinf_halfplanes
    from igtmpc.scenarios import make_batch
    P, cinf = O.Params(), cinf_halfplanes()
    b = make_batch(64, dtype=np.float64)
    args = (b['x0'], b['u_prev'], b['kparams'], b['flags'], b['obs_xy'], *cinf, P)
    sol = O.solve_batch(*args) if cand == 'lattice' else O.solve_batch_refined(*args, refine_iters=0, cand='track')[0]
    idx = np.flatnonzero(sol['status'] == 0)
    return b, idx, sol['u'][idx], sol['cost'][idx], P, cinf


@pytest.mark.parametrize('cand, solved', [('lattice', 49), ('track', 58)])
def test_restatement_is_feasible_monotone_and_moves_every_seed(cand, solved):
    b, idx, u, J, P, cinf = _seeds(cand)
    assert len(idx) == solved
    Js, fs, _ = R.evaluate(b, idx, u[:, None], P, cinf)
    assert fs.all() and np.array_equal(Js[:, 0], J)          # the seeds are the oracle's own winners
    hist, _ = R.polish(b, idx, u, J, 4, P, cinf)
    for it in range(1, 5):
        uk, Jk = hist[it]
        Je, fe, _ = R.evaluate(b, idx, uk[:, None], P, cinf)
        assert fe.all(), f'{cand}: infeasible plan after {it} iterations'
        assert np.array_equal(Je[:, 0], Jk)
        assert (Jk <= hist[it - 1][1]).all() and (Jk <= J).all()
    drop1 = J - hist[1][1]
    print(f'{cand}: mean drop after 1 / 2 / 4 iterations',
          ' / '.join(f'{(J - hist[k][1]).mean():.4f}' for k in (1, 2, 4)), f'-- lowered by iteration 1: {(drop1 > 0).sum()} of {len(idx)}')
    assert (drop1 > 0).all()
