"""-m gpu : the pooled float64 lattice search comes in two builds (igt_kernels_f64.hip search_f64_kernel_pool, CKPT).  The one
without checkpoint slots -- three or more solves in flight, so emit rolls the winner in one piece -- reads sin(beta_k) / l_r and
the rotation by beta_k - beta_k-1 from a table laid out once per (steering column, k) (igt_fast64.h fill_pool_table) instead of
forming them per lane and step; the one with checkpoint slots (one solve at a time, emit in pieces) keeps the three-double
table.  Both leave d0 / d1 alone in a whole control step taken as K == 0.  The tabulated values come from the statements the
lanes ran on the same operands, so every solve must equal the 64-candidate units' (DEV_NO_REFILL) bit for bit: x, u, cost,
argmin, status.
Sizes: the smallest at which launch_search64 takes pools -- B = 4096 with igt_set_concurrency(4) (no checkpoints), B = 8192
with one solve at a time (checkpoints).  Cases: obstacles in reach (Cartesian rows rolled) and out of reach, the benchmark mix,
most scenarios inside their arc (the K = k_v and per-sub-step variants beside K == 0, on routes with break-points), a short
horizon whose checkpoint steps are 2, 4 and 6, the previous steering on the clamp (columns that sit at +-df_max from k = 0) and at
zero, G N at the table's limit (16 x 22 = 352 <= 360 entries) and one past it (N = 23: units on both sides).
"""
import numpy as np
import pytest

from igtmpc._lib import DEV_NO_REFILL

pytestmark = pytest.mark.gpu

KEYS = ('x', 'u', 'cost', 'argmin', 'status')


@pytest.fixture(scope='module')
def igt():
    import igtmpc
    igtmpc.load_library()
    return igtmpc


def _cinf():
    from igtmpc.cinf import cinf_halfplanes
    return cinf_halfplanes()


def _batch(B, N, obstacles, arc, steer, df_max, seed=2027):
    from igtmpc.scenarios import make_batch
    b = make_batch(B, N=N, dtype=np.float64, seed=seed)
    obs = b['obs_xy']
    if obstacles == 'far':               # out of every candidate's reach: the roll-outs without the Cartesian rows
        obs = obs + 1.0e4
    elif obstacles == 'near':            # parked 15 m from the ego's start: within reach of every scenario
        obs = np.broadcast_to(b['x0'][:, None, 0:2, None] + np.array([12.0, 9.0])[None, None, :, None], obs.shape).copy()
    b['obs_xy'] = np.ascontiguousarray(obs)
    if arc:                              # most scenarios start inside a bend of the route
        kp = b['kparams'].copy()
        s0 = b['x0'][:, 2]
        inside = np.arange(B) % 4 != 0
        kp[inside, 0] = s0[inside] - 3.0
        kp[inside, 1] = s0[inside] + 60.0
        kp[inside, 2] = np.where(np.arange(B)[inside] % 2 == 0, 0.08, -0.06)
        b['kparams'] = kp
    if steer == 'edge':                  # a quarter each: +df_max, -df_max, exactly zero, as generated
        up = b['u_prev'].copy()
        q = np.arange(B) % 4
        up[q == 0, 1] = df_max
        up[q == 1, 1] = -df_max
        up[q == 2, 1] = 0.0
        b['u_prev'] = up
    return b


def _solve(igt, monkeypatch, b, N, flags, conc):
    monkeypatch.setenv('IGT_DEV_FLAGS', str(flags))
    with igt.BatchSolver(dtype='f64', cand_mode='lattice', N=N, n_obs=1) as s:
        s.set_cinf(*_cinf())
        s.set_concurrency(conc)
        o = s.solve(b['x0'], b['u_prev'], b['kparams'], b['flags'], b['obs_xy'])
    monkeypatch.delenv('IGT_DEV_FLAGS')
    return {k: np.asarray(o[k]) for k in KEYS}


NO_CKPT = (4096, 4)      # B, solves in flight: pools without checkpoint slots
CKPT = (8192, 1)         # pools that leave the winner's checkpoints for emit in pieces


@pytest.mark.parametrize('build,N,obstacles,arc,steer', [
    (NO_CKPT, 20, 'near', False, 'as generated'),
    (NO_CKPT, 20, 'far', False, 'as generated'),
    (NO_CKPT, 20, 'as generated', False, 'as generated'),      # the benchmark mix
    (NO_CKPT, 20, 'as generated', True, 'as generated'),
    (NO_CKPT, 20, 'near', True, 'as generated'),
    (CKPT, 20, 'as generated', False, 'as generated'),
    (CKPT, 20, 'as generated', True, 'as generated'),
    (CKPT, 9, 'as generated', False, 'as generated'),          # checkpoint steps 2, 4, 6
    (NO_CKPT, 9, 'as generated', False, 'as generated'),
    (NO_CKPT, 20, 'as generated', False, 'edge'),
    (NO_CKPT, 20, 'as generated', True, 'edge'),
    (CKPT, 20, 'as generated', False, 'edge'),
    (CKPT, 9, 'as generated', False, 'edge'),
    (NO_CKPT, 22, 'as generated', False, 'as generated'),      # 352 of the table's 360 entries
    (CKPT, 22, 'as generated', False, 'as generated'),
    (NO_CKPT, 23, 'as generated', False, 'as generated'),      # 368 entries: search_pools() falls back to the units
    (CKPT, 23, 'as generated', False, 'as generated'),
])
def test_pool_step_equals_units(igt, monkeypatch, build, N, obstacles, arc, steer):
    B, conc = build
    with igt.BatchSolver(dtype='f64', cand_mode='lattice', N=N, n_obs=1) as s:
        df_max = float(s.params.df_max)
    b = _batch(B, N, obstacles, arc, steer, df_max)
    pool = _solve(igt, monkeypatch, b, N, 0, conc)
    units = _solve(igt, monkeypatch, b, N, DEV_NO_REFILL, conc)
    solved = float((units['status'] == 0).mean())
    print(f'B={B} conc={conc} N={N} {obstacles} arc={arc} steer={steer}: solved share {solved:.3f}')
    # winners to compare: a fifth of a generated batch is solved at the least (tests/test_gpu_lane_refill.py); of the edge
    # batches a quarter is as generated
    assert solved > (0.05 if steer == 'edge' else 0.2), 'too few feasible scenarios to compare winners'
    for k in KEYS:
        assert np.array_equal(pool[k], units[k], equal_nan=True), (build, N, obstacles, arc, steer, k)
