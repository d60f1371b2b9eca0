"""-m gpu : the float64 lattice search rolls each scenario's live candidates as one pool whose lanes refill (igt_fast64.h
rollout_pool, igt_kernels_f64.hip search_pool64).  Which candidate a lane rolls when, and which sub-step variant a wave votes
for, differ from the 64-candidate units; the statements each candidate runs do not.  So the solve must equal the units'
(DEV_NO_REFILL) bit for bit: x, u, cost, argmin, status -- with and without the queue builder (B <= 4096 sorts the queues),
a ragged last block, the large batch, horizons whose checkpoint pieces are uneven, a horizon whose steering table does not
fit (the units run either way), one to four obstacles, batches where every obstacle is out of reach, where none is, and
where most scenarios start inside their arc, and several solves in flight (igt_set_concurrency(4)).
Pools are taken with at least four scenarios per wave slot: B >= 8192 with one solve at a time (which also leaves the winner's
checkpoints for emit in pieces), B >= 4096 with igt_set_concurrency(4) (one wave per SIMD).  B = 1536 stays below that: units
on both sides.
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


def _batch(B, N=20, n_obs=1, obstacles='as generated', arc=False, seed=2026):
    from igtmpc.scenarios import make_batch
    b = make_batch(B, N=N, dtype=np.float64, seed=seed)
    obs = b['obs_xy']
    if obstacles == 'far':               # out of every candidate's reach: the roll-outs without the Cartesian rows
        obs = obs + 1.0e4
    elif obstacles == 'near':            # parked 15 m from the ego's start: within reach of every scenario, so every one is judged
        obs = np.broadcast_to(b['x0'][:, None, 0:2, None] + np.array([12.0, 9.0])[None, None, :, None], obs.shape).copy()
    # more vehicles: the forecast shifted sideways, one more per obstacle
    obs = np.concatenate([obs + 2.5 * m * np.array([1.0, -1.0])[None, None, :, None] for m in range(n_obs)], axis=1)
    b['obs_xy'] = np.ascontiguousarray(obs)
    if arc:                              # most scenarios start inside a bend of the route
        kp = b['kparams'].copy()
        s0 = b['x0'][:, 2]
        inside = np.arange(B) % 4 != 0
        kp[inside, 0] = s0[inside] - 3.0
        kp[inside, 1] = s0[inside] + 60.0
        kp[inside, 2] = np.where(np.arange(B)[inside] % 2 == 0, 0.08, -0.06)
        b['kparams'] = kp
    return b


def _solve(igt, monkeypatch, b, N, n_obs, flags, conc=1):
    monkeypatch.setenv('IGT_DEV_FLAGS', str(flags))
    with igt.BatchSolver(dtype='f64', cand_mode='lattice', N=N, n_obs=n_obs) as s:
        s.set_cinf(*_cinf())
        s.set_concurrency(conc)
        o = s.solve(b['x0'], b['u_prev'], b['kparams'], b['flags'], b['obs_xy'])
    monkeypatch.delenv('IGT_DEV_FLAGS')
    return {k: np.asarray(o[k]) for k in KEYS}


def _same(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


@pytest.mark.parametrize('B,N,n_obs,obstacles,arc,conc', [
    (1536, 20, 1, 'as generated', False, 1),      # below the pools' batch size
    (4096, 20, 1, 'as generated', False, 4),      # the benchmark batch, queue builder inside accel_rows_kernel
    (4097, 20, 2, 'as generated', False, 4),      # ragged: no queue order, a hole in the last block of 8
    (8200, 20, 1, 'as generated', False, 1),      # checkpoint records, ragged
    (65536, 20, 1, 'as generated', False, 1),     # BASELINE configs[2]
    (8192, 8, 1, 'as generated', False, 1),       # short horizon: checkpoint pieces of two steps
    (8192, 18, 3, 'as generated', False, 1),      # uneven pieces (4, 9, 13)
    (8192, 24, 1, 'as generated', False, 1),      # 16 columns x 24 steps do not fit the table: the units run either way
    (8192, 20, 4, 'far', False, 1),               # every scenario far
    (8192, 20, 2, 'near', False, 1),              # no scenario far
    (8192, 20, 1, 'as generated', True, 1),       # most scenarios inside their arc: the sub-step votes mix
    (4096, 20, 1, 'near', True, 4),
])
def test_pools_equal_units(igt, monkeypatch, B, N, n_obs, obstacles, arc, conc):
    b = _batch(B, N=N, n_obs=n_obs, obstacles=obstacles, arc=arc)
    pool = _solve(igt, monkeypatch, b, N, n_obs, 0, conc)
    units = _solve(igt, monkeypatch, b, N, n_obs, DEV_NO_REFILL, conc)
    assert (units['status'] == 0).mean() > 0.2, 'too few feasible scenarios to compare winners'
    _same(pool, units, (B, N, n_obs, obstacles, arc))


def test_pools_in_flight_equal_units(igt, monkeypatch):
    """Four handles on four streams with igt_set_concurrency(4) -- the benchmark's regime: the search takes one wave per SIMD
    and emit rolls the winner in one piece -- against the same batches solved alone through the units."""
    import torch
    F, B = 4, 4096
    host = [_batch(B, seed=11 + q) for q in range(F)]
    units = [_solve(igt, monkeypatch, host[q], 20, 1, DEV_NO_REFILL) for q in range(F)]
    keys = ('x0', 'u_prev', 'kparams', 'flags', 'obs_xy')
    dev = [[torch.from_numpy(h[k].view(np.int32) if h[k].dtype == np.uint32 else h[k]).cuda() for k in keys] for h in host]
    solvers = []
    for q in range(F):
        s = igt.BatchSolver(dtype='f64', cand_mode='lattice')
        s.set_cinf(*_cinf())
        s.set_concurrency(F)
        solvers.append(s)
    for q in range(F):                   # the workspaces grow on first use: not while overlapped
        solvers[q].solve(*dev[q])
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(F)]
    outs = [None] * F
    for rnd in range(2):
        for q in range(F):
            with torch.cuda.stream(streams[q]):
                outs[q] = solvers[q].solve(*dev[q])
        torch.cuda.synchronize()
        for q in range(F):
            got = {k: outs[q][k].cpu().numpy() for k in KEYS}
            _same(got, units[q], ('in flight', rnd, q))
    for s in solvers:
        s.close()
