"""-m gpu : a pooled lane gives up a failed candidate at the end of the step that reached the failing state (igt_fast64.h
rollout_pool): |ey| of state k + 1 and the collision of state k are tested after step k, k + 1 < N, instead of by the next step's
step_head; state N stays with horizon_end.  A candidate retired so could never have finished feasible and the survivors fold the
same operands, so every solve must equal the 64-candidate units' (DEV_NO_REFILL, untouched code) bit for bit: x, u, cost, argmin,
status.
Sizes: the smallest at which launch_search64 takes pools -- B = 4096 with igt_set_concurrency(4) (no checkpoints), B = 8192 with
one solve at a time (checkpoints).  Cases, for where an early retirement can go wrong:
  the benchmark mix at N = 20 and N = 9 -- on the CPU (oracle, B = 256, live rows) first lane departures fall on every state
    from 2 to N, the last two included: the k + 1 == N boundary that must be left to horizon_end, and ordinary retirements;
  a crafted start -- a quarter of the scenarios at |ey0| = 0.25 (state 0 fails: every candidate dies in its first step, status
    "none"), a quarter at |ey0| = 0.195 with epsi0 = 0.1 rad of the same sign (state 1 fails for most candidates), half as
    generated; the oracle confirms both kinds of failure in the batch before anything is compared;
  obstacles near (collision as first failure, the loop with the Cartesian rows) and far;
  most scenarios inside an arc (the K = k_v and per-sub-step variants, voted by a changed set of lanes);
  N = 3, where almost nothing dies and no retirement comes before horizon_end.
"""
import numpy as np
import pytest

from igtmpc._lib import DEV_NO_REFILL

pytestmark = pytest.mark.gpu

KEYS = ('x', 'u', 'cost', 'argmin', 'status')
EY_OUT, EY_EDGE, EPSI_EDGE = 0.25, 0.195, 0.1


@pytest.fixture(scope='module')
def igt():
    import igtmpc
    igtmpc.load_library()
    return igtmpc


def _cinf():
    from igtmpc.cinf import cinf_halfplanes
    return cinf_halfplanes()


def _set_start(b, rows, ey, epsi):
    """ey0, epsi0 of `rows`, with x, y, psi moved along so that the start stays one consistent pose on its route"""
    x0 = b['x0']
    th = x0[rows, 6] - x0[rows, 4]
    cx = x0[rows, 0] + x0[rows, 3] * np.sin(th)
    cy = x0[rows, 1] - x0[rows, 3] * np.cos(th)
    x0[rows, 3], x0[rows, 4] = ey, epsi
    x0[rows, 0] = cx - ey * np.sin(th)
    x0[rows, 1] = cy + ey * np.cos(th)
    x0[rows, 6] = th + epsi


def _batch(B, N, obstacles='as generated', arc=False, start='as generated', seed=2027):
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
    if start == 'crafted':               # quarters: outside the lane, at its edge and heading out, as generated (two)
        q = np.arange(B) % 4
        sign = np.where((np.arange(B) // 4) % 2 == 0, 1.0, -1.0)
        _set_start(b, q == 0, (sign * EY_OUT)[q == 0], b['x0'][q == 0, 4])
        _set_start(b, q == 1, (sign * EY_EDGE)[q == 1], (sign * EPSI_EDGE)[q == 1])
    return b


def _oracle_first_states(b, N, rows):
    """|ey| - ey_lim > tol at state 0 and at state 1, for all lattice candidates of `rows` (oracle roll-outs) -> two [rows, C]"""
    import np_oracle as O
    P = O.Params(N=N)
    x0 = O.apply_flags(b['x0'][rows], b['flags'][rows])
    U = O.candidates_lattice(b['u_prev'][rows], P, 256)
    X = O.rollout_frenet(x0[:, None, :], U, b['kparams'][rows][:, None, :], P)
    out = np.abs(X[..., O.IEY, :2]) - P.ey_lim > P.feas_tol
    return out[..., 0], out[..., 1]


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

CASES = [
    (20, 'as generated', False, 'as generated'),      # the benchmark mix
    (9, 'as generated', False, 'as generated'),
    (20, 'as generated', False, 'crafted'),
    (20, 'near', False, 'as generated'),
    (20, 'far', False, 'as generated'),
    (20, 'as generated', True, 'as generated'),
    (3, 'as generated', False, 'as generated'),
]


@pytest.mark.parametrize('build', [NO_CKPT, CKPT], ids=['no_ckpt', 'ckpt'])
@pytest.mark.parametrize('N,obstacles,arc,start', CASES)
def test_pool_retire_equals_units(igt, monkeypatch, build, N, obstacles, arc, start):
    B, conc = build
    b = _batch(B, N, obstacles, arc, start)
    if start == 'crafted':
        q = np.arange(B) % 4
        out0, _ = _oracle_first_states(b, N, np.flatnonzero(q == 0)[:64])
        in0, out1 = _oracle_first_states(b, N, np.flatnonzero(q == 1)[:64])
        print(f'crafted start: state 0 fails for {out0.mean():.3f} of the candidates of the first quarter; of the second, state 0 '
              f'for {in0.mean():.3f} and state 1 for {out1.mean():.3f}')
        assert out0.all(), 'every candidate of a scenario outside the lane fails at state 0'
        assert not in0.any() and out1.mean() > 0.5, 'most candidates at the edge, heading out, first fail at state 1'
    pool = _solve(igt, monkeypatch, b, N, 0, conc)
    units = _solve(igt, monkeypatch, b, N, DEV_NO_REFILL, conc)
    solved = float((units['status'] == 0).mean())
    print(f'B={B} conc={conc} N={N} {obstacles} arc={arc} start={start}: solved share {solved:.3f}')
    # winners to compare: a fifth of a generated batch is solved at the least (tests/test_gpu_pool_step.py,
    # tests/test_gpu_lane_refill.py); of the crafted batch half is as generated
    assert solved > (0.1 if start == 'crafted' else 0.2), 'too few feasible scenarios to compare winners'
    if start == 'crafted':
        assert (units['status'][np.arange(B) % 4 == 0] != 0).all(), 'a start outside the lane has no feasible candidate'
    for k in KEYS:
        assert np.array_equal(pool[k], units[k], equal_nan=True), (build, N, obstacles, arc, start, k)
