"""-m gpu : the bookkeeping of the pool roll-out's control-step loop (igt_fast64.h rollout_pool) -- the refill reads a table
laid out per window of candidate numbers, the finished-candidate reduction runs only when a finisher can replace the wave's
best -- changes when that work runs, never what a candidate computes.  So, as in test_gpu_lane_refill.py, every case must
equal the 64-candidate units (DEV_NO_REFILL) bit for bit: x, u, cost, argmin, status.

Cases: pools of fewer than 64 candidates, of a number that is no multiple of 64, and of none (no live acceleration row);
scenarios in which two candidates have exactly the same cost, the winner among them; horizons whose checkpoint pieces are
uneven.  N = 40 cannot reach the pool (16 x 40 steering entries do not fit the table: units on both sides) and is left out.

What the tie case does and does not reach: the two tied candidates are numbered within the first 64 of the pool (columns 8 and
7 are ranks 0 and 1, R <= 16 rows each), start together and finish in the same iteration, so the tie is decided by the butterfly
that the guard lets through, not by the guard's own clause (Jq == wJ and c < wC).  That clause needs a tied candidate of lower
index that finishes in a LATER iteration than its partner.  At C = 256 the exact ties that can be constructed (mirrored
steering on a straight route) are between the columns of least steering, which win and start together; a pair handed out
apart (columns 10 and 5, also exact mirrors) costs more than the winner and never meets an incumbent of its own cost.  At
C = 4096 (G = 64, N <= 5) the second column is handed out after the first, but batches of that size with 4096 candidates are
run nowhere else in the suite and were not taken on here.  So the guard's tie clause is covered by reasoning (igt_fast64.h),
not by a test.

The pools are taken with at least four scenarios per wave slot (B >= 8192 one solve at a time, B >= 4096 with four in flight, on
the 256 compute units of an MI355X); on a part where that does not hold both sides run the units and the cases pass trivially,
as in test_gpu_lane_refill.py.

How many rows are live is decided on the device (accel_rows_kernel: speed box and terminal set).  The tests count rows with
the speed box alone (the terminal set can only remove more), on a batch that sweeps v0 across v_max, and require many
scenarios in each class, so the classes are covered whatever the terminal set removes.
"""
import numpy as np
import pytest

import np_oracle as O
from igtmpc._lib import DEV_NO_REFILL

pytestmark = pytest.mark.gpu

KEYS = ('x', 'u', 'cost', 'argmin', 'status')
G = 16


@pytest.fixture(scope='module')
def igt():
    import igtmpc
    igtmpc.load_library()
    return igtmpc


def _cinf():
    from igtmpc.cinf import cinf_halfplanes
    return cinf_halfplanes()


def _solve(igt, monkeypatch, b, N, flags, conc=1):
    monkeypatch.setenv('IGT_DEV_FLAGS', str(flags))
    with igt.BatchSolver(dtype='f64', cand_mode='lattice', N=N, n_obs=1) as s:
        s.set_cinf(*_cinf())
        s.set_concurrency(conc)
        o = s.solve(b['x0'], b['u_prev'], b['kparams'], b['flags'], b['obs_xy'])
    monkeypatch.delenv('IGT_DEV_FLAGS')
    return {k: np.asarray(o[k]) for k in KEYS}


def _both(igt, monkeypatch, b, N, conc=1):
    pool = _solve(igt, monkeypatch, b, N, 0, conc)
    units = _solve(igt, monkeypatch, b, N, DEV_NO_REFILL, conc)
    for k in KEYS:
        assert np.array_equal(pool[k], units[k], equal_nan=True), k
    return units


def _rows_in_speed_box(b, N):
    """[B, G]: whether the row's (a, v) recurrence keeps the speed box at states 0 .. N-1 (the device also asks the terminal set)"""
    P = O.Params(N=N)
    U = O.candidates_lattice(b['u_prev'], P, G * G)[:, ::G]              # one candidate per row
    B = U.shape[0]
    v = b['x0'][:, 5:6, None] + np.concatenate([np.zeros((B, G, 1)), np.cumsum(P.dt * U[:, :, 0, :], -1)], -1)
    return ~(np.maximum(P.v_min - v[..., :N], v[..., :N] - P.v_max) > P.feas_tol).any(-1)


def _near_v_max(B, N, seed=7):
    """v0 swept across v_max and a_prev across zero: from all rows live to none"""
    from igtmpc.scenarios import make_batch
    b = make_batch(B, N=N, dtype=np.float64, seed=seed)
    i = np.arange(B)
    b['x0'][:, 5] = 4.0 + 1.1 * ((i % 128) / 127.0)                     # 4.0 .. 5.1 (v_max = 5)
    b['u_prev'][:, 0] = -0.6 + 1.6 * ((i // 128) / (B // 128 - 1.0))    # -0.6 .. 1.0
    b['obs_xy'] = b['obs_xy'] + 1.0e4                                   # the obstacle decides nothing here
    return b


@pytest.mark.parametrize('B,conc', [(8192, 1), (4096, 4)])
def test_small_ragged_and_empty_pools(igt, monkeypatch, B, conc):
    N = 20
    b = _near_v_max(B, N)
    R = _rows_in_speed_box(b, N).sum(-1)
    print('live rows (speed box only), scenarios per count:', np.bincount(R, minlength=G + 1))
    assert ((R >= 1) & (R <= 3)).sum() >= 64, 'pools with n < 64'
    assert (R % 4 != 0).sum() >= 256, 'n not a multiple of 64'
    assert (R == 0).sum() >= 64, 'n = 0'
    assert (R == G).sum() >= 64, 'whole pools beside them'
    units = _both(igt, monkeypatch, b, N, conc)
    ok = units['status'] == 0
    print('feasible:', ok.mean(), ' among <= 3 rows:', ok[(R >= 1) & (R <= 3)].mean())
    assert ok[R == 0].sum() == 0 and ok.mean() > 0.1


def _tied(B, N, seed=5):
    """Exact ties by construction: a straight route entered on its axis (e_y = e_psi = 0, delta_f_prev = 0).  The increments of
    the steering columns 7 and 8 are exact negatives of each other (checked by the test), every operation of the roll-out
    is odd or even in the sign of the steering, so the two candidates of a row mirror each other and cost the same to the last
    bit.  They are the columns of least steering -- where the winner is.  Both are handed out in the first refill and finish in
    the same iteration: the butterfly's tie rule decides, through the guard (see the module's docstring).
    (Rows held at a_min or a_max by a_prev at the limit are identical control sequences too, but the terminal set refuses
    every one of them; they were tried and dropped.)"""
    from igtmpc.scenarios import make_batch
    b = make_batch(B, N=N, dtype=np.float64, seed=seed)
    sym = b['kparams'][:, 2] == 0.0
    th = b['x0'][:, 6] - b['x0'][:, 4]
    b['x0'][sym, 0] += b['x0'][sym, 3] * np.sin(th[sym])
    b['x0'][sym, 1] -= b['x0'][sym, 3] * np.cos(th[sym])
    b['x0'][sym, 3] = 0.0
    b['x0'][sym, 4] = 0.0
    b['x0'][sym, 6] = th[sym]
    b['u_prev'][sym, 1] = 0.0
    b['obs_xy'] = b['obs_xy'] + 1.0e4
    return b, sym


@pytest.mark.parametrize('N', [8, 20])
def test_tied_costs(igt, monkeypatch, N):
    B = 8192
    b, sym = _tied(B, N)
    P = O.Params(N=N)
    rd = np.float64(P.dt) * np.float64(P.steer_rate)
    ddf = [-rd + (2 * rd) * np.float64(j) / np.float64(G - 1) for j in range(G)]      # steer_column's expression
    assert ddf[7] == -ddf[8] and ddf[7] != 0.0
    assert sym.sum() >= 2048
    units = _both(igt, monkeypatch, b, N)
    ok = (units['status'] == 0) & sym
    col = units['argmin'] % G
    print(f'N = {N}: symmetric scenarios {sym.sum()}, feasible {ok.sum()}; winner in column 7: {(ok & (col == 7)).sum()}, '
          f'in column 8: {(ok & (col == 8)).sum()}, elsewhere: {(ok & (col != 7) & (col != 8)).sum()}')
    assert (ok & (col == 7)).sum() >= 64, 'the tied pair must hold winners for the tie rule to be tested'
    assert (ok & (col == 8)).sum() == 0, 'ties go to the lowest candidate index'


@pytest.mark.parametrize('N', [22, 10, 13])
def test_checkpoint_records_through_the_guarded_reduction(igt, monkeypatch, N):
    """B >= 8192 one solve at a time: the search leaves the winner's checkpoint records and emit rolls the horizon in pieces from
    them -- a record copied from the wrong lane or at the wrong moment shows in x.  N = 22: pieces from steps 5, 11, 16 (16 x 22
    table entries: the largest horizon that fits); N = 10, 13: uneven pieces."""
    from igtmpc.scenarios import make_batch
    b = make_batch(8200, N=N, dtype=np.float64, seed=2026)
    units = _both(igt, monkeypatch, b, N)
    assert (units['status'] == 0).mean() > 0.1, 'too few feasible scenarios to compare winners'
