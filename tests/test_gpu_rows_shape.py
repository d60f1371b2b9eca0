"""-m gpu : with three or more solves in flight (igt_set_concurrency) the acceleration-row pass ahead of the float64 search
(accel_rows_kernel) runs in one-wave workgroups instead of 256-thread ones (igt_launch.h plan_search64 rows_threads), and its
queue builders sort in 32 trips of 64 threads instead of 8 of 256.  The lane mapping, the row masks, the travel sums and the
order table are meant to be the same, so a solve must be the same bits -- x, u, cost, argmin, status -- with the shape chosen at
concurrency 4, at the same concurrency with the 256 threads switched back on (DEV_WIDE_ROWS), and alone at concurrency 1.

The smallest shapes at which the kernel can go wrong (256 compute units):
  B = 1027, C = 256, N = 20, lattice    row pass on (B W > 4096), 64-candidate units, a ragged last workgroup (1027 = 64 * 16 + 3)
  B = 1027, C = 256, N = 20, tracking   the travel sums and the twin test across the wave's lanes
  B = 4100, C = 256, N = 20, lattice    the pool search; the builders sort one item per scenario (pool_units > 0)
  B = 4100, C = 64,  N = 8,  lattice    G = 8: eight scenarios per wave
"""
import numpy as np
import pytest

from igtmpc._lib import DEV_WIDE_ROWS

pytestmark = pytest.mark.gpu

KEYS = ('x', 'u', 'cost', 'argmin', 'status')
IN = ('x0', 'u_prev', 'kparams', 'flags', 'obs_xy')
CASES = [(1027, 256, 20, 'lattice'), (1027, 256, 20, 'track'), (4100, 256, 20, 'lattice'), (4100, 64, 8, 'lattice')]


@pytest.fixture(scope='module')
def igt():
    import igtmpc
    igtmpc.load_library()
    return igtmpc


def _solve(igt, monkeypatch, b, case, flags, conc):
    from igtmpc.cinf import cinf_halfplanes
    _, C, N, cand = case
    monkeypatch.setenv('IGT_DEV_FLAGS', str(flags))
    with igt.BatchSolver(dtype='f64', cand_mode=cand, N=N, C=C, n_obs=1) as s:
        s.set_cinf(*cinf_halfplanes())
        s.set_concurrency(conc)
        o = s.solve(*[b[k] for k in IN])
    monkeypatch.delenv('IGT_DEV_FLAGS')
    return {k: np.asarray(o[k]) for k in KEYS}


@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_one_wave_row_workgroups_change_no_bit(igt, monkeypatch, case):
    from igtmpc.scenarios import make_batch
    b = make_batch(case[0], N=case[2], dtype=np.float64, seed=2031)
    alone = _solve(igt, monkeypatch, b, case, 0, 1)
    assert (alone['status'] == 0).mean() > 0.2, 'too few feasible scenarios to compare winners'
    narrow = _solve(igt, monkeypatch, b, case, 0, 4)
    wide = _solve(igt, monkeypatch, b, case, DEV_WIDE_ROWS, 4)
    for got, ref, what in ((narrow, wide, 'one wave against 256 threads, concurrency 4'), (narrow, alone, 'one wave against the solve alone'),
                           (wide, alone, '256 threads, concurrency 4, against the solve alone')):
        for k in KEYS:
            assert np.array_equal(got[k], ref[k], equal_nan=True), (what, k)
