"""-m gpu : with three or more solves in flight (igt_set_concurrency) the one-piece float64 emit behind the pool search raises
its wave priority once at its top (igt_launch.h plan_search64 emit_priority; emit_f64_kernel<..., PRIO>, a build of its own).  The
priority changes when the wave's instructions issue and nothing they compute, so a solve must be the same bits -- x, u, cost,
argmin, status -- with the raised build at concurrency 4, at the same concurrency with priority 0 switched back on
(DEV_EMIT_PRIO0), and alone at concurrency 1, where the plan asks for no priority.

The smallest shapes that reach the code (256 compute units):
  B = 4100, C = 256, N = 20, lattice, concurrency 4   the pool search, the raised emit; a ragged last wave (4100 = 64 * 64 + 4)
  B = 4100, C = 64,  N = 8,  lattice, concurrency 4   G = 8, one unit per scenario, a short horizon
  B = 8200, C = 256, N = 20, lattice, concurrency 1   the pool at two waves per SIMD: emit in pieces, the switch must change nothing
  B = 1027, C = 256, N = 20, tracking, concurrency 4  64-candidate units: the one-piece emit stays at priority 0 (its build has no other)
In the first case the speed x0[:, 5] of a few scenarios is put above v_max -- no candidate is feasible, and the raised wave takes
the branch that writes status 1 and NaN rows for those lanes -- and that of their neighbours in the same emit wave just inside it,
where only candidates that brake at once stay in the speed box: lanes that leave early beside lanes that roll a winner.
"""
import numpy as np
import pytest

from igtmpc._lib import DEV_EMIT_PRIO0

pytestmark = pytest.mark.gpu

KEYS = ('x', 'u', 'cost', 'argmin', 'status')
IN = ('x0', 'u_prev', 'kparams', 'flags', 'obs_xy')
CASES = [(4100, 256, 20, 'lattice', 4), (4100, 64, 8, 'lattice', 4), (8200, 256, 20, 'lattice', 1), (1027, 256, 20, 'track', 4)]
ABOVE = (3, 700, 1500, 2047, 4099)        # scenarios whose speed is put above v_max (first case)
INSIDE = (5, 701, 1501, 2046, 4098)       # ... and just inside it: each in the emit wave (64 consecutive scenarios) of one above


@pytest.fixture(scope='module')
def igt():
    import igtmpc
    igtmpc.load_library()
    return igtmpc


def _solve(igt, monkeypatch, b, case, flags, conc):
    from igtmpc.cinf import cinf_halfplanes
    _, C, N, cand, _ = case
    monkeypatch.setenv('IGT_DEV_FLAGS', str(flags))
    with igt.BatchSolver(dtype='f64', cand_mode=cand, N=N, C=C, n_obs=1) as s:
        s.set_cinf(*cinf_halfplanes())
        s.set_concurrency(conc)
        o = s.solve(*[b[k] for k in IN])
    monkeypatch.delenv('IGT_DEV_FLAGS')
    return {k: np.asarray(o[k]) for k in KEYS}


@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_raised_emit_priority_changes_no_bit(igt, monkeypatch, case):
    from igtmpc.scenarios import make_batch
    B, C, N, cand, conc = case
    b = make_batch(B, N=N, dtype=np.float64, seed=2031)
    if case == CASES[0]:
        with igt.BatchSolver(dtype='f64', cand_mode=cand, N=N, C=C, n_obs=1) as s:
            v_max, tol = s.params.v_max, s.params.feas_tol
        b['x0'] = b['x0'].copy()
        b['x0'][list(ABOVE), 5] = v_max + 0.5
        b['x0'][list(INSIDE), 5] = v_max - 1e-3
    alone = _solve(igt, monkeypatch, b, case, 0, 1)
    if case == CASES[0]:
        assert (alone['status'][list(ABOVE)] == 1).all() and (alone['argmin'][list(ABOVE)] == -1).all()
        assert np.isnan(alone['x'][list(ABOVE)]).all() and np.isinf(alone['cost'][list(ABOVE)]).all()
        assert all(a // 64 == i // 64 for a, i in zip(ABOVE, INSIDE))
        solved = alone['status'][list(INSIDE)] == 0      # a winner just inside the box starts at the edited speed and never exceeds v_max
        assert (alone['x'][list(INSIDE)][solved][:, 5, 0] == v_max - 1e-3).all()
        assert (alone['x'][list(INSIDE)][solved][:, 5, :N] <= v_max + tol).all()
    assert (alone['status'] == 0).mean() > 0.2, 'too few feasible scenarios to compare winners'
    raised = _solve(igt, monkeypatch, b, case, 0, conc)
    level0 = _solve(igt, monkeypatch, b, case, DEV_EMIT_PRIO0, conc)
    for got, ref, what in ((raised, level0, 'default against DEV_EMIT_PRIO0'), (raised, alone, 'default against the solve alone'),
                           (level0, alone, 'DEV_EMIT_PRIO0 against the solve alone')):
        for k in KEYS:
            assert np.array_equal(got[k], ref[k], equal_nan=True), (what, k)
