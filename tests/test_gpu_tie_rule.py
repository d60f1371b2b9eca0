"""The winner rule over a scenario's partials -- (J, c) lexicographic, ties to the lowest candidate index whatever the unit order
(csrc/igt_device.h beats, csrc/igt_kernels_common.h best_partial) -- on every emit kernel.

A table whose second half is a bit-exact copy of its first gives every scenario two units with the same 64 (float64) or 128
(float32) candidates: every cost is attained twice, C/2 apart, in two different units, and the reduction of the partials sees an
exact tie between unit 0 and unit 1.  The answer must be the copy in the first half, and it must be the first minimal index of
the costs that rollout_all of the same handle gives.  What this pins is the strict `<` on the cost: a reduction that lets the
equal cost of a later unit win answers C/2 too high.  (The table family's units are in index order, so the copy in the later
unit always has the higher index and `<` or `<=` on the index cannot show here: profiles/solve_variants_identity.txt.)"""
import numpy as np
import pytest

import np_oracle as O
from igtmpc import _lib as L

B, DT, N_RK4, SEED = 5, 0.1, 4, 7
# case -> (dtype, N, IGT_DEV_FLAGS): the emit kernel each one reaches (csrc/igt_launch.h plan_search64 / plan_search32)
CASES = {
    'emit_gather_f64_kernel': ('f64', 8, 0),                                          # B C / 64 units: trajectories are kept
    'emit_seg_f64_kernel': ('f64', 8, L.DEV_NO_CAPTURE),                              # ... not kept: the emit in pieces
    'emit_f64_kernel': ('f64', 8, L.DEV_NO_CAPTURE | L.DEV_NO_SEG_EMIT),              # ... and in one piece
    'emit_seg_kernel': ('f32', 8, 0),                                                 # N % 4 == 0: four pieces
    'emit_fast_kernel': ('f32', 7, 0),                                                # an odd horizon: one piece
}


def n_candidates(dtype):
    return 128 if dtype == 'f64' else 256          # two units: 64 candidates a unit in float64, 128 in float32


def tie_case(dtype, N):
    """-> (args of solve / rollout_all, table[C,2,N]): five scenarios that share scenario 0's previous controls (a table's controls
    are held to the rate limits from u_prev) and a table made of two copies of every 256 / (C/2)-th lattice candidate around them."""
    from igtmpc.scenarios import make_batch
    npdt = np.float64 if dtype == 'f64' else np.float32
    C = n_candidates(dtype)
    b = make_batch(8, N=N, dt=DT, seed=SEED, dtype=npdt)
    b = {k: np.ascontiguousarray(v[:B]) for k, v in b.items() if isinstance(v, np.ndarray) and len(v) >= B}
    b['u_prev'] = np.ascontiguousarray(np.broadcast_to(b['u_prev'][:1], b['u_prev'].shape))
    lattice = O.candidates_lattice(b['u_prev'][:1].astype(np.float64), O.Params(N=N, dt=DT, n_rk4=N_RK4), 256)[0]
    half = lattice[::256 // (C // 2)]
    table = np.ascontiguousarray(np.concatenate([half, half]))
    assert table.shape == (C, 2, N) and (table[:C // 2] == table[C // 2:]).all()
    return (b['x0'], b['u_prev'], b['kparams'], b['flags'], b['obs_xy']), table


def first_minimum(cost, ok):
    """-> (index of the first minimal feasible cost per scenario, whether there is one)."""
    J = np.where(ok, cost.astype(np.float64), np.inf)
    return J.argmin(axis=1), np.isfinite(J.min(axis=1))


@pytest.mark.parametrize('dtype,N', sorted({(d, n) for d, n, _ in CASES.values()}))
def test_the_tie_cases_tie_where_they_should(dtype, N):
    """The oracle alone: at least four of the five scenarios are feasible, and their best cost is attained at exactly two indices,
    C/2 apart; the next cost lies more than 1e-3 max(1, |best|) above it, so the float32 costs of rollout_all (rounded to 6e-8
    relative) keep the order."""
    (x0, u_prev, kp, flags, obs), table = tie_case(dtype, N)
    C = n_candidates(dtype)
    f8 = lambda a: a.astype(np.float64)
    ref = O.solve_batch(f8(x0), f8(u_prev), f8(kp), flags, f8(obs), None, None, O.Params(N=N, dt=DT, n_rk4=N_RK4), C=C, U=table,
                        return_all=True)
    J = np.where(ref['feas'], ref['J'], np.inf)
    feasible = np.flatnonzero(ref['status'] == 0)
    assert len(feasible) >= 4
    for b in feasible:
        at = np.flatnonzero(J[b] == J[b].min())
        assert len(at) == 2 and at[1] - at[0] == C // 2, (b, at)
        rest = np.delete(J[b], at)
        assert rest.min() - J[b].min() > 1e-3 * max(1.0, abs(J[b].min())), (b, rest.min(), J[b].min())


@pytest.mark.gpu
@pytest.mark.parametrize('kernel', sorted(CASES))
def test_an_exact_tie_between_two_units_goes_to_the_lower_index(kernel, monkeypatch):
    import igtmpc
    dtype, N, dev = CASES[kernel]
    C = n_candidates(dtype)
    args, table = tie_case(dtype, N)
    monkeypatch.setenv('IGT_DEV_FLAGS', str(dev))
    with igtmpc.BatchSolver(N=N, dt=DT, n_rk4=N_RK4, C=C, n_obs=1, dtype=dtype, cand_mode='table') as s:
        s.set_candidate_table(table)
        got = s.solve(*args)
        every = s.rollout_all(*args, want_X=False, want_U=False)
    first, any_feasible = first_minimum(every['cost'], (every['viol'] == 0) & np.isfinite(every['cost']))
    solved = got['status'] == 0
    assert solved.sum() >= 4
    assert (solved == any_feasible).all()
    assert (got['argmin'][solved] < C // 2).all(), got['argmin']
    assert (got['argmin'][solved] == first[solved]).all(), (got['argmin'], first)
    assert (got['argmin'][~solved] == -1).all()
