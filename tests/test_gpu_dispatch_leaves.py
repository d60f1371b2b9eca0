"""-m gpu : every leaf of the launchers' dispatch (csrc/igt_dispatch.h) at the smallest shape that selects it.

The launchers turn (cand_mode, hi_order, n_rk4 == 4) into template arguments through one helper; search, emit and rollout-all
share its mapping, so a wrong mapping would agree with itself.  Each case (parity_cases.leaf_case: B = 5, C = 64, N = 8, one
obstacle, dt = 0.1; four families x n_rk4 in 4, 3, 2, 7 x both precisions) therefore asserts
  (a) the standing invariant: (cost, argmin, x, u) of the solve are, bit for bit, rollout-all's entry at the feasible minimum of
      rollout-all's costs, ties to the lowest index;
  (b) the numpy oracle's answer through the shared comparison (parity_cases.check_case) at the suite's bars: 1e-9 in float64,
      REL_TOL and the float32 set-aside widths in float32.  The oracle alone sets none of these scenarios aside (recorded in
      tests/golden/parity_floors.json, held to the inputs by tests/test_parity_floors_host.py).
n_rk4 = 4 is the build of the reference's discretisation (HI = false, NRK = 4); 3 and 2 set KP::hi_order at these limits
(HI = true, NRK = 0); 7 is the short polynomials with the sub-steps counted at run time (HI = false, NRK = 0).  At B = 5 the
float64 search keeps trajectories where it can (n_rk4 = 4: search_f64_kernel_cap, emit_gather_f64_kernel) and runs the _o2 /
_o2w builds and emit_f64_kernel otherwise; the polish cases run polish_f64_kernel's three builds in both gradient modes.
What needs a larger batch keeps its tests: the (HI = false, NRK = 4) builds of _o2 / _o2w and of emit_f64_kernel, every family,
and emit_seg_f64_kernel: test_gpu_parity.py::test_emit_in_pieces_is_the_emit_in_one_piece (B = 700 to 8200, with and without
DEV_NO_SEG_EMIT) and test_search_and_emit_agree_bitwise[2304-*-f64]; the pool search and the live rows: test_gpu_pool_loop.py,
test_gpu_pool_step.py, test_gpu_lane_refill.py; the float search without checkpoints: test_search_and_emit_agree_bitwise at
B = 2304 and 9000.  The roll-out's call sites (csrc/igt_fast64.h rollout_one / rollout_pool, csrc/igt_fast_impl.inc
rollout_pair) and the tests that reach each are listed in profiles/rollout_options_identity.txt; the one that none of them
reached, the literal wave-per-trajectory mapping of the developer library, has its case at the end of this file."""
import numpy as np
import pytest

import np_oracle as O
import parity_cases as PC
from helpers import oracle_params, rel_err
from igtmpc._lib import DEV_LITERAL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def igt():
    import igtmpc
    igtmpc.load_library()
    return igtmpc


def test_cases_cover_the_three_discretisations(igt):
    """By the parameters the library reports for each case's solver (open_solver holds them equal to the case's), through
    the rule of csrc/igt_api.hip (parity_cases.leaf_hi_order; test_host_logic.py holds it to the source)."""
    hi = {}
    for n in PC.LEAF_N_RK4:
        case = PC.leaf_case('f64', 'lattice', n)
        with PC.open_solver(igt, case) as s:
            hi[n] = bool(PC.leaf_hi_order(oracle_params(s)))
    assert hi == {4: False, 3: True, 2: True, 7: False}
    assert {(hi[n], 4 if n == 4 and not hi[n] else 0) for n in hi} == {(True, 0), (False, 4), (False, 0)}


@pytest.mark.parametrize('n_rk4', PC.LEAF_N_RK4)
@pytest.mark.parametrize('cand', PC.LEAF_FAMILIES)
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_solve_is_rollout_all_bitwise_and_the_oracles(igt, dtype, cand, n_rk4):
    case = PC.leaf_case(dtype, cand, n_rk4)
    with PC.open_solver(igt, case) as s:
        got = PC.device_solve(s, case)
        pos, _ = PC.solve_args(case)
        allc = s.rollout_all(*pos[:5])
    # (a)
    J = np.where(allc['viol'] == 0, allc['cost'].astype(np.float64), np.inf)
    assert 0 < np.isfinite(J.min(axis=1)).sum() < case['B']            # solved and unsolved scenarios
    for i in range(case['B']):
        if not np.isfinite(J[i].min()):
            assert got['status'][i] == 1 and got['argmin'][i] == -1
            continue
        c = int(np.argmin(J[i]))                                       # the first of equal minima
        assert got['status'][i] == 0 and got['argmin'][i] == c, (i, got['argmin'][i], c)
        assert got['cost'][i] == allc['cost'][i, c]
        assert np.array_equal(got['x'][i], allc['X'][i, c]) and np.array_equal(got['u'][i], allc['U'][i, c])
    # (b)
    m = PC.check_case(case, got, PC.oracle_passes(case))
    assert m['compared'] == m['B']


@pytest.mark.parametrize('n_rk4', PC.LEAF_N_RK4)
@pytest.mark.parametrize('grad', ['fd', 'adjoint'])
def test_polished_solve_is_its_table_rollout_bitwise_and_the_oracles(igt, grad, n_rk4):
    """polish_iters = 1: (a) x_out and cost_out are rollout-all's for u_out fed back as a table, bit for bit, no verdict raised;
    (b) they are the oracle's roll-out and cost of u_out within 1e-9, feasible by the oracle's verdicts, no dearer than the
    unpolished winner, whose arg-min and status stay."""
    case = PC.leaf_case('f64', 'lattice', n_rk4)
    pos, _ = PC.solve_args(case)
    with PC.open_solver(igt, case) as s:
        plain = PC.device_solve(s, case)
    with PC.open_solver(igt, case, polish_iters=1, polish_grad=grad) as s:
        got = PC.device_solve(s, case)
    assert np.array_equal(got['argmin'], plain['argmin']) and np.array_equal(got['status'], plain['status'])
    idx = np.flatnonzero(got['status'] == 0)
    assert len(idx) >= case['B'] // 2
    assert (got['cost'][idx] <= plain['cost'][idx]).all() and (got['cost'][idx] < plain['cost'][idx]).any()
    U = np.zeros((case['C'], 2, case['N']))
    U[:len(idx)] = got['u'][idx]
    table = dict(case, cand='table', table=U, key=case['key'] + '/table')
    with PC.open_solver(igt, table) as t:
        r = t.rollout_all(*[np.ascontiguousarray(a[idx]) for a in pos[:5]])
    d = np.arange(len(idx))
    assert np.array_equal(r['X'][d, d], got['x'][idx]) and np.array_equal(r['cost'][d, d], got['cost'][idx])
    assert (r['viol'][d, d] == 0).all()
    a = case['args']
    X = O.rollout_frenet(O.apply_flags(a['x0'][idx], a['flags'][idx]), got['u'][idx], a['kparams'][idx], case['P'])
    J = O.stage_cost(X, got['u'][idx], case['P'])
    g, mask = O.constraint_violation(X, got['u'][idx], a['u_prev'][idx], a['obs'][idx], case['cinf'][0], case['cinf'][1], case['P'],
                                     check_rate=True)
    ex, ej = rel_err(got['x'][idx], X).max(), rel_err(got['cost'][idx], J).max()
    print(f'polish {grad} n_rk4={n_rk4}: max rel err x {ex:.2e} cost {ej:.2e}; worst margin {g.max():.3e}')
    assert ex <= 1e-9 and ej <= 1e-9
    assert (mask == 0).all()


@pytest.mark.parametrize('cand,n_rk4', [(c, 4) for c in PC.LEAF_FAMILIES] + [('lattice', 3)])
def test_literal_mapping_picks_rollout_alls_minimum(igt, monkeypatch, cand, n_rk4):
    """search_literal_f64_kernel (libigtmpc_dev.so, IGT_DEV_FLAGS = DEV_LITERAL): lane 0 of a wave rolls the candidate through
    rollout_one without cost or verdicts, and the wave sums the stage terms of the stored states in another order than the
    roll-out does (stage-parallel, then a butterfly), so its cost is rollout-all's only to rounding and the bit-for-bit
    invariant of this file holds for what emit_f64_kernel re-rolls, not for the cost.  Asserted: the same scenarios solved;
    (x, u) are rollout-all's entry at the arg-min, bit for bit; the cost is rollout-all's at the arg-min, and the arg-min's
    cost rollout-all's feasible minimum, within the bound of two summations of the same n = 3 N + 2 non-negative terms in any
    order, 2 (n - 1) 2^-53 times their sum (= cost + progress), plus the rounding of the final subtraction: 64 2^-53 (|cost| +
    2 |progress|) at N = 8.  n_rk4 = 3: the long polynomials (HI)."""
    case = PC.leaf_case('f64', cand, n_rk4)
    monkeypatch.setenv('IGT_DEV_FLAGS', str(DEV_LITERAL))
    with PC.open_solver(igt, case) as s:
        got = PC.device_solve(s, case)
        pos, _ = PC.solve_args(case)
        allc = s.rollout_all(*pos[:5])
    J = np.where(allc['viol'] == 0, allc['cost'].astype(np.float64), np.inf)
    assert 0 < np.isfinite(J.min(axis=1)).sum() < case['B']
    for i in range(case['B']):
        if not np.isfinite(J[i].min()):
            assert got['status'][i] == 1 and got['argmin'][i] == -1
            continue
        c = int(got['argmin'][i])
        assert got['status'][i] == 0 and c >= 0 and allc['viol'][i, c] == 0, (i, c)
        assert np.array_equal(got['x'][i], allc['X'][i, c]) and np.array_equal(got['u'][i], allc['U'][i, c])
        ds = allc['X'][i, c, 2, -1] - allc['X'][i, c, 2, 0]
        bound = 64 * 2.0 ** -53 * (abs(J[i, c]) + 2 * abs(ds))
        print(f'literal {cand} n_rk4={n_rk4} scenario {i}: |cost - rollout-all| {abs(got["cost"][i] - J[i, c]):.2e}, '
              f'above the minimum {J[i, c] - J[i].min():.2e}, bound {bound:.2e}')
        assert abs(got['cost'][i] - J[i, c]) <= bound
        assert J[i, c] - J[i].min() <= 2 * bound
